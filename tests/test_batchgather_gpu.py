"""GPU tier of the batch gather (csrc/batchgather.hip): exact equality with the numpy restatement (tests/batchgather_ref.py) for the
three output kinds, with and without flips, at every shape class the kernel distinguishes; the grid-stride wrap, unaligned
outputs, offsets past 2^31, the argument checks of the entry and the row check of the Python layer."""
import numpy as np
import pytest
import torch

import batchgather_ref as R

pytestmark = pytest.mark.gpu

SEED = 0x5EED
GI_ERR_INVALID = -1
TORCH_OF = {0: torch.float32, 1: torch.int64, 2: torch.uint8}


def _entry(store, rows, out_kind, keys=None, seed=SEED, out=None):
    """gi_batch_gather on device tensors -> the (n,h,w) output on the host."""
    import gan_inpainting_amd  # noqa: F401
    from gan_inpainting_amd import backend as B
    n_store, h, w = store.shape
    rows_d = torch.tensor(list(rows), dtype=torch.int64, device="cuda")
    keys_d = None if keys is None else torch.tensor(list(keys), dtype=torch.int64, device="cuda")
    if out is None:
        out = torch.empty((len(rows), h, w), dtype=TORCH_OF[out_kind], device="cuda")
    B.check(B.lib().gi_batch_gather(B.get_ctx(), B.ptr(store), n_store, h, w, B.ptr(rows_d), len(rows), B.ptr(keys_d), seed, out_kind,
                                    out.data_ptr()))
    torch.cuda.synchronize()
    return out.cpu().numpy()


def _store(n, h, w, seed=1):
    rng = np.random.Generator(np.random.PCG64(seed))
    return rng.integers(0, 256, (n, h, w), dtype=np.uint8)


def _keys(n, epoch=0):
    return [R.key_of("train", epoch, r) for r in range(n)]


def _same(got, ref):
    return got.dtype == ref.dtype and got.shape == ref.shape and np.array_equal(got.view(np.uint8), ref.view(np.uint8))   # bit for bit


# (16,16), (8,8): the vector path. (5,7): h*w odd, every image base misaligned. (3,4): a vector width. (4,3), (1,1): narrower than
# a lane's four pixels. (6,10): a tail after full quads
SHAPES = [(16, 16), (8, 8), (5, 7), (3, 4), (4, 3), (1, 1), (6, 10)]


@pytest.mark.parametrize("h,w", SHAPES, ids=[f"{h}x{w}" for h, w in SHAPES])
@pytest.mark.parametrize("out_kind", [0, 1, 2], ids=["fp32", "int64", "uint8"])
def test_equals_the_restatement_exactly(h, w, out_kind):
    store = _store(7, h, w)
    dev = torch.from_numpy(store).cuda()
    keys = _keys(64)
    bits = R.flip_bits(SEED, keys)
    rows = [3, 0, 6, 6, 2, 5, 1, 4, 0]
    use = keys[:len(rows)]
    assert {bits[i] for i in range(len(rows))} == {0, 1}                      # both flip states in one launch
    assert _same(_entry(dev, rows, out_kind), R.gather(store, rows, out_kind))
    assert _same(_entry(dev, rows, out_kind, use), R.gather(store, rows, out_kind, use, SEED))
    all_flip = [k for k, b in zip(keys, bits) if b][:len(rows)]
    assert _same(_entry(dev, rows, out_kind, all_flip), np.ascontiguousarray(R.gather(store, rows, out_kind)[:, :, ::-1]))
    none_flip = [k for k, b in zip(keys, bits) if not b][:len(rows)]
    assert _same(_entry(dev, rows, out_kind, none_flip), R.gather(store, rows, out_kind))
    assert _same(_entry(dev, rows, out_kind, use, SEED + 1), R.gather(store, rows, out_kind, use, SEED + 1))      # the seed counts


def test_every_byte_value_has_the_float32_quotient():
    store = np.arange(256, dtype=np.uint8).reshape(1, 16, 16)
    got = _entry(torch.from_numpy(store).cuda(), [0], 0)
    ref = (np.arange(256, dtype=np.float32) / np.float32(255)).reshape(1, 16, 16)
    assert _same(got, ref)
    assert got.flat[0] == 0.0 and got.flat[255] == 1.0
    # the scalar path computes the same quotients
    store2 = np.arange(255, dtype=np.uint8).reshape(1, 17, 15)
    assert _same(_entry(torch.from_numpy(store2).cuda(), [0], 0), (np.arange(255, dtype=np.float32) / np.float32(255)).reshape(1, 17, 15))


@pytest.mark.parametrize("rows", [[2, 2, 2, 2], [4, 3, 2, 1, 0], [0, 4], [4], [0]], ids=["repeated", "reversed", "first-last", "last-n1", "first-n1"])
@pytest.mark.parametrize("h,w", [(8, 8), (5, 7)], ids=["8x8", "5x7"])
def test_row_patterns(rows, h, w):
    store = _store(5, h, w, seed=2)
    dev = torch.from_numpy(store).cuda()
    keys = _keys(len(rows), epoch=1)
    for out_kind in (0, 1, 2):
        assert _same(_entry(dev, rows, out_kind), R.gather(store, rows, out_kind))
        assert _same(_entry(dev, rows, out_kind, keys), R.gather(store, rows, out_kind, keys, SEED))


@pytest.mark.parametrize("h,w", [(64, 64), (33, 63)], ids=["64x64-vector", "33x63-scalar"])
def test_more_work_than_the_grid_cap(h, w):
    """600 rows of 64 x 64: 600 * 4 chunks of 256 quads against the 2048 workgroups of the capped grid, so the stride loop wraps
    (33 x 63: 600 * 3 = 1800 chunks stay under it - the same rows on the scalar path, then 800 rows = 2400 chunks wrap there too)."""
    store = _store(3, h, w, seed=3)
    dev = torch.from_numpy(store).cuda()
    n = 600 if (h, w) == (64, 64) else 800
    assert n * ((h * ((w + 3) // 4) + 255) // 256) > 2048
    rows = [(i * 7 + i // 5) % 3 for i in range(n)]
    keys = _keys(n)
    for out_kind in (0, 1, 2):
        assert _same(_entry(dev, rows, out_kind, keys), R.gather(store, rows, out_kind, keys, SEED))


@pytest.mark.parametrize("out_kind", [0, 1, 2], ids=["fp32", "int64", "uint8"])
def test_an_unaligned_output_takes_the_scalar_path(out_kind):
    """An output 4, 8 and 12 bytes past a 16-byte boundary (for uint8 also 1 byte): the same values, nothing outside the tensor."""
    h, w, rows = 6, 8, [1, 0, 2, 1]
    store = _store(3, h, w, seed=4)
    dev = torch.from_numpy(store).cuda()
    keys = _keys(len(rows), epoch=2)
    ref = R.gather(store, rows, out_kind, keys, SEED).reshape(-1)
    esize = {0: 4, 1: 8, 2: 1}[out_kind]
    offs = [o for o in (1, 4, 8, 12) if o % esize == 0]
    count = ref.size
    for off in offs:
        pad = 16 // esize
        buf = torch.full((count + 2 * pad,), 5, dtype=TORCH_OF[out_kind], device="cuda")
        assert buf.data_ptr() % 16 == 0
        e0 = off // esize
        view = buf[e0:e0 + count]
        assert view.data_ptr() % 16 == off
        got = _entry(dev, rows, out_kind, keys, out=view)
        assert _same(got, ref)
        host = buf.cpu()
        assert bool((host[:e0] == 5).all()) and bool((host[e0 + count:] == 5).all())          # the guards on both sides


def test_offsets_past_2_to_the_31():
    """A (32770, 256, 256) store, uninitialised but for images 0, 32768 and 32769: rows[i] * h * w >= 2^31 for the last two."""
    h = w = 256
    dev = torch.empty((32770, h, w), dtype=torch.uint8, device="cuda")
    imgs = _store(3, h, w, seed=5)
    at = [0, 32768, 32769]
    for i, r in enumerate(at):
        dev[r] = torch.from_numpy(imgs[i]).cuda()
    assert at[1] * h * w >= 2 ** 31
    rows, sel = [32769, 0, 32768, 32769], [2, 0, 1, 2]
    keys = _keys(4, epoch=1)
    for out_kind in (0, 1, 2):
        assert _same(_entry(dev, rows, out_kind, keys), R.gather(imgs, sel, out_kind, keys, SEED))
    del dev
    torch.cuda.empty_cache()


def test_invalid_arguments_are_refused_on_the_host():
    import gan_inpainting_amd  # noqa: F401
    from gan_inpainting_amd import backend as B
    lib, ctx = B.lib(), B.get_ctx()
    store = torch.from_numpy(_store(3, 8, 8)).cuda()
    rows = torch.tensor([0, 1], dtype=torch.int64, device="cuda")
    out = torch.full((2, 8, 8), 7.0, device="cuda")
    s, r, o = B.ptr(store), B.ptr(rows), B.ptr(out)
    assert lib.gi_batch_gather(None, s, 3, 8, 8, r, 2, None, 0, 0, o) == GI_ERR_INVALID
    assert lib.gi_batch_gather(ctx, None, 3, 8, 8, r, 2, None, 0, 0, o) == GI_ERR_INVALID
    assert lib.gi_batch_gather(ctx, s, 3, 8, 8, None, 2, None, 0, 0, o) == GI_ERR_INVALID
    assert lib.gi_batch_gather(ctx, s, 3, 8, 8, r, 2, None, 0, 0, None) == GI_ERR_INVALID
    assert lib.gi_batch_gather(ctx, s, 3, 8, 8, r, 0, None, 0, 0, o) == GI_ERR_INVALID          # n
    assert lib.gi_batch_gather(ctx, s, 3, 8, 8, r, -2, None, 0, 0, o) == GI_ERR_INVALID
    assert lib.gi_batch_gather(ctx, s, 0, 8, 8, r, 2, None, 0, 0, o) == GI_ERR_INVALID          # n_store
    assert lib.gi_batch_gather(ctx, s, 3, 0, 8, r, 2, None, 0, 0, o) == GI_ERR_INVALID          # h
    assert lib.gi_batch_gather(ctx, s, 3, 8, -1, r, 2, None, 0, 0, o) == GI_ERR_INVALID         # w
    assert lib.gi_batch_gather(ctx, s, 3, 8, 8, r, 2, None, 0, 3, o) == GI_ERR_INVALID          # out_kind
    assert lib.gi_batch_gather(ctx, s, 3, 8, 8, r, 2, None, 0, -1, o) == GI_ERR_INVALID
    assert b"batch_gather" in lib.gi_last_error()
    torch.cuda.synchronize()
    assert bool((out == 7.0).all())          # nothing was launched
    assert lib.gi_batch_gather(ctx, s, 3, 8, 8, r, 2, None, 0, 0, o) == 0
    torch.cuda.synchronize()
    assert _same(out.cpu().numpy(), R.gather(store.cpu().numpy(), [0, 1], 0))


def test_the_python_layer_refuses_rows_outside_the_store():
    """No out-of-range row reaches the device: cache.gather checks host and device indices alike."""
    import gan_inpainting_amd  # noqa: F401
    from gan_inpainting_amd.lib.data.cache import DeviceImageCache
    store = _store(5, 8, 12, seed=6)
    cache = DeviceImageCache(torch.from_numpy(store).cuda(), None, None, torch.arange(5))
    for bad in ([5], [-1], [0, 4, 7]):
        with pytest.raises(IndexError):
            cache.gather(bad, "ground")
        with pytest.raises(IndexError):
            cache.gather(torch.tensor(bad, device="cuda"), "ground")
    with pytest.raises(ValueError):
        cache.gather(torch.tensor([1], dtype=torch.int32, device="cuda"), "ground")
    with pytest.raises(ValueError):
        cache.gather([1], "mask")            # no such store
    got = cache.gather(torch.tensor([4, 0], device="cuda"), "ground")
    assert tuple(got.shape) == (2, 1, 8, 12) and _same(got.cpu().numpy()[:, 0], R.gather(store, [4, 0], 0))
    raw = cache.gather([4, 0], "ground", raw=True)
    assert _same(raw.cpu().numpy(), store[[4, 0]])
