"""GPU tier of the device mask generator (csrc/maskgen.hip): exact equality with the numpy restatement of DESIGN.md 4.1e-2
(tests/maskgen_ref.py) at every shape class the kernel distinguishes, the coverage counts, independence of the batch, argument
checks, and plugin runs on generated masks."""
import numpy as np
import pytest
import torch

import maskgen_ref as R

pytestmark = pytest.mark.gpu

SEED = 0x5EED


def _generate(kind, seed, keys, H, W, coverage=True):
    import gan_inpainting_amd  # noqa: F401
    from gan_inpainting_amd.lib.data.masks import DeviceMaskGenerator
    gen = DeviceMaskGenerator(kind, H, W, seed)
    out = gen(torch.tensor(list(keys), dtype=torch.int64), return_coverage=coverage)
    torch.cuda.synchronize()
    return out


def _train_keys(n):
    import gan_inpainting_amd  # noqa: F401
    from gan_inpainting_amd.lib.data.masks import mask_key
    return [mask_key("train", 7, i) for i in range(n)]


# (kinds, n, H, W, keys): the issue's table, then the two sizes either side of the 32-bit / 64-bit cross-product switch
# ((W + H - 2) * max(2, min(H, W) / 8) <= 65535 holds at 512 x 512 with 65408 and fails at 520 x 520) and a one-row last band
CASES = [
    pytest.param(("rect", "freeform"), 3, 64, 64, None, id="64x64"),
    pytest.param(("rect", "freeform"), 5, 37, 53, None, id="37x53-ragged"),
    pytest.param(("rect", "freeform"), 2, 48, 80, None, id="48x80"),
    pytest.param(("freeform",), 2, 256, 256, None, id="256x256-bands"),
    pytest.param(("freeform",), 1, 1024, 1024, None, id="1024x1024-wide"),
    pytest.param(("rect", "freeform"), 33, 64, 64, "train7", id="64x64-keys-above-2^32"),
    pytest.param(("freeform",), 1, 512, 512, None, id="512x512-last-narrow"),
    pytest.param(("freeform",), 1, 520, 520, None, id="520x520-first-wide"),
    pytest.param(("rect", "freeform"), 2, 17, 16, None, id="17x16-smallest"),
]


@pytest.mark.parametrize("kinds,n,H,W,keys", CASES)
def test_equals_the_restatement_exactly(kinds, n, H, W, keys):
    keys = _train_keys(n) if keys == "train7" else list(range(n))
    for kind in kinds:
        ref = R.masks(kind, SEED, keys, H, W)
        got, cover = _generate(kind, SEED, keys, H, W)
        assert got.dtype == torch.float32 and tuple(got.shape) == (n, 1, H, W)
        got = got.cpu().numpy()
        diff = int((got != ref).sum())
        print(f"{kind} {n}x{H}x{W}: {diff} pixels differ, coverage {ref.mean():.3f}")
        assert diff == 0, f"{kind} {H}x{W}: {diff} of {ref.size} pixels differ from the restatement"
        assert cover.dtype == torch.int32
        assert cover.cpu().tolist() == [int(m.sum()) for m in ref]      # coverage_out = number of ones per image
        assert cover.cpu().tolist() == got.reshape(n, -1).sum(1).astype(np.int64).tolist()


@pytest.mark.parametrize("kind", ["rect", "freeform"])
def test_a_key_gives_one_mask_whatever_the_batch(kind):
    keys = _train_keys(9)
    whole = _generate(kind, SEED, keys, 40, 56, coverage=False)
    alone = _generate(kind, SEED, [keys[4]], 40, 56, coverage=False)
    assert torch.equal(alone[0], whole[4])
    shuffled = _generate(kind, SEED, keys[::-1], 40, 56, coverage=False)
    assert torch.equal(shuffled.flip(0), whole)
    assert torch.equal(_generate(kind, SEED, keys, 40, 56, coverage=False), whole)          # the same seed twice
    other = _generate(kind, SEED + 1, keys, 40, 56, coverage=False)
    assert not torch.equal(other, whole)
    assert all(not torch.equal(other[i], whole[i]) for i in range(9)) or kind == "rect"     # (two rectangles may coincide)
    # without coverage_out, and with device keys
    import gan_inpainting_amd  # noqa: F401
    from gan_inpainting_amd.lib.data.masks import DeviceMaskGenerator
    dev = DeviceMaskGenerator(kind, 40, 56, SEED)(torch.tensor(keys, dtype=torch.int64, device="cuda"))
    assert torch.equal(dev, whole)


def test_invalid_arguments_are_refused_on_the_host():
    import gan_inpainting_amd  # noqa: F401
    from gan_inpainting_amd import backend as B
    lib, ctx = B.lib(), B.get_ctx()
    keys = torch.zeros(4, dtype=torch.int64, device="cuda")
    out = torch.full((4, 1, 64, 64), 7.0, device="cuda")
    GI_ERR_INVALID = -1
    assert lib.gi_mask_generate(ctx, 2, 0, B.ptr(keys), 4, 64, 64, B.ptr(out), None) == GI_ERR_INVALID       # kind
    assert lib.gi_mask_generate(ctx, -1, 0, B.ptr(keys), 4, 64, 64, B.ptr(out), None) == GI_ERR_INVALID
    assert lib.gi_mask_generate(ctx, 1, 0, B.ptr(keys), 4, 8, 64, B.ptr(out), None) == GI_ERR_INVALID        # H = 8
    assert lib.gi_mask_generate(ctx, 1, 0, B.ptr(keys), 4, 64, 4097, B.ptr(out), None) == GI_ERR_INVALID
    assert lib.gi_mask_generate(ctx, 0, 0, B.ptr(keys), 0, 64, 64, B.ptr(out), None) == GI_ERR_INVALID       # n = 0
    assert lib.gi_mask_generate(ctx, 0, 0, None, 4, 64, 64, B.ptr(out), None) == GI_ERR_INVALID
    assert b"mask_generate" in lib.gi_last_error()
    torch.cuda.synchronize()
    assert bool((out == 7.0).all())          # nothing was launched
    assert lib.gi_mask_generate(ctx, 0, 0, B.ptr(keys), 4, 64, 64, B.ptr(out), None) == 0
    torch.cuda.synchronize()
    assert set(out.unique().tolist()) == {0.0, 1.0}


@pytest.mark.parametrize("W", [37, 40])
def test_an_unaligned_output_takes_the_same_quads(W):
    """mask_out only has to be 4-byte aligned: the 16-byte stores are aligned in memory, not to the row. W = 40: every row has the
    tensor's own shift and the kernel counts the quads of a row from it; W = 37: the shift changes from row to row."""
    import gan_inpainting_amd  # noqa: F401
    from gan_inpainting_amd import backend as B
    H, n = 24, 3
    keys = torch.arange(n, dtype=torch.int64, device="cuda")
    ref = torch.from_numpy(R.masks("freeform", SEED, range(n), H, W)).reshape(-1)
    for off in (1, 2, 3):
        buf = torch.full((n * H * W + 8,), 5.0, device="cuda")
        view = buf[off:off + n * H * W]
        assert view.data_ptr() % 16 == 4 * off
        B.check(B.lib().gi_mask_generate(B.get_ctx(), 1, SEED, B.ptr(keys), n, H, W, view.data_ptr(), None))
        torch.cuda.synchronize()
        assert torch.equal(view.cpu(), ref)
        assert bool((buf[:off] == 5.0).all()) and bool((buf[off + n * H * W:] == 5.0).all())      # nothing outside the tensor


def test_plugin_run_on_generated_masks(tmp_path, monkeypatch):
    """wgan_l1 over epochs 0..2 of four batches at 64 x 64 with --masks freeform: finite losses, test masks that do not change with
    the epoch, training masks that do, and a composite that leaves the ground truth outside the hole untouched."""
    import pickle
    import gan_inpainting_amd  # noqa: F401
    from gan_inpainting_amd import train, trainer
    from gan_inpainting_amd.lib.data import masks as M

    made, steps = [], []
    gen_call, step_call = M.DeviceMaskGenerator.__call__, trainer.WGANStep.__call__

    def recording_gen(self, keys, *a, **kw):
        out = gen_call(self, keys, *a, **kw)
        made.append((keys.cpu().tolist(), out.cpu()))
        return out

    def recording_step(self, ground, mask, update_g):
        L = step_call(self, ground, mask, update_g)
        torch.cuda.synchronize()
        steps.append((ground.cpu(), mask.cpu(), self.inpainted[:ground.shape[0]].cpu()))
        return L

    monkeypatch.setattr(M.DeviceMaskGenerator, "__call__", recording_gen)
    monkeypatch.setattr(trainer.WGANStep, "__call__", recording_step)
    train.main(["-exp", "wgan_l1", "-ep", "2", "-b", "4", "--imagedim", "64", "--saveevery", "10", "--evalevery", "1", "--samples", "16",
                "--outdir", str(tmp_path), "--dtype", "fp32", "--g-every", "2", "--masks", "freeform", "--mask-seed", str(SEED)])

    with open(tmp_path / "model" / "wgan_l1" / "training_epoch_history.obj", "rb") as h:
        hist = pickle.load(h)
    assert len(hist) == 3 and all(np.isfinite(v) for rec in hist for v in rec["losses"].values())

    by_key = {}
    for keys, out in made:
        for k, m in zip(keys, out):
            by_key.setdefault(k, []).append(m)
    split = lambda k: k >> 56              # noqa: E731
    epoch = lambda k: (k >> 32) & 0xFFFFFF   # noqa: E731
    row = lambda k: k & 0xFFFFFFFF         # noqa: E731
    # every mask is the restatement's, whichever pass asked for it
    for k, ms in by_key.items():
        ref = torch.from_numpy(R.masks("freeform", SEED, [k], 64, 64)[0])
        assert all(torch.equal(m, ref) for m in ms)
    # test split: epoch 0 in the key, generated by the evaluation passes of epochs 1 and 2 -> each key twice, one mask
    test_keys = [k for k in by_key if split(k) == 1]
    assert len(test_keys) == 64 and all(epoch(k) == 0 for k in test_keys) and all(len(by_key[k]) == 2 for k in test_keys)
    # training split: the 16 rows under epochs 0, 1, 2; a row's mask differs between epochs
    train_keys = [k for k in by_key if split(k) == 0]
    assert sorted({epoch(k) for k in train_keys}) == [0, 1, 2] and sorted({row(k) for k in train_keys}) == list(range(16))
    for r in range(16):
        m1, m2 = by_key[(1 << 32) | r][0], by_key[(2 << 32) | r][0]
        assert not torch.equal(m1, m2)

    assert len(steps) == 12
    for ground, mask, inpainted in steps:
        assert set(mask.unique().tolist()) <= {0.0, 1.0} and 0.0 < float(mask.mean()) < 0.6
        outside = mask == 0
        assert torch.equal(inpainted.view(torch.int32)[outside], ground.view(torch.int32)[outside])      # bit for bit
        assert not torch.equal(inpainted[mask == 1], ground[mask == 1])


@pytest.mark.parametrize("exp,kind", [("experiment1_global_local_D", "rect"), ("wgan_perceptual_style_faceparsing", "freeform")])
def test_other_plugins_take_generated_masks_unchanged(tmp_path, exp, kind):
    """The dual-discriminator plugin and config 5 (which also passes the loader's third item on) run on row ids as they do on mask
    pixels: the conversion happens in the shared loop, in front of every plugin."""
    import pickle
    import gan_inpainting_amd  # noqa: F401
    from gan_inpainting_amd import train
    if exp == "wgan_perceptual_style_faceparsing":      # the 7-level face-parsing network needs 128 x 128
        extra = ["-b", "2", "--imagedim", "128", "--samples", "8", "--dtype", "fp16", "--face-parsing", "random", "--g-every", "2"]
    else:
        extra = ["-b", "4", "--imagedim", "64", "--samples", "8", "--dtype", "fp32"]
    train.main(["-exp", exp, "-ep", "1", "--saveevery", "10", "--evalevery", "1", "--outdir", str(tmp_path), "--masks", kind] + extra)
    with open(tmp_path / "model" / exp / "training_epoch_history.obj", "rb") as h:
        hist = pickle.load(h)
    assert len(hist) == 2 and all(np.isfinite(v) for rec in hist for v in rec["losses"].values())
    with open(tmp_path / "model" / exp / "eval_history.obj", "rb") as h:
        ev = pickle.load(h)
    assert set(ev[-1]) == {"train", "test"} and all(np.isfinite(part["recon_l1_local"]) for part in ev[-1].values())
