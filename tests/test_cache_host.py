"""Host tier of the device dataset cache (lib/data/cache.py, train.py --cache / --flip): the flags, the pass order, the memory
budget, the row check and the flip bits of the restatement (tests/batchgather_ref.py). No GPU."""
import pytest
import torch

import batchgather_ref as R

SEED = 0x5EED
BASE = ["-exp", "wgan_l1"]


def _parser():
    import gan_inpainting_amd  # noqa: F401
    from gan_inpainting_amd import train
    return train.build_parser()


def test_parser_takes_the_cache_flags():
    a = _parser().parse_args(BASE)
    assert a.cache == "off" and a.flip is False and a.cache_budget_gb is None
    a = _parser().parse_args(BASE + ["--data", "/d", "--cache", "device", "--flip", "--cache-budget-gb", "1.5"])
    assert a.cache == "device" and a.flip is True and a.cache_budget_gb == 1.5
    a = _parser().parse_args(BASE + ["--data", "/d", "--cache", "device"])
    assert a.flip is False


@pytest.mark.parametrize("extra", [["--flip"], ["--data", "/d", "--flip"], ["--data", "/d", "--cache", "off", "--flip"],
                                   ["--cache", "device"], ["--data", "/d", "--cache", "host"],
                                   ["--data", "/d", "--cache", "device", "--cache-budget-gb", "0"]])
def test_parser_refuses(extra):
    with pytest.raises(SystemExit) as e:
        _parser().parse_args(BASE + extra)
    assert e.value.code == 2          # argparse's error exit


def test_epoch_order_is_a_pure_permutation():
    import gan_inpainting_amd  # noqa: F401
    from gan_inpainting_amd.lib.data.cache import epoch_order
    for n in (1, 2, 12, 1000):
        o = epoch_order(n, 7, 0)
        assert o.dtype == torch.int64 and sorted(o.tolist()) == list(range(n))
    a, b = epoch_order(1000, 7, 3), epoch_order(1000, 7, 3)
    assert torch.equal(a, b)
    torch.manual_seed(1)                                   # the order does not read the global generator
    assert torch.equal(epoch_order(1000, 7, 3), a)
    assert not torch.equal(epoch_order(1000, 7, 4), a)     # another pass
    assert not torch.equal(epoch_order(1000, 8, 3), a)     # another seed
    assert len({tuple(epoch_order(12, 7, p).tolist()) for p in range(6)}) == 6


def test_cache_bytes_and_the_budget():
    import gan_inpainting_amd  # noqa: F401
    from gan_inpainting_amd.lib.data import cache
    assert cache.cache_bytes(200000, 128, 128) == 200000 * 128 * 128          # the issue's 3.3 GB
    assert cache.cache_bytes(200000, 256, 256) == 13107200000                 # and 13 GB: past 2^32, no wrap
    assert cache.cache_bytes(12, 32, 32, masks=True) == 2 * 12 * 1024
    assert cache.cache_bytes(12, 32, 40, masks=True, segments=True) == 3 * 12 * 32 * 40
    cache.check_budget(1000, 1000)
    with pytest.raises(cache.CacheBudgetError) as e:
        cache.check_budget(13107200000, 4294967296)
    assert "13107200000" in str(e.value) and "4294967296" in str(e.value)     # both numbers


def test_rows_are_checked_on_the_host():
    import gan_inpainting_amd  # noqa: F401
    from gan_inpainting_amd.lib.data.cache import _check_rows
    assert _check_rows([0, 11, 3, 3], 12).tolist() == [0, 11, 3, 3]
    assert _check_rows(torch.tensor([11]), 12).dtype == torch.int64
    for bad in ([12], [-1], [0, 5, 12], [0, -3, 2]):
        with pytest.raises(IndexError):
            _check_rows(bad, 12)
    for bad in (torch.tensor([1], dtype=torch.int32), torch.zeros((2, 2), dtype=torch.int64), torch.zeros(0, dtype=torch.int64),
                torch.tensor([1.0])):
        with pytest.raises(ValueError):
            _check_rows(bad, 12)


def test_flip_bits_of_the_restatement():
    """Seed 0x5EED, split train, rows 0..63: 27, 32 and 34 flips in epochs 0, 1 and 2, computed from the formula of DESIGN 4.1e-3
    (stream = mix((seed ^ 0x666C6970) + G * (key + 1)), flip = mix(stream + G) >> 63) on the CPU."""
    import gan_inpainting_amd  # noqa: F401
    from gan_inpainting_amd.lib.data.masks import mask_key
    pats = []
    for epoch in range(3):
        keys = [R.key_of("train", epoch, r) for r in range(64)]
        assert keys == mask_key("train", epoch, torch.arange(64)).tolist()        # the product's keys
        bits = R.flip_bits(SEED, keys)
        # the formula, written out
        G = 0x9E3779B97F4A7C15
        assert bits == [R.mix(R.mix((SEED ^ 0x666C6970) + G * (k + 1)) + G) >> 63 for k in keys]
        pats.append(bits)
    assert [sum(p) for p in pats] == [27, 32, 34]
    assert pats[0] != pats[1] and pats[1] != pats[2] and pats[0] != pats[2]       # the rows that flip change with the epoch
    # the test split ignores the epoch; another seed gives another pattern
    assert R.flip_bits(SEED, [R.key_of("test", 0, r) for r in range(64)]) == R.flip_bits(SEED, [R.key_of("test", 5, r) for r in range(64)])
    assert R.flip_bits(SEED + 1, [R.key_of("train", 0, r) for r in range(64)]) != pats[0]


def test_restatement_gathers_and_flips():
    import numpy as np
    store = np.arange(2 * 2 * 3, dtype=np.uint8).reshape(2, 2, 3)
    keys = [R.key_of("train", 0, r) for r in range(64)]
    bits = R.flip_bits(SEED, keys)
    f, nf = bits.index(1), bits.index(0)
    out = R.gather(store, [1, 1, 0], 2, [keys[f], keys[nf], keys[f]], SEED)
    assert out.dtype == np.uint8 and out.tolist() == [[[8, 7, 6], [11, 10, 9]], [[6, 7, 8], [9, 10, 11]], [[2, 1, 0], [5, 4, 3]]]
    assert R.gather(store, [0], 1).dtype == np.int64 and R.gather(store, [0], 1).tolist() == [[[0, 1, 2], [3, 4, 5]]]
    q = R.gather(store, [1], 0)
    assert q.dtype == np.float32 and q[0, 1, 2] == np.float32(11) / np.float32(255)
