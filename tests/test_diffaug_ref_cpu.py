"""CPU tier: the numpy restatement of the differentiable augmentation (tests/diffaug_ref.py) checked on its own -
its adjoint against torch autograd of its forward in fp64, the adjoint identity, the ranges and the coverage of the draws, the
independence of the operations' draws and of the keys - before the GPU tier relies on it."""
import itertools

import numpy as np
import pytest
import torch

import diffaug_ref as R

SIZES = [(5, 7), (16, 16), (9, 4)]


def hand_params(H, W):
    """Shifts of both signs and windows clipped at each of the four borders (plus an interior and an empty one)."""
    ch, cw = H // 2, W // 2
    out = []
    shifts = [(0, 0), (1, -1), (-1, 2), (max(1, H // 8), max(1, W // 8)), (-max(1, H // 8), -max(1, W // 8)), (H, 0), (0, -W)]
    windows = [(0, 0, 0, 0), (-ch // 2, 1, ch, cw), (H - ch // 2, 1, ch, cw), (1, -cw // 2, ch, cw), (1, W - cw // 2, ch, cw),
               (1, 1, ch, cw), (0, 0, H, W)]
    for k, ((ty, tx), (y0, x0, h, w)) in enumerate(itertools.product(shifts, windows)):
        out.append((0.25 - 0.125 * (k % 5), 0.5 + 0.125 * (k % 8), ty, tx, y0, x0, h, w))
    return out


def torch_fwd(x, p, colour):
    """The definition written with torch ops (differentiable): colour, then shift with zero fill, then the window."""
    b, c, ty, tx = p[:4]
    H, W = x.shape
    v = c * (x - x.mean()) + (x.mean() + b) if colour else x
    keep = torch.from_numpy(R.keep_mask(p, H, W))
    qy, qx = torch.nonzero(keep, as_tuple=True)
    y = torch.zeros_like(x)
    return y.index_put((qy, qx), v[qy - ty, qx - tx])


@pytest.mark.parametrize("H,W", SIZES)
@pytest.mark.parametrize("colour", [False, True])
def test_bwd_is_autograd_of_fwd(H, W, colour):
    rng = np.random.default_rng(H * 100 + W)
    worst = 0.0
    for p in hand_params(H, W):
        x, dy = rng.standard_normal((H, W)), rng.standard_normal((H, W))
        xt = torch.from_numpy(x).requires_grad_(True)
        yt = torch_fwd(xt, p, colour)
        assert np.abs(yt.detach().numpy() - R.fwd(x, p, colour)).max() <= 1e-14
        yt.backward(torch.from_numpy(dy))
        worst = max(worst, np.abs(xt.grad.numpy() - R.bwd(dy, p, colour)).max())
        # <T x, dy> = <x, T* dy>
        lhs, rhs = (R.fwd(x, p, colour) * dy).sum(), (x * R.bwd(dy, p, colour)).sum()
        if not colour:
            assert abs(lhs - rhs) <= 1e-12 * max(1.0, abs(lhs))
    print(f"{H}x{W} colour={colour}: worst |autograd - bwd| = {worst:.2e}")
    assert worst <= 1e-14


@pytest.mark.parametrize("H,W", SIZES)
def test_adjoint_identity_of_the_linear_part(H, W):
    """With colour on T is affine (the brightness is a constant): <T x - T 0, dy> = <x, T* dy>."""
    rng = np.random.default_rng(7)
    for p in hand_params(H, W):
        x, dy = rng.standard_normal((H, W)), rng.standard_normal((H, W))
        lhs = ((R.fwd(x, p, True) - R.fwd(np.zeros((H, W)), p, True)) * dy).sum()
        rhs = (x * R.bwd(dy, p, True)).sum()
        assert abs(lhs - rhs) <= 1e-12 * max(1.0, abs(lhs))


def test_draw_ranges_and_coverage():
    H = W = 64
    tys, txs, cys, cxs = set(), set(), set(), set()
    for key in range(4096):
        b, c, ty, tx, y0, x0, ch, cw = R.params(7, 0, key, H, W)
        assert -0.5 <= b < 0.5 and 0.5 <= c < 1.5
        assert np.float32(b) == b and np.float32(c) == c, "b and c are exactly representable in fp32"
        assert -8 <= ty <= 8 and -8 <= tx <= 8
        assert (ch, cw) == (32, 32)
        cy, cx = y0 + ch // 2, x0 + cw // 2
        assert 0 <= cy <= H and 0 <= cx <= W
        tys.add(ty), txs.add(tx), cys.add(cy), cxs.add(cx)
    assert tys == set(range(-8, 9)) and txs == set(range(-8, 9))
    assert {0, H} <= cys and {0, W} <= cxs


@pytest.mark.parametrize("H,W", [(1, 1), (5, 7), (17, 33), (64, 96)])
def test_ranges_at_other_sizes(H, W):
    for key in range(256):
        b, c, ty, tx, y0, x0, ch, cw = R.params(7, 3, key, H, W)
        assert abs(ty) <= H // 8 and abs(tx) <= W // 8
        assert (ch, cw) == (H // 2, W // 2)
        assert -(ch // 2) <= y0 <= H - ch // 2 and -(cw // 2) <= x0 <= W - cw // 2


def test_operations_do_not_disturb_each_other():
    full = R.params(7, 5, 1234, 64, 96)
    off = (0.0, 1.0, 0, 0, 0, 0, 0, 0)
    groups = {R.COLOUR: (0, 1), R.TRANSLATION: (2, 3), R.CUTOUT: (4, 5, 6, 7)}
    for bits in range(1, 8):
        p = R.params(bits, 5, 1234, 64, 96)
        for bit, idx in groups.items():
            for i in idx:
                assert p[i] == (full[i] if bits & bit else off[i]), (bits, i)


def test_policy_strings():
    assert R.policy_bits("color,translation,cutout") == 7
    assert R.policy_bits("cutout") == 4 and R.policy_bits("translation, color") == 3


def test_keys_give_distinct_streams():
    n = 8
    keys = {}
    for step, call, rank, i in itertools.product(range(6), range(3), range(3), range(n)):
        keys[(step, call, rank, i)] = R.key_of(step, call, rank, n, i)
    assert len(set(keys.values())) == len(keys)
    assert max(keys.values()) >= 1 << 32
    streams = {R.stream_of(R.SALT, k) for k in keys.values()}
    assert len(streams) == len(keys)
    tables = {R.params(7, 0, k, 64, 64) for k in keys.values()}
    assert len(tables) == len(keys)
    # the salt: the same (seed, key) does not replay the mask generator's stream
    assert R.stream_of(0 ^ R.SALT, 5) != R.stream_of(0, 5)


def test_fp32_restatement_is_within_its_bounds():
    """fwd32 / bwd32 given the fp32-rounded exact mean stay within fwd_bound / bwd_bound of the fp64 pair."""
    rng = np.random.default_rng(3)
    for H, W in [(5, 7), (17, 33), (64, 64)]:
        for key in range(8):
            p = R.params(7, 1, key, H, W)
            x = rng.standard_normal((H, W)).astype(np.float32)
            dy = rng.standard_normal((H, W)).astype(np.float32)
            y32 = R.fwd32(x, p, np.float32(x.astype(np.float64).mean()))
            assert y32.dtype == np.float32
            assert (np.abs(y32 - R.fwd(x, p, True)) <= R.fwd_bound(x, p)).all()
            dv = R.move_adjoint(dy.astype(np.float64), p)
            dx32 = R.bwd32(dy, p, np.float32(dv.mean()))
            assert (np.abs(dx32 - R.bwd(dy, p, True)) <= R.bwd_bound(dy, p)).all()
