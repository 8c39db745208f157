"""GPU tier: the kernels of the LPIPS backward (csrc/lpips.hip) one at a time through their gi_debug_lpips_* entries, against
tests/lpips_grad_ref.py: the seed within its per-element bound, the per-image scales, the activation backward bit for bit, the first-layer
adjoint exactly on exact data and within its bound on random data, the transposed pack bit for bit."""
import numpy as np
import pytest
import torch

import lpips_grad_ref as G

pytestmark = pytest.mark.gpu


def _B():
    import gan_inpainting_amd  # noqa: F401
    from gan_inpainting_amd import backend as B
    return B


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).cuda()


def _nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous().cuda()


def _nchw(t):
    return t.cpu().permute(0, 3, 1, 2).contiguous()


def _seed(fa, fb, lin):
    """fa, fb (n,C,h,w) float16 tensors -> (smax (n,) float32 bit patterns as floats, sc (2n,), stored (n,C,h,w) float16 = sc[i] * seed)."""
    B = _B()
    n, C, H, W = fa.shape
    Fd = _nhwc(torch.cat([fa, fb]))
    smax = torch.zeros(n, dtype=torch.int32, device="cuda")
    sc = torch.empty(2 * n, dtype=torch.float32, device="cuda")
    dlin = _dev(lin)
    lib, ctx = B.lib(), B.get_ctx()
    B.check(lib.gi_debug_lpips_seed(ctx, 0, B.ptr(Fd), n, H * W, C, B.ptr(dlin), B.ptr(smax), None))
    B.check(lib.gi_debug_lpips_scale(ctx, B.ptr(smax), B.ptr(sc), n))
    B.check(lib.gi_debug_lpips_seed(ctx, 1, B.ptr(Fd), n, H * W, C, B.ptr(dlin), None, B.ptr(sc)))
    torch.cuda.synchronize()
    assert torch.equal(_nchw(Fd[:n]), fa), "the a half must be left alone"
    return smax.cpu().view(torch.float32), sc.cpu(), _nchw(Fd[n:])


def _maps(seed, n, C, h, w):
    rng = np.random.Generator(np.random.PCG64(seed))
    fa = np.maximum(rng.standard_normal((n, C, h, w)) + 0.3, 0.0) * (rng.random((n, C, h, w)) > 0.3)
    fb = np.maximum(fa + 0.5 * rng.standard_normal((n, C, h, w)), 0.0)
    lin = (rng.random(C) * 2.0 / C).astype(np.float32)
    return torch.from_numpy(fa.astype(np.float16)), torch.from_numpy(fb.astype(np.float16)), lin


# 70 x 70 = 4900 pixels at C = 64 (32 pixels per workgroup): 154 workgroups' worth, past the cap of 128, so the grid-stride loop runs twice
SEED_CASES = [(C, shape) for C in (64, 128, 256, 512) for shape in ((1, 1), (3, 5), (16, 16))] + [(64, (70, 70))]


@pytest.mark.parametrize("C,shape", SEED_CASES)
def test_seed_within_its_bound(C, shape):
    h, w = shape
    n = 2
    fa, fb, lin = _maps(300 + C + h, n, C, h, w)
    if h > 1:
        fa[0, :, 0, 1] = 0          # a zero a vector: a zero seed
        fb[1, :, 0, 2] = 0          # a zero b vector: finite
    smax, sc, stored = _seed(fa, fb, lin)
    ref = G.seed_closed(fa, fb, lin)
    s = sc[:n].double()
    assert torch.equal(sc[n:], 1.0 / sc[:n])
    bound = G.stored_seed_bound(fa, fb, lin, s)
    err = (stored.double() - s.reshape(-1, 1, 1, 1) * ref).abs()
    print(f"lpips seed C={C} {h}x{w}: max err / bound {float((err / bound).max()):.3f}, scales {sc[:n].tolist()}")
    assert torch.isfinite(stored).all()
    assert bool((err <= bound).all())
    if h > 1:
        assert float(stored[0, :, 0, 1].abs().max()) == 0.0
    # each image's largest scaled seed sits in [2^-3, 2^-2), and the maximum is the fp32 seed's within the bound
    for i in range(n):
        m = float(smax[i])
        assert abs(m - float(ref[i].abs().max())) <= float(G.seed_bound(fa, fb, lin)[i].max())
        assert float(sc[i]) == G.pow2_scale(m)
        assert 2.0 ** -3 <= m * float(sc[i]) < 2.0 ** -2


def test_seed_identical_maps_and_per_image_exponents():
    C = 128
    fa, fb, lin = _maps(41, 3, C, 6, 6)
    fb[0] = fa[0]                                                   # identical: all zero, word 0, scale 1
    fb[1] = torch.from_numpy(G.R.near_identical(fa[1].numpy(), 5))  # a few elements one fp16 step apart: a tiny distance
    smax, sc, stored = _seed(fa, fb, lin)
    assert int(smax.view(torch.int32)[0]) == 0 and float(sc[0]) == 1.0 and float(sc[3]) == 1.0
    assert float(stored[0].abs().max()) == 0.0
    m1, m2 = float(smax[1]), float(smax[2])
    assert 0 < m1 < m2 / 16, (m1, m2)
    assert float(sc[1]) > float(sc[2])
    for i in (1, 2):
        assert 2.0 ** -3 <= float(smax[i]) * float(sc[i]) < 2.0 ** -2
        top = float(stored[i].abs().max())          # its fp16 rounding may reach the upper end
        assert 2.0 ** -3 <= top <= 2.0 ** -2, (i, top)
    # an image has the same bits alone and inside the batch of three
    for i in range(3):
        sm1, sc1, st1 = _seed(fa[i:i + 1], fb[i:i + 1], lin)
        assert torch.equal(sm1.view(torch.int32), smax.view(torch.int32)[i:i + 1]) and float(sc1[0]) == float(sc[i])
        assert torch.equal(st1.view(torch.int16), stored[i:i + 1].view(torch.int16))


def _act_bwd(g, act, seed, pool, relu=1):
    B = _B()
    n, C, H, W = act.shape
    dg, da, ds = (None if t is None else _nhwc(t) for t in (g, act, seed))
    out = torch.full((n, H, W, C), float("nan"), dtype=torch.float16, device="cuda")
    B.check(B.lib().gi_debug_lpips_act_bwd(B.get_ctx(), int(pool), B.ptr(dg), B.ptr(da), B.ptr(ds), B.ptr(out), n, H, W, C, relu))
    return _nchw(out)


@pytest.mark.parametrize("relu", [1, 0])
@pytest.mark.parametrize("pool", [False, True])
@pytest.mark.parametrize("shape", [(6, 10), (16, 16)])
@pytest.mark.parametrize("C", [64, 512])
def test_act_bwd_bit_for_bit(C, shape, pool, relu):
    h, w = shape
    rng = np.random.Generator(np.random.PCG64(500 + C + h))
    # coarse values: ties inside the 2x2 windows (several maxima, all-zero windows) are common
    act = torch.from_numpy((np.maximum(rng.integers(-2, 4, (2, C, h, w)), 0) / 2.0).astype(np.float16))
    gs = (h // 2, w // 2) if pool else (h, w)
    g = torch.from_numpy((rng.standard_normal((2, C) + gs) * 0.05).astype(np.float16))
    seed = torch.from_numpy((rng.standard_normal((2, C, h, w)) * 0.05).astype(np.float16))
    ties = 0
    if pool:
        win = act.float().reshape(2, C, h // 2, 2, w // 2, 2).permute(0, 1, 2, 4, 3, 5).reshape(2, C, h // 2, w // 2, 4)
        ties = int(((win == win.max(-1, keepdim=True).values).sum(-1) > 1).sum())
        assert ties > 100
    for sd in (seed, None):
        got = _act_bwd(g, act, sd, pool, relu)
        ref = G.act_bwd_emulate(g, act, sd, pool, bool(relu))
        assert torch.equal(got.view(torch.int16), ref.view(torch.int16))
    if not pool:    # the top of the chain: no gradient from above
        assert torch.equal(_act_bwd(None, act, seed, False, relu).view(torch.int16), G.act_bwd_emulate(None, act, seed, False, bool(relu)).view(torch.int16))


def test_act_bwd_pool_tie_goes_to_the_first_position():
    C = 64
    act = torch.zeros(1, C, 2, 4, dtype=torch.float16)
    act[0, :, :, 0:2] = 1.0                     # window 0: four equal maxima -> (0, 0)
    act[0, :, 1, 2:4] = 2.0                     # window 1: the two bottom positions tie -> (1, 0) of the window
    g = torch.full((1, C, 1, 2), 0.5, dtype=torch.float16)
    out = _act_bwd(g, act, None, True)
    want = torch.zeros(2, 4)
    want[0, 0] = 0.5
    want[1, 2] = 0.5
    assert torch.equal(out[0, 0].float(), want) and torch.equal(out[0, C - 1].float(), want)


def _adjoint(D, wA, sc_inv, gscale):
    B = _B()
    n, _, H, W = D.shape
    dD, dw, dsc = _nhwc(D), _dev(wA), _dev(sc_inv)
    out = torch.full((n, 1, H, W), float("nan"), dtype=torch.float32, device="cuda")
    B.check(B.lib().gi_debug_lpips_conv1_adjoint(B.get_ctx(), B.ptr(dD), B.ptr(dw), B.ptr(dsc), float(gscale), B.ptr(out), n, H, W))
    return out.cpu().double()


@pytest.mark.parametrize("shape", [(16, 16), (16, 48), (32, 32)])
def test_adjoint_exact_and_within_its_bound(shape):
    rng = np.random.Generator(np.random.PCG64(700 + shape[1]))
    n = 3
    sc_inv = np.array([1.0, 2.0 ** -7, 2.0 ** 5], np.float32)          # per image 1 / s_i
    # small-integer D, dyadic wA: every product and sum is exact in fp32
    D = torch.from_numpy(rng.integers(-3, 4, (n, 64) + shape).astype(np.float16))
    wA = (rng.integers(-8, 9, (64, 9)) / 8.0).astype(np.float32)
    got = _adjoint(D, wA, sc_inv, 4.0)
    ref = G.conv1_adjoint(wA, D, 4.0 * sc_inv.astype(np.float64))
    assert torch.equal(got, ref) and float(ref.abs().max()) > 1.0
    # random data, a gscale that is no power of two
    D = torch.from_numpy((rng.standard_normal((n, 64) + shape) * 0.1).astype(np.float16))
    wA = rng.standard_normal((64, 9)).astype(np.float32)
    got = _adjoint(D, wA, sc_inv, 3.0)
    mul = 3.0 * sc_inv.astype(np.float64)
    ref, bound = G.conv1_adjoint(wA, D, mul), G.adjoint_bound(wA, D, mul)
    err = (got - ref).abs()
    print(f"lpips conv1 adjoint {shape}: max err / bound {float((err / bound).max()):.3f}")
    assert bool((err <= bound).all())
    # the factor of image i alone: the same D in every slot gives outputs in the ratio of the factors, exactly (powers of two)
    D1 = D[:1].repeat(n, 1, 1, 1)
    g1 = _adjoint(D1, wA, sc_inv, 1.0)
    assert torch.equal(g1[1], g1[0] * 2.0 ** -7) and torch.equal(g1[2], g1[0] * 2.0 ** 5)


@pytest.mark.parametrize("cout,cin", [(64, 64), (128, 64), (512, 256)])
def test_transposed_pack_bit_for_bit(cout, cin):
    B = _B()
    w = np.random.Generator(np.random.PCG64(cout + cin)).standard_normal((cout, cin, 3, 3)).astype(np.float32)
    out = torch.empty(cin, 9, cout, dtype=torch.float16, device="cuda")
    dw = _dev(w)
    B.check(B.lib().gi_debug_lpips_pack_t(B.get_ctx(), B.ptr(dw), B.ptr(out), cout, cin))
    assert np.array_equal(out.cpu().numpy().view(np.int16), G.pack_t(w).view(np.int16))
