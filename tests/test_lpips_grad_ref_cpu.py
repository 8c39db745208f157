"""CPU tier: the differentiable restatement of LPIPS (tests/lpips_grad_ref.py) that the backward of csrc/lpips.hip is tested against, checked
against lpips_ref.py, torch autograd and finite differences; the per-element bounds checked against fp32 emulations of the kernels."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import lpips_grad_ref as G
import lpips_ref as R


def _maps(seed, n, C, h, w, zero_frac=0.3):
    """Two post-ReLU-like fp16 maps (n,C,h,w): non-negative with zeros, as float64 tensors."""
    rng = np.random.Generator(np.random.PCG64(seed))
    fa = np.maximum(rng.standard_normal((n, C, h, w)) + 0.3, 0.0) * (rng.random((n, C, h, w)) > zero_frac)
    fb = np.maximum(fa + 0.5 * rng.standard_normal((n, C, h, w)), 0.0)
    lin = (rng.random(C) * 2.0 / C).astype(np.float32)
    return torch.from_numpy(fa.astype(np.float16)).double(), torch.from_numpy(fb.astype(np.float16)).double(), lin


def test_values_equal_lpips_ref():
    P = R.make_params(3)
    a, b = R.make_images(4, 2, 32, 32), R.make_images(5, 2, 32, 32)
    for fp16 in (False, True):
        d, per = G.distance(P, G._t(a), G._t(b), fp16)
        d0, per0 = R.distance(P, a, b, fp16)
        assert float(((d - d0).abs() / d0).max()) <= 1e-14
        assert float(((per - per0).abs() / per0).max()) <= 1e-14


@pytest.mark.parametrize("C", [64, 128, 256, 512])
def test_closed_form_seed_equals_autograd(C):
    fa, fb, lin = _maps(10 + C, 2, C, 3, 5)
    x = fa.clone().requires_grad_(True)
    g, = torch.autograd.grad(G.tap_distance(x, fb, lin).sum(), x)
    s = G.seed_closed(fa, fb, lin)
    assert float((s - g).abs().max()) <= 1e-13 * float(g.abs().max())
    # no zero vector in these maps: the unguarded form agrees too
    x = fa.clone().requires_grad_(True)
    g0, = torch.autograd.grad(G.tap_distance(x, fb, lin, guarded=False).sum(), x)
    assert torch.isfinite(g0).all() and float((s - g0).abs().max()) <= 1e-13 * float(g.abs().max())


def test_zero_vector_guard():
    """A pixel whose pre-activations are all <= 0: unguarded autograd of the distance w.r.t. the post-ReLU map is NaN there, the guarded
    seed is 0, and the gradient w.r.t. the pre-activations - what the chain carries on - is the same and finite: the ReLU mask removes
    every channel of that pixel whatever the seed."""
    rng = np.random.Generator(np.random.PCG64(2))
    z = torch.from_numpy(rng.standard_normal((1, 64, 4, 4)))
    z[0, :, 1, 2] = -z[0, :, 1, 2].abs()
    z[0, :, 3, 0] = 0.0
    fb = torch.from_numpy(np.maximum(rng.standard_normal((1, 64, 4, 4)), 0.0))
    lin = (rng.random(64) / 32).astype(np.float32)
    res = {}
    for guarded in (False, True):
        zz = z.clone().requires_grad_(True)
        a = F.relu(zz)
        a.retain_grad()
        G.tap_distance(a, fb, lin, guarded).sum().backward()
        res[guarded] = (a.grad.clone(), zz.grad.clone())
    assert torch.isnan(res[False][0][0, :, 1, 2]).all() and torch.isnan(res[False][0][0, :, 3, 0]).all()
    assert torch.equal(res[True][0][0, :, 1, 2], torch.zeros(64, dtype=torch.float64))
    assert torch.equal(G.seed_closed(F.relu(z), fb, lin)[0, :, 3, 0], torch.zeros(64, dtype=torch.float64))
    live = torch.ones(4, 4, dtype=torch.bool)
    live[1, 2] = live[3, 0] = False
    # elsewhere the two agree on the post-ReLU gradient, and everywhere on the pre-activation gradient once the mask is applied
    assert torch.equal(res[True][0][0][:, live], res[False][0][0][:, live])
    masked = torch.where(z > 0, torch.nan_to_num(res[False][0], nan=123.0), torch.zeros_like(z))
    assert torch.isfinite(res[True][1]).all() and torch.equal(res[True][1], masked)
    assert float(res[True][1][0, :, 1, 2].abs().max()) == 0.0


def test_directional_derivative_16x16():
    P = R.make_params(6)
    a, b = R.make_images(7, 1, 16, 16).astype(np.float64), R.make_images(8, 1, 16, 16).astype(np.float64)
    _, g = G.grad(P, a, b)
    rng = np.random.Generator(np.random.PCG64(9))
    worst = 0.0
    for _ in range(3):
        v = rng.standard_normal(a.shape)
        v /= np.linalg.norm(v)
        h = 1e-6
        with torch.no_grad():
            dp, _ = G.distance(P, G._t(a + h * v), G._t(b))
            dm, _ = G.distance(P, G._t(a - h * v), G._t(b))
        fd = float((dp - dm).sum()) / (2 * h)
        an = float((g * G._t(v)).sum())
        worst = max(worst, abs(fd - an) / abs(an))
    print(f"directional derivative: worst relative difference {worst:.2e}")
    assert worst <= 1e-5


def test_first_layer_adjoint_equals_autograd():
    P = R.make_params(11)
    w, bias = P["features.0.weight"], P["features.0.bias"]
    wA, _ = R.fold(w, P["scaling_layer.shift"], P["scaling_layer.scale"])
    x = G._t(R.make_images(12, 2, 16, 32)).requires_grad_(True)
    h = (2.0 * x.repeat(1, 3, 1, 1) - 1.0 - G._t(P["scaling_layer.shift"])) / G._t(P["scaling_layer.scale"])
    pre = F.conv2d(h, G._t(w), G._t(bias), padding=1)
    assert float((F.relu(pre).detach() - R.conv1_three_channel(w, bias, P["scaling_layer.shift"], P["scaling_layer.scale"], x.detach().numpy())).abs().max()) == 0.0
    Dm = torch.from_numpy(np.random.Generator(np.random.PCG64(13)).standard_normal(pre.shape))
    g, = torch.autograd.grad((pre * Dm).sum(), x)
    mul = torch.tensor([1.0, 0.25])
    got = G.conv1_adjoint(wA, Dm, mul)
    assert float((got - g * mul.double().reshape(-1, 1, 1, 1)).abs().max()) <= 1e-12 * float(g.abs().max())


def test_identical_inputs_give_exactly_zero():
    P = R.make_params(14)
    a = R.make_images(15, 2, 32, 32)
    for fp16 in (False, True):
        d, g = G.grad(P, a, a, fp16)
        assert torch.equal(d, torch.zeros_like(d)) and torch.equal(g, torch.zeros_like(g))


@pytest.mark.parametrize("seed,n,h,w", [(5, 2, 32, 32)])
def test_fp16_storage_emulation_is_the_yardstick(seed, n, h, w):
    """Its values are lpips_ref's yardstick (b); its gradient error against fp64 is what the device is measured with (printed)."""
    P = R.make_params(seed)
    a, b = R.make_images(seed + 1, n, h, w), R.make_images(seed + 2, n, h, w)
    d16, g16 = G.grad(P, a, b, fp16=True)
    d0, _ = R.distance(P, a, b, fp16=True)
    assert float(((d16 - d0).abs() / d0).max()) <= 1e-14
    d, g = G.grad(P, a, b)
    rel, cos = G.rel_l2(g16, g), G.cosine(g16, g)
    print(f"fp16-storage emulation, seed {seed} n {n} {h}x{w}: gradient rel L2 {rel:.3e}, cosine {cos:.6f}")
    assert torch.isfinite(g).all() and torch.isfinite(g16).all() and 0 < rel < 0.1


@pytest.mark.parametrize("C", [64, 128, 256, 512])
def test_seed_bound_holds_for_the_fp32_emulation(C):
    fa, fb, lin = _maps(20 + C, 2, C, 5, 7)
    fa[0, :, 0, 0] = 0.0            # a zero a vector: seed 0
    fb[0, :, 1, 1] = 0.0            # a zero b vector: finite
    fb[1] = fa[1]                   # an identical image: all zero
    ref, emu, bound = G.seed_closed(fa, fb, lin), G.seed_emulate(fa, fb, lin), G.seed_bound(fa, fb, lin)
    assert torch.isfinite(emu).all()
    assert float(emu[0, :, 0, 0].abs().max()) == 0.0 and float(emu[1].abs().max()) == 0.0
    err = (emu - ref).abs()
    print(f"C={C}: worst err / bound {float((err[bound > 0] / bound[bound > 0]).max()):.3f}")
    assert bool((err <= bound).all())
    # the bound is sharp enough to tell a wrong coefficient: 1 % off is far outside
    assert not bool(((1.01 * ref - ref).abs() <= bound).all())


def test_adjoint_bound_holds_for_the_fp32_emulation():
    rng = np.random.Generator(np.random.PCG64(31))
    wA = rng.standard_normal((64, 9)).astype(np.float32)
    D = torch.from_numpy((rng.standard_normal((2, 64, 16, 16)) * 0.1).astype(np.float16))
    mul = torch.tensor([4.0, 0.5 * 3.0])
    err = (G.conv1_adjoint_emulate(wA, D, mul) - G.conv1_adjoint(wA, D, mul)).abs()
    assert bool((err <= G.adjoint_bound(wA, D, mul)).all())


def test_act_bwd_emulation_ties_and_pack():
    act = torch.tensor([[1.0, 1.0], [1.0, 0.5]]).reshape(1, 1, 2, 2).repeat(1, 8, 1, 1).half()
    g = torch.full((1, 8, 1, 1), 2.0).half()
    seed = torch.full((1, 8, 2, 2), 0.25).half()
    out = G.act_bwd_emulate(g, act, seed, pool=True)
    assert out[0, 0].tolist() == [[2.25, 0.25], [0.25, 0.25]]          # the tie goes to the first window position
    act[0, :, 1, 1] = 0.0
    assert G.act_bwd_emulate(g, act, seed, pool=True)[0, 0, 1, 1] == 0.0
    w = np.arange(2 * 3 * 9, dtype=np.float32).reshape(2, 3, 3, 3)
    t = G.pack_t(w)
    assert t.shape == (3, 9, 2) and t[1, 0, 1] == w[1, 1, 2, 2] and t[2, 8, 0] == w[0, 2, 0, 0]
