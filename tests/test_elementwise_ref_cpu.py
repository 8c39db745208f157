"""CPU tier: tests/elementwise_ref.py is honest. Its float64 values equal torch in float64 (the loss functions and autograd, the
optimizers of torch.optim over several steps, conv_transpose2d for the phase layout of the weight pack), so the GPU tier does not
merely compare the kernels with a copy of themselves; and its bounds are bounds: a float32 evaluation in numpy, fused or not, stays
inside them, and a deliberately wrong one leaves them."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import elementwise_ref as R

F64 = torch.float64


def _rng(seed):
    return np.random.default_rng(seed)


def _data(seed, n, frac_mask=True):
    r = _rng(seed)
    a = (r.standard_normal(n) * 10.0 ** r.integers(-3, 4, n)).astype(np.float32)
    b = (r.standard_normal(n) * 10.0 ** r.integers(-3, 4, n)).astype(np.float32)
    m = r.choice(np.array([0.0, 1.0, 0.3, 0.75, 1e-3], dtype=np.float32), n) if frac_mask else r.integers(0, 2, n).astype(np.float32)
    return a, b, m


# ---- losses against torch.nn.functional and autograd ------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 7, 1023])
@pytest.mark.parametrize("gscale", [1.0, -3.0])
def test_reconstruction_losses_equal_torch(n, gscale):
    a, b, _ = _data(n, n)
    for kind, fn in (("l1", F.l1_loss), ("mse", F.mse_loss), ("rmse", lambda x, y: torch.sqrt(F.mse_loss(x, y) + R.RMSE_EPS))):
        ta = torch.from_numpy(a).to(F64).requires_grad_(True)
        v = fn(ta, torch.from_numpy(b).to(F64))
        (v * gscale).backward()
        r = R.loss(kind, a, b, None, R.RMSE_EPS, gscale)
        assert abs(float(v.detach()) - r["value"]) <= 1e-13 * abs(float(v.detach())), kind
        assert np.allclose(r["grad"], ta.grad.numpy(), rtol=1e-12, atol=0), kind
        assert r["den"] == n


def _local_loss_torch(yhat, y, mask, base):
    """lib/models/loss.py:24-47 as coded: sum(base(y * m, yhat * m)) / count(m != 0); 'rmse' the sqrt of the masked mean square + eps"""
    d = y * mask - yhat * mask
    cnt = (mask != 0).to(d.dtype).sum()
    if base == "l1":
        return torch.abs(d).sum() / cnt
    if base == "mse":
        return (d * d).sum() / cnt
    return torch.sqrt((d * d).sum() / cnt + 1e-16)


@pytest.mark.parametrize("n", [5, 1023])
@pytest.mark.parametrize("gscale", [1.0, 0.5])
def test_masked_losses_equal_the_reference_formula(n, gscale):
    a, b, m = _data(n + 1, n)
    m[0] = 0.75
    for kind in ("l1", "mse", "rmse"):
        ta = torch.from_numpy(a).to(F64).requires_grad_(True)
        v = _local_loss_torch(ta, torch.from_numpy(b).to(F64), torch.from_numpy(m).to(F64), kind)
        (v * gscale).backward()
        r = R.loss(kind, a, b, m, 1e-16, gscale)
        assert abs(float(v.detach()) - r["value"]) <= 1e-13 * abs(float(v.detach())), kind
        assert np.allclose(r["grad"], ta.grad.numpy(), rtol=1e-12, atol=0), kind
        assert r["den"] == np.count_nonzero(m)


def test_equal_inputs_give_sqrt_eps_and_no_gradient():
    a, _, m = _data(3, 257)
    for mask in (None, m):
        r = R.loss("rmse", a, a, mask, 1e-16)
        assert r["value"] == np.sqrt(np.float64(np.float32(1e-16))) and not r["grad"].any()


@pytest.mark.parametrize("n", [1, 65, 1000])
@pytest.mark.parametrize("target", [0.0, 1.0])
def test_adversarial_losses_equal_torch(n, target):
    r = _rng(n)
    p = r.uniform(0.01, 0.99, n).astype(np.float32)
    sat = np.array([0.0, 1.0, 2.0 ** -149, 1.0 - 2.0 ** -24, 2.0 ** -30], dtype=np.float32)
    for pred in (p, sat):
        k = pred.size
        tp = torch.from_numpy(pred).to(F64).requires_grad_(True)
        tt = torch.full((k,), target, dtype=F64)
        for kind, fn in ((0, lambda x: F.binary_cross_entropy(x, tt)), (1, lambda x: F.mse_loss(x, tt)), (2, lambda x: x.mean())):
            tp.grad = None
            v = fn(tp)
            (v * -3.0).backward()
            val, g = R.adv_loss(kind, pred, target, -3.0)
            assert abs(float(v.detach()) - val) <= 1e-13 * max(abs(float(v.detach())), 1e-300), (kind, float(v.detach()), val)
            assert np.allclose(g, tp.grad.numpy(), rtol=1e-12, atol=0), kind


# ---- optimizers against torch.optim on double parameters ----------------------------------------------------------------------------
def _opt_data(n):
    r = _rng(11)
    w0 = (r.standard_normal(n) * 0.05).astype(np.float32)
    gs = [(r.standard_normal(n) * 10.0 ** r.integers(-5, 2, n)).astype(np.float32) for _ in range(5)]
    for g in gs:
        g[::7] = 0.0
    return w0, gs


def _close(what, got, ref, rel, floor=0.0):
    """per element |got - ref| <= rel * |ref| + floor"""
    err = np.abs(got - ref)
    bad = np.flatnonzero(err > rel * np.abs(ref) + floor)
    assert bad.size == 0, f"{what}: element {bad[0]}: {got[bad[0]]!r} against torch's {ref[bad[0]]!r}"


# The kernel's constants are fp32 roundings of torch's doubles (beta, 1 - beta, lr / bias_correction1, sqrt(bias_correction2), eps:
# 6e-8 relative each). A moment is a sum of positive multiples of them (v, sq) or of a few of them (m), so after t steps it is within
# about t * 2e-7 of torch's, relative to the sum of its terms' magnitudes; 2e-6 leaves room for five steps and for m's cancellation
# down to a tenth of its terms, with a floor for deeper cancellation. One move is within 1e-6 of itself, so p after t moves is within
# t * 1e-6 * lr * |move / lr|, and |move / lr| is at most a few.
def test_adam_step_equals_torch_optim_over_five_steps():
    n = 300
    w0, gs = _opt_data(n)
    q = torch.nn.Parameter(torch.from_numpy(w0).to(F64))
    opt = torch.optim.Adam([q], lr=0.0002, betas=(0.5, 0.999), eps=1e-8)
    p, m, v = w0.astype(np.float64), np.zeros(n), np.zeros(n)
    for t, g in enumerate(gs, 1):
        q.grad = torch.from_numpy(g).to(F64)
        opt.step()
        r = R.adam_step(p, g, m, v, 0.0002, 0.5, 0.999, 1e-8, t)          # float64 state in, float64 state out: the function the GPU tier uses
        p, m, v = r["p"], r["m"], r["v"]
        assert p.dtype == np.float64 and (t == 1 or (np.abs(m) > 0).sum() > n // 2)
        st = opt.state[q]
        _close(f"adam step {t} m", m, st["exp_avg"].numpy(), 2e-6, 2e-6 * float(np.abs(g).max()))
        _close(f"adam step {t} v", v, st["exp_avg_sq"].numpy(), 2e-6)
        _close(f"adam step {t} p", p, q.detach().numpy(), 0.0, 1e-5 * 0.0002 * t)
    assert float(np.abs(p - w0).max()) > 3 * 0.0002, "the parameters hardly moved: the comparison of p would prove nothing"
    c = R.adam_constants(0.0002, 0.5, 0.999, 1)
    assert abs(c["omb1"] - 0.5) == 0 and abs(c["omb2"] - 0.001) < 1e-10 and abs(c["step_size"] - 0.0004) < 1e-10
    # float32 state is read as float32, and a gradient of 0 on zero moments moves nothing
    r = R.adam_step(w0, gs[0], np.zeros(n, np.float32), np.zeros(n, np.float32), 0.0002, 0.5, 0.999, 1e-8, 1)
    assert not r["move"][::7].any() and np.array_equal(r["p"][::7], w0[::7].astype(np.float64))
    assert not r["m"][::7].any() and not r["v"][::7].any()


def test_adam_step_below_one_counts_as_one():
    assert R.adam_constants(0.0002, 0.5, 0.999, -2) == R.adam_constants(0.0002, 0.5, 0.999, 1)
    assert R.adam_constants(0.0002, 0.5, 0.999, 2) != R.adam_constants(0.0002, 0.5, 0.999, 1)


@pytest.mark.parametrize("clampv", [0.0, 0.01])
def test_rmsprop_step_equals_torch_optim_over_five_steps(clampv):
    n = 300
    w0, gs = _opt_data(n)
    if clampv > 0:
        w0 = (w0 * 0.1).astype(np.float32)        # most parameters inside the clamp, so that their moves are compared
    q = torch.nn.Parameter(torch.from_numpy(w0).to(F64))
    opt = torch.optim.RMSprop([q], lr=0.00005, alpha=0.99, eps=1e-8)
    p, sq = w0.astype(np.float64), np.zeros(n)
    for t, g in enumerate(gs, 1):
        q.grad = torch.from_numpy(g).to(F64)
        opt.step()
        if clampv > 0:
            q.data.clamp_(-clampv, clampv)
        r = R.rmsprop_step(p, g, sq, 0.00005, 0.99, 1e-8, clampv)
        p, sq = r["p"], r["sq"]
        assert t == 1 or (sq > 0).sum() > n // 2
        _close(f"rmsprop step {t} sq", sq, opt.state[q]["square_avg"].numpy(), 2e-6)
        _close(f"rmsprop step {t} p", p, q.detach().numpy(), 0.0, 1e-5 * 0.00005 * t + 1e-7 * clampv)     # the clamp is a float: 6e-8 relative
        if clampv > 0:
            assert float(np.abs(p).max()) <= np.float32(clampv)
    inside = np.abs(p) < 0.99 * clampv if clampv > 0 else np.ones(n, bool)
    assert inside.sum() > n // 2 and float(np.abs(p - w0)[inside].max()) > 3 * 0.00005
    r = R.rmsprop_step(w0, gs[0], np.zeros(n, np.float32), 0.00005, 0.99, 1e-8, clampv)
    assert not r["move"][::7].any() and not r["sq"][::7].any()


# ---- the phase layout of the weight pack against conv_transpose2d ---------------------------------------------------------------------
@pytest.mark.parametrize("ca,cb", [(3, 5), (1, 4), (8, 2)])
def test_phase_copy_builds_the_transposed_convolution(ca, cb):
    """out[n, b, 2Y + py, 2X + px] = sum_{ty, tx, a} x[n, a, Y + py - ty, X + px - tx] * phase[ph][b][t][a]: the four 2 x 2
    sub-convolutions of the [ph][b][t][a] copy give F.conv_transpose2d(x, w, stride=2, padding=1)"""
    r = _rng(ca * 10 + cb)
    n, H, W = 2, 5, 4
    w = r.standard_normal((ca, cb, 4, 4)).astype(np.float32)
    x = torch.from_numpy(r.standard_normal((n, ca, H, W))).to(F64)
    ref = F.conv_transpose2d(x, torch.from_numpy(w).to(F64), stride=2, padding=1)
    master = np.ascontiguousarray(w.transpose(0, 2, 3, 1)).reshape(ca, 16, cb)         # [a][ky][kx][b]
    packed, phase = R.pack(master, ca, cb, half=False)
    assert R.same_bits(packed, master)
    xp = F.pad(x, (1, 1, 1, 1))                                                         # one zero pixel all round
    out = torch.zeros(n, cb, 2 * H, 2 * W, dtype=F64)
    ph64 = torch.from_numpy(phase.astype(np.float64))
    for ph in range(4):
        py, px = ph >> 1, ph & 1
        for t in range(4):
            ty, tx = t >> 1, t & 1
            sl = xp[:, :, 1 + py - ty:1 + py - ty + H, 1 + px - tx:1 + px - tx + W]      # x[n, a, Y + py - ty, X + px - tx]
            out[:, :, py::2, px::2] += torch.einsum("nayx,ba->nbyx", sl, ph64[ph, :, t, :])
    assert torch.allclose(out, ref, rtol=1e-12, atol=1e-12)


def test_pack_scale_and_half():
    r = _rng(4)
    ca, cb = 3, 5
    w = r.standard_normal((ca, 16, cb)).astype(np.float32)
    sa, sb = r.uniform(0.5, 2, ca).astype(np.float32), r.uniform(0.5, 2, cb).astype(np.float32)
    pa, pha = R.pack(w, ca, cb, True, sa, False)
    pb, _ = R.pack(w, ca, cb, True, sb, True)
    assert pa.dtype == np.float16 and R.same_bits(pa, (w * sa[:, None, None]).astype(np.float32).astype(np.float16))
    assert R.same_bits(pb, (w * sb[None, None, :]).astype(np.float32).astype(np.float16))
    ky, kx = R.phase_taps(2, 1)                                                         # py 1, px 0, ty 0, tx 1
    assert (ky, kx) == (0, 3) and R.same_bits(pha[2, :, 1, :], np.ascontiguousarray(pa[:, ky * 4 + kx, :].T))


# ---- the bounds are bounds, and not loose enough to hide a wrong op --------------------------------------------------------------------
def test_float32_evaluations_stay_inside_the_bounds():
    a, b, m = _data(9, 4099)
    f32 = np.float32
    for alpha in (1.0, -1.0, 0.25, 1e-3):
        E, bd = R.add(a, b, alpha)
        unfused = (a + (f32(alpha) * b).astype(f32)).astype(f32)
        fused = (a.astype(np.float64) + np.float64(f32(alpha)) * b.astype(np.float64)).astype(f32)
        assert R.worst_ratio(unfused, E, bd) <= 1.0 and R.worst_ratio(fused, E, bd) <= 1.0
        assert R.worst_ratio((a - (f32(alpha) * b)).astype(f32), E, bd) > 1.0
    eps = np.array([0.0, 1.0, 0.37], dtype=f32)
    real, fake = a[:3 * 1000].reshape(3, 1000), b[:3 * 1000].reshape(3, 1000)
    E, bd = R.interpolate(real, fake, eps)
    e = eps[:, None]
    out = ((e * real).astype(f32) + ((f32(1) - e).astype(f32) * fake).astype(f32)).astype(f32)
    assert R.worst_ratio(out, E, bd) <= 1.0
    assert R.same_bits(out[0], fake[0]) and R.same_bits(out[1], real[1])
    assert R.worst_ratio(np.roll(out, 1, axis=1), E, bd) > 1.0
    # the masked loss in float32, unfused, as torch evaluates it in fp32
    for kind in ("l1", "mse", "rmse"):
        r = R.loss(kind, a, b, m, 1e-16, 0.5)
        ta = torch.from_numpy(a).requires_grad_(True)
        v = _local_loss_torch(ta, torch.from_numpy(b), torch.from_numpy(m), kind)
        (v * 0.5).backward()
        assert R.worst_ratio(ta.grad.numpy(), r["grad"], r["grad_bound"]) <= 1.0, kind
    # Adam with beta2 in the place of beta1 leaves the moment's bound
    mom = (np.abs(a) * 0.1).astype(f32)
    r = R.adam_step(a, b, mom, np.abs(mom), 0.0002, 0.5, 0.999, 1e-8, 3)
    good = (f32(0.5) * mom + f32(0.5) * b).astype(f32)
    wrong = (f32(0.999) * mom + f32(0.5) * b).astype(f32)
    assert R.worst_ratio(good, r["m"], r["m_bound"]) <= 1.0 < R.worst_ratio(wrong, r["m"], r["m_bound"])


def test_composite_inputs_tell_fused_from_unfused():
    r = _rng(1)
    n = 4099
    masked, gen = r.standard_normal(n).astype(np.float32), r.standard_normal(n).astype(np.float32)
    mc = r.uniform(0.05, 0.95, n).astype(np.float32)
    two, one = R.mask_composite(masked, gen, mc), R.mask_composite_fused(masked, gen, mc)
    share = float(np.mean(two.view(np.uint32) != one.view(np.uint32)))
    assert share >= 0.10, share
    binary = (mc > 0.5).astype(np.float32)
    assert R.same_bits(R.mask_composite(masked, gen, binary), R.mask_composite_fused(masked, gen, binary))


def test_small_helpers():
    assert R.nblocks(1) == 1 and R.nblocks(1024) == 1 and R.nblocks(1025) == 2 and R.nblocks(2 ** 21 + 3) == 2048
    assert R.check_finite_stride(2048) == 256 and R.check_finite_stride(2049) == 512 and R.check_finite_stride(2 ** 22 + 4099) == 2048 * 256
    assert R.py_float(np.float32(0.999)) == 0.999 and R.py_float(np.float32(0.0002)) == 0.0002
    g = np.array([np.nan, 1.0, -3.0, np.nan, 0.0, 0.0], dtype=np.float32)
    assert R.grad_absmean(g, [1, 4], [2, 2]).tolist() == [2.0, 0.0]
    assert R.ulp_distance(np.float32(1.0), np.nextafter(np.float32(1.0), np.float32(2.0))) == 1
    m, masked = R.mask_apply(np.array([2.0, 2.0, 2.0], np.float32), np.array([0.0, 1e-30, 0.25], np.float32), 3)
    assert m.tolist() == [1.0, 0.0, 0.0] and masked.tolist() == [0.0, 2.0, 2.0]
    h = R.convert(np.array([65504.0, 65520.0, -0.0, 2.0 ** -25, 1.0 + 2.0 ** -11], np.float32), True)
    assert h.tolist()[:2] == [65504.0, float("inf")] and np.signbit(h[2]) and h[3] == 0 and h[4] == 1.0
