"""CPU tier: tests/norm_ref.py (the fp64 restatement tests/test_norm_ops_gpu.py compares the kernels with) against torch in fp64:
F.batch_norm / F.instance_norm with autograd through [dropout mask] o act o norm, one and two populations, eval mode, the
tangent-injection term against a double backward, the gradient-penalty direction against autograd, the hash and the fixed-point
rules against their definitions."""
import math

import pytest
import torch
import torch.nn.functional as F

import norm_ref as R

F64 = torch.float64
TOL = 1e-11


def _close(a, b, tol=TOL):
    err = float((a.double() - b.double()).abs().max())
    scale = float(b.double().abs().max()) + 1e-300
    assert err <= tol * scale, (err, scale)


def _torch_act(t, act):
    return t if act == R.ACT_NONE else (F.relu(t) if act == R.ACT_RELU else F.leaky_relu(t, 0.2))


def _data(P, c, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(P, c, dtype=F64, generator=g) * 1.5 + torch.randn(c, dtype=F64, generator=g)
    gamma = torch.rand(c, dtype=F64, generator=g) + 0.5
    beta = torch.randn(c, dtype=F64, generator=g) * 0.3
    rmean = torch.randn(c, dtype=F64, generator=g) * 0.2
    rvar = torch.rand(c, dtype=F64, generator=g) + 0.5
    g1 = torch.randn(P, c, dtype=F64, generator=g)
    g2 = torch.randn(P, c, dtype=F64, generator=g)
    drop = (torch.rand(P, c, generator=g) > 0.5).to(torch.uint8)
    return x, gamma, beta, rmean, rvar, g1, g2, drop


def _nchw(x, n):
    """(n * hw, c) -> (n, c, hw, 1)"""
    return x.reshape(n, -1, x.shape[1]).permute(0, 2, 1).unsqueeze(-1)


def _back(t):
    return t.squeeze(-1).permute(0, 2, 1).reshape(-1, t.shape[1])


# (dropout is representable only behind a ReLU: the backward reads the zeros from y > 0)
@pytest.mark.parametrize("act,use_drop", [(R.ACT_NONE, False), (R.ACT_RELU, False), (R.ACT_LRELU, False), (R.ACT_RELU, True)])
@pytest.mark.parametrize("groups", [1, 2])
def test_batchnorm_train_forward_backward(act, groups, use_drop):
    P, c, n = 24, 5, 4
    x, gamma, beta, rmean, rvar, g1, g2, drop = _data(P, c, 1 + act + 10 * groups)
    pg = P // groups
    drop_scale = 2.0 if use_drop else 1.0
    # torch: the populations one call after the other on the same module state
    xt = x.clone().requires_grad_(True)
    gt, bt = gamma.clone().requires_grad_(True), beta.clone().requires_grad_(True)
    rm, rv = rmean.clone(), rvar.clone()
    ys = []
    for j in range(groups):
        xn = F.batch_norm(_nchw(xt[j * pg:(j + 1) * pg], n // groups), rm, rv, gt, bt, True, 0.1, 1e-5)
        ys.append(_back(_torch_act(xn, act)))
    y = torch.cat(ys, 0)
    if use_drop:
        y = y * drop.double() * drop_scale
    # upstream: g1 reaches y directly, g2 through the parent's in-place ReLU on the concatenated copy of y
    (y * g1).sum().backward(retain_graph=True)
    (F.relu(y) * g2).sum().backward()
    # restatement
    sums = [R.col_sums(x[j * pg:(j + 1) * pg]) for j in range(groups)]
    rs = R.bn_from_sums_groups(sums, pg, gamma, beta, rmean, rvar)
    yr = R.bn_apply(x, [r["scale"] for r in rs], [r["shift"] for r in rs], act, drop if use_drop else None, drop_scale, pg if groups == 2 else 0)
    _close(yr, y.detach())
    _close(rs[-1]["rmean"], rm)
    _close(rs[-1]["rvar"], rv)
    dz = R.dz_of(g1, g2, yr, act, drop_scale)
    dx, dbeta, dgamma, abs_b, abs_g = R.act_bn_bwd(dz, x, gamma, [r["mean"] for r in rs], [r["inv"] for r in rs], groups)
    _close(dx, xt.grad)
    _close(dbeta, bt.grad)
    _close(dgamma, gt.grad)
    assert (abs_b >= dbeta.abs() - 1e-12).all() and (abs_g >= dgamma.abs() - 1e-12).all()
    # the sign of the activation's input is as good as y (no dropout): fma(x, scale, shift)
    if not use_drop:
        pre = R.bn_apply(x, [r["scale"] for r in rs], [r["shift"] for r in rs], R.ACT_NONE, pg=pg if groups == 2 else 0)
        assert torch.equal(R.dz_of(g1, g2, pre, act), dz) or act == R.ACT_NONE


def test_batchnorm_eval():
    P, c, n = 24, 5, 4
    x, gamma, beta, rmean, rvar, g1, g2, _ = _data(P, c, 5)
    xt = x.clone().requires_grad_(True)
    y = _back(F.leaky_relu(F.batch_norm(_nchw(xt, n), rmean.clone(), rvar.clone(), gamma, beta, False, 0.1, 1e-5), 0.2))
    (y * g1).sum().backward()
    r = R.bn_from_sums(None, None, P, gamma, beta, rmean, rvar, train=False)
    yr = R.bn_apply(x, r["scale"], r["shift"], R.ACT_LRELU)
    _close(yr, y.detach())
    assert torch.equal(r["rmean"], rmean) and torch.equal(r["rvar"], rvar)
    dx, dbeta, dgamma, _, _ = R.act_bn_bwd(R.dz_of(g1, None, yr, R.ACT_LRELU), x, gamma, [r["mean"]], [r["inv"]], 1, eval_bn=True)
    _close(dx, xt.grad)
    assert not dbeta.any() and not dgamma.any()


def test_batchnorm_count_one_keeps_the_biased_variance():
    c = 4
    x = torch.randn(1, c, dtype=F64)
    s, q = R.col_sums(x)
    r = R.bn_from_sums(s, q, 1, torch.ones(c), torch.zeros(c), torch.zeros(c), torch.ones(c))
    _close(r["rvar"], torch.full((c,), 0.9, dtype=F64))
    _close(r["inv"], torch.full((c,), 1.0 / math.sqrt(1e-5), dtype=F64))


@pytest.mark.parametrize("act", [R.ACT_NONE, R.ACT_RELU, R.ACT_LRELU])
@pytest.mark.parametrize("hw", [2, 7])
def test_instancenorm_forward_backward(act, hw):
    n, c = 3, 5
    x, _, _, _, _, g1, g2, drop = _data(n * hw, c, 20 + hw)
    use_drop = act == R.ACT_RELU
    drop_scale = 2.0 if use_drop else 1.0
    xt = x.clone().requires_grad_(True)
    y = _back(_torch_act(F.instance_norm(_nchw(xt, n), eps=1e-5), act))
    if use_drop:
        y = y * drop.double() * drop_scale
    (y * g1).sum().backward(retain_graph=True)
    (F.relu(y) * g2).sum().backward()
    yr, mean, inv = R.in_forward(x, n, hw, act, drop if use_drop else None, drop_scale)
    _close(yr, y.detach())
    dx = R.act_in_bwd(R.dz_of(g1, g2, yr, act, drop_scale), x, n, hw, mean, inv)
    _close(dx, xt.grad, 1e-9)


def test_instancenorm_single_pixel():
    """hw = 1 (torch refuses it): variance 0, y = 0, inv = 1 / sqrt(eps), and a constant plane passes no gradient"""
    n, c = 3, 5
    x, _, _, _, _, g1, _, _ = _data(n, c, 9)
    yr, mean, inv = R.in_forward(x, n, 1, R.ACT_LRELU)
    assert not yr.any() and torch.equal(mean, x)
    _close(inv, torch.full_like(inv, 1.0 / math.sqrt(1e-5)))
    assert not R.act_in_bwd(R.dz_of(g1, None, yr, R.ACT_NONE), x, n, 1, mean, inv).any()


def test_tangent_injection_against_double_backward():
    P, c = 40, 6
    x, gamma, _, _, _, dta, tx, _ = _data(P, c, 33)
    y = torch.randn(P, c, dtype=F64, generator=torch.Generator().manual_seed(2))
    xt, gt = x.clone().requires_grad_(True), gamma.clone().requires_grad_(True)
    mean = xt.mean(0)
    var = ((xt - mean) ** 2).mean(0)
    inv_t = 1.0 / torch.sqrt(var + 1e-5)
    # the BatchNorm tangent map as a jvp of the train-mode forward z(x) = gamma * (x - mean) * inv in direction tx
    def z_of(xx):
        m = xx.mean(0)
        return gt * (xx - m) / torch.sqrt(((xx - m) ** 2).mean(0) + 1e-5)
    _, tz = torch.autograd.functional.jvp(z_of, (xt,), (tx,), create_graph=True)
    a = dta * R.lrelu_slope(y)
    (a * tz).sum().backward()
    inj, dgamma = R.bn_tangent_inject(dta, y, tx, x, gamma, mean.detach(), inv_t.detach())
    _close(inj, xt.grad, 1e-10)
    _close(dgamma, gt.grad, 1e-10)


@pytest.mark.parametrize("hw", [1, 50])
def test_gp_direction_against_autograd(hw):
    n, lam = 4, 10.0
    g = (torch.randn(n, hw, dtype=F64, generator=torch.Generator().manual_seed(hw)) * 0.7).requires_grad_(True)
    pen = lam * ((g.norm(dim=1) - 1.0) ** 2).mean()
    pen.backward()
    v, s, p = R.gp_direction(g.detach(), lam)
    _close(v, g.grad)
    assert abs(p - float(pen.detach())) <= 1e-12 * abs(float(pen.detach()))
    assert math.log2(s) == int(math.log2(s)) and 1.0 <= float(v.abs().max()) * s < 2.0
    v0, s0, p0 = R.gp_direction(torch.zeros(2, 3), lam)
    assert not v0.any() and s0 == 1.0 and p0 == lam


def test_small_ops():
    y = torch.tanh(torch.randn(50, dtype=F64)).requires_grad_(False)
    z = torch.randn(50, dtype=F64).requires_grad_(True)
    dy = torch.randn(50, dtype=F64)
    (torch.tanh(z) * dy).sum().backward()
    _close(R.tanh_bwd(dy, torch.tanh(z.detach()), 3.0), 3.0 * z.grad)
    m = torch.arange(2 * 3 * 5, dtype=torch.uint8)
    nhwc = R.mask_layout(m, 2, 3, 5, True)
    assert torch.equal(nhwc, m.reshape(2, 3, 5).permute(0, 2, 1)) and torch.equal(R.mask_layout(nhwc.reshape(-1), 2, 3, 5, False).reshape(-1), m)
    t, a = torch.randn(30, dtype=F64), torch.randn(30, dtype=F64)
    ar = a.clone().requires_grad_(True)
    (F.leaky_relu(ar, 0.2) * t).sum().backward()
    _close(R.mul_slope(t, F.leaky_relu(a, 0.2)), ar.grad)


def test_dropout_hash():
    # splitmix64: the published first outputs for seed 0 are mix64 of the counter 1, 2, 3 strides
    assert R.mix64(0x9E3779B97F4A7C15) == 0xE220A8397B1DCDAF
    assert R.mix64((2 * 0x9E3779B97F4A7C15) & ((1 << 64) - 1)) == 0x6E789E6AA1B965F4
    assert R.dropout_thresh(0.5) == 1 << 31 and R.dropout_thresh(0.0) == 1 and R.dropout_thresh(1.0) == 0xFFFFFFFF
    m = R.dropout_mask(1234, 20000, 0.5)
    assert abs(float(m.float().mean()) - 0.5) < 0.02
    assert not torch.equal(m, R.dropout_mask(1235, 20000, 0.5))
    assert abs(float(R.dropout_mask(7, 20000, 0.25).float().mean()) - 0.75) < 0.02


def test_stat_acc_rules():
    from fractions import Fraction
    f32 = lambda v: float(torch.tensor(v, dtype=torch.float32))   # noqa: E731
    adds = [f32(1.5), f32(-2.25), f32(3e-9), f32(-7e-13), f32(1e11), f32(-1e11 + 4096)]
    # one unit of 2^-40 is cut toward -inf per addend with bits below it
    exact = sum(Fraction(math.floor(Fraction(a) * 2 ** 40), 2 ** 40) for a in adds)
    assert R.stat_acc_total(adds) == float(exact)
    assert R.stat_acc_total(list(reversed(adds))) == R.stat_acc_total(adds)
    assert R.stat_acc_total([f32(-2.0 ** -41)]) == -2.0 ** -40 and R.stat_acc_total([f32(2.0 ** -41)]) == 0.0
    big = f32(2.0 ** 40 - 2.0 ** 16)
    assert R.stat_acc_total([big, big]) == 2.0 * big
    for bad in (2.0 ** 40, -2.0 ** 40, float("inf"), float("nan")):
        assert math.isnan(R.stat_acc_total([1.0, bad]))
