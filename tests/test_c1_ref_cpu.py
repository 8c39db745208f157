"""CPU tier: keeps tests/c1_ref.py honest. (1) Its fp64 references against an independent restatement with explicit 2y-1+ky loops
at 3x5 maps. (2) A numpy emulation of each kernel's rounding points (fp32 accumulation in a scrambled order, fp16 col storage, fp16
output rounding) sits inside the derived bound at every element of every input of the rounding tests of tests/test_c1_gpu.py, and
its worst error / bound ratio is above 0.05: the bounds hold for arithmetic of that kind and are not vacuous."""
import math

import pytest
import torch

import c1_ref as R

FLOOR = 0.05


# ---- (1) direct loops ---------------------------------------------------------------------------------------------------------------
def _loop_gather(img, w, bias, act, in_scale):
    n, H, W = img.shape
    Hs, Ws, c = H // 2, W // 2, w.shape[0]
    out = torch.zeros(n, Hs, Ws, c, dtype=torch.float64)
    for nn in range(n):
        for y in range(Hs):
            for x in range(Ws):
                for ch in range(c):
                    s = 0.0 if bias is None else float(bias[ch])
                    for ky in range(4):
                        for kx in range(4):
                            iy, ix = 2 * y - 1 + ky, 2 * x - 1 + kx
                            if 0 <= iy < H and 0 <= ix < W:
                                s += float(img[nn, iy, ix]) * in_scale * float(w[ch, ky * 4 + kx])
                    if act == R.ACT_RELU:
                        s = max(s, 0.0)
                    if act == R.ACT_LRELU:
                        s = s if s > 0 else R.SLOPE * s
                    out[nn, y, x, ch] = s
    return out


def _loop_scatter_pre(X, w, bias, relu_in):
    n, Hs, Ws, c = X.shape
    out = torch.full((n, 2 * Hs, 2 * Ws), 0.0 if bias is None else float(bias[0]), dtype=torch.float64)
    for nn in range(n):
        for y in range(Hs):
            for x in range(Ws):
                for ky in range(4):
                    for kx in range(4):
                        oy, ox = 2 * y - 1 + ky, 2 * x - 1 + kx
                        if 0 <= oy < 2 * Hs and 0 <= ox < 2 * Ws:
                            for ch in range(c):
                                v = float(X[nn, y, x, ch])
                                out[nn, oy, ox] += (max(v, 0.0) if relu_in else v) * float(w[ch, ky * 4 + kx])
    return out


def _loop_wgrad(X, img, relu_in, scale, img_scale):
    n, Hs, Ws, c = X.shape
    dW = torch.zeros(c, 16, dtype=torch.float64)
    for nn in range(n):
        for y in range(Hs):
            for x in range(Ws):
                for ky in range(4):
                    for kx in range(4):
                        iy, ix = 2 * y - 1 + ky, 2 * x - 1 + kx
                        if 0 <= iy < 2 * Hs and 0 <= ix < 2 * Ws:
                            xv = X[nn, y, x].double()
                            dW[:, ky * 4 + kx] += scale * (xv.clamp(min=0) if relu_in else xv) * float(img[nn, iy, ix]) * img_scale
    return dW


N, HS, WS, CH = 2, 3, 5, 8


@pytest.mark.parametrize("act", [R.ACT_NONE, R.ACT_RELU, R.ACT_LRELU])
def test_gather_ref_against_loops(act):
    img, w, b = R.gather_inputs(False, False, N, HS, WS, CH, True, 3)
    ref, A = R.gather_ref(img, w, b, act, 0.5)
    assert torch.allclose(ref, _loop_gather(img, w, b, act, 0.5), rtol=0, atol=1e-13)
    assert torch.allclose(A, _loop_gather(img.abs(), w.abs(), b.abs(), R.ACT_NONE, 0.5), rtol=0, atol=1e-13)
    assert bool((A >= ref.abs() - 1e-13).all())


@pytest.mark.parametrize("relu_in", [0, 1])
def test_scatter_ref_against_loops(relu_in):
    X, w, b, _ = R.scatter_inputs(False, False, N, HS, WS, CH, True, 5)
    X = X - 0.3
    r = R.scatter_ref(X, w, b, relu_in, 1, 0.25)
    pre = _loop_scatter_pre(X, w, b, relu_in)
    assert torch.allclose(r["pre"], pre, rtol=0, atol=1e-13)
    assert torch.allclose(r["value"], torch.tanh(pre) * 0.25, rtol=0, atol=1e-13)
    Xa = X.clamp(min=0) if relu_in else X
    assert torch.allclose(r["A"], _loop_scatter_pre(Xa.abs(), w.abs(), b.abs(), 0), rtol=0, atol=1e-13)
    # col and S4: the overlap-add of col is the pre-activation, S4 bounds it and is bounded by A
    assert torch.allclose(R.overlap_add(r["col"]) + float(b[0]), pre, rtol=0, atol=1e-13)
    assert bool((r["S4"] + abs(float(b[0])) >= pre.abs() - 1e-13).all()) and bool((r["S4"] <= r["A"] + 1e-13).all())
    assert torch.allclose(r["col"][1, 2, 3], (Xa[1, 2, 3].double()[:, None] * w.double()).sum(0), rtol=0, atol=1e-13)


def test_scatter_ref_affine_half():
    X, w, b, aff = R.scatter_inputs(True, True, N, HS, WS, 16, True, 7, affine=True)     # integers: fused or not, the same
    x2, sc, sh = aff
    upper = torch.clamp(torch.addcmul(sh, x2, sc), min=0).half().double()      # fp32 multiply-add, ReLU, fp16
    assert 0 < int((upper == 0).sum()) < upper.numel()
    full = torch.cat([X[..., :8].double(), upper], -1)
    assert torch.equal(R.affine_x(X, aff), full)
    assert torch.allclose(R.scatter_ref(X, w, b, 0, 0, 1.0, aff)["pre"], _loop_scatter_pre(full, w, b, 0), rtol=0, atol=1e-13)
    assert torch.allclose(R.wgrad_ref(X, X.new_ones(N, 2 * HS, 2 * WS), 0, 1.0, 1.0, aff)[0],
                          _loop_wgrad(full, torch.ones(N, 2 * HS, 2 * WS), 0, 1.0, 1.0), rtol=0, atol=1e-12)


@pytest.mark.parametrize("relu_in", [0, 1])
def test_wgrad_ref_against_loops(relu_in):
    X, img, _ = R.wgrad_inputs(False, False, N, HS, WS, CH, 9)
    ref, A = R.wgrad_ref(X, img - 0.5, relu_in, 0.25, 0.5)
    assert torch.allclose(ref, _loop_wgrad(X, img - 0.5, relu_in, 0.25, 0.5), rtol=0, atol=1e-13)
    Xa = X.clamp(min=0) if relu_in else X
    assert torch.allclose(A, _loop_wgrad(Xa.abs(), (img - 0.5).abs(), 0, 0.25, 0.5), rtol=0, atol=1e-13)


def test_head4_refs_against_loops():
    X, w4, b, g = R.head4_inputs(False, N, HS, WS, 13, c=CH)
    r = R.head4_forward_ref(X, w4, b, 1)
    for o in range(4):
        pre = _loop_scatter_pre(X, w4[:, :, o], b[o:o + 1], 1)
        assert torch.allclose(r["pre"][:, o], pre, rtol=0, atol=1e-13)
        assert torch.allclose(r["value"][:, o], torch.tanh(pre), rtol=0, atol=1e-13)
    ref, A = R.head4_dgrad_ref(g, w4)
    want = sum(_loop_gather(g[:, o], w4[:, :, o], None, R.ACT_NONE, 1.0) for o in range(4))
    assert torch.allclose(ref, want, rtol=0, atol=1e-13)
    # the forward and the input gradient are adjoint: <convT(X), g> = <X, dgrad(g)>
    lin = R.head4_forward_ref(X, w4, None, 0)["pre"]
    assert math.isclose(float((lin * g.double()).sum()), float((X.double() * ref).sum()), rel_tol=1e-12)


def test_gather_and_scatter_refs_are_adjoint():
    img, w, _ = R.gather_inputs(False, False, N, HS, WS, CH, False, 15)
    X = R.uni((N, HS, WS, CH), 16, fp16=False)
    lhs = float((R.gather_ref(img, w)[0] * X.double()).sum())
    rhs = float((R.scatter_ref(X, w)["pre"] * img.double()).sum())
    assert math.isclose(lhs, rhs, rel_tol=1e-12)
    assert torch.allclose(R.wgrad_ref(X, img)[0], torch.autograd.functional.jacobian(
        lambda ww: (R.gather_ref(img, ww)[0] * X.double()).sum(), w.double()), rtol=0, atol=1e-12)


def test_reduce_ref():
    part, d0 = R.reduce_inputs(True, 20, 17, 1)
    ref, A = R.reduce_ref(part, d0)
    assert torch.equal(ref, d0.double() + part.double().sum(0)) and torch.equal(A, part.double().abs().sum(0))


# ---- (2) the emulation inside the bounds, and not far inside ----------------------------------------------------------------------------
def _judge(what, err, bound):
    ratio = R.worst_ratio(err, bound)
    print(f"{what}: emulation worst err / bound = {ratio:.3f}")
    assert ratio <= 1.0, f"{what}: the emulated arithmetic breaks the bound ({ratio:.3f})"
    assert ratio > FLOOR, f"{what}: the bound is vacuous on these inputs ({ratio:.4f} <= {FLOOR})"


@pytest.mark.parametrize("case", R.GATHER_ROUNDING, ids=[c[0] for c in R.GATHER_ROUNDING])
def test_gather_bound(case):
    fp16, n, Hs, Ws, c, bias, act, in_scale, _ = case[1]
    img, w, b = R.gather_inputs(False, fp16, n, Hs, Ws, c, bias, R.SEED)
    ref, A = R.gather_ref(img, w, b, act, in_scale)
    _judge(case[0], R.emulate_gather(fp16, img, w, b, act, in_scale) - ref, R.bound_gather(fp16, ref, A))


@pytest.mark.parametrize("case", R.SCATTER_ROUNDING, ids=[c[0] for c in R.SCATTER_ROUNDING])
def test_scatter_bound(case):
    fp16, n, Hs, Ws, c, bias, relu_in, post, out_scale, affine, _, _, kind, _ = case[1]
    X, w, b, aff = R.scatter_inputs(False, fp16, n, Hs, Ws, c, bias, R.SEED, affine)
    r = R.scatter_ref(X, w, b, relu_in, post, out_scale, aff)
    _judge(case[0], R.emulate_scatter(kind, X, w, b, relu_in, post, out_scale, aff) - r["value"], R.bound_scatter(kind, r, c, post, out_scale))


@pytest.mark.parametrize("case", R.WGRAD_ROUNDING, ids=[c[0] for c in R.WGRAD_ROUNDING])
def test_wgrad_bound(case):
    fp16, n, Hs, Ws, c, relu_in, scale, img_scale, affine, _, _ = case[1]
    X, img, aff = R.wgrad_inputs(False, fp16, n, Hs, Ws, c, R.SEED, affine)
    ref, A = R.wgrad_ref(X, img, relu_in, scale, img_scale, aff)
    _judge(case[0], R.emulate_wgrad(X, img, relu_in, scale, img_scale, aff) - ref, R.bound_fp32(n * Hs * Ws, A))


@pytest.mark.parametrize("case", R.REDUCE_ROUNDING, ids=[c[0] for c in R.REDUCE_ROUNDING])
def test_reduce_bound(case):
    count, blocks, _ = case[1]
    part, d0 = R.reduce_inputs(False, count, blocks, R.SEED)
    ref, A = R.reduce_ref(part, d0)
    _judge(case[0], R.emulate_reduce(part, d0) - ref, R.bound_fp32(blocks, A))


@pytest.mark.parametrize("case", R.HEAD4_MAPS, ids=[c[0] for c in R.HEAD4_MAPS])
def test_head4_bounds(case):
    n, Hs, Ws = case[1]
    X, w4, b, g = R.head4_inputs(False, n, Hs, Ws, R.SEED)
    ref, A = R.head4_dgrad_ref(g, w4)
    _judge(case[0] + " dgrad", R.emulate_head4_dgrad(g, w4) - ref, R.bound_gather(True, ref, A, 64))
    r = R.head4_forward_ref(X, w4, b, 1)
    for o in range(4):
        ro = R.scatter_ref(X, w4[:, :, o], b[o:o + 1], 1, 1, 1.0)
        assert torch.equal(ro["value"], r["value"][:, o])
        _judge(f"{case[0]} forward channel {o}", R.emulate_scatter("col", X, w4[:, :, o], b[o:o + 1], 1, 1, 1.0, None) - ro["value"],
               R.bound_scatter("col", ro, 128, 1, 1.0))


def test_exact_inputs_are_exact_in_fp16():
    """the premise of the exact tests: with the integer inputs every col value and every gather output is an fp16 number"""
    X, w, b, aff = R.scatter_inputs(True, True, 2, 3, 32, 128, True, R.SEED, affine=True)
    col = R.scatter_ref(X, w, b, 1, 0, 1.0, aff)["col"]
    assert torch.equal(col.half().double(), col) and float(col.abs().max()) <= 896
    img, w, b = R.gather_inputs(True, True, 2, 3, 16, 64, True, R.SEED)
    ref = R.gather_ref(img, w, b, R.ACT_NONE, 0.5)[0]
    assert torch.equal(ref.half().double(), ref)
    X, w4, b4, g = R.head4_inputs(True, 2, 4, 16, R.SEED)
    ref = R.head4_dgrad_ref(g, w4)[0]
    assert torch.equal(ref.half().double(), ref)
    r = R.head4_forward_ref(X, w4, b4, 1)
    for o in range(4):
        col = R.scatter_ref(X, w4[:, :, o], None, 1)["col"]
        assert torch.equal(col.half().double(), col)
    assert torch.equal(r["pre"].float().double(), r["pre"]) and 1.0 < float(r["pre"].abs().max()) < 8.0
