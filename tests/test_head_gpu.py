"""GPU tier: every kernel of csrc/head.hip (the PatchGAN critic head: Conv2d(c,1,4,1,0) + Flatten + Linear(P,1) [+ Sigmoid], forward
and backward), ONE OPERATION AT A TIME through the C-ABI seam (gi_debug_head_forward / gi_debug_head_backward), against the fp64
references of tests/head_ref.py, with an assertion on WHICH path served the shape (gi_debug_last_kernel). Two kinds of test per path:

  exact     small-integer inputs (powers of two for the scales): every product and every fp32 partial sum is an integer below 2^24,
            so the result must EQUAL the reference - a wrong tap at a map edge, a missed partial, a ragged tile or band, a second
            population reading the first one's vectors shows as a non-zero difference. The sigmoid and the float-atomics forms are
            rounding-only; the accumulator-derived BatchNorm form (its vectors are no powers of two) must equal, bit for bit, the
            given-vectors form run on the vectors it published, which is itself exact-tested.
  rounding  uniform inputs already rounded to the compute type: |err| <= the per-element bound derived in head_ref.py
            (tests/test_head_ref_cpu.py shows on inputs of the same kind that arithmetic of this form stays inside it and that a
            wrong kernel leaves it). The worst ratio of every case is recorded (gpu_util.record).

Every output element is judged. Guard zones surround every written buffer and every input; whatever a kernel may not read is NaN
(the gap between two populations' vectors, a4 of a frozen backward, tbuf and the scratch before use)."""
import ctypes as C
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

import head_ref as R  # noqa: E402
import norm_ref as NR  # noqa: E402
from gpu_util import B, record, tdt  # noqa: E402

F16, F32 = B.GI_F16, B.GI_F32
NAN = float("nan")
SENT = -777.0          # an fp16 number no test produces
GUARD = 1024           # elements before and after every buffer
GSTRIDE = 2048         # floats between two populations' vectors, as the networks pass it
LS = 256.0
FAST_FWD, AFF_CASES, FAST_BWD, RAW_CASES, GENERIC, GEN_MAPS = R.FAST_FWD, R.AFF_CASES, R.FAST_BWD, R.RAW_CASES, R.GENERIC, R.GEN_MAPS
VEC_TOL = 2e-5         # of max|ref|: what tests/test_norm_ops_gpu.py holds the same accumulator-to-vector arithmetic (bn_acc.h) to


class Buf:
    """a device buffer of `shape` between two guard zones, all filled with `fill` (tests/test_c1_gpu.py)"""

    def __init__(self, shape, dtype, fill=SENT):
        numel = 1
        for k in shape:
            numel *= k
        self.full = torch.full((numel + 2 * GUARD,), fill, dtype=dtype, device="cuda")
        self.t = self.full[GUARD:GUARD + numel].view(shape)
        self.fill = fill

    def guards_intact(self):
        g = torch.cat([self.full[:GUARD], self.full[-GUARD:]])
        return bool(torch.isnan(g).all()) if self.fill != self.fill else bool((g == self.fill).all())


def _exact(what, got, ref, dtype):
    """torch.equal against the fp64 reference brought to the output type (fp64 -> fp32 -> type: the kernels round an fp32 value)"""
    want = ref.to(torch.float32).to(dtype)
    if not torch.equal(got, want):
        d = (got.double() - want.double()).abs()
        idx = tuple(int(i) for i in (d == d.max()).nonzero()[0])
        raise AssertionError(f"{what}: {int((d != 0).sum())} of {d.numel()} elements differ, worst {float(d.max()):.6g} at {idx}: "
                             f"got {float(got[idx])} want {float(want[idx])}")


def _code(fp16):
    return F16 if fp16 else F32


def _sync():
    torch.cuda.synchronize()


def _in(t, dtype=torch.float32):
    """an input on the device between two NaN guard zones (a read outside it poisons the result)"""
    b = Buf(tuple(t.shape), dtype, NAN)
    b.t.copy_(t.to(dtype))
    return b


def _vecs(v, c):
    """(G, c) -> device buffer (G * GSTRIDE) with NaN between the populations' vectors"""
    G = v.shape[0]
    b = Buf((G, GSTRIDE), torch.float32, NAN)
    b.t[:, :c] = v.float().cuda()
    return b


def _rounding(what, got, ref, bound):
    ratio = R.worst_ratio(got.double() - ref, bound)
    print(f"{what}: worst err / bound = {ratio:.4f}")
    record(f"head {what}", ratio)
    assert ratio <= 1.0, f"{what}: error {ratio:.3f} times the bound"


@functools.lru_cache(maxsize=6)
def _inputs(exact, fp16, n, Hh, Wh, c, groups=0, sigmoid=0):
    return R.inputs(exact, fp16, n, Hh, Wh, c, groups=groups, sigmoid=sigmoid)


@functools.lru_cache(maxsize=6)
def _fwd_ref(exact, fp16, n, Hh, Wh, c, groups, fast):
    d = _inputs(exact, fp16, n, Hh, Wh, c, groups)
    return R.forward_ref(d["a4"], d["w5"], d["wl"], d["bl"], 0, fast, d["aff"])


@functools.lru_cache(maxsize=6)
def _bwd_ref(exact, fp16, n, Hh, Wh, c, groups, sigmoid, pre, want_w):
    d = _inputs(exact, fp16, n, Hh, Wh, c, groups, sigmoid)
    return R.backward_ref(d["a4"], Hh, Wh, d["w5"], d["wl"], d["h"], d["out"], d["dy"], sigmoid, LS, d["aff"], d["pre"] if pre else None, want_w)


# ================================================================ forward ========================================================
def _run_forward(d, fp16, n, Hh, Wh, c, sigmoid, kernel, out2=False, tbuf=None, aff=None, bn=None, expect_error=False):
    """-> h (n, P), out (n) on the CPU. aff = (scale Buf, shift Buf, n_per_group) on the device. tbuf: None, 'ok' or 'short'."""
    code, P, npx = _code(fp16), (Hh - 3) * (Wh - 3), Hh * Wh
    a4, w5, wl, bl = _in(d["a4"], tdt(code)), _in(d["w5"]), _in(d["wl"]), _in(d["bl"])
    h, out, o2 = Buf((n, P), torch.float32), Buf((n,), torch.float32), Buf((n,), torch.float32)
    tb = Buf((n * npx * 16,), torch.float32, NAN)
    tbytes = 0 if tbuf is None else n * npx * 64 - (4 if tbuf == "short" else 0)
    a = B.HeadArgs(a4=B.ptr(a4.t), w5=B.ptr(w5.t), wl=B.ptr(wl.t), bl=B.ptr(bl.t), h=B.ptr(h.t), out=B.ptr(out.t), n=n, Hh=Hh, Wh=Wh, c=c,
                   sigmoid=sigmoid, out2=B.ptr(o2.t) if out2 else None, tbuf=B.ptr(tb.t) if tbuf else None, tbuf_bytes=tbytes)
    if aff is not None:
        a.scale4, a.shift4, a.n_per_group, a.gstride = B.ptr(aff[0].t), B.ptr(aff[1].t), aff[2], GSTRIDE
    if bn is not None:
        a.bn = C.pointer(bn)
    before = B.last_kernel()
    st = B.lib().gi_debug_head_forward(B.get_ctx(), code, C.byref(a))
    _sync()
    bufs = [a4, w5, wl, bl, h, out, o2, tb] + (list(aff[:2]) if aff is not None else [])
    assert all(b.guards_intact() for b in bufs), "the forward wrote outside its buffers"
    if expect_error:
        assert st != 0, "the call was accepted"
        assert B.last_kernel() == before, f"a rejected call launched {B.last_kernel()}"
        assert all(bool((b.t == SENT).all()) for b in (h, out, o2)) and bool(torch.isnan(tb.t).all()), "a rejected call wrote its outputs"
        return None
    B.check(st)
    assert B.last_kernel() == kernel, (B.last_kernel(), kernel)
    if kernel != "head_fwd512_sliced":
        assert bool(torch.isnan(tb.t).all()), "tbuf written by an unsliced forward"
    if out2:
        assert torch.equal(out.t, o2.t), "the second copy of the output differs"
    else:
        assert bool((o2.t == SENT).all())
    return h.t.cpu(), out.t.cpu()


def _judge_forward(what, exact, got, f, c, P, sigmoid):
    h, out = got
    if exact:
        _exact(f"{what} h", h, f["h"], torch.float32)
        _exact(f"{what} out", out, f["out"], torch.float32)
    else:
        _rounding(f"{what} h", h, f["h"], R.bound_h(c, f["A_h"]))
        ref = torch.sigmoid(f["pre"]) if sigmoid else f["pre"]
        _rounding(f"{what} out", out, ref, R.bound_out(c, P, f["A_out"], sigmoid))


def _fid(case):
    n, Hh, Wh, tbuf, kernel = case
    return f"n{n}-{Hh}x{Wh}-tbuf_{tbuf}-{kernel}"


@pytest.mark.parametrize("out2", [False, True], ids=["", "out2"])
@pytest.mark.parametrize("case", FAST_FWD, ids=_fid)
def test_fast_forward_exact(case, out2):
    n, Hh, Wh, tbuf, kernel = case
    assert (R.slices(n, Hh * Wh) > 1 and tbuf == "ok") == (kernel == "head_fwd512_sliced")
    d = _inputs(True, True, n, Hh, Wh, 512)
    got = _run_forward(d, True, n, Hh, Wh, 512, 0, kernel, out2, tbuf)
    _judge_forward(f"fast forward exact {_fid(case)}", True, got, _fwd_ref(True, True, n, Hh, Wh, 512, 0, True), 512, (Hh - 3) * (Wh - 3), 0)


@pytest.mark.parametrize("out2", [False, True], ids=["", "out2"])
@pytest.mark.parametrize("sigmoid", [0, 1], ids=["linear", "sigmoid"])
@pytest.mark.parametrize("case", FAST_FWD, ids=_fid)
def test_fast_forward_rounding(case, sigmoid, out2):
    n, Hh, Wh, tbuf, kernel = case
    d = _inputs(False, True, n, Hh, Wh, 512)
    got = _run_forward(d, True, n, Hh, Wh, 512, sigmoid, kernel, out2, tbuf)
    _judge_forward(f"fast forward {_fid(case)} sigmoid={sigmoid}", False, got, _fwd_ref(False, True, n, Hh, Wh, 512, 0, True), 512, (Hh - 3) * (Wh - 3), sigmoid)


def _aid(case):
    n, g, Hh, Wh = case
    return f"n{n}-pops{g}-{Hh}x{Wh}-head_fwd512"


@pytest.mark.parametrize("exact", [True, False], ids=["exact", "rounding"])
@pytest.mark.parametrize("case", AFF_CASES, ids=_aid)
def test_fast_forward_affine(case, exact):
    n, g, Hh, Wh = case
    d = _inputs(exact, True, n, Hh, Wh, 512, g)
    sc, sh, npg = d["aff"]
    got = _run_forward(d, True, n, Hh, Wh, 512, 0, "head_fwd512", aff=(_vecs(sc, 512), _vecs(sh, 512), npg if g == 2 else 0))
    _judge_forward(f"fast forward affine {_aid(case)}", exact, got, _fwd_ref(exact, True, n, Hh, Wh, 512, g, True), 512, (Hh - 3) * (Wh - 3), 0)


def _acc_block(c):
    return torch.zeros(B.lib().gi_stat_acc_words(c), dtype=torch.int64, device="cuda")


def _totals(addends):
    return torch.tensor([NR.stat_acc_total(addends[:, ch].tolist()) for ch in range(addends.shape[1])], dtype=torch.float64)


@pytest.mark.parametrize("reps", [1, 4], ids=["reps1-head_fwd512", "reps4-head_fwd512"])
@pytest.mark.parametrize("Hh,Wh", [(5, 7), (16, 16)], ids=["n4-pops2-5x7", "n4-pops2-16x16"])
def test_fast_forward_bn_from_accumulators(Hh, Wh, reps):
    """HeadArgs::bn, two populations of two images: the vectors derived by the head (workgroups 1 .. 3 derive their own, workgroup 0
    publishes both populations'), the running statistics moved population by population, zero_next cleared; h and out judged with
    the published fp32 vectors as the affine map's inputs, and bit-identical to the given-vectors form on those vectors."""
    n, G, c, npx = 4, 2, 512, Hh * Wh
    npg = n // G
    d = dict(_inputs(False, True, n, Hh, Wh, c))
    acc, sums = _acc_block(c), []
    for j in range(G):
        xs = d["a4"][j * npg:(j + 1) * npg].double().reshape(-1, c)
        rows = xs.shape[0]
        cut = [rows * k // 5 for k in range(6)]
        for q in (0, 1):
            add = torch.stack([(xs[cut[k]:cut[k + 1]] ** (q + 1)).sum(0) for k in range(5)]).float()
            B.check(B.lib().gi_debug_stat_acc_add(B.get_ctx(), B.ptr(acc), c, reps, j, q, B.ptr(add.cuda()), 5))
            sums.append(_totals(add))
    _sync()
    gen = torch.Generator().manual_seed(7)
    gamma, beta = torch.rand(c, generator=gen) + 0.5, torch.randn(c, generator=gen) * 0.5
    rmean, rvar = torch.randn(c, generator=gen) * 0.1, torch.rand(c, generator=gen) + 0.5
    rs = NR.bn_from_sums_groups([(sums[0], sums[1]), (sums[2], sums[3])], npg * npx, gamma, beta, rmean, rvar)
    pub = [Buf((G, GSTRIDE), torch.float32, NAN) for _ in range(4)]
    gd, bd, rm, rv = _in(gamma), _in(beta), _in(rmean), _in(rvar)
    zn = Buf((600,), torch.int64, 0x0101010101010101)
    bn = B.BnAccArgs(acc=B.ptr(acc), reps=reps, gamma=B.ptr(gd.t), beta=B.ptr(bd.t), running_mean=B.ptr(rm.t), running_var=B.ptr(rv.t),
                     scale=B.ptr(pub[0].t), shift=B.ptr(pub[1].t), save_mean=B.ptr(pub[2].t), save_invstd=B.ptr(pub[3].t), count=npg * npx,
                     momentum=0.1, eps=1e-5, groups=G, out_stride=GSTRIDE, zero_next=B.ptr(zn.t), zero_words=300)
    got = _run_forward(d, True, n, Hh, Wh, c, 0, "head_fwd512", aff=(pub[0], pub[1], npg), bn=bn)
    what = f"fast forward bn {Hh}x{Wh} reps={reps}"
    assert all(p.guards_intact() for p in pub + [gd, bd, rm, rv, zn]) and all(bool(torch.isnan(p.t[:, c:]).all()) for p in pub), "vectors written outside their channels"
    assert not zn.t[:300].any() and bool((zn.t[300:] == 0x0101010101010101).all()), "zero_next"

    def vec(name, gotv, ref):
        rel = float((gotv.cpu().double() - ref).abs().max() / (ref.abs().max() + 1e-30))
        print(f"{what} {name}: rel {rel:.3e}")
        record(f"head {what} {name}", rel / VEC_TOL)
        assert rel <= VEC_TOL, f"{what} {name}: {rel:.3e}"
    for j in range(G):
        for k, key in enumerate(("scale", "shift", "mean", "inv")):
            vec(f"{key}[{j}]", pub[k].t[j, :c], rs[j][key])
    vec("running_mean", rm.t, rs[-1]["rmean"])
    vec("running_var", rv.t, rs[-1]["rvar"])
    d["aff"] = (pub[0].t[:, :c].cpu(), pub[1].t[:, :c].cpu(), npg)
    f = R.forward_ref(d["a4"], d["w5"], d["wl"], d["bl"], 0, True, d["aff"])
    _judge_forward(what, False, got, f, c, (Hh - 3) * (Wh - 3), 0)
    given = _run_forward(d, True, n, Hh, Wh, c, 0, "head_fwd512", aff=(_vecs(d["aff"][0], c), _vecs(d["aff"][1], c), npg))
    assert torch.equal(got[0], given[0]) and torch.equal(got[1], given[1]), "the derived form differs from the given-vectors form on the published vectors"


# ================================================================ backward =======================================================
def _run_backward(d, fp16, n, Hh, Wh, c, sigmoid, kernel, mode="grads", scratch="ok", aff=None, fuse=None, expect_error=False):
    """mode 'grads': dw5 / dwl / dbl preloaded with d['pre']; 'frozen': all three NULL and a4 NaN. scratch: 'ok' (what the serving
    path needs), 'short' (one float less than the fp16 c = 512 kernels need) or None. fuse = (x, scale, shift, mean, inv Bufs, npg,
    reps, acc). -> dict of CPU tensors (+ 'bits': every written buffer, for the determinism tests)"""
    code, P, npx = _code(fp16), (Hh - 3) * (Wh - 3), Hh * Wh
    T = tdt(code)
    frozen = mode == "frozen"
    a4 = Buf((n, Hh, Wh, c), T, NAN) if frozen else _in(d["a4"], T)
    w5, wl, hh, oo, dy = _in(d["w5"]), _in(d["wl"]), _in(d["h"]), _in(d["out"]), _in(d["dy"])
    da4, dh = Buf((n, Hh, Wh, c), T), Buf((n, P), torch.float32)
    dw5, dwl, dbl = Buf((16, c), torch.float32), Buf((P,), torch.float32), Buf((1,), torch.float32)
    if not frozen:
        for b, p in zip((dw5, dwl, dbl), d["pre"]):
            b.t.copy_(p)
    fast = kernel == "head_bwd512"
    floats = n * R.bands(n, npx) * 8192 if (fast or scratch == "short") else n * (2 if Hh - 3 >= 8 else 1) * 16 * c
    sbytes = 0 if scratch is None else floats * 4 - (4 if scratch == "short" else 0)
    sb = Buf((floats,), torch.float32, NAN)
    a = B.HeadBwdArgs(a4=B.ptr(a4.t), w5=B.ptr(w5.t), wl=B.ptr(wl.t), h=B.ptr(hh.t), out=B.ptr(oo.t), dy=B.ptr(dy.t), da4=B.ptr(da4.t),
                      dw5=None if frozen else B.ptr(dw5.t), dwl=None if frozen else B.ptr(dwl.t), dbl=None if frozen else B.ptr(dbl.t),
                      dh=B.ptr(dh.t), n=n, Hh=Hh, Wh=Wh, c=c, sigmoid=sigmoid, loss_scale=LS, scratch=B.ptr(sb.t) if scratch else None,
                      scratch_bytes=sbytes, bwd_reps=1, bwd_slope=1.0, bwd_applied=-1)
    if aff is not None:
        a.scale4, a.shift4, a.n_per_group, a.gstride = B.ptr(aff[0].t), B.ptr(aff[1].t), aff[2], GSTRIDE
    if fuse is not None:
        x, fsc, fsh, fmu, fiv, npg, reps, acc = fuse
        a.bwd_x, a.bwd_scale, a.bwd_shift, a.bwd_mean, a.bwd_inv = B.ptr(x.t), B.ptr(fsc.t), B.ptr(fsh.t), B.ptr(fmu.t), B.ptr(fiv.t)
        a.bwd_stride, a.bwd_n_per_group, a.bwd_reps, a.bwd_slope, a.bwd_acc = GSTRIDE, npg, reps, R.SLOPE, B.ptr(acc)
    before = B.last_kernel()
    st = B.lib().gi_debug_head_backward(B.get_ctx(), code, C.byref(a))
    _sync()
    bufs = [a4, w5, wl, hh, oo, dy, da4, dh, dw5, dwl, dbl, sb] + (list(aff[:2]) if aff is not None else []) + (list(fuse[:5]) if fuse is not None else [])
    assert all(b.guards_intact() for b in bufs), "the backward wrote outside its buffers"
    if expect_error:
        assert st != 0, "the call was accepted"
        assert B.last_kernel() == before, f"a rejected call launched {B.last_kernel()}"
        assert all(bool((b.t == SENT).all()) for b in (da4, dh)) and bool(torch.isnan(sb.t).all()), "a rejected call wrote its outputs"
        assert frozen or all(torch.equal(b.t.cpu(), p) for b, p in zip((dw5, dwl, dbl), d["pre"])), "a rejected call changed the gradients"
        return None
    B.check(st)
    assert B.last_kernel() == kernel, (B.last_kernel(), kernel)
    assert a.bwd_applied == (1 if fuse is not None and fast else 0), a.bwd_applied
    r = dict(da4=da4.t.cpu())
    if fast:
        assert bool((dh.t == SENT).all()), "dh written by the fp16 c = 512 kernels"
    else:
        r["dh"] = dh.t.cpu()
    if frozen:
        assert all(bool((b.t == SENT).all()) for b in (dw5, dwl, dbl)) and bool(torch.isnan(sb.t).all()), "a frozen backward wrote more than da4"
        assert bool(torch.isfinite(da4.t).all()), "a frozen backward read a4"
    else:
        r.update(dw5=dw5.t.cpu(), dwl=dwl.t.cpu(), dbl=dbl.t.cpu())
    return r


def _judge_backward(what, exact, fp16, got, ref, n, P):
    bounds = dict(dh=lambda v, A: R.bound_dh(v), da4=lambda v, A: R.bound_da4(fp16, v, A), dw5=lambda v, A: R.bound_dw5(n, P, A),
                  dwl=lambda v, A: R.bound_dwl(n, A), dbl=lambda v, A: R.bound_dwl(n, A))
    for k, g in got.items():
        v, A = ref[k]
        if exact:
            _exact(f"{what} {k}", g, v.reshape(g.shape), g.dtype)
        else:
            _rounding(f"{what} {k}", g, v.reshape(g.shape), bounds[k](v, A).reshape(g.shape))


def _bid(case):
    n, Hh, Wh = case
    return f"n{n}-{Hh}x{Wh}-bands{R.bands(n, Hh * Wh)}-head_bwd512"


@pytest.mark.parametrize("mode", ["grads", "frozen"])
@pytest.mark.parametrize("case", FAST_BWD, ids=_bid)
def test_fast_backward_exact(case, mode):
    n, Hh, Wh = case
    d = _inputs(True, True, n, Hh, Wh, 512)
    got = _run_backward(d, True, n, Hh, Wh, 512, 0, "head_bwd512", mode)
    _judge_backward(f"fast backward exact {_bid(case)} {mode}", True, True, got, _bwd_ref(True, True, n, Hh, Wh, 512, 0, 0, True, mode == "grads"), n, (Hh - 3) * (Wh - 3))


@pytest.mark.parametrize("mode", ["grads", "frozen", "sigmoid"])
@pytest.mark.parametrize("case", FAST_BWD, ids=_bid)
def test_fast_backward_rounding(case, mode):
    n, Hh, Wh = case
    sig = 1 if mode == "sigmoid" else 0
    d = _inputs(False, True, n, Hh, Wh, 512, 0, sig)
    got = _run_backward(d, True, n, Hh, Wh, 512, sig, "head_bwd512", "frozen" if mode == "frozen" else "grads")
    _judge_backward(f"fast backward {_bid(case)} {mode}", False, True, got, _bwd_ref(False, True, n, Hh, Wh, 512, 0, sig, True, mode != "frozen"), n, (Hh - 3) * (Wh - 3))


@pytest.mark.parametrize("exact", [True, False], ids=["exact", "rounding"])
@pytest.mark.parametrize("case", RAW_CASES, ids=lambda c: f"n{c[0]}-pops{c[1]}-{c[2]}x{c[3]}-head_bwd512")
def test_fast_backward_raw_a4(case, exact):
    """a4 is the raw conv4 output: the weight-gradient blocks apply the affine map and the LeakyReLU themselves"""
    n, g, Hh, Wh = case
    d = _inputs(exact, True, n, Hh, Wh, 512, g)
    sc, sh, npg = d["aff"]
    got = _run_backward(d, True, n, Hh, Wh, 512, 0, "head_bwd512", aff=(_vecs(sc, 512), _vecs(sh, 512), npg if g == 2 else 0))
    _judge_backward(f"fast backward raw a4 n{n} pops{g} {Hh}x{Wh}", exact, True, got, _bwd_ref(exact, True, n, Hh, Wh, 512, g, 0, True, True), n, (Hh - 3) * (Wh - 3))


@pytest.mark.parametrize("reps", [1, 2, 4], ids=["reps1-head_bwd512", "reps2-head_bwd512", "reps4-head_bwd512"])
@pytest.mark.parametrize("Hh,Wh", [(13, 9), (16, 16)], ids=["n2-pops2-13x9", "n2-pops2-16x16"])
def test_fast_backward_bn_sums(Hh, Wh, reps):
    """the fused BatchNorm-backward sums, two populations: judged in fp64 against the sums formed from the kernel's own stored da4"""
    n, G, c = 2, 2, 512
    d = _inputs(False, True, n, Hh, Wh, c)
    x, sc, sh, mu, iv = R.bn_bwd_inputs(n, Hh, Wh, c, G)
    acc = _acc_block(c)
    fuse = (_in(x, torch.float16), _vecs(sc, c), _vecs(sh, c), _vecs(mu, c), _vecs(iv, c), n // G, reps, acc)
    got = _run_backward(d, True, n, Hh, Wh, c, 0, "head_bwd512", fuse=fuse)
    what = f"fast backward bn sums {Hh}x{Wh} reps={reps}"
    _judge_backward(what, False, True, got, _bwd_ref(False, True, n, Hh, Wh, c, 0, 0, True, True), n, (Hh - 3) * (Wh - 3))
    s, A = R.bn_sums_ref(got["da4"], x, sc, sh, mu, iv, n // G)
    sums = torch.full((G, 2, c), NAN, dtype=torch.float64, device="cuda")
    for g in range(G):
        B.check(B.lib().gi_stat_acc_read(B.get_ctx(), B.ptr(acc), c, reps, g, B.ptr(sums[g])))
    _sync()
    _rounding(what + " sums", sums.cpu(), s, R.bound_bn_sums((n // G) * Hh * Wh, (n // G) * R.bands(n, Hh * Wh), A))


@pytest.mark.parametrize("case", [(2, 13, 9), (1, 17, 17), (17, 4, 4)], ids=_bid)
def test_fast_backward_is_deterministic(case):
    n, Hh, Wh = case
    d = _inputs(False, True, n, Hh, Wh, 512)
    r1, r2 = (_run_backward(d, True, n, Hh, Wh, 512, 0, "head_bwd512") for _ in range(2))
    assert all(torch.equal(r1[k], r2[k]) for k in r1), "two runs of the fp16 c = 512 backward differ"


@pytest.mark.parametrize("exact", [True, False], ids=["exact-head_bwd", "rounding-head_bwd"])
def test_fast_backward_scratch_too_small_falls_back(exact):
    """scratch one float short of n * bands * 8192: the generic kernels serve the call (float atomics: that scratch is too small for
    their partials as well; on the integer inputs atomics are exact too) and the results are still right"""
    n, Hh, Wh = 2, 13, 9
    d = _inputs(exact, True, n, Hh, Wh, 512)
    got = _run_backward(d, True, n, Hh, Wh, 512, 0, "head_bwd", scratch="short")
    _judge_backward(f"fast backward short scratch [head_bwd] exact={exact}", exact, True, got, _bwd_ref(exact, True, n, Hh, Wh, 512, 0, 0, True, True), n, (Hh - 3) * (Wh - 3))


def _tiny_forward():
    """a valid generic forward: afterwards gi_debug_last_kernel() says 'head_fwd'"""
    _run_forward(_inputs(True, False, 1, 4, 4, 4), False, 1, 4, 4, 4, 0, "head_fwd")


def _tiny_backward():
    _run_backward(_inputs(True, False, 1, 4, 4, 4), False, 1, 4, 4, 4, 0, "head_bwd")


def test_fast_backward_scratch_too_small_with_scale4_is_an_error():
    n, Hh, Wh = 2, 13, 9
    d = _inputs(True, True, n, Hh, Wh, 512, 2)
    sc, sh, npg = d["aff"]
    _tiny_forward()
    _run_backward(d, True, n, Hh, Wh, 512, 0, "head_bwd512", scratch="short", aff=(_vecs(sc, 512), _vecs(sh, 512), npg), expect_error=True)


# ================================================================ generic kernels ================================================
@pytest.fixture
def head_fast():
    """sets GI_HEAD_FAST for one test and puts the default back after it"""
    yield lambda v: B.set_option("GI_HEAD_FAST", v)
    B.set_option("GI_HEAD_FAST", -1)


@pytest.mark.parametrize("kind", ["exact", "rounding", "rounding-sigmoid"])
@pytest.mark.parametrize("Hh,Wh", GEN_MAPS, ids=[f"n2-{a}x{b}" for a, b in GEN_MAPS])
@pytest.mark.parametrize("g", GENERIC, ids=[g[0] + "-head_fwd" for g in GENERIC])
def test_generic_forward(g, Hh, Wh, kind, head_fast):
    name, fp16, c, off = g
    if off:
        head_fast(0)
    n, exact, sig = 2, kind == "exact", int(kind.endswith("sigmoid"))
    d = _inputs(exact, fp16, n, Hh, Wh, c)
    got = _run_forward(d, fp16, n, Hh, Wh, c, sig, "head_fwd", out2=sig == 0)
    _judge_forward(f"generic forward {name} {Hh}x{Wh} {kind} [head_fwd]", exact, got, _fwd_ref(exact, fp16, n, Hh, Wh, c, 0, False), c, (Hh - 3) * (Wh - 3), sig)


@pytest.mark.parametrize("kind", ["exact", "rounding", "rounding-sigmoid", "rounding-atomics", "exact-frozen"])
@pytest.mark.parametrize("Hh,Wh", GEN_MAPS, ids=[f"n2-{a}x{b}" for a, b in GEN_MAPS])
@pytest.mark.parametrize("g", GENERIC, ids=[g[0] + "-head_bwd" for g in GENERIC])
def test_generic_backward(g, Hh, Wh, kind, head_fast):
    name, fp16, c, off = g
    if off:
        head_fast(0)
    n, exact, sig = 2, kind.startswith("exact"), int(kind.endswith("sigmoid"))
    mode, scratch = ("frozen" if kind.endswith("frozen") else "grads"), (None if kind.endswith("atomics") else "ok")
    d = _inputs(exact, fp16, n, Hh, Wh, c, 0, sig)
    got = _run_backward(d, fp16, n, Hh, Wh, c, sig, "head_bwd", mode, scratch)
    _judge_backward(f"generic backward {name} {Hh}x{Wh} {kind} [head_bwd]", exact, fp16, got,
                    _bwd_ref(exact, fp16, n, Hh, Wh, c, 0, sig, True, mode == "grads"), n, (Hh - 3) * (Wh - 3))
    if kind == "rounding":      # the partials are added in a fixed order
        again = _run_backward(d, fp16, n, Hh, Wh, c, sig, "head_bwd", mode, scratch)
        assert torch.equal(got["dw5"], again["dw5"]) and torch.equal(got["da4"], again["da4"]), "two runs with scratch differ"


# ================================================================ host-side rejections ===========================================
@pytest.mark.parametrize("fp16,c", [(True, 512), (False, 24)], ids=["f16-c512", "f32-c24"])
def test_rejects_a_map_below_the_kernel(fp16, c):
    d = _inputs(True, fp16, 1, 3, 5, c)
    _tiny_backward()
    _run_forward(d, fp16, 1, 3, 5, c, 0, None, expect_error=True)
    _tiny_forward()
    _run_backward(d, fp16, 1, 3, 5, c, 0, "head_bwd", expect_error=True)


def test_rejects_a_map_over_the_lds_limit():
    """46 x 46 pixels need more than 160 KiB of LDS in the fp16 c = 512 forward"""
    d = _inputs(False, True, 1, 46, 46, 512)
    _tiny_backward()
    _run_forward(d, True, 1, 46, 46, 512, 0, None, expect_error=True)


def test_rejects_scale4_outside_the_fast_path(head_fast):
    d32 = _inputs(True, False, 2, 5, 7, 512, 1)
    d16 = _inputs(True, True, 2, 5, 7, 512, 1)
    for d, fp16, off in ((d32, False, False), (d16, True, True)):
        if off:
            head_fast(0)
        sc, sh, _ = d["aff"]
        _tiny_backward()
        _run_forward(d, fp16, 2, 5, 7, 512, 0, None, aff=(_vecs(sc, 512), _vecs(sh, 512), 0), expect_error=True)
        _tiny_forward()
        _run_backward(d, fp16, 2, 5, 7, 512, 0, "head_bwd", aff=(_vecs(sc, 512), _vecs(sh, 512), 0), expect_error=True)


def test_rejects_bn_without_scale4():
    c = 512
    d = _inputs(True, True, 2, 5, 7, c)
    acc = _acc_block(c)
    v = [Buf((c,), torch.float32, 1.0) for _ in range(8)]
    bn = B.BnAccArgs(acc=B.ptr(acc), reps=1, gamma=B.ptr(v[0].t), beta=B.ptr(v[1].t), running_mean=B.ptr(v[2].t), running_var=B.ptr(v[3].t),
                     scale=B.ptr(v[4].t), shift=B.ptr(v[5].t), save_mean=B.ptr(v[6].t), save_invstd=B.ptr(v[7].t), count=70, momentum=0.1,
                     eps=1e-5, groups=1, out_stride=c, zero_next=None, zero_words=0)
    _tiny_backward()
    _run_forward(d, True, 2, 5, 7, c, 0, None, bn=bn, expect_error=True)
    assert all(bool((b.t == 1.0).all()) and b.guards_intact() for b in v), "a rejected call touched the BatchNorm vectors"


def test_rejects_dw5_without_dwl():
    n, Hh, Wh, c = 2, 5, 7, 512
    d = _inputs(True, True, n, Hh, Wh, c)
    P = (Hh - 3) * (Wh - 3)
    a4, w5, wl, hh, oo, dy = _in(d["a4"], torch.float16), _in(d["w5"]), _in(d["wl"]), _in(d["h"]), _in(d["out"]), _in(d["dy"])
    da4, dh, dw5, dbl = Buf((n, Hh, Wh, c), torch.float16), Buf((n, P), torch.float32), Buf((16, c), torch.float32), Buf((1,), torch.float32)
    sb = Buf((n * 8192,), torch.float32, NAN)
    a = B.HeadBwdArgs(a4=B.ptr(a4.t), w5=B.ptr(w5.t), wl=B.ptr(wl.t), h=B.ptr(hh.t), out=B.ptr(oo.t), dy=B.ptr(dy.t), da4=B.ptr(da4.t),
                      dw5=B.ptr(dw5.t), dwl=None, dbl=B.ptr(dbl.t), dh=B.ptr(dh.t), n=n, Hh=Hh, Wh=Wh, c=c, sigmoid=0, loss_scale=LS,
                      scratch=B.ptr(sb.t), scratch_bytes=n * 8192 * 4, bwd_reps=1, bwd_slope=1.0)
    _tiny_forward()
    assert B.lib().gi_debug_head_backward(B.get_ctx(), F16, C.byref(a)) != 0
    _sync()
    assert B.last_kernel() == "head_fwd", "a rejected call launched a kernel"
    assert all(bool((b.t == SENT).all()) and b.guards_intact() for b in (da4, dh, dw5, dbl)) and bool(torch.isnan(sb.t).all())
