"""GPU tier: every kernel of csrc/c1.hip that serves a layer with one channel on its large side, ONE LAYER AT A TIME through the
C-ABI seam (gi_c1_gather / gi_c1_scatter / gi_c1_wgrad / gi_c1_wgrad_reduce / gi_c1_head4_*), against the fp64 references of
tests/c1_ref.py, with an assertion on WHICH kernel served the shape (gi_debug_last_kernel). Two kinds of test per variant:

  exact     small-integer inputs (powers of two for the scales): every product, every fp16 col value and every fp32 sum is exact,
            so the result must EQUAL the reference - a wrong tap, padding, fragment, swizzle, prefetch register or band halo shows
            as a non-zero difference, in fp16 as in fp32. tanh is not exact: the head4 forward, which always applies it, is judged
            on exact pre-activations with the tanhf allowance alone.
  rounding  uniform random inputs already rounded to the compute type: |err| <= the per-element bound derived in c1_ref.py
            (tests/test_c1_ref_cpu.py shows on the same inputs that arithmetic of this kind stays inside it and comes near it).

Every output element is judged. Buffers are wide where the kernel takes a pitch: the channels outside the written range, the row
tails and guard zones around every written buffer must keep their sentinel; the parts of the inputs no kernel may read are NaN.
The shapes are the smallest that reach each hazard: one 16- or 32-pixel group per row (left and right padding in one group),
rows that are no multiple of the tile, ragged last row bands, pixel counts that leave a partial group, and one case per
grid-capped persistent loop that makes it wrap."""
import ctypes as C

import pytest
import torch

pytestmark = pytest.mark.gpu

import c1_ref as R  # noqa: E402
from gpu_util import B, record, tdt  # noqa: E402

F16, F32 = B.GI_F16, B.GI_F32
SENT = -777.0          # an fp16 number no test produces
GUARD = 1024           # elements before and after every written buffer


def _code(fp16):
    return F16 if fp16 else F32


class Buf:
    """a device buffer of `shape` between two guard zones, all filled with `fill`"""

    def __init__(self, shape, dtype, fill=SENT):
        numel = 1
        for s in shape:
            numel *= s
        self.full = torch.full((numel + 2 * GUARD,), fill, dtype=dtype, device="cuda")
        self.t = self.full[GUARD:GUARD + numel].view(shape)
        self.fill = fill

    def guards_intact(self):
        g = torch.cat([self.full[:GUARD], self.full[-GUARD:]])
        return bool(torch.isnan(g).all()) if self.fill != self.fill else bool((g == self.fill).all())


def _wide_in(x, code, wide, dead_upper=False):
    """x (..., c) on the CPU -> device buffer (P, ld) of the compute type, NaN wherever no kernel may read; returns it, ld, coff"""
    c = x.shape[-1]
    ld, coff = (2 * c, c) if wide else (c, 0)
    buf = torch.full((x.numel() // c, ld), float("nan"), dtype=tdt(code), device="cuda")
    live = c // 2 if dead_upper else c       # the affine form never reads channels [c/2, c) of X
    buf[:, coff:coff + live] = x.reshape(-1, c)[:, :live].to(tdt(code)).cuda()
    return buf, ld, coff


def _aff_dev(aff, c):
    """(x2, scale2, shift2) on the device, x2 with a row pitch above c/2 and a NaN tail"""
    if aff is None:
        return None, 0, None, None
    x2, sc, sh = aff
    ld2 = c // 2 + 8
    buf = torch.full((x2.numel() // (c // 2), ld2), float("nan"), dtype=torch.float16, device="cuda")
    buf[:, :c // 2] = x2.reshape(-1, c // 2).half().cuda()
    return buf, ld2, sc.float().cuda(), sh.float().cuda()


def _untouched(buf2d, coff, c):
    """the columns outside [coff, coff + c) of a (P, ld) output still hold the sentinel"""
    return bool((buf2d[:, :coff] == SENT).all()) and bool((buf2d[:, coff + c:] == SENT).all())


def _exact(what, got, ref, dtype):
    """torch.equal against the fp64 reference brought to the output type (fp64 -> fp32 -> type: the kernels round an fp32 value)"""
    want = ref.to(torch.float32).to(dtype)
    if not torch.equal(got, want):
        d = (got.double() - want.double()).abs()
        idx = tuple(int(i) for i in (d == d.max()).nonzero()[0])
        raise AssertionError(f"{what}: {int((d != 0).sum())} of {d.numel()} elements differ, worst {float(d.max()):.6g} at {idx}: "
                             f"got {float(got[idx])} want {float(want[idx])}")


def _rounding(what, got, ref, bound):
    ratio = R.worst_ratio(got.double() - ref, bound)
    print(f"{what}: worst err / bound = {ratio:.4f}")
    record(f"c1 {what}", ratio)
    assert ratio <= 1.0, f"{what}: error {ratio:.3f} times the bound"


def _sign_words(y):
    """one 64-bit word per pixel, bit c = [y[p][c] > 0], as 8 bytes (little endian): tests/test_dispatch_gpu.py::_sign_words"""
    pos = (y[..., :64] > 0).to(torch.int32).reshape(-1, 8, 8)
    return (pos << torch.arange(8, device=pos.device, dtype=torch.int32)).sum(-1).to(torch.uint8).contiguous()


# ================================================================ gather =========================================================
def _run_gather(fp16, img, w, bias, act, in_scale, wide, kernel):
    """-> the (n, Hs, Ws, c) output on the CPU in its own type; asserts the kernel, the sentinels and the sign words"""
    code = _code(fp16)
    n, H, W = img.shape
    Hs, Ws, c = H // 2, W // 2, w.shape[0]
    P = n * Hs * Ws
    ld, coff = (2 * c, c) if wide else (c, 0)
    out = Buf((P, ld), tdt(code))
    bits = Buf((P * 8,), torch.uint8, 0xA5)
    written = C.c_int(-1)
    imgd, wd, bd = img.float().cuda(), w.float().cuda(), None if bias is None else bias.float().cuda()
    B.check(B.lib().gi_c1_gather(B.get_ctx(), code, B.ptr(imgd), B.ptr(wd), B.ptr(out.t), n, Hs, Ws, c, ld, coff, act, in_scale,
                                 B.ptr(bd), B.ptr(bits.t), C.byref(written)))
    torch.cuda.synchronize()
    assert B.last_kernel() == kernel, (B.last_kernel(), kernel)
    assert out.guards_intact() and bits.guards_intact() and _untouched(out.t, coff, c), "gather wrote outside its channels"
    y = out.t[:, coff:coff + c]
    if kernel == "c1_gather_mfma<4>":
        assert written.value == 1
        assert torch.equal(bits.t.view(P, 8), _sign_words(y)), "sign words differ from the signs of the kernel's own output"
    else:
        assert written.value == 0 and bool((bits.t == 0xA5).all()), "sign words written by a form that does not announce them"
    return y.cpu().reshape(n, Hs, Ws, c)


# (id, fp16, n, Hs, Ws, c, bias, act, in_scale, wide, kernel); the last three of each family make its persistent loop wrap
GATHER_EXACT = [
    ("mfma64-1group-none", True, 2, 3, 16, 64, False, R.ACT_NONE, 1.0, False, "c1_gather_mfma<4>"),
    ("mfma64-1group-relu", True, 2, 3, 16, 64, False, R.ACT_RELU, 1.0, True, "c1_gather_mfma<4>"),
    ("mfma64-1group-lrelu", True, 2, 3, 16, 64, False, R.ACT_LRELU, 0.5, False, "c1_gather_mfma<4>"),
    ("mfma128-1group-none", True, 2, 3, 16, 128, False, R.ACT_NONE, 0.5, True, "c1_gather_mfma<8>"),
    ("mfma128-1group-relu", True, 2, 3, 16, 128, False, R.ACT_RELU, 1.0, False, "c1_gather_mfma<8>"),
    ("mfma128-1group-lrelu", True, 2, 3, 16, 128, False, R.ACT_LRELU, 1.0, False, "c1_gather_mfma<8>"),
    ("mfma64-gpr3", True, 3, 5, 48, 64, False, R.ACT_LRELU, 1.0, True, "c1_gather_mfma<4>"),
    ("mfma128-gpr3", True, 3, 5, 48, 128, False, R.ACT_NONE, 1.0, True, "c1_gather_mfma<8>"),
    ("mfma64-wrap", True, 3, 256, 256, 64, False, R.ACT_LRELU, 1.0, False, "c1_gather_mfma<4>"),           # 12288 groups > 8192 waves
    ("strip32-f32-64", False, 2, 3, 32, 64, False, R.ACT_NONE, 1.0, True, "c1_gather_strip"),
    ("strip96-f32-64", False, 2, 3, 96, 64, True, R.ACT_LRELU, 0.5, False, "c1_gather_strip"),
    ("strip-f16-64-bias", True, 2, 3, 32, 64, True, R.ACT_RELU, 1.0, True, "c1_gather_strip"),
    ("strip-f16-32", True, 2, 3, 64, 32, False, R.ACT_NONE, 1.0, False, "c1_gather_strip"),
    ("strip-f16-256", True, 2, 3, 16, 256, False, R.ACT_LRELU, 1.0, True, "c1_gather_strip"),
    ("strip-f32-wrap", False, 3, 700, 32, 64, True, R.ACT_NONE, 1.0, False, "c1_gather_strip"),             # 2100 strips > 2048 workgroups
    ("generic24-f32", False, 2, 3, 24, 64, False, R.ACT_NONE, 1.0, True, "c1_gather"),
    ("generic24-f32-bias", False, 2, 3, 24, 64, True, R.ACT_RELU, 0.5, False, "c1_gather"),
    ("generic20-f32", False, 2, 5, 20, 128, True, R.ACT_LRELU, 1.0, False, "c1_gather"),
    ("generic20-f32-nobias", False, 2, 5, 20, 128, False, R.ACT_NONE, 1.0, True, "c1_gather"),
    ("generic24-f16", True, 2, 3, 24, 64, False, R.ACT_LRELU, 1.0, True, "c1_gather"),
    ("generic24-f16-bias", True, 2, 3, 24, 64, True, R.ACT_NONE, 1.0, False, "c1_gather"),
    ("generic20-f16", True, 2, 5, 20, 128, False, R.ACT_RELU, 0.5, True, "c1_gather"),
    ("generic20-f16-bias", True, 2, 5, 20, 128, True, R.ACT_LRELU, 1.0, False, "c1_gather"),
    ("generic1x1-f32", False, 3, 1, 1, 64, True, R.ACT_NONE, 1.0, True, "c1_gather"),
    ("generic1x1-f16", True, 3, 1, 1, 64, False, R.ACT_NONE, 1.0, False, "c1_gather"),
    ("generic-f16-wrap", True, 2, 270, 250, 64, True, R.ACT_NONE, 1.0, False, "c1_gather"),                # 135000 * 8 threads > 2^20
]


@pytest.mark.parametrize("case", GATHER_EXACT, ids=[c[0] for c in GATHER_EXACT])
def test_gather_exact(case):
    name, fp16, n, Hs, Ws, c, bias, act, in_scale, wide, kernel = case
    img, w, b = R.gather_inputs(True, fp16, n, Hs, Ws, c, bias, R.SEED)
    ref, _ = R.gather_ref(img, w, b, act, in_scale)
    got = _run_gather(fp16, img, w, b, act, in_scale, wide, kernel)
    _exact(f"gather {name}", got, ref, tdt(_code(fp16)))


@pytest.mark.parametrize("case", R.GATHER_ROUNDING, ids=[c[0] for c in R.GATHER_ROUNDING])
def test_gather_rounding(case):
    fp16, n, Hs, Ws, c, bias, act, in_scale, kernel = case[1]
    img, w, b = R.gather_inputs(False, fp16, n, Hs, Ws, c, bias, R.SEED)
    ref, A = R.gather_ref(img, w, b, act, in_scale)
    got = _run_gather(fp16, img, w, b, act, in_scale, True, kernel)
    _rounding(f"gather {case[0]} [{kernel}]", got, ref, R.bound_gather(fp16, ref, A))


# ================================================================ scatter ========================================================
def _run_scatter(fp16, X, w, bias, relu_in, post, out_scale, aff, col, wide, kernel, second=True):
    """-> (n, 2Hs, 2Ws) fp32 on the CPU; asserts the kernel, that img2 equals img bit for bit and the guard zones"""
    code = _code(fp16)
    n, Hs, Ws, c = X.shape
    xd, ld, coff = _wide_in(X, code, wide, dead_upper=aff is not None)
    x2, ld2, sc, sh = _aff_dev(aff, c)
    img, img2 = Buf((n, 2 * Hs, 2 * Ws), torch.float32), Buf((n, 2 * Hs, 2 * Ws), torch.float32)
    cols = Buf((n * Hs * Ws * 16,), torch.float16) if col else None
    wd, bd = w.float().cuda(), None if bias is None else bias.float().cuda()
    B.check(B.lib().gi_c1_scatter(B.get_ctx(), code, B.ptr(xd), B.ptr(wd), B.ptr(bd), B.ptr(img.t), n, Hs, Ws, c, ld, coff, relu_in, post,
                                  out_scale, B.ptr(cols.t) if col else None, B.ptr(img2.t) if second else None, B.ptr(x2), ld2, B.ptr(sc), B.ptr(sh)))
    torch.cuda.synchronize()
    assert B.last_kernel() == kernel, (B.last_kernel(), kernel)
    assert img.guards_intact() and img2.guards_intact() and (cols is None or cols.guards_intact()), "scatter wrote outside its buffers"
    if second:
        assert torch.equal(img.t, img2.t), "the second copy of the output differs"
    else:
        assert bool((img2.t == SENT).all())
    return img.t.cpu()


@pytest.fixture
def c1_fused():
    """sets GI_C1_FUSED for one test and restores the default after it"""
    yield lambda v: B.set_option("GI_C1_FUSED", v)
    B.set_option("GI_C1_FUSED", -1)


# (id, fp16, n, Hs, Ws, c, bias, relu_in, out_scale, affine, col_scratch, wide, kernel); post = 0 (tanh is not exact)
SCATTER_EXACT = [
    ("fused2-1row", True, 2, 1, 16, 64, False, 0, 1.0, False, True, False, "c1_scatter_fused<2>"),
    ("fused4-1row", True, 2, 1, 16, 128, True, 1, 1.0, False, True, True, "c1_scatter_fused<4>"),
    ("fused2-2bands", True, 2, 24, 64, 64, True, 1, 1.0 / 1024, False, True, True, "c1_scatter_fused<2>"),      # TH = 16: 16 + 8 rows
    ("fused4-2bands", True, 2, 24, 64, 128, False, 0, 1.0, False, True, False, "c1_scatter_fused<4>"),
    ("fused2-3bands", True, 1, 10, 256, 64, False, 0, 1.0, False, True, False, "c1_scatter_fused<2>"),          # TH = 4: 4 + 4 + 2 rows
    ("fused4-3bands", True, 1, 10, 256, 128, True, 1, 1.0, False, True, True, "c1_scatter_fused<4>"),
    ("fused2-th21", True, 3, 7, 48, 64, True, 0, 1.0, False, True, True, "c1_scatter_fused<2>"),                # TH = 21 > Hs
    ("fused4-th21", True, 3, 7, 48, 128, False, 1, 1.0 / 1024, False, True, False, "c1_scatter_fused<4>"),
    ("fused2-affine", True, 2, 3, 32, 64, True, 0, 1.0, True, True, True, "c1_scatter_fused<2>"),
    ("fused4-affine", True, 1, 5, 64, 128, False, 0, 1.0, True, True, False, "c1_scatter_fused<4>"),
    ("col2-ws24", True, 1, 5, 24, 64, True, 1, 1.0, False, True, True, "c1_col+col2im<2>"),                     # P = 120 = 7 * 16 + 8
    ("col4-ws24", True, 3, 3, 24, 128, False, 0, 1.0 / 1024, False, True, False, "c1_col+col2im<4>"),           # P = 216 = 13 * 16 + 8
    ("col2-ws512", True, 1, 2, 512, 64, False, 0, 1.0, False, True, False, "c1_col+col2im<2>"),                 # 4 rows of 512 do not fit LDS
    ("col4-ws512", True, 1, 2, 512, 128, True, 1, 1.0, False, True, True, "c1_col+col2im<4>"),
    ("col2-wrap", True, 2, 2741, 24, 64, True, 1, 1.0, False, True, False, "c1_col+col2im<2>"),                 # 8223 groups > 8192 waves
    ("scalar-f32-16", False, 2, 3, 5, 16, True, 0, 1.0, False, False, True, "c1_scatter"),                      # 30 pixels, 64 per workgroup
    ("scalar-f32-64", False, 2, 3, 5, 64, False, 1, 1.0 / 1024, False, False, False, "c1_scatter"),             # 16 per workgroup
    ("scalar-f32-256", False, 1, 3, 7, 256, True, 1, 1.0, False, True, True, "c1_scatter"),                     # 4 per workgroup, 21 pixels
    ("scalar-f16-32", True, 2, 3, 5, 32, True, 1, 1.0, False, True, True, "c1_scatter"),
    ("scalar-f16-512", True, 1, 3, 7, 512, False, 0, 1.0, False, True, False, "c1_scatter"),
    ("scalar-f16-64-noscratch", True, 2, 3, 16, 64, True, 0, 1.0, False, False, True, "c1_scatter"),
]


@pytest.mark.parametrize("case", SCATTER_EXACT, ids=[c[0] for c in SCATTER_EXACT])
def test_scatter_exact(case):
    name, fp16, n, Hs, Ws, c, bias, relu_in, out_scale, affine, col, wide, kernel = case
    X, w, b, aff = R.scatter_inputs(True, fp16, n, Hs, Ws, c, bias, R.SEED, affine)
    r = R.scatter_ref(X, w, b, relu_in, 0, out_scale, aff)
    got = _run_scatter(fp16, X, w, b, relu_in, 0, out_scale, aff, col, wide, kernel)
    _exact(f"scatter {name}", got, r["value"], torch.float32)


FUSED_CASES = [c for c in SCATTER_EXACT if c[-1].startswith("c1_scatter_fused")]


@pytest.mark.parametrize("case", FUSED_CASES, ids=[c[0] for c in FUSED_CASES])
@pytest.mark.parametrize("exact", [True, False], ids=["integers", "random"])
def test_scatter_unfused_equals_fused(case, exact, c1_fused):
    """GI_C1_FUSED = 0 at the shapes of the fused kernel: the col tensor and the overlap-add launch, the same fp16 rounding of col
    and the same order of additions - bit-identical output (the kernel comment's own claim), tanh included"""
    name, fp16, n, Hs, Ws, c, bias, relu_in, out_scale, affine, col, wide, kernel = case
    X, w, b, aff = R.scatter_inputs(exact, fp16, n, Hs, Ws, c, bias, R.SEED + 1, affine)
    post = 0 if exact else 1
    r = R.scatter_ref(X, w, b, relu_in, post, out_scale, aff)
    on = _run_scatter(fp16, X, w, b, relu_in, post, out_scale, aff, col, wide, kernel)
    c1_fused(0)
    off = _run_scatter(fp16, X, w, b, relu_in, post, out_scale, aff, col, wide, f"c1_col+col2im<{c // 32}>", second=False)
    assert torch.equal(on, off), f"{name}: fused and two-launch forms differ at {int((on != off).sum())} elements"
    if exact:
        _exact(f"scatter {name} unfused", off, r["value"], torch.float32)
    else:
        _rounding(f"scatter {name} unfused random [c1_col+col2im<{c // 32}>]", off, r["value"], R.bound_scatter("col", r, c, post, out_scale))


@pytest.mark.parametrize("case", R.SCATTER_ROUNDING, ids=[c[0] for c in R.SCATTER_ROUNDING])
def test_scatter_rounding(case, c1_fused):
    """post = 1: the pre-activation bound (tanh is 1-Lipschitz) plus 2^-22 for tanhf itself"""
    fp16, n, Hs, Ws, c, bias, relu_in, post, out_scale, affine, col, fused, kind, kernel = case[1]
    X, w, b, aff = R.scatter_inputs(False, fp16, n, Hs, Ws, c, bias, R.SEED, affine)
    r = R.scatter_ref(X, w, b, relu_in, post, out_scale, aff)
    if not fused:
        c1_fused(0)
    got = _run_scatter(fp16, X, w, b, relu_in, post, out_scale, aff, col, True, kernel)
    _rounding(f"scatter {case[0]} [{kernel}]", got, r["value"], R.bound_scatter(kind, r, c, post, out_scale))


# ================================================================ weight gradient ================================================
def _run_wgrad(fp16, X, img, relu_in, scale, img_scale, aff, scratch, wide, kernel, dW0=0.0):
    code = _code(fp16)
    n, Hs, Ws, c = X.shape
    xd, ld, coff = _wide_in(X, code, wide, dead_upper=aff is not None)
    x2, ld2, sc, sh = _aff_dev(aff, c)
    dW = Buf((c, 16), torch.float32, dW0)
    ws = Buf((1024 * c * 16,), torch.float32, float("nan")) if scratch else None
    imgd = img.float().cuda()
    B.check(B.lib().gi_c1_wgrad(B.get_ctx(), code, B.ptr(xd), B.ptr(imgd), B.ptr(dW.t), n, Hs, Ws, c, ld, coff, relu_in, scale, img_scale,
                                B.ptr(x2), ld2, B.ptr(sc), B.ptr(sh), B.ptr(ws.t) if scratch else None, 1024 * c * 16 if scratch else 0))
    torch.cuda.synchronize()
    assert B.last_kernel() == kernel, (B.last_kernel(), kernel)
    assert dW.guards_intact() and (ws is None or ws.guards_intact()), "wgrad wrote outside its buffers"
    return dW.t.cpu()


# (id, fp16, n, Hs, Ws, c, relu_in, scale, img_scale, affine, wide, range, kernel without ",atomics")
WGRAD_EXACT = [
    ("mfma64-1tile", True, 1, 1, 32, 64, 0, 1.0, 1.0, False, False, 2, "c1_wgrad_mfma"),              # three idle waves
    ("mfma128-1tile", True, 1, 1, 32, 128, 1, 0.25, 0.5, False, True, 2, "c1_wgrad_mfma"),
    ("mfma64-rows", True, 2, 3, 32, 64, 1, 1.0, 1.0, False, True, 2, "c1_wgrad_mfma"),                # one tile per row
    ("mfma128-rows", True, 2, 3, 32, 128, 0, 1.0, 1.0, False, False, 2, "c1_wgrad_mfma"),
    ("mfma64-ws96", True, 3, 5, 96, 64, 0, 0.25, 0.5, False, False, 2, "c1_wgrad_mfma"),
    ("mfma128-ws96", True, 3, 5, 96, 128, 1, 1.0, 1.0, False, True, 2, "c1_wgrad_mfma"),
    ("mfma64-affine", True, 2, 3, 32, 64, 0, 1.0, 1.0, True, True, 2, "c1_wgrad_mfma"),
    ("mfma128-affine", True, 1, 5, 64, 128, 0, 0.25, 1.0, True, False, 2, "c1_wgrad_mfma"),
    ("mfma64-wrap", True, 5, 128, 128, 64, 1, 1.0, 1.0, False, False, 8, "c1_wgrad_mfma"),            # 2560 tiles > 2048 waves; sums < 2^24
    ("scalar-f16-ws24", True, 1, 3, 24, 64, 1, 1.0, 1.0, False, True, 2, "c1_wgrad"),
    ("scalar-f32-ws24", False, 1, 3, 24, 64, 0, 0.25, 0.5, False, False, 2, "c1_wgrad"),
    ("scalar-f32-8x32", False, 2, 8, 32, 64, 1, 1.0, 1.0, False, True, 2, "c1_wgrad"),
    ("scalar-f32-1x1", False, 3, 1, 1, 16, 0, 1.0, 1.0, False, False, 2, "c1_wgrad"),
    ("scalar-f16-1x1", True, 3, 1, 1, 32, 0, 1.0, 1.0, False, True, 2, "c1_wgrad"),
]


@pytest.mark.parametrize("scratch", [True, False], ids=["scratch", "atomics"])
@pytest.mark.parametrize("case", WGRAD_EXACT, ids=[c[0] for c in WGRAD_EXACT])
def test_wgrad_exact(case, scratch):
    """integers: float atomics in any order and the fixed-order partial sums both give the exact sum; dW holds 1.0 before the call
    and 1 + ref after it (dW += ...); with the scratch buffer two runs are bit-identical"""
    name, fp16, n, Hs, Ws, c, relu_in, scale, img_scale, affine, wide, rng, kernel = case
    X, img, aff = R.wgrad_inputs(True, fp16, n, Hs, Ws, c, R.SEED, affine, rng)
    ref, A = R.wgrad_ref(X, img, relu_in, scale, img_scale, aff)
    assert float(A.max()) / abs(scale) < 2 ** 24
    kernel = kernel if scratch else kernel + ",atomics"
    got = _run_wgrad(fp16, X, img, relu_in, scale, img_scale, aff, scratch, wide, kernel, dW0=1.0)
    _exact(f"wgrad {name}", got, 1.0 + ref, torch.float32)
    if scratch:
        assert torch.equal(got, _run_wgrad(fp16, X, img, relu_in, scale, img_scale, aff, scratch, wide, kernel, dW0=1.0))


@pytest.mark.parametrize("case", R.WGRAD_ROUNDING, ids=[c[0] for c in R.WGRAD_ROUNDING])
def test_wgrad_rounding(case):
    fp16, n, Hs, Ws, c, relu_in, scale, img_scale, affine, scratch, kernel = case[1]
    X, img, aff = R.wgrad_inputs(False, fp16, n, Hs, Ws, c, R.SEED, affine)
    ref, A = R.wgrad_ref(X, img, relu_in, scale, img_scale, aff)
    got = _run_wgrad(fp16, X, img, relu_in, scale, img_scale, aff, scratch, True, kernel)
    _rounding(f"wgrad {case[0]} [{kernel}]", got, ref, R.bound_fp32(n * Hs * Ws, A))
    if scratch:
        assert torch.equal(got, _run_wgrad(fp16, X, img, relu_in, scale, img_scale, aff, scratch, True, kernel)), "fixed-order sums differ between runs"


def _run_reduce(part, dW0, scratch):
    count = part.shape[1]
    dW = Buf((count,), torch.float32)
    dW.t.copy_(dW0)
    ws = Buf((64 * count,), torch.float32, float("nan")) if scratch else None
    pd = part.float().cuda()
    B.check(B.lib().gi_c1_wgrad_reduce(B.get_ctx(), B.ptr(pd), B.ptr(dW.t), count, part.shape[0], B.ptr(ws.t) if scratch else None,
                                       64 * count if scratch else 0))
    torch.cuda.synchronize()
    assert dW.guards_intact() and (ws is None or ws.guards_intact()), "wgrad_reduce wrote outside its buffers"
    return dW.t.cpu()


@pytest.mark.parametrize("scratch", [False, True], ids=["direct", "scratch"])
@pytest.mark.parametrize("blocks", [1, 15, 16, 17, 255, 256, 300, 2048])
@pytest.mark.parametrize("count", [1024, 2048, 20])
def test_wgrad_reduce_exact(count, blocks, scratch):
    """integer rows onto an integer dW (dW += ...): 256 rows or more with the scratch buffer go through c1_wgrad_rows_kernel first;
    count = 20 leaves the second workgroup of c1_wgrad_reduce_kernel partial, blocks < 16 and blocks % 16 != 0 its row ranges"""
    part, dW0 = R.reduce_inputs(True, count, blocks, R.SEED)
    ref, _ = R.reduce_ref(part, dW0)
    _exact(f"wgrad_reduce {count}x{blocks}", _run_reduce(part, dW0, scratch), ref, torch.float32)


@pytest.mark.parametrize("case", R.REDUCE_ROUNDING, ids=[c[0] for c in R.REDUCE_ROUNDING])
def test_wgrad_reduce_rounding(case):
    count, blocks, scratch = case[1]
    part, dW0 = R.reduce_inputs(False, count, blocks, R.SEED)
    ref, A = R.reduce_ref(part, dW0)
    _rounding(f"wgrad_reduce {case[0]}", _run_reduce(part, dW0, scratch), ref, R.bound_fp32(blocks, A))


# ================================================================ the 4-class head ===============================================
def _run_head4_forward(X, w4, bias, relu_in, second):
    n, Hs, Ws, c = X.shape
    xd, ld, coff = _wide_in(X, F16, True)
    out, out2 = Buf((n, 4, 2 * Hs, 2 * Ws), torch.float32), Buf((n, 4, 2 * Hs, 2 * Ws), torch.float32)
    nbytes = B.lib().gi_c1_head4_col_bytes(n, Hs, Ws)
    assert nbytes == n * Hs * Ws * 16 * 4 * 2
    col = Buf((nbytes // 2,), torch.float16)
    wd, bd = w4.float().contiguous().cuda(), bias.float().cuda()
    B.check(B.lib().gi_c1_head4_forward(B.get_ctx(), B.ptr(xd), B.ptr(wd), B.ptr(bd), B.ptr(out.t), B.ptr(out2.t) if second else None, n, Hs, Ws,
                                        ld, coff, relu_in, B.ptr(col.t)))
    torch.cuda.synchronize()
    assert B.last_kernel() == "c1_head4"
    assert out.guards_intact() and out2.guards_intact() and col.guards_intact(), "head4 forward wrote outside its buffers"
    assert torch.equal(out.t, out2.t) if second else bool((out2.t == SENT).all())
    return out.t.cpu()


@pytest.mark.parametrize("second", [True, False], ids=["out+out2", "out"])
@pytest.mark.parametrize("relu_in", [0, 1])
@pytest.mark.parametrize("case", R.HEAD4_MAPS, ids=[c[0] for c in R.HEAD4_MAPS])
def test_head4_forward_exact_preactivation(case, relu_in, second):
    """integers times powers of two: the pre-activation is exact, the whole error is tanhf's - at most the allowance"""
    n, Hs, Ws = case[1]
    X, w4, b, _ = R.head4_inputs(True, n, Hs, Ws, R.SEED)
    r = R.head4_forward_ref(X, w4, b, relu_in)
    got = _run_head4_forward(X, w4, b, relu_in, second)
    _rounding(f"head4 forward {case[0]} relu_in={relu_in} exact pre-activation, tanhf alone", got, r["value"], torch.full_like(r["value"], R.TANH_ALLOWANCE))


@pytest.mark.parametrize("relu_in", [0, 1])
@pytest.mark.parametrize("case", R.HEAD4_MAPS, ids=[c[0] for c in R.HEAD4_MAPS])
def test_head4_forward_rounding(case, relu_in):
    n, Hs, Ws = case[1]
    X, w4, b, _ = R.head4_inputs(False, n, Hs, Ws, R.SEED)
    r = R.head4_forward_ref(X, w4, b, relu_in)
    got = _run_head4_forward(X, w4, b, relu_in, True)
    _rounding(f"head4 forward {case[0]} relu_in={relu_in} [c1_head4]", got, r["value"], R.bound_scatter("col", r, 128, 1, 1.0))


def _run_head4_dgrad(g, w4):
    n, _, H, W = g.shape
    Hs, Ws, c = H // 2, W // 2, w4.shape[0]
    out = Buf((n * Hs * Ws, 256), torch.float16)
    gd, wd = g.float().contiguous().cuda(), w4.float().contiguous().cuda()
    B.check(B.lib().gi_c1_head4_dgrad(B.get_ctx(), B.ptr(gd), B.ptr(wd), B.ptr(out.t), n, Hs, Ws, 256, 128))
    torch.cuda.synchronize()
    assert B.last_kernel() == "c1_head4_dgrad"
    assert out.guards_intact() and _untouched(out.t, 128, c), "head4 dgrad wrote outside its channels"
    return out.t[:, 128:128 + c].cpu().reshape(n, Hs, Ws, c)


HEAD4_DGRAD_MAPS = R.HEAD4_MAPS + [("wrap", (2, 260, 256))]       # 8320 pixel groups > 8192 waves: the prefetch loop runs twice


@pytest.mark.parametrize("case", HEAD4_DGRAD_MAPS, ids=[c[0] for c in HEAD4_DGRAD_MAPS])
def test_head4_dgrad_exact(case):
    n, Hs, Ws = case[1]
    _, _, _, g = R.head4_inputs(True, n, Hs, Ws, R.SEED)
    w4 = R.ints((128, 16, 4), R.SEED + 1)
    _exact(f"head4 dgrad {case[0]}", _run_head4_dgrad(g, w4), R.head4_dgrad_ref(g, w4)[0], torch.float16)


@pytest.mark.parametrize("case", R.HEAD4_MAPS, ids=[c[0] for c in R.HEAD4_MAPS])
def test_head4_dgrad_rounding(case):
    n, Hs, Ws = case[1]
    _, w4, _, g = R.head4_inputs(False, n, Hs, Ws, R.SEED)
    ref, A = R.head4_dgrad_ref(g, w4)
    _rounding(f"head4 dgrad {case[0]} [c1_head4_dgrad]", _run_head4_dgrad(g, w4), ref, R.bound_gather(True, ref, A, 64))


# ================================================================ what the dispatchers refuse ====================================
def test_gather_refuses_channel_counts_it_cannot_split():
    """c / 8 = 24 is no power of two: the generic form (reached at Ws = 24) would mis-split its thread index; c = 12 is no multiple
    of 8. Both are errors and nothing is launched."""
    for c in (192, 12):
        for fp16 in (False, True):
            code = _code(fp16)
            out = Buf((2 * 3 * 24, c), tdt(code))
            img, w = torch.ones(2, 6, 48, device="cuda"), torch.ones(c, 16, device="cuda")
            rc = B.lib().gi_c1_gather(B.get_ctx(), code, B.ptr(img), B.ptr(w), B.ptr(out.t), 2, 3, 24, c, c, 0, 0, 1.0, None, None, None)
            torch.cuda.synchronize()
            assert rc != 0 and B.lib().gi_last_error(), (c, fp16, rc)
            assert bool((out.full == SENT).all()), "a refused gather wrote its output"


def test_affine_form_refuses_rows_that_are_no_multiple_of_32():
    n, Hs, Ws, c = 1, 2, 48, 64
    X, w, b, aff = R.scatter_inputs(True, True, n, Hs, Ws, c, False, R.SEED, affine=True)
    xd, ld, coff = _wide_in(X, F16, False, dead_upper=True)
    x2, ld2, sc, sh = _aff_dev(aff, c)
    img, col, dW = Buf((n, 2 * Hs, 2 * Ws), torch.float32), Buf((n * Hs * Ws * 16,), torch.float16), Buf((c, 16), torch.float32)
    wd = w.cuda()
    rc = B.lib().gi_c1_scatter(B.get_ctx(), F16, B.ptr(xd), B.ptr(wd), None, B.ptr(img.t), n, Hs, Ws, c, ld, coff, 0, 0, 1.0, B.ptr(col.t), None,
                               B.ptr(x2), ld2, B.ptr(sc), B.ptr(sh))
    torch.cuda.synchronize()
    assert rc != 0 and bool((img.full == SENT).all()) and bool((col.full == SENT).all())
    imgd = torch.ones(n, 2 * Hs, 2 * Ws, device="cuda")
    rc = B.lib().gi_c1_wgrad(B.get_ctx(), F16, B.ptr(xd), B.ptr(imgd), B.ptr(dW.t), n, Hs, Ws, c, ld, coff, 0, 1.0, 1.0, B.ptr(x2), ld2, B.ptr(sc),
                             B.ptr(sh), None, 0)
    torch.cuda.synchronize()
    assert rc != 0 and bool((dW.full == SENT).all())
