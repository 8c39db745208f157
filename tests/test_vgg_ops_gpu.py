"""GPU tier: the kernels of the VGG-19 perceptual / style loss path (csrc/vgg.hip and the 3x3 mode of igemm3 / igemm5 / igemm8) ONE OP
AT A TIME through the gi_debug_vgg_* seam, against the fp64 restatements of tests/vgg_ops_ref.py (proved against torch, autograd and
the oracle's loss functions by tests/test_vgg_ops_ref_cpu.py). fp16 only: mode 2 has no fp32 form.

  exact    wherever every product and partial sum is exact (small integers) the result must EQUAL the reference: a wrong tap, a
           dropped row or a mirrored tile shows whatever the tolerance.
  bounds   derived from the arithmetic of each kernel, per element, never from its output: the derivation stands in each test's
           docstring. The convolutions take the project's fp16 GEMM bound, 2e-3 * max|ref| per element (tests/test_kernels_gpu.py).

Every op prints its worst error / bound ratio and records it (gpu_util.record)."""
import ctypes as C
import functools
import math

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

import vgg_ops_ref as R  # noqa: E402
from gpu_util import B, record  # noqa: E402

F64 = torch.float64
NONE, RELU = B.ACT_NONE, B.ACT_RELU
TOL = 2e-3
SENT = -777.0
U24, U23 = 2.0 ** -24, 2.0 ** -23


def _gen(seed):
    return torch.Generator().manual_seed(seed)


_KEEP = []


@pytest.fixture(autouse=True)
def _release_device_buffers():
    yield
    _KEEP.clear()


def _dev(t, dtype=torch.float32):
    """a device copy that lives until the test ends (a temporary handed over as a bare pointer would return to the allocator at once)"""
    _KEEP.append(t.to(dtype).contiguous().cuda())
    return _KEEP[-1]


def _h(t):
    return _dev(t, torch.float16)


def _call(status):
    if status != 0 and b"->" in (B.lib().gi_last_error() or b""):     # a HIP error, not a rejected argument: nothing may follow it
        pytest.exit("HIP error: " + B.lib().gi_last_error().decode(errors="replace"), returncode=3)
    B.check(status)


def _sync():
    try:
        torch.cuda.synchronize()
    except RuntimeError as e:     # a fault of the device: the session ends here, no further launch
        pytest.exit(f"device error: {e}", returncode=3)


def judge(name, got, ref, bound):
    """per element |got - ref| <= bound; prints and records the worst ratio"""
    got, ref = got.detach().cpu().to(F64), ref.to(F64)
    assert got.shape == ref.shape, (name, got.shape, ref.shape)
    assert bool(torch.isfinite(got).all()), f"{name}: non-finite values"
    bound = torch.as_tensor(bound, dtype=F64).expand(ref.shape) if not torch.is_tensor(bound) else bound.to(F64)
    ratio = float(((got - ref).abs() / (bound + 1e-300)).max())
    print(f"{name}: worst |err| / bound = {ratio:.3f}")
    record("vgg_ops " + name, ratio)
    assert ratio <= 1.0, f"{name}: |err| / bound = {ratio:.3f}"


def _bits(v):
    """fp32 value -> device word holding its bit pattern"""
    return _dev(torch.tensor([v], dtype=torch.float32).view(torch.int32), torch.int32)


def _float_of(word):
    return float(word.cpu().view(torch.float32)[0])


# =================================================================================================================
# 3x3 convolutions: every mode-2 kernel, forward and input gradient, every epilogue
# =================================================================================================================
@functools.lru_cache(maxsize=None)
def _conv_data(shape, d, kind):
    """operands (CPU, fp16-valued) and the fp64 convolution of one case; shared by its epilogue variants and left unchanged"""
    n, H, W, ci, co = shape
    g = _gen(sum(v * 31 ** i for i, v in enumerate(shape)) + (7 if d == "T" else 0) + (13 if kind == "exact" else 0))
    wshape = (co, ci, 3, 3) if d == "F" else (ci, co, 3, 3)       # the master weights of the VGG layer
    if kind == "exact":
        x = torch.randint(-2, 3, (n, H, W, ci), generator=g).float()
        w = torch.randint(-1, 2, wshape, generator=g).float()
        bias = torch.randint(-3, 4, (co,), generator=g).float()
        add = torch.randint(-2, 3, (n, H, W, co), generator=g).float()
    else:
        x = torch.randn(n, H, W, ci, generator=g).half().float()
        w = (torch.randn(wshape, generator=g) / math.sqrt(9 * ci)).half().float()
        bias = torch.randn(co, generator=g) * 0.5
        add = torch.randn(n, H, W, co, generator=g).half().float()
    mask = torch.randn(n, H, W, co, generator=g).half().float()
    mask[:, ::3, ::2] = 0.0                                         # exact zeros on a lattice: the epilogue's test is > 0
    conv = R.conv3x3(x, w) if d == "F" else R.conv3x3_input_grad(x, w)
    return x, w, bias, add, mask, conv


def _conv_run(shape, d, x, w, bias, relu, pool2, mask, add, opts):
    n, H, W, ci, co = shape
    mcin, mcout = (ci, co) if d == "F" else (co, ci)
    out = torch.full((n * H * W * co,), SENT, dtype=torch.float16, device="cuda")
    wpk = torch.zeros(ci * 9 * co, dtype=torch.float16, device="cuda")
    pa, ma = C.c_int(-1), C.c_int(-1)
    for k, v in opts.items():
        B.set_option(k, v)
    try:
        _call(B.lib().gi_debug_vgg_conv3x3(B.get_ctx(), B.ptr(_h(x)), B.ptr(_dev(w)), B.ptr(wpk), B.ptr(out), n, H, W, mcin, mcout, 1 if d == "T" else 0,
                                           B.ptr(_dev(bias)) if bias is not None else None, RELU if relu else NONE, pool2,
                                           B.ptr(_h(mask)) if mask is not None else None, B.ptr(_h(add)) if add is not None else None, C.byref(pa), C.byref(ma)))
        _sync()
        kernel = B.last_kernel()
    finally:
        for k in opts:
            B.set_option(k, -1)
    return out, pa.value, ma.value, kernel


CONV_IDS = [f"{k}|{'x'.join(map(str, s))}|{d}|{e}" for k, _, s, d, e, _, _ in R.conv_variants()]


@pytest.mark.parametrize("kind", ["exact", "random"])
@pytest.mark.parametrize("kernel,opts,shape,d,epi,pool_applied,mask_applied", R.conv_variants(), ids=CONV_IDS)
def test_conv3x3(kernel, opts, shape, d, epi, pool_applied, mask_applied, kind):
    """(a) exact: inputs in [-2, 2], weights in [-1, 1], bias in [-3, 3], addend in [-2, 2], all integers: every fp32 partial sum
    and - the reference stays within 2048, asserted - every fp16 result is exact, torch.equal. (b) random: |err| <= 2e-3 * max|ref|.
    The pooled store is bit-equal to maxpool2 of the same call's full map (the maximum of roundings is the rounding of the maximum).
    Measured on MI355X: worst |err| / bound over the random cases 0.26 (igemm8<2>, 256 -> 256 input gradient with
    mask + add), at most 0.25 for the other five kernels; every exact case equal."""
    n, H, W, ci, co = shape
    x, w, bias, add, mask, conv = _conv_data(shape, d, kind)
    fwd = d == "F"
    name = f"conv3x3 {kernel} {shape} {d} {epi} {kind}"
    ref = conv + bias.double() if fwd else conv
    ref = torch.relu(ref) if fwd else ref
    if epi.startswith("mask") and mask_applied:     # a kernel without that epilogue (igemm3) returns the plain GEMM and says so
        ref = R.mask_add(ref, mask, add if epi == "mask+add" else None)
    if kind == "exact":
        assert float(ref.abs().max()) <= 2048 and float(conv.abs().max()) <= 2048, "the exact case left fp16's integer range"
    out, pa, ma, kname = _conv_run(shape, d, x, w, bias if fwd else None, fwd, 1 if epi == "pool" else 0, mask if epi.startswith("mask") else None,
                                   add if epi == "mask+add" else None, opts)
    assert kname == kernel, f"{name}: served by {kname}"
    assert (pa, ma) == (pool_applied, mask_applied), f"{name}: pool_applied={pa} mask_applied={ma}"
    bound = TOL * float(ref.abs().max())
    if epi == "pool":
        full, pa0, _, k0 = _conv_run(shape, d, x, w, bias, True, 0, None, None, opts)
        assert pa0 == 0 and k0 == kernel
        if pa:
            q = n * (H // 2) * (W // 2) * co
            pooled = torch.full((q,), SENT, dtype=torch.float16, device="cuda")
            _call(B.lib().gi_debug_vgg_maxpool2(B.get_ctx(), B.ptr(full), B.ptr(pooled), n, H // 2, W // 2, co))
            _sync()
            assert torch.equal(out[:q], pooled), f"{name}: the pooled store differs from maxpool2 of the full map"
            assert bool((out[q:] == SENT).all()), f"{name}: the pooled store wrote beyond the pooled map"
            out, ref = out[:q].view(n, H // 2, W // 2, co), R.maxpool2(ref)
        else:
            assert torch.equal(out, full), f"{name}: pool2 declined, yet the map differs from the plain call's"
    out = out.view(ref.shape)
    if kind == "exact":
        assert torch.equal(out.cpu().double(), ref), f"{name}: {int((out.cpu().double() != ref).sum())} of {ref.numel()} elements differ"
    else:
        judge(name, out, ref, bound)


def test_conv3x3_rejects_bad_arguments():
    t = torch.zeros(4096, device="cuda")
    p, pa, ma = B.ptr(t), C.c_int(0), C.c_int(0)
    f = B.lib().gi_debug_vgg_conv3x3
    ok = dict(n=1, H=2, W=2, cin=64, cout=64, tr=0, pool=0, mask=None, add=None, inp=p)
    for change in (dict(cin=60), dict(cout=8), dict(n=0), dict(pool=1, H=3), dict(add=p), dict(inp=None), dict(n=1 << 20, H=1 << 10, W=1 << 10)):
        a = dict(ok, **change)
        rc = f(B.get_ctx(), a["inp"], p, p, p, a["n"], a["H"], a["W"], a["cin"], a["cout"], a["tr"], None, NONE, a["pool"], a["mask"], a["add"],
               C.byref(pa), C.byref(ma))
        assert rc == -1 and B.lib().gi_last_error(), change
    assert B.lib().gi_debug_vgg_conv1(B.get_ctx(), p, p, 1, 16, 24, p, p, p, p) == -1
    assert B.lib().gi_debug_vgg_maxpool2(B.get_ctx(), p, p, 1, 2, 2, 12) == -1
    sp = C.c_int(0)
    assert B.lib().gi_debug_vgg_tap_terms(B.get_ctx(), p, 1, 16, 96, 0, p, 1 << 30, p, None, None, C.byref(sp)) == -1
    assert B.lib().gi_debug_vgg_tap_terms(B.get_ctx(), p, 1, 16, 64, 0, p, 1024, p, None, None, C.byref(sp)) == -1
    assert B.lib().gi_debug_vgg_seed(B.get_ctx(), 1, p, p, p, p, p, p, 1, 16, 32, 1.0, 1.0) == -1
    assert B.lib().gi_debug_vgg_seed(B.get_ctx(), 0, p, p, p, p, None, p, 1, 16, 64, 1.0, 1.0) == -1
    assert B.lib().gi_debug_vgg_act_bwd(B.get_ctx(), 1, p, p, None, p, 1, 3, 4, 64, 1) == -1
    assert B.lib().gi_debug_vgg_act_bwd(B.get_ctx(), 1, None, p, None, p, 1, 4, 4, 64, 1) == -1
    assert B.lib().gi_debug_vgg_act_bwd(B.get_ctx(), 0, p, p, p, p, 1, 4, 4, 12, 1) == -1
    assert B.lib().gi_debug_vgg_conv1_adjoint(B.get_ctx(), p, p, None, 1.0, p, 1, 4, 4) == -1
    _sync()
    assert not t.any()


# =================================================================================================================
# conv1_1
# =================================================================================================================
def _conv1_run(xa, xb, w, b):
    n, H, W = xa.shape
    out = torch.full((2 * n, H, W, 64), SENT, dtype=torch.float16, device="cuda")
    w1 = torch.full((64, 9), float("nan"), device="cuda")
    _call(B.lib().gi_debug_vgg_conv1(B.get_ctx(), B.ptr(_dev(xa)), B.ptr(_dev(xb)), n, H, W, B.ptr(_dev(w)), B.ptr(_dev(b)), B.ptr(w1), B.ptr(out)))
    _sync()
    return out, w1


@pytest.mark.parametrize("n,H,W", [(1, 16, 16), (2, 16, 48), (3, 128, 256)])
def test_conv1(n, H, W):
    """|err| <= 2^-11 |ref| + 16 * 2^-24 (sum |w1 x| + |b|) + 2^-25: one fp16 rounding of the result, fp32 accumulation over K = 9
    padded to 16 behind the bias, fp16's subnormal floor. 3 x 128 x 256 has 12288 sixteen-pixel groups, more than the 8192 waves
    of the capped grid: the strided prefetch loop runs with the xa / xb boundary inside it. Measured on MI355X: worst ratio 0.997
    (every shape: the fp16 rounding term, which round-to-nearest attains)."""
    g = _gen(n * H + W)
    xa, xb = torch.randn(n, H, W, generator=g) * 0.5, torch.randn(n, H, W, generator=g) * 0.5 + 0.1
    w, b = torch.randn(64, 3, 3, 3, generator=g) * 0.2, torch.randn(64, generator=g) * 0.1
    out, w1 = _conv1_run(xa, xb, w, b)
    assert torch.equal(w1.cpu(), R.w1_of(w)), "sum_cin: not the ascending fp32 sum over the input channels"
    ref, mag = R.conv1(xa, xb, R.w1_of(w), b)
    judge(f"conv1 {n}x{H}x{W}", out, ref, 2.0 ** -11 * ref.abs() + 16 * U24 * mag + 2.0 ** -25)


def test_conv1_exact_integers():
    n, H, W = 2, 16, 48
    g = _gen(5)
    xa, xb = (torch.randint(-2, 3, (n, H, W), generator=g).float() for _ in range(2))
    w, b = torch.randint(-1, 2, (64, 3, 3, 3), generator=g).float(), torch.randint(-3, 4, (64,), generator=g).float()
    out, _ = _conv1_run(xa, xb, w, b)
    ref, _ = R.conv1(xa, xb, R.w1_of(w), b)
    assert float(ref.abs().max()) <= 2048 and torch.equal(out.cpu().double(), ref)


# =================================================================================================================
# maxpool2
# =================================================================================================================
@pytest.mark.parametrize("n,Ho,Wo,Cn", [(3, 3, 5, 64), (2, 8, 8, 512)])
def test_maxpool2(n, Ho, Wo, Cn):
    """bit-exact against F.max_pool2d on the fp16 values; half-integers in [-3, 3]: negative windows and ties"""
    x = (torch.randint(-6, 7, (n, 2 * Ho, 2 * Wo, Cn), generator=_gen(Ho)).float() / 2).half()
    out = torch.full((n, Ho, Wo, Cn), SENT, dtype=torch.float16, device="cuda")
    _call(B.lib().gi_debug_vgg_maxpool2(B.get_ctx(), B.ptr(_h(x)), B.ptr(out), n, Ho, Wo, Cn))
    _sync()
    ref = F.max_pool2d(x.float().permute(0, 3, 1, 2), 2, 2).permute(0, 2, 3, 1)
    assert torch.equal(out.cpu().float(), ref) and torch.equal(ref.double(), R.maxpool2(x.double()))


# =================================================================================================================
# the two terms of a tap, its dense Gram difference
# =================================================================================================================
def _tap_run(Fm, n, force):
    _, HW, Cn = Fm.shape
    nbytes = B.lib().gi_debug_vgg_tap_ws_bytes()
    ws = torch.full((nbytes // 4,), float("nan"), device="cuda")
    terms = torch.full((2,), float("nan"), device="cuda")
    dg = torch.full((n, Cn, Cn), float("nan"), device="cuda")
    amax = torch.full((1,), 0x7fffffff, dtype=torch.int32, device="cuda")
    split = C.c_int(-1)
    _call(B.lib().gi_debug_vgg_tap_terms(B.get_ctx(), B.ptr(_h(Fm)), n, HW, Cn, force, B.ptr(ws), nbytes, B.ptr(terms), B.ptr(dg), B.ptr(amax), C.byref(split)))
    _sync()
    return terms.cpu().double(), dg.cpu(), amax, split.value


# (n, HW, C, forced split, the split that must run): gram2_kernel<32> (C = 64) and <64>, one / three / ten tiles, HW no multiple of 32;
# splits beyond 8 reach gram_delta's eight-way loop and its remainder
TAP_CASES = [(2, 15, 512, 0, 1), (1, 1, 512, 0, 1), (2, 256, 64, 0, 2), (2, 256, 64, 3, 3), (2, 1024, 128, 0, 8), (2, 1024, 128, 11, 11),
             (1, 3840, 256, 0, 30)]


@pytest.mark.parametrize("n,HW,Cn,force,split", TAP_CASES)
def test_tap_terms_exact_integers(n, HW, Cn, force, split):
    """F integer in [0, 3]: every partial Gram is an exact fp32 integer (at most 9 * 3840), so go and gt are exact and
    dG = go * scale - gt * scale errs by the rounding of scale, of the two products and of the difference (or of one product and
    a fused multiply-subtract): at most 2 * 2^-23 * (|G_o| + |G_t|). dG is exactly symmetric, amax = max |dG| bit for bit."""
    Fm = torch.randint(0, 4, (2 * n, HW, Cn), generator=_gen(HW + Cn)).float()
    terms, dg, amax, used = _tap_run(Fm, n, force)
    assert used == split, f"split {used}, expected {split}"
    Go, Gt = R.gram(Fm[:n]), R.gram(Fm[n:])
    p, s, dG = R.tap_terms(Fm, n)
    judge(f"tap dG exact n={n} HW={HW} C={Cn} split={used}", dg, dG, 2 * U23 * (Go + Gt))
    assert torch.equal(dg, dg.transpose(1, 2)), "dG is not symmetric"
    assert _float_of(amax) == float(dg.abs().max()), "amax is not max |dG|"


@pytest.mark.parametrize("n,HW,Cn,force,split", TAP_CASES)
def test_tap_terms_random(n, HW, Cn, force, split):
    """post-ReLU-like maps (non-negative, about half zeros): every product is non-negative, so sum |terms| is the reference itself
    and the worst-case fp32 accumulation bound HW * 2^-24 relative (+ one fp32 ulp for the final rounding) is sharp.
    Measured on MI355X: worst ratio perceptual 0.04, style 0.10, dG 0.19 (exact-integer dG: 0.46)."""
    Fm = (torch.relu(torch.randn(2 * n, HW, Cn, generator=_gen(HW * 3 + Cn))) * 1.5).half().float()
    Fm[n:] = Fm[n:] * 0.5                                  # the target maps: another scale, so that G_o - G_t does not cancel
    Fm = Fm.half().float()
    terms, dg, amax, used = _tap_run(Fm, n, force)
    assert used == split
    p, s, dG = R.tap_terms(Fm, n)
    name = f"tap random n={n} HW={HW} C={Cn} split={used}"
    judge(name + " perceptual", terms[:1], p.reshape(1), (HW * U24 + U23) * p)
    judge(name + " style", terms[1:], s.reshape(1), (HW * U24 + U23) * s)
    Go, Gt = R.gram(Fm[:n]), R.gram(Fm[n:])
    judge(name + " dG", dg, dG, (HW * U24 + 2 * U23) * (Go + Gt))
    assert torch.equal(dg, dg.transpose(1, 2)) and _float_of(amax) == float(dg.abs().max())


# =================================================================================================================
# seeds and their scale
# =================================================================================================================
@functools.lru_cache(maxsize=None)
def _seed_data(n, HW, Cn):
    g = _gen(HW + 7 * Cn + n)
    Fm = (torch.relu(torch.randn(2 * n, HW, Cn, generator=g)) * 1.5).half().float()
    Fm[n:] = (Fm[n:] * 0.5 + torch.relu(torch.randn(n, HW, Cn, generator=g)) * 0.3)
    Fm = Fm.half().double()
    dG = R.tap_terms(Fm, n)[2].float()                    # symmetric by construction, as production's
    assert torch.equal(dG, dG.transpose(1, 2))
    return Fm[:n], Fm[n:], dG, float(dG.abs().max())


def _seed_run(store, Fo, Ft, dG, dmax, sc, wp, ws, guard=256):
    n, HW, Cn = Fo.shape
    fo = _h(Fo)
    ft = torch.full((n * HW * Cn + guard * Cn,), SENT, dtype=torch.float16, device="cuda")
    ft[:n * HW * Cn] = Ft.reshape(-1).half().cuda()
    smax = torch.zeros(1, dtype=torch.int32, device="cuda")
    _call(B.lib().gi_debug_vgg_seed(B.get_ctx(), store, B.ptr(fo), B.ptr(ft), B.ptr(_dev(dG)), B.ptr(_bits(dmax)), B.ptr(smax),
                                    B.ptr(_dev(torch.tensor(sc))) if sc else None, n, HW, Cn, wp, ws))
    _sync()
    assert torch.equal(fo.cpu().double(), Fo), "F_o was written"
    assert bool((ft[n * HW * Cn:] == SENT).all()), "pixels beyond HW were written"
    assert store or torch.equal(ft[:n * HW * Cn].cpu().double(), Ft.reshape(-1)), "the maximum pass wrote F_t"
    return ft[:n * HW * Cn].view(n, HW, Cn), smax


# 2304 pixels: nb = 9, the sampled pass's clamp branch (block 8 + 3 does not exist); 3840: nb = 15; 4096: nb = 16
SEED_SHAPES = [(2, 15, 512), (1, 1, 512), (1, 2304, 64), (1, 3840, 64), (1, 4096, 128), (2, 256, 256)]
SEED_WEIGHTS = [pytest.param(1.0, 0.0, id="cp"), pytest.param(0.0, 1.0, id="cs"), pytest.param(0.05, 100.0, id="both")]


@pytest.mark.parametrize("wp,ws", SEED_WEIGHTS)
@pytest.mark.parametrize("n,HW,Cn", SEED_SHAPES)
def test_seed(n, HW, Cn, wp, ws):
    """v = cs' sum_k dGq[c][k] F_o[p][k] + cp (F_o - F_t), cs' = cs 2^ex, dGq = fp16(dG 2^-ex) - operands the restatement shares, so
    what is left is fp32 accumulation over K = C of exact products (C * 2^-24 * cs' * sum |dGq F_o|), the roundings of cs', of the
    cp product, of the fused multiply-add and of v * s (4 * 2^-24 |v|), and in the store pass one fp16 rounding of v * s
    (2^-11 |v s|, subnormal floor 2^-25). The maximum pass: the maximum over the sampled blocks within the largest such bound, and
    never above the full maximum. Measured on MI355X: worst ratio store 0.998 (the fp16 rounding term, which
    round-to-nearest attains), maximum 0.37."""
    Fo, Ft, dG, dmax = _seed_data(n, HW, Cn)
    v, mag, _ = R.seed(Fo, Ft, dG, dmax, n, wp, ws)
    acc = Cn * U24 * mag + 4 * U24 * v.abs()
    name = f"seed n={n} HW={HW} C={Cn} wp={wp} ws={ws}"
    _, smax = _seed_run(0, Fo, Ft, dG, dmax, None, wp, ws)
    got = _float_of(smax)
    sampled = R.sampled_mask(HW)
    assert bool(sampled.all()) == (HW <= 2048)
    ref_max, full_max = float(v[:, sampled].abs().max()), float(v.abs().max())
    slack = float(acc.max())
    judge(name + " max", torch.tensor([got]), torch.tensor([ref_max]), slack)
    assert got <= full_max + slack, f"{name}: the sampled maximum {got} exceeds the full maximum {full_max}"
    s = R.scale(full_max)
    out, _ = _seed_run(1, Fo, Ft, dG, dmax, [s, 1.0 / s], wp, ws)
    judge(name + " store", out, v * s, 2.0 ** -11 * (v * s).abs() + 2.0 ** -25 + s * acc)


def test_seed_of_identical_maps_is_zero():
    """output == target: dG = 0, dmax = 0 (no normalisation exponent), every seed is zero and nothing is NaN"""
    n, HW, Cn = 2, 300, 64
    Fo = _seed_data(n, HW, Cn)[0]
    dG = torch.zeros(n, Cn, Cn)
    out, _ = _seed_run(1, Fo, Fo, dG, 0.0, [1.0, 1.0], 0.05, 100.0)
    assert not out.any() and not bool(torch.isnan(out).any())
    _, smax = _seed_run(0, Fo, Fo, dG, 0.0, None, 0.05, 100.0)
    assert int(smax) == 0


def test_scale():
    """exact powers of two putting the maximum into [2^-3, 2^-2); 0, inf and NaN give 1; the exponent is clamped to +-100"""
    for am in (0.3, 1.0, 0.249, 0.25, 6e4, 1e-30, 2.0 ** -110, 2.0 ** 127, 0.0, math.inf, math.nan):
        sc = torch.full((2,), float("nan"), device="cuda")
        _call(B.lib().gi_debug_vgg_scale(B.get_ctx(), B.ptr(_bits(am)), B.ptr(sc)))
        _sync()
        s = R.scale(float(torch.tensor(am, dtype=torch.float32)))
        assert sc.tolist() == [s, 1.0 / s], (am, sc.tolist(), s)
    assert R.scale(2.0 ** -110) == 2.0 ** 100 and R.scale(2.0 ** 127) == 2.0 ** -100 and R.scale(0.3) == 0.5


# =================================================================================================================
# activation backward, plain and through the pool
# =================================================================================================================
@pytest.mark.parametrize("relu", [0, 1])
@pytest.mark.parametrize("has_g,has_seed,alias", [(0, 1, 0), (1, 1, 1), (1, 0, 1), (1, 1, 0), (0, 0, 0)])
@pytest.mark.parametrize("n,H,W,Cn", [(3, 3, 5, 64), (2, 8, 8, 512)])
def test_act_bwd(n, H, W, Cn, has_g, has_seed, alias, relu):
    """bit-exact: [act > 0 or not relu] * fp16(fp32(g) + fp32(seed))"""
    g = _gen(H + Cn + has_g)
    act = torch.randn(n, H, W, Cn, generator=g).half()
    act[:, ::2, 1::2] = 0.0
    gg = (torch.randn(n, H, W, Cn, generator=g) * 3).half() if has_g else None
    sd = torch.randn(n, H, W, Cn, generator=g).half() if has_seed else None
    gd = _h(gg) if has_g else None
    out = gd if alias else torch.full((n, H, W, Cn), SENT, dtype=torch.float16, device="cuda")
    _call(B.lib().gi_debug_vgg_act_bwd(B.get_ctx(), 0, B.ptr(gd), B.ptr(_h(act)), B.ptr(_h(sd)) if has_seed else None, B.ptr(out), n, H, W, Cn, relu))
    _sync()
    assert torch.equal(out.cpu().double(), R.act_bwd(gg, act, sd, relu))
    if has_g and not alias:
        assert torch.equal(gd.cpu(), gg), "g was written"


@pytest.mark.parametrize("relu", [0, 1])
@pytest.mark.parametrize("n,H,W,Cn", [(3, 6, 10, 64), (2, 16, 16, 512)])
def test_act_bwd_pool(n, H, W, Cn, relu):
    """bit-exact against autograd of F.max_pool2d (first maximum in row-major order), times [max > 0] when relu; ties inside windows,
    windows that are zero throughout; every position of every window is written"""
    g = _gen(H * Cn + relu)
    act = torch.randint(0, 3, (n, H, W, Cn), generator=g).float()
    act[:, :2, :2] = 0.0
    act[:, 2:4, 2:4] = 1.0
    if not relu:
        act = act - 1.0                                     # the post-ReLU map of the replayed layer may be anything; negative maxima pass
    gg = torch.randn(n, H // 2, W // 2, Cn, generator=g).half()
    out = torch.full((n, H, W, Cn), SENT, dtype=torch.float16, device="cuda")
    _call(B.lib().gi_debug_vgg_act_bwd(B.get_ctx(), 1, B.ptr(_h(gg)), B.ptr(_h(act)), None, B.ptr(out), n, H, W, Cn, relu))
    _sync()
    a = act.double().permute(0, 3, 1, 2).requires_grad_(True)
    pooled = F.max_pool2d(a, 2, 2)
    up = gg.double().permute(0, 3, 1, 2)
    pooled.backward(torch.where(pooled.detach() > 0, up, torch.zeros_like(up)) if relu else up)
    ref = a.grad.permute(0, 2, 3, 1)
    assert torch.equal(ref, R.pool_bwd(gg, act, relu))
    assert torch.equal(out.cpu().double(), ref), f"{int((out.cpu().double() != ref).sum())} elements differ"


# =================================================================================================================
# conv1_1 adjoint
# =================================================================================================================
def _adjoint_run(D, w1, sc, gscale):
    n, H, W, _ = D.shape
    out = torch.full((n, H, W), float("nan"), device="cuda")
    _call(B.lib().gi_debug_vgg_conv1_adjoint(B.get_ctx(), B.ptr(_h(D)), B.ptr(_dev(w1)), B.ptr(_dev(torch.tensor(sc))), gscale, B.ptr(out), n, H, W))
    _sync()
    return out


@pytest.mark.parametrize("n,H,W", [(1, 16, 16), (2, 16, 48), (2, 48, 80)])
def test_conv1_adjoint(n, H, W):
    """|err| <= 80 * 2^-24 * |mul| * sum |w1 D| + 2 fp32 ulps: 64 channels + 9 taps of fp32 accumulation (+ slack for the
    order), the rounding of mul and of the final product. 16 x 48: a partial 32-wide tile; 48 x 80: several tiles and their seams.
    Measured on MI355X: worst ratio 0.010."""
    g = _gen(H + W)
    D = (torch.randn(n, H, W, 64, generator=g) * 0.3).half()
    w1 = R.w1_of(torch.randn(64, 3, 3, 3, generator=g) * 0.2)
    sc, gscale = [4.0, 0.25], 0.375
    out = _adjoint_run(D, w1, sc, gscale)
    mul = gscale * sc[1]
    ref, mag = R.conv1_adjoint(D.double(), w1, mul)
    judge(f"conv1_adjoint {n}x{H}x{W}", out, ref, 80 * U24 * abs(mul) * mag + 2 * U23 * ref.abs())


def test_conv1_adjoint_exact_integers():
    n, H, W = 2, 48, 80
    g = _gen(9)
    D = torch.randint(-2, 3, (n, H, W, 64), generator=g).half()
    w1 = R.w1_of(torch.randint(-1, 2, (64, 3, 3, 3), generator=g).float())
    out = _adjoint_run(D, w1, [4.0, 0.25], 2.0)
    ref, _ = R.conv1_adjoint(D.double(), w1, 0.5)
    assert torch.equal(out.cpu().double(), ref)
