"""GPU tier: the normalisation and activation-backward passes of csrc/norm.hip ONE OP AT A TIME through the gi_debug_*
seam, against the fp64 restatement of tests/norm_ref.py (proved against torch by tests/test_norm_ref_cpu.py), in both compute types.

  kinks    the backward ops take mean, invstd, scale and shift as inputs, so the test decides every activation input itself: x is
           moved until no fma(x, scale, shift) lies within 2^-6 of zero (asserted on the CPU, after quantising); no sign decision
           is ambiguous, the reference needs no band and every element is judged.
  exact    wherever the quantity is a sum (partial rows, accumulator totals, dbeta, dgamma at mean = 0 / inv = 1, bias_grad) an
           integer-valued case whose fp32 partial sums are all exact must EQUAL the reference: a dropped or doubled row shows
           whatever the tolerance.
  bounds   the single-layer bounds of tests/test_kernels_gpu.py: max|err| / max|ref| <= 2e-5 (fp32 tensors and every fp32
           per-channel vector), 2e-3 (tensors stored in fp16); float-valued dgamma / dbeta: |err| <= 2e-5 * sum|addends| per
           channel (the pre-filled value counts as one addend), the addends taken from the fp64 reference.

Inputs are NaN wherever no kernel may read, outputs carry a sentinel wherever none may write. The id of every test_act_bn_bwd case
names the kernels op_act_bn_bwd launches for it (K.dispatch restates the dispatch conditions of the launcher).

Found by this file: with ONE sample per population (BatchNorm count 1, InstanceNorm on a 1 x 1 plane) the fp32 passes took
E[x^2] - m^2 from an fp32-rounded square, so a "variance" of up to 6e-8 x^2 stood next to eps = 1e-5 and invstd was off by up to
2 % (seven fp32 cases failed: test_col_stats_bn_finalize[*-1-fp32], test_instance_norm[1-*-fp32]). The passes now take the
variance of a single sample as zero.

Bit records: with GI_NORM_HASHES naming a file, every output that check / check_sum judge, and the outputs asserted with torch.equal
(exact dgamma / dbeta, the zero_next words, the drawn dropout mask), is recorded there as key -> sha256 of its bytes. The key names
the test function, the compute type, the case's own fields and the output - not the kernels that served it - so two builds of the
library that compute the same thing give equal records (profiles/norm_ops_hashes_*.json: two such records, condensed by
tools/condense_hashes.py)."""
import ctypes as C
import hashlib
import json
import math
import os

import pytest
import torch

pytestmark = pytest.mark.gpu

import norm_ref as R  # noqa: E402
from gpu_util import B, quant, record, report, tdt  # noqa: E402

F16, F32 = B.GI_F16, B.GI_F32
CODES = [pytest.param(F32, id="fp32"), pytest.param(F16, id="fp16")]
NONE, RELU, LRELU = B.ACT_NONE, B.ACT_RELU, B.ACT_LRELU
ACT_NAME = {NONE: "none", RELU: "relu", LRELU: "lrelu"}
KINK = 2.0 ** -6
VEC_TOL = 2e-5
SUM_TOL = 2e-5
F64 = torch.float64


def _tol(code):
    return 2e-3 if code == F16 else 2e-5


def _epc(code):
    return 8 if code == F16 else 4


def _c(c, code):
    """channel counts given in chunks: 'q1' = one chunk, 'q3' = three, 'q256' = 256"""
    return int(c[1:]) * _epc(code) if isinstance(c, str) else c


def _gen(seed):
    return torch.Generator().manual_seed(seed)


_KEEP = []


@pytest.fixture(autouse=True)
def _release_device_buffers():
    yield
    _KEEP.clear()


HASH_OUT = os.environ.get("GI_NORM_HASHES", "")
_TEST = {"name": "", "code": ""}


@pytest.fixture(autouse=True)
def _hash_context(request):
    params = getattr(getattr(request.node, "callspec", None), "params", {})
    _TEST["name"] = request.node.originalname
    _TEST["code"] = {F16: "fp16", F32: "fp32"}.get(params.get("code"), "-")
    yield


def record_bits(key, got):
    """GI_NORM_HASHES: key -> sha256 of the bytes of `got` as the device produced them"""
    if HASH_OUT:
        d = json.load(open(HASH_OUT)) if os.path.exists(HASH_OUT) else {}
        t = got.detach().cpu().contiguous()
        d[f"{_TEST['name']}|{_TEST['code']}|{key}"] = hashlib.sha256(t.view(torch.uint8).numpy().tobytes()).hexdigest()
        json.dump(d, open(HASH_OUT, "w"), indent=0, sort_keys=True)


def _dev(t, dtype=torch.float32):
    """a device copy that lives until the test ends: a temporary handed over as a bare pointer would return to the allocator at
    once and the next copy would land on it before the kernel has run"""
    _KEEP.append(t.to(dtype).contiguous().cuda())
    return _KEEP[-1]


def _call(status):
    if status != 0 and b"->" in (B.lib().gi_last_error() or b""):     # a HIP error, not a rejected argument: nothing may follow it
        pytest.exit("HIP error: " + B.lib().gi_last_error().decode(errors="replace"), returncode=3)
    B.check(status)


def _sync():
    try:
        torch.cuda.synchronize()
    except RuntimeError as e:     # a fault of the device: the session ends here, no further launch
        pytest.exit(f"device error: {e}", returncode=3)


def check(name, got, ref, tol, key=None):
    """key: the name of the output in the bit record, where `name` also says which kernels ran"""
    record_bits(key or name, got)
    got, ref = got.detach().cpu().double(), ref.double()
    ok, msg = report(name, got, ref, tol)
    record("norm_ops " + name, float((got - ref).abs().max() / (ref.abs().max() + 1e-30)) / tol)
    assert ok, msg


def check_sum(name, got, ref, abs_terms, tol=SUM_TOL, key=None):
    """per channel |got - ref| <= tol * sum|addends|"""
    record_bits(key or name, got)
    got, ref = got.detach().cpu().double(), ref.double()
    ratio = ((got - ref).abs() / (abs_terms.double() + 1e-30)).max().item()
    print(f"{name}: max |err| / sum|terms| = {ratio:.3e} tol={tol:.1e}")
    record("norm_ops " + name, ratio / tol)
    assert ratio <= tol, f"{name}: {ratio:.3e} > {tol:.1e}"


def wide(t, code):
    """(P, c) CPU values -> device (P, 2c) buffer of the compute type holding them at channel offset c, NaN elsewhere"""
    P, c = t.shape
    buf = torch.full((P, 2 * c), float("nan"), dtype=tdt(code), device="cuda")
    buf[:, c:] = t.to(tdt(code)).cuda()
    return buf, 2 * c, c


SENT = -777.0


def out_wide(P, c, code):
    return torch.full((P, 2 * c + _epc(code)), SENT, dtype=tdt(code), device="cuda"), 2 * c + _epc(code), c


def tail_untouched(buf, c, coff):
    return bool((buf[:, :coff] == SENT).all()) and bool((buf[:, coff + c:] == SENT).all())


def settle(x, sc, sh, code):
    """x (P, c), sc / sh broadcastable fp32: x rounded to the compute type with every fma(x, sc, sh) at least 2^-6 from zero
    (offenders are moved to +-2^-5 first). Asserts the construction."""
    x = quant(x.float(), code)
    t = x.double() * sc.double() + sh.double()
    bad = t.abs() < KINK
    target = torch.where(t >= 0, torch.full_like(t, 2 * KINK), torch.full_like(t, -2 * KINK))
    x = quant(torch.where(bad, (target - sh.double()) / sc.double(), x.double()).float(), code)
    t = x.double() * sc.double() + sh.double()
    assert float(t.abs().min()) >= KINK, "an activation input within 2^-6 of zero survived the construction"
    return x, t


def rows_rule(pixels):
    """rows of a column pass (one partial row per workgroup): 32 rows at least, 1024 workgroups at most"""
    rpb = max(32, (pixels + 1023) // 1024)
    return (pixels + rpb - 1) // rpb, rpb


# =================================================================================================================
# statistics: col_stats -> bn_finalize (the three-launch path)
# =================================================================================================================
def _col_stats(x_dev, code, pixels, c):
    part = torch.full(((pixels // 32 + 8) * 2 * c,), float("nan"), dtype=torch.float32, device="cuda")
    rows = C.c_int(0)
    _call(B.lib().gi_debug_col_stats(B.get_ctx(), code, B.ptr(x_dev), pixels, c, B.ptr(part), C.byref(rows)))
    _sync()
    return part, rows.value


def _bn_params(c, seed):
    g = _gen(seed)
    return (torch.rand(c, generator=g) + 0.5, torch.randn(c, generator=g) * 0.3, torch.randn(c, generator=g) * 0.2,
            torch.rand(c, generator=g) + 0.5)


def _finalize(part, rows, c, count, gamma, beta, rmean, rvar, train, groups=1, part_stride=0, out_stride=0):
    n = max(out_stride, c) * groups
    outs = [torch.full((n,), float("nan"), dtype=torch.float32, device="cuda") for _ in range(4)]
    rm, rv = _dev(rmean), _dev(rvar)
    _call(B.lib().gi_debug_bn_finalize(B.get_ctx(), B.ptr(part), rows, c, count, B.ptr(_dev(gamma)), B.ptr(_dev(beta)), B.ptr(rm), B.ptr(rv),
                                       B.ptr(outs[0]), B.ptr(outs[1]), B.ptr(outs[2]), B.ptr(outs[3]), train, 0.1, 1e-5, groups, part_stride,
                                       out_stride))
    _sync()
    return outs, rm, rv


def _check_bn_vectors(name, outs, rm, rv, rs, c, out_stride):
    for j, r in enumerate(rs):
        o = j * out_stride
        for k, key in enumerate(("scale", "shift", "mean", "inv")):
            check(f"{name} {key}[{j}]", outs[k][o:o + c], r[key], VEC_TOL)
    check(f"{name} running_mean", rm, rs[-1]["rmean"], VEC_TOL)
    check(f"{name} running_var", rv, rs[-1]["rvar"], VEC_TOL)


STAT_SHAPES = [("q1", 1), ("q1", 31), ("q1", 33), ("q1", 40001), (64, 1), (64, 31), (64, 33), (64, 40001), (512, 1), (512, 31), (512, 33),
               ("q256", 1), ("q256", 31), ("q256", 33)]


@pytest.mark.parametrize("code", CODES)
@pytest.mark.parametrize("c,pixels", STAT_SHAPES)
def test_col_stats_bn_finalize(code, c, pixels):
    c = _c(c, code)
    g = _gen(pixels + c)
    x = quant(torch.randn(pixels, c, generator=g) * 1.3 + torch.randn(c, generator=g) * 0.5, code)
    part, rows = _col_stats(_dev(x, tdt(code)), code, pixels, c)
    assert rows == rows_rule(pixels)[0]
    p = part[:rows * 2 * c].view(rows, 2, c).cpu().double()
    s, q = R.col_sums(x)
    name = f"stats c={c} p={pixels}"
    check_sum(name + " sum", p[:, 0].sum(0), s, x.double().abs().sum(0))
    check_sum(name + " sumsq", p[:, 1].sum(0), q, q)
    gamma, beta, rmean, rvar = _bn_params(c, 3)
    outs, rm, rv = _finalize(part, rows, c, pixels, gamma, beta, rmean, rvar, 1)
    # the reference takes the statistics from x itself: the partial rows' own error is part of what is judged
    _check_bn_vectors(name, outs, rm, rv, [R.bn_from_sums(s, q, pixels, gamma, beta, rmean, rvar)], c, 0)


@pytest.mark.parametrize("code", CODES)
@pytest.mark.parametrize("c,pixels", [("q1", 40001), (64, 33), (64, 40001), ("q256", 33)])
def test_col_stats_exact_integers(code, c, pixels):
    c = _c(c, code)
    x = torch.randint(-4, 5, (pixels, c), generator=_gen(c + pixels)).float()
    part, rows = _col_stats(_dev(x, tdt(code)), code, pixels, c)
    nrows, rpb = rows_rule(pixels)
    assert rows == nrows
    p = part[:rows * 2 * c].view(rows, 2, c).cpu().double()
    for b in range(rows):     # every partial row is the sum of its own block of pixels
        blk = x[b * rpb:(b + 1) * rpb].double()
        assert torch.equal(p[b, 0], blk.sum(0)) and torch.equal(p[b, 1], (blk * blk).sum(0)), f"partial row {b} of {rows}"


@pytest.mark.parametrize("code", CODES)
def test_bn_finalize_two_populations_and_eval(code):
    c, pg = 64, 1000
    g = _gen(5)
    x = quant(torch.randn(2 * pg, c, generator=g) * torch.tensor([1.0, 2.0]).repeat_interleave(pg)[:, None] + 0.3, code)
    xd = _dev(x, tdt(code))
    rows, _ = rows_rule(pg)
    part_stride = rows * 2 * c + 24
    part = torch.full((2 * part_stride,), float("nan"), dtype=torch.float32, device="cuda")
    for j in range(2):
        pj, rj = _col_stats(xd[j * pg:(j + 1) * pg], code, pg, c)
        assert rj == rows
        part[j * part_stride:j * part_stride + rows * 2 * c] = pj[:rows * 2 * c]
    gamma, beta, rmean, rvar = _bn_params(c, 8)
    out_stride = c + 8
    outs, rm, rv = _finalize(part, rows, c, pg, gamma, beta, rmean, rvar, 1, 2, part_stride, out_stride)
    rs = R.bn_from_sums_groups([R.col_sums(x[:pg]), R.col_sums(x[pg:])], pg, gamma, beta, rmean, rvar)
    _check_bn_vectors("finalize two populations", outs, rm, rv, rs, c, out_stride)
    assert all(bool(torch.isnan(o[c:out_stride]).all()) for o in outs), "the gap between the populations' vectors was written"
    # eval mode: the running statistics normalise and stay as they are; no partial row is read
    outs, rm, rv = _finalize(None, 0, c, pg, gamma, beta, rmean, rvar, 0)
    _check_bn_vectors("finalize eval", outs, rm, rv, [R.bn_from_sums(None, None, pg, gamma, beta, rmean, rvar, train=False)], c, 0)
    assert torch.equal(rm.cpu(), rmean) and torch.equal(rv.cpu(), rvar)


@pytest.mark.parametrize("code", CODES)
@pytest.mark.parametrize("pixels", [33, 40001])
def test_col_stats_bn_finalize_offset_mean(code, pixels):
    """per-channel mean = 8 std: E[x^2] - m^2 cancels 65-fold; the flat bound still holds"""
    c = 64
    g = _gen(pixels)
    std = torch.rand(c, generator=g) + 0.5
    x = quant(torch.randn(pixels, c, generator=g) * std + 8.0 * std * torch.where(torch.rand(c, generator=g) > 0.5, 1.0, -1.0), code)
    part, rows = _col_stats(_dev(x, tdt(code)), code, pixels, c)
    gamma, beta, rmean, rvar = _bn_params(c, 4)
    outs, rm, rv = _finalize(part, rows, c, pixels, gamma, beta, rmean, rvar, 1)
    s, q = R.col_sums(x)
    _check_bn_vectors(f"stats offset mean p={pixels}", outs, rm, rv, [R.bn_from_sums(s, q, pixels, gamma, beta, rmean, rvar)], c, 0)


# =================================================================================================================
# exact accumulators
# =================================================================================================================
def _acc_block(c):
    return torch.zeros(B.lib().gi_stat_acc_words(c), dtype=torch.int64, device="cuda")


def _acc_add(acc, c, reps, group, q, addends):
    a = _dev(addends)
    _call(B.lib().gi_debug_stat_acc_add(B.get_ctx(), B.ptr(acc), c, reps, group, q, B.ptr(a), addends.shape[0]))
    _sync()


def _acc_read(acc, c, reps, group):
    out = torch.full((2, c), float("nan"), dtype=F64, device="cuda")
    _call(B.lib().gi_stat_acc_read(B.get_ctx(), B.ptr(acc), c, reps, group, B.ptr(out)))
    _sync()
    return out.cpu()


def _totals(addends):
    return torch.tensor([R.stat_acc_total(addends[:, ch].tolist()) for ch in range(addends.shape[1])], dtype=F64)


def _same(a, b):
    """bit-for-bit equal, NaN in the same places"""
    return bool(((a == b) | (torch.isnan(a) & torch.isnan(b))).all())


def test_stat_acc_totals():
    c, rows = 70, 37
    g = _gen(1)
    add = torch.randn(rows, c, generator=g) * torch.tensor([1e-9, 1e-3, 1.0, 1e5, 1e9])[torch.randint(0, 5, (rows, c), generator=g)]
    add[0, 0] = -(2.0 ** -41)                 # bits below 2^-40 only: one unit toward -inf
    add[1, 1] = 2.0 ** 40 - 2.0 ** 16         # the largest accepted magnitude
    add[2, 1] = 2.0 ** 40 - 2.0 ** 16
    add[3, 2] = -(2.0 ** 40 - 2.0 ** 16)
    add = add.float()
    ref = _totals(add)
    assert bool(torch.isfinite(ref).all())
    other = torch.randint(-5, 6, (rows, c), generator=g).float()
    got = {}
    for reps in (1, 2, 3, 4):
        for order in ("fwd", "perm"):
            a = add if order == "fwd" else add[torch.randperm(rows, generator=g)]
            acc = _acc_block(c)
            _acc_add(acc, c, reps, 0, 0, a)
            _acc_add(acc, c, reps, 0, 1, other)
            _acc_add(acc, c, reps, 1, 1, a)
            r0, r1 = _acc_read(acc, c, reps, 0), _acc_read(acc, c, reps, 1)
            assert torch.equal(r0[0], ref), f"reps={reps} {order}: worst {float((r0[0] - ref).abs().max()):.3e}"
            assert torch.equal(r0[1], other.double().sum(0)) and torch.equal(r1[1], ref) and not r1[0].any()
            got[(reps, order)] = r0[0]
    assert all(torch.equal(v, got[(1, "fwd")]) for v in got.values()), "totals depend on the row order or the replicas"


@pytest.mark.parametrize("bad", [2.0 ** 40, -2.0 ** 40, float("inf"), float("nan")])
def test_stat_acc_poison(bad):
    c, rows, reps = 70, 9, 4
    add = torch.randn(rows, c, generator=_gen(2))
    ref = _totals(add.float())
    acc = _acc_block(c)
    _acc_add(acc, c, reps, 0, 0, add)
    _acc_add(acc, c, reps, 0, 1, add)
    _acc_add(acc, c, reps, 1, 0, add)
    poison = torch.zeros(1, c)
    poison[0, 33] = bad
    _acc_add(acc, c, reps, 0, 1, poison)
    r0, r1 = _acc_read(acc, c, reps, 0), _acc_read(acc, c, reps, 1)
    exp = ref.clone()
    exp[33] = float("nan")
    assert _same(r0[1], exp), "only channel 33 of the poisoned quantity may read NaN"
    assert torch.equal(r0[0], ref) and torch.equal(r1[0], ref), "the other quantity / the other population must not be poisoned"


def test_stat_acc_add_rejects_bad_arguments():
    acc, a = _acc_block(8), torch.zeros(1, 8, device="cuda")
    for reps, group, q in ((0, 0, 0), (5, 0, 0), (1, 2, 0), (1, 0, 2)):
        assert B.lib().gi_debug_stat_acc_add(B.get_ctx(), B.ptr(acc), 8, reps, group, q, B.ptr(a), 1) != 0
        assert B.lib().gi_last_error()


# =================================================================================================================
# bn_apply / bn_apply_acc
# =================================================================================================================
def _fwd_data(pixels, c, code, seed, offset_mean=False):
    g = _gen(seed)
    std = torch.rand(c, generator=g) + 0.5
    mean = 8.0 * std if offset_mean else torch.randn(c, generator=g) * 0.5
    return quant(torch.randn(pixels, c, generator=g) * std + mean, code)


def _drop_mask(pixels, c, seed):
    return (torch.rand(pixels, c, generator=_gen(seed)) > 0.5).to(torch.uint8)


APPLY_CASES = [
    # pixels, c, act, two populations, dropout mask read
    (1, "q1", NONE, False, False), (1, 64, LRELU, False, True), (33, 64, RELU, False, False), (33, "q256", LRELU, False, False),
    (1000, 64, NONE, False, True), (1000, 512, RELU, True, False), (1000, "q1", LRELU, True, True), (40001, 64, LRELU, False, False),
    (40001, "q1", RELU, False, True), (40000, 64, NONE, True, False),
]


@pytest.mark.parametrize("code", CODES)
@pytest.mark.parametrize("pixels,c,act,two,drop", APPLY_CASES)
def test_bn_apply(code, pixels, c, act, two, drop):
    c = _c(c, code)
    x = _fwd_data(pixels, c, code, pixels + c)
    g = _gen(c)
    gstride = c + 16
    sc = torch.rand(2, c, generator=g) + 0.5
    sh = torch.randn(2, c, generator=g) * 0.5
    vec = torch.full((2, 2, gstride), float("nan"))
    vec[0, :, :c], vec[1, :, :c] = sc, sh
    vd = _dev(vec)
    pg = (pixels * 3 // 8) if two else 0     # the populations need not be halves here
    mask = _drop_mask(pixels, c, 9) if drop else None
    md = _dev(mask, torch.uint8) if drop else None
    y, ldy, coffy = out_wide(pixels, c, code)
    _call(B.lib().gi_debug_bn_apply(B.get_ctx(), code, B.ptr(_dev(x, tdt(code))), B.ptr(y), pixels, c, ldy, coffy, B.ptr(vd[0]), B.ptr(vd[1]), act,
                                    B.ptr(md), 2.0, pg, gstride))
    _sync()
    ref = R.bn_apply(x, [sc[0], sc[1]] if two else sc[0], [sh[0], sh[1]] if two else sh[0], act, mask, 2.0, pg)
    check(f"bn_apply p={pixels} c={c} {ACT_NAME[act]} two={two} drop={drop}", y[:, coffy:coffy + c], ref, _tol(code))
    assert tail_untouched(y, c, coffy), "bn_apply wrote outside its channels"


def _acc_case(x, c, groups, reps, seed, zero_next=False, out_stride=None):
    """accumulators filled from per-slice fp32 sums of x (the addends a GEMM's tiles would add) + the reference from the SAME addends"""
    pixels = x.shape[0]
    pg = pixels // groups
    acc = _acc_block(c)
    sums = []
    for j in range(groups):
        xs = x[j * pg:(j + 1) * pg].double()
        nt = min(5, pg)
        bounds = [pg * k // nt for k in range(nt + 1)]
        a0 = torch.stack([xs[bounds[k]:bounds[k + 1]].sum(0) for k in range(nt)]).float()
        a1 = torch.stack([(xs[bounds[k]:bounds[k + 1]] ** 2).sum(0) for k in range(nt)]).float()
        _acc_add(acc, c, reps, j, 0, a0)
        _acc_add(acc, c, reps, j, 1, a1)
        sums.append((_totals(a0), _totals(a1)))
    gamma, beta, rmean, rvar = _bn_params(c, seed)
    out_stride = out_stride or c
    outs = [torch.full((out_stride * groups,), float("nan"), dtype=torch.float32, device="cuda") for _ in range(4)]
    rm, rv = _dev(rmean), _dev(rvar)
    zn = torch.full((600,), 0x0101010101010101, dtype=torch.int64, device="cuda")
    keep = [_dev(gamma), _dev(beta)]
    b = B.BnAccArgs(acc=B.ptr(acc), reps=reps, gamma=B.ptr(keep[0]), beta=B.ptr(keep[1]), running_mean=B.ptr(rm), running_var=B.ptr(rv),
                    scale=B.ptr(outs[0]), shift=B.ptr(outs[1]), save_mean=B.ptr(outs[2]), save_invstd=B.ptr(outs[3]), count=pg, momentum=0.1,
                    eps=1e-5, groups=groups, out_stride=out_stride, zero_next=B.ptr(zn) if zero_next else None, zero_words=300 if zero_next else 0)
    rs = R.bn_from_sums_groups(sums, pg, gamma, beta, rmean, rvar)
    return b, (acc, keep, outs, rm, rv, zn), rs


def _check_zero_next(zn, used, key):
    record_bits(key + " zero_next", zn)
    z = zn.cpu()
    if used:
        assert not z[:300].any(), "zero_next was not cleared"
        assert bool((z[300:] == 0x0101010101010101).all()), "words beyond zero_words were touched"
    else:
        assert bool((z == 0x0101010101010101).all())


ACC_CASES = [
    # pixels, c, act, groups, reps, dropout (0 none, 1 read, 2 draw), side copy, zero_next
    (1, "q1", LRELU, 1, 1, 0, False, False), (33, 64, RELU, 1, 2, 2, True, True), (1000, 64, NONE, 1, 3, 1, True, False),
    (1000, 512, LRELU, 2, 4, 0, False, True), (40001, 64, RELU, 1, 4, 2, False, False), (40000, "q1", NONE, 2, 2, 1, True, True),
    (33, "q256", LRELU, 1, 4, 0, True, False),
]


@pytest.mark.parametrize("code", CODES)
@pytest.mark.parametrize("pixels,c,act,groups,reps,drop,side,zero_next", ACC_CASES)
def test_bn_apply_acc(code, pixels, c, act, groups, reps, drop, side, zero_next):
    c = _c(c, code)
    x = _fwd_data(pixels, c, code, pixels + c + 1)
    out_stride = c + 8 if groups == 2 else c
    b, hold, rs = _acc_case(x, c, groups, reps, 21, zero_next, out_stride)
    _, _, outs, rm, rv, zn = hold
    seed, p = 0x1234567887654321, 0.5
    mask = _drop_mask(pixels, c, 4) if drop == 1 else None
    md = _dev(mask, torch.uint8) if drop == 1 else (torch.full((pixels, c), 7, dtype=torch.uint8, device="cuda") if drop == 2 else None)
    side_chunks = 3333
    src = torch.randint(-2 ** 31, 2 ** 31, (side_chunks * 4 + 8,), dtype=torch.int64, generator=_gen(6)).to(torch.int32).cuda() if side else None
    dst = torch.full((side_chunks * 4 + 8,), 42, dtype=torch.int32, device="cuda") if side else None
    y, ldy, coffy = out_wide(pixels, c, code)
    _call(B.lib().gi_debug_bn_apply_acc(B.get_ctx(), code, B.ptr(_dev(x, tdt(code))), B.ptr(y), pixels, c, ldy, coffy, act, B.ptr(md), 2.0, seed,
                                        p if drop == 2 else 0.0, C.byref(b), B.ptr(src), B.ptr(dst), side_chunks * 16 if side else 0))
    _sync()
    name = f"bn_apply_acc p={pixels} c={c} {ACT_NAME[act]} groups={groups} reps={reps} drop={drop}"
    if drop == 2:     # the stored mask, a mask filled by the stand-alone pass and the host restatement of the hash agree bit for bit
        filled = torch.full((pixels * c,), 9, dtype=torch.uint8, device="cuda")
        _call(B.lib().gi_debug_fill_dropout(B.get_ctx(), B.ptr(filled), pixels * c, seed, p))
        _sync()
        record_bits(name + " mask", md)
        assert torch.equal(md.view(-1), filled), "the mask drawn in the pass differs from gi_debug_fill_dropout's"
        nhost = min(pixels * c, 20000)
        assert torch.equal(filled[:nhost].cpu(), R.dropout_mask(seed, nhost, p)), "the device draw differs from the splitmix64 restatement"
        mask = md.cpu()
    ref = R.bn_apply(x, [r["scale"] for r in rs], [r["shift"] for r in rs], act, mask, 2.0, pixels // groups if groups == 2 else 0)
    check(name, y[:, coffy:coffy + c], ref, _tol(code))
    assert tail_untouched(y, c, coffy), "bn_apply_acc wrote outside its channels"
    _check_bn_vectors(name, outs, rm, rv, rs, c, out_stride)
    _check_zero_next(zn, zero_next, name)
    if side:
        assert torch.equal(dst[:side_chunks * 4], src[:side_chunks * 4]) and bool((dst[side_chunks * 4:] == 42).all()), "side copy"


@pytest.mark.parametrize("code", CODES)
def test_bn_apply_acc_offset_mean(code):
    pixels, c = 1000, 64
    x = _fwd_data(pixels, c, code, 77, offset_mean=True)
    b, hold, rs = _acc_case(x, c, 1, 4, 22)
    _, _, outs, rm, rv, _ = hold
    y, ldy, coffy = out_wide(pixels, c, code)
    _call(B.lib().gi_debug_bn_apply_acc(B.get_ctx(), code, B.ptr(_dev(x, tdt(code))), B.ptr(y), pixels, c, ldy, coffy, LRELU, None, 1.0, 0, 0.0,
                                        C.byref(b), None, None, 0))
    _sync()
    check("bn_apply_acc offset mean", y[:, coffy:coffy + c], R.bn_apply(x, rs[0]["scale"], rs[0]["shift"], LRELU), _tol(code))
    _check_bn_vectors("bn_apply_acc offset mean", outs, rm, rv, rs, c, c)


def test_bn_apply_large_grid_caps():
    """33000 pixels x 512 channels in fp16: 2.11 M chunks, past the 2048-workgroup cap of the plain pass (4 chunks per thread) and the
    1024-workgroup cap of the accumulator pass (8 per thread): every thread's persistent loop runs beyond its first prefetch rounds"""
    pixels, c, code = 33000, 512, F16
    xh = (torch.randn(pixels, c, generator=_gen(3)) * 1.2 + 0.25).half()
    xd = xh.cuda()
    ref = xh.double().numpy()
    g = _gen(4)
    sc, sh = torch.rand(c, generator=g) + 0.5, torch.randn(c, generator=g) * 0.5
    y = torch.full((pixels, c), SENT, dtype=torch.float16, device="cuda")
    _call(B.lib().gi_debug_bn_apply(B.get_ctx(), code, B.ptr(xd), B.ptr(y), pixels, c, c, 0, B.ptr(_dev(sc)), B.ptr(_dev(sh)), LRELU, None, 1.0, 0, 0))
    _sync()
    r = ref * sc.double().numpy() + sh.double().numpy()
    r[r < 0] *= 0.2
    check("bn_apply 33000x512", y, torch.from_numpy(r), _tol(code))
    del r
    # the accumulator pass on the same tensor: per-channel totals of the whole tensor as the addends
    x64 = torch.from_numpy(ref)
    a0, a1 = x64.sum(0)[None].float(), (x64 * x64).sum(0)[None].float()
    acc = _acc_block(c)
    _acc_add(acc, c, 1, 0, 0, a0)
    _acc_add(acc, c, 1, 0, 1, a1)
    gamma, beta, rmean, rvar = _bn_params(c, 5)
    rs = R.bn_from_sums(_totals(a0), _totals(a1), pixels, gamma, beta, rmean, rvar)
    outs = [torch.empty(c, dtype=torch.float32, device="cuda") for _ in range(4)]
    keep = [_dev(gamma), _dev(beta), _dev(rmean), _dev(rvar)]
    b = B.BnAccArgs(acc=B.ptr(acc), reps=1, gamma=B.ptr(keep[0]), beta=B.ptr(keep[1]), running_mean=B.ptr(keep[2]), running_var=B.ptr(keep[3]),
                    scale=B.ptr(outs[0]), shift=B.ptr(outs[1]), save_mean=B.ptr(outs[2]), save_invstd=B.ptr(outs[3]), count=pixels, momentum=0.1,
                    eps=1e-5, groups=1, out_stride=c, zero_next=None, zero_words=0)
    y.fill_(SENT)
    _call(B.lib().gi_debug_bn_apply_acc(B.get_ctx(), code, B.ptr(xd), B.ptr(y), pixels, c, c, 0, RELU, None, 1.0, 0, 0.0, C.byref(b), None, None, 0))
    _sync()
    r = ref
    r *= rs["scale"].numpy()
    r += rs["shift"].numpy()
    r[r < 0] = 0.0
    check("bn_apply_acc 33000x512", y, torch.from_numpy(r), _tol(code))


@pytest.mark.parametrize("code", CODES)
def test_bn_finalize_acc(code):
    c = 70 if code == F32 else 520      # the stand-alone form takes any channel count
    x = _fwd_data(64, c, code, 12)
    b, hold, rs = _acc_case(x, c, 2, 3, 23, True, c + 2)
    _, _, outs, rm, rv, zn = hold
    _call(B.lib().gi_debug_bn_finalize_acc(B.get_ctx(), c, C.byref(b)))
    _sync()
    _check_bn_vectors("bn_finalize_acc", outs, rm, rv, rs, c, c + 2)
    _check_zero_next(zn, True, "bn_finalize_acc")


# =================================================================================================================
# act_bn_bwd
# =================================================================================================================
class K:
    """one case of the backward: what the caller passes; dispatch() restates which kernels op_act_bn_bwd then launches"""

    def __init__(self, pixels, c, inp, act, sign, bn="train", groups=1, acc=0, reduce_done=False, zero_next=False, drop=False, small=None,
                 exact=False):
        self.pixels, self.c, self.inp, self.act, self.sign, self.bn, self.groups = pixels, c, inp, act, sign, bn, groups
        self.acc, self.reduce_done, self.zero_next, self.drop, self.small, self.exact = acc, reduce_done, zero_next, drop, small, exact

    def dispatch(self):
        inm = {"g1": 1, "g2": 2, "both": 3}[self.inp]
        need_y = inm & 2 or self.act != NONE
        load_y = bool(need_y and not (self.bn != "none" and self.sign == "scale"))
        ly = "y" if load_y else "-"
        if self.bn == "none":
            return "apply<bn=0>"
        groups = 2 if self.groups == 2 and self.bn == "train" else 1
        small_max = min(self.small if self.small is not None else 512, 2048)
        if self.bn == "train" and groups == 1 and self.pixels <= small_max and not self.reduce_done:
            nit = (self.pixels + 255) // 256
            return f"small<NIT={1 if nit <= 1 else 2 if nit <= 2 else 4 if nit <= 4 else 8}>"
        red = f"reduce<{inm},{ly}>"
        if self.acc:
            first = "" if self.bn == "eval" or self.reduce_done else red + "+"
            special = (inm, load_y, groups) in {(1, False, 2), (1, False, 1), (3, False, 1), (2, False, 1), (2, True, 1)}
            return first + (f"apply_acc<{inm},{ly},G{groups}>" if special else f"apply<bn=2,G{groups}>")
        if self.bn == "eval":
            return "sums(0 rows)+apply<bn=1,G1>"
        return f"{red}+sums+apply<bn=1,G{groups}>"

    def id(self):
        return f"{self.dispatch()}|{self.fields()}"

    def fields(self):
        s = f"p{self.pixels}|c{self.c}|{self.inp}|{ACT_NAME[self.act]}|sign={self.sign}"
        for flag, text in ((self.bn == "eval", "eval"), (self.acc, f"reps{self.acc}"), (self.reduce_done, "reduce_done"),
                           (self.zero_next, "zero_next"), (self.drop, "drop"), (self.small is not None, f"SMALL={self.small}"),
                           (self.exact, "exact")):
            if flag:
                s += "|" + text
        return s

    def key(self):
        """the case in the bit record: its own fields, not the kernels"""
        return f"{self.fields()}|bn={self.bn}|groups={self.groups}"


BWD_CASES = [
    # no BatchNorm: every input combination and activation
    K(1000, 64, "g1", NONE, None, "none"), K(1000, 64, "g1", RELU, "y", "none", drop=True), K(1000, 64, "g1", LRELU, "y", "none"),
    K(33, "q1", "g2", NONE, "y", "none"), K(40001, 64, "g2", RELU, "y", "none"), K(1000, "q256", "g2", LRELU, "y", "none"),
    K(1000, 64, "both", NONE, "y", "none"), K(1, 64, "both", RELU, "y", "none", drop=True), K(40001, "q1", "both", LRELU, "y", "none"),
    # the one-launch kernel
    K(1, 64, "g1", LRELU, "scale"), K(200, 64, "both", LRELU, "scale"), K(256, "q1", "g2", RELU, "y", drop=True),
    K(257, 64, "both", RELU, "y"), K(512, 512, "g1", LRELU, "scale"), K(512, 64, "g2", RELU, "scale", acc=2, zero_next=True),
    K(257, 64, "g1", NONE, None, exact=True), K(512, "q256", "both", RELU, "scale", exact=True),
    K(1000, 64, "both", LRELU, "scale", small=2048), K(1000, 64, "g2", RELU, "y", small=2048, drop=True),
    K(2048, 64, "g1", LRELU, "y", small=2048), K(2048, "q1", "both", RELU, "scale", small=2048, exact=True),
    K(513, 64, "g1", LRELU, "scale", small=0, acc=1),     # GI_BN_BWD_SMALL = 0 turns the one-launch kernel off
    # three launches
    K(513, 64, "g1", LRELU, "scale"), K(513, "q256", "both", RELU, "y", drop=True), K(40001, 64, "g2", RELU, "scale"),
    K(40001, "q1", "g1", LRELU, "y"), K(40001, 64, "both", NONE, "y", exact=True), K(2048, 64, "g1", LRELU, "scale", groups=2),
    K(2048, 64, "both", RELU, "y", groups=2, exact=True), K(2048, 64, "g2", LRELU, "y", groups=2),
    # exact accumulators: the five specialised apply kernels ...
    K(2048, 64, "g1", LRELU, "scale", groups=2, acc=4, zero_next=True), K(1000, 64, "g1", LRELU, "scale", acc=1),
    K(40001, 64, "both", LRELU, "scale", acc=2), K(1000, 512, "g2", RELU, "scale", acc=4, zero_next=True),
    K(1000, 64, "g2", RELU, "y", acc=2, drop=True), K(40001, "q1", "g1", NONE, None, acc=4, exact=True),
    K(2048, 64, "g1", RELU, "scale", groups=2, acc=2, exact=True), K(1000, 64, "both", RELU, "scale", acc=1, exact=True),
    # ... and the generic one
    K(1000, 64, "both", LRELU, "y", acc=2), K(2048, 64, "both", LRELU, "scale", groups=2, acc=4), K(1000, 64, "g1", LRELU, "y", acc=1, zero_next=True),
    K(2048, "q1", "g1", RELU, "y", groups=2, acc=2, drop=True), K(2048, 64, "both", RELU, "y", groups=2, acc=1, exact=True),
    # the sums already in the accumulators
    K(1000, 64, "g1", LRELU, "scale", acc=2, reduce_done=True), K(200, 64, "both", LRELU, "scale", acc=4, reduce_done=True, zero_next=True),
    K(2048, 64, "g1", LRELU, "scale", groups=2, acc=1, reduce_done=True),
    # running-statistics BatchNorm
    K(1000, 64, "g1", LRELU, "scale", "eval"), K(200, 64, "both", RELU, "y", "eval"), K(1000, 64, "g1", LRELU, "scale", "eval", acc=2),
    K(1000, 64, "both", LRELU, "y", "eval", acc=1), K(200, 64, "g2", RELU, "y", "eval", acc=4, drop=True),
]


def _bwd_inputs(k, code):
    c, P = _c(k.c, code), k.pixels
    groups = k.groups if k.bn == "train" else 1
    pg = P // groups
    g = _gen(P * 7 + c + len(k.id()))
    d = {"c": c, "groups": groups, "pg": pg}
    stride = c + 8 if groups == 2 else c
    if k.exact:
        x = torch.randint(-3, 4, (P, c), generator=g).float()
        mean, inv = torch.zeros(groups, c), torch.ones(groups, c)
        scale, shift = torch.ones(groups, c), torch.full((groups, c), 0.5)
        gamma = torch.randint(1, 3, (c,), generator=g).float()
        g1, g2 = (torch.randint(-2, 3, (P, c), generator=g).float() for _ in range(2))
        pre_g, pre_b = (torch.randint(-9, 10, (c,), generator=g).float() for _ in range(2))
        d["ils"] = 0.25
    else:
        x = torch.randn(P, c, generator=g) * 1.2 + torch.randn(c, generator=g) * 0.5
        if groups == 2:
            x[pg:] = x[pg:] * 1.5 - 0.3
        gamma = torch.rand(c, generator=g) + 0.5
        beta = torch.randn(c, generator=g) * 0.3
        xg = x.reshape(groups, pg, c).double()
        mean = xg.mean(1).float()
        if pg == 1:
            # one pixel: with mean = x every term of dx cancels and nothing but rounding is left to compare. The mean is an input
            # like any other: off the pixel, xhat is of order one and dx = -gamma * inv * xhat^2 * dz is a well-conditioned result
            mean = mean + 0.7
        # (an input like any other: the 0.1 keeps a one-pixel population's scale moderate, so that x can be moved off the kink)
        inv = (1.0 / torch.sqrt(xg.var(1, unbiased=False) + 0.1)).float()
        scale = (gamma * inv).float()
        shift = (beta - mean * scale).float()
        g1, g2 = (quant(torch.randn(P, c, generator=g), code) for _ in range(2))
        pre_g, pre_b = torch.randn(c, generator=g), torch.randn(c, generator=g)
        d["ils"] = 0.375
    rep = lambda v: v.repeat_interleave(pg, 0)   # noqa: E731
    x, t = settle(x, rep(scale), rep(shift), code)
    drop_scale = 2.0 if k.drop else 1.0
    mask = _drop_mask(P, c, 31) if k.drop else None
    y = R.act_fwd(t, k.act)
    if k.drop:
        y = torch.where(mask.bool(), y * drop_scale, torch.zeros_like(y))
    y = quant(y.float(), code)
    if k.act == NONE and k.bn == "none":
        # no activation in front: y is a free input; keep it off zero all the same
        y = torch.where(y.abs() < KINK, torch.full_like(y, 2 * KINK), y)
    assert bool(((y != 0) | (t < 0) | (mask == 0 if k.drop else False)).all()), "a live activation output rounded to zero"
    sgn = {"y": y, "scale": t, None: None}[k.sign]
    a1 = g1 if k.inp in ("g1", "both") else None
    a2 = g2 if k.inp in ("g2", "both") else None
    d.update(x=x, y=y, g1=a1, g2=a2, gamma=gamma, mean=mean, inv=inv, scale=scale, shift=shift, stride=stride, pre_g=pre_g, pre_b=pre_b,
             drop_scale=drop_scale, dz=R.dz_of(a1, a2, sgn, k.act, drop_scale))
    return d


def _strided(v, stride):
    """(groups, c) -> device vector with the populations `stride` floats apart, NaN between"""
    out = torch.full((v.shape[0], stride), float("nan"))
    out[:, :v.shape[1]] = v
    return _dev(out.reshape(-1))


@pytest.mark.parametrize("code", CODES)
@pytest.mark.parametrize("k", [pytest.param(k, id=k.id()) for k in BWD_CASES])
def test_act_bn_bwd(code, k):
    d = _bwd_inputs(k, code)
    c, P, groups, pg = d["c"], k.pixels, d["groups"], d["pg"]
    has_bn = k.bn != "none"
    hold = {}
    a = B.ActBnBwdArgs()
    for nm in ("g1", "g2"):
        if d[nm] is not None:
            hold[nm], ld, coff = wide(d[nm], code)
            setattr(a, nm, B.ptr(hold[nm])), setattr(a, "ld" + nm, ld), setattr(a, "coff" + nm, coff)
    if k.sign == "y" or not has_bn:
        hold["y"], a.ldy, a.coffy = wide(d["y"], code)
        a.y = B.ptr(hold["y"])
    dx = torch.full((P, c), float("nan"), dtype=tdt(code), device="cuda")
    a.dx, a.pixels, a.c, a.act, a.drop_scale = B.ptr(dx), P, c, k.act, d["drop_scale"]
    a.has_bn, a.eval_bn, a.groups, a.stat_stride = int(has_bn), int(k.bn == "eval"), k.groups, d["stride"]
    dgamma, dbeta = _dev(d["pre_g"]), _dev(d["pre_b"])
    a.dgamma, a.dbeta, a.inv_loss_scale = B.ptr(dgamma), B.ptr(dbeta), d["ils"]
    zn = torch.full((600,), 0x0101010101010101, dtype=torch.int64, device="cuda")
    sums_given = None
    if has_bn:
        hold["x"] = _dev(d["x"], tdt(code))
        hold["v"] = [_dev(d["gamma"]), _strided(d["mean"], d["stride"]), _strided(d["inv"], d["stride"])]
        a.x, a.gamma, a.save_mean, a.save_invstd = B.ptr(hold["x"]), B.ptr(hold["v"][0]), B.ptr(hold["v"][1]), B.ptr(hold["v"][2])
        hold["scr"] = [torch.full(((P // 32 + 8) * 2 * c,), float("nan"), device="cuda"), torch.full((groups * 8 * c,), float("nan"), device="cuda")]
        a.partials, a.sums = B.ptr(hold["scr"][0]), B.ptr(hold["scr"][1])
        if k.sign == "scale":
            hold["f"] = [_strided(d["scale"], d["stride"]), _strided(d["shift"], d["stride"])]
            a.fwd_scale, a.fwd_shift = B.ptr(hold["f"][0]), B.ptr(hold["f"][1])
        if k.acc:
            hold["acc"] = _acc_block(c)
            a.acc, a.acc_reps = B.ptr(hold["acc"]), k.acc
            if k.zero_next:
                a.zero_next, a.zero_words = B.ptr(zn), 300
            if k.reduce_done:     # the test adds the two sums itself, three addends each; the reference works from the same addends
                sums_given = []
                for j in range(groups):
                    sl = slice(j * pg, (j + 1) * pg)
                    xhat = (d["x"][sl].double() - d["mean"][j].double()) * d["inv"][j].double()
                    pair = []
                    for q, s in enumerate((d["dz"][sl].sum(0), (d["dz"][sl] * xhat).sum(0))):
                        third = (s / 3).float()
                        add = torch.stack([third, third, (s - 2 * third.double()).float()])
                        _acc_add(hold["acc"], c, k.acc, j, q, add)
                        pair.append(_totals(add))
                    sums_given.append(tuple(pair))
                a.reduce_done = 1
    if k.small is not None:
        B.set_option("GI_BN_BWD_SMALL", k.small)
    try:
        _call(B.lib().gi_debug_act_bn_bwd(B.get_ctx(), code, C.byref(a)))
        _sync()
    finally:
        if k.small is not None:
            B.set_option("GI_BN_BWD_SMALL", -1)
    name, key = f"act_bn_bwd {k.id()}", f"act_bn_bwd {k.key()}"
    pre_g, pre_b, ils = d["pre_g"].double(), d["pre_b"].double(), d["ils"]
    if not has_bn:
        ref = d["dz"]
    else:
        ref, rb, rg, ab, ag = R.act_bn_bwd(d["dz"], d["x"], d["gamma"], list(d["mean"]), list(d["inv"]), groups, k.bn == "eval", sums_given)
    check(name + " dx", dx, ref, _tol(code), key + " dx")
    if k.bn == "train":
        if k.exact:
            record_bits(key + " dbeta", dbeta), record_bits(key + " dgamma", dgamma)
            assert torch.equal(dbeta.cpu().double(), pre_b + ils * rb), name + ": dbeta is not the exact sum"
            assert torch.equal(dgamma.cpu().double(), pre_g + ils * rg), name + ": dgamma is not the exact sum"
        else:
            check_sum(name + " dbeta", dbeta, pre_b + ils * rb, pre_b.abs() + ils * ab, key=key + " dbeta")
            check_sum(name + " dgamma", dgamma, pre_g + ils * rg, pre_g.abs() + ils * ag, key=key + " dgamma")
    else:
        record_bits(key + " dbeta", dbeta), record_bits(key + " dgamma", dgamma)
        assert torch.equal(dbeta.cpu().double(), pre_b) and torch.equal(dgamma.cpu().double(), pre_g), name + ": parameter gradients were touched"
    _check_zero_next(zn, bool(k.zero_next and k.acc and k.bn == "train"), key)


def test_act_bn_bwd_rejects_dropout_behind_lrelu():
    c, P = 64, 16
    t = torch.ones(P, c, device="cuda")
    dx = torch.empty_like(t)
    a = B.ActBnBwdArgs(g1=B.ptr(t), ldg1=c, y=B.ptr(t), ldy=c, dx=B.ptr(dx), pixels=P, c=c, act=LRELU, drop_scale=2.0, groups=1,
                       inv_loss_scale=1.0)
    assert B.lib().gi_debug_act_bn_bwd(B.get_ctx(), F32, C.byref(a)) != 0
    why = B.lib().gi_last_error().decode()
    assert "drop_scale" in why and "y > 0" in why, why
    a.act = NONE
    assert B.lib().gi_debug_act_bn_bwd(B.get_ctx(), F32, C.byref(a)) != 0
    a.act, a.groups = RELU, 3
    assert B.lib().gi_debug_act_bn_bwd(B.get_ctx(), F32, C.byref(a)) != 0 and "groups" in B.lib().gi_last_error().decode()
    a.groups = 1
    _call(B.lib().gi_debug_act_bn_bwd(B.get_ctx(), F32, C.byref(a)))
    _sync()


# =================================================================================================================
# InstanceNorm
# =================================================================================================================
IN_OPTS = [(NONE, False), (RELU, True), (LRELU, False)]


def _in_data(n, hw, c, code, g):
    """x (n * hw, c) of the compute type with no (x - mean) * inv of its own planes within 2^-6 of zero (hw > 1). Asserts it."""
    P = n * hw
    x = quant(torch.randn(P, c, generator=g) * (torch.rand(c, generator=g) + 0.5) + torch.randn(c, generator=g) * 0.5, code)
    # the activation's input is (x - mean) * inv of x itself: move offenders along x, keep the statistics the reference's own
    for _ in range(4):
        _, mean, inv = R.in_forward(x, n, hw, NONE)
        t = (x.double().reshape(n, hw, c) - mean[:, None]) * inv[:, None]
        bad = (t.abs() < 2 * KINK).reshape(P, c)
        if hw == 1 or not bad.any():
            break
        x = quant(torch.where(bad, x + torch.where(t.reshape(P, c) >= 0, 1.0, -1.0) * 4 * KINK / inv.repeat_interleave(hw, 0).float(), x), code)
    assert hw == 1 or float(t.abs().min()) >= KINK, "an activation input within 2^-6 of zero survived the construction"
    return x


@pytest.mark.parametrize("code", CODES)
@pytest.mark.parametrize("c", ["q1", "q3", 512])
@pytest.mark.parametrize("hw", [1, 4, 255, 256, 257, 4096])
def test_instance_norm(code, c, hw):
    n, c = 3, _c(c, code)
    act, drop = IN_OPTS[(hw + c) % 3]
    P = n * hw
    g = _gen(hw + c)
    x = _in_data(n, hw, c, code, g)
    drop_scale = 2.0 if drop else 1.0
    mask = _drop_mask(P, c, 3) if drop else None
    yref, mean, inv = R.in_forward(x, n, hw, act, mask, drop_scale)
    xd = _dev(x, tdt(code))
    y, ldy, coffy = out_wide(P, c, code)
    stats = torch.full((n, c, 2), float("nan"), device="cuda")
    md = _dev(mask, torch.uint8) if drop else None
    _call(B.lib().gi_debug_in_forward(B.get_ctx(), code, B.ptr(xd), B.ptr(y), n, hw, c, ldy, coffy, act, B.ptr(md), drop_scale, 1e-5, B.ptr(stats)))
    _sync()
    name = f"instance_norm hw={hw} c={c} {ACT_NAME[act]} drop={drop}"
    check(name + " mean", stats[:, :, 0], mean, VEC_TOL)
    check(name + " inv", stats[:, :, 1], inv, VEC_TOL)
    if hw == 1:
        assert not y[:, coffy:coffy + c].any(), "one pixel per plane: y must be 0"
        assert torch.equal(stats[:, :, 0].cpu(), x.reshape(n, c))
    check(name + " y", y[:, coffy:coffy + c], yref, _tol(code))
    assert tail_untouched(y, c, coffy)
    # backward from the forward's own saved output and statistics
    g1, g2 = (quant(torch.randn(P, c, generator=g), code) for _ in range(2))
    ysaved = y[:, coffy:coffy + c].float().cpu()
    if hw > 1:
        assert torch.equal(ysaved > 0, yref > 0), "the saved output's signs differ from the reference's although no input is near the kink"
    hold = [wide(g1, code), wide(g2, code)]
    dx = torch.full((P, c), float("nan"), dtype=tdt(code), device="cuda")
    a = B.ActBnBwdArgs(g1=B.ptr(hold[0][0]), ldg1=hold[0][1], coffg1=hold[0][2], g2=B.ptr(hold[1][0]), ldg2=hold[1][1], coffg2=hold[1][2],
                       y=B.ptr(y), ldy=ldy, coffy=coffy, x=B.ptr(xd), dx=B.ptr(dx), pixels=P, c=c, act=act, drop_scale=drop_scale, groups=1,
                       inv_loss_scale=1.0)
    _call(B.lib().gi_debug_act_in_bwd(B.get_ctx(), code, C.byref(a), n, hw, B.ptr(stats)))
    _sync()
    sm, si = stats[:, :, 0].cpu(), stats[:, :, 1].cpu()
    ref = R.act_in_bwd(R.dz_of(g1, g2, ysaved, act, drop_scale), x, n, hw, sm, si)
    if hw == 1:
        assert not dx.any(), "one pixel per plane passes no gradient"
    check(name + " dx", dx, ref, _tol(code))


@pytest.mark.parametrize("code", CODES)
@pytest.mark.parametrize("hw", [257, 4096])
def test_instance_norm_offset_mean(code, hw):
    n, c = 3, 64
    g = _gen(hw)
    std = torch.rand(c, generator=g) + 0.5
    x = quant(torch.randn(n * hw, c, generator=g) * std + 8.0 * std, code)
    yref, mean, inv = R.in_forward(x, n, hw, LRELU)
    y, ldy, coffy = out_wide(n * hw, c, code)
    stats = torch.full((n, c, 2), float("nan"), device="cuda")
    _call(B.lib().gi_debug_in_forward(B.get_ctx(), code, B.ptr(_dev(x, tdt(code))), B.ptr(y), n, hw, c, ldy, coffy, LRELU, None, 1.0, 1e-5, B.ptr(stats)))
    _sync()
    check(f"instance_norm offset mean hw={hw} mean", stats[:, :, 0], mean, VEC_TOL)
    check(f"instance_norm offset mean hw={hw} inv", stats[:, :, 1], inv, VEC_TOL)
    check(f"instance_norm offset mean hw={hw} y", y[:, coffy:coffy + c], yref, _tol(code))


# =================================================================================================================
# the small ops
# =================================================================================================================
@pytest.mark.parametrize("code", CODES)
@pytest.mark.parametrize("pixels", [1, 33, 40001])
def test_bias_grad(code, pixels):
    c = 64
    g = _gen(pixels)
    scratch = torch.full(((pixels // 32 + 8) * 2 * c,), float("nan"), device="cuda")
    dz = quant(torch.randn(pixels, c, generator=g), code)
    pre = torch.randn(c, generator=g)
    db = _dev(pre)
    _call(B.lib().gi_debug_bias_grad(B.get_ctx(), code, B.ptr(_dev(dz, tdt(code))), pixels, c, 0.375, B.ptr(db), B.ptr(scratch)))
    _sync()
    check_sum(f"bias_grad p={pixels}", db, pre.double() + 0.375 * dz.double().sum(0), pre.abs().double() + 0.375 * dz.double().abs().sum(0))
    dz = torch.randint(-4, 5, (pixels, c), generator=g).float()
    pre = torch.randint(-9, 10, (c,), generator=g).float()
    db = _dev(pre)
    _call(B.lib().gi_debug_bias_grad(B.get_ctx(), code, B.ptr(_dev(dz, tdt(code))), pixels, c, 0.25, B.ptr(db), B.ptr(scratch)))
    _sync()
    assert torch.equal(db.cpu().double(), pre.double() + 0.25 * dz.double().sum(0)), "bias_grad: not the exact sum"


def test_tanh_bwd():
    n = 70001
    g = _gen(1)
    dy, y = torch.randn(n, generator=g), torch.tanh(torch.randn(n, generator=g) * 2)
    dx = torch.full((n + 8,), SENT, device="cuda")
    _call(B.lib().gi_debug_tanh_bwd(B.get_ctx(), B.ptr(_dev(dy)), B.ptr(_dev(y)), B.ptr(dx), n, 0.375))
    _sync()
    check("tanh_bwd", dx[:n], R.tanh_bwd(dy, y, 0.375), 2e-5)
    assert bool((dx[n:] == SENT).all())


@pytest.mark.parametrize("to_nhwc", [1, 0])
def test_mask_layout(to_nhwc):
    n, c, hw = 3, 40, 77
    src = torch.randint(0, 256, (n * c * hw,), generator=_gen(2)).to(torch.uint8)
    dst = torch.full((n * c * hw + 64,), 201, dtype=torch.uint8, device="cuda")
    _call(B.lib().gi_debug_mask_layout(B.get_ctx(), B.ptr(_dev(src, torch.uint8)), B.ptr(dst), n, c, hw, to_nhwc))
    _sync()
    assert torch.equal(dst[:n * c * hw].cpu(), R.mask_layout(src, n, c, hw, bool(to_nhwc)).reshape(-1))
    assert bool((dst[n * c * hw:] == 201).all())


def test_fill_dropout_matches_the_hash():
    n, seed = 20011, 0xFEDCBA9876543210
    for p in (0.5, 0.25):
        m = torch.full((n + 16,), 9, dtype=torch.uint8, device="cuda")
        _call(B.lib().gi_debug_fill_dropout(B.get_ctx(), B.ptr(m), n, seed, p))
        _sync()
        assert torch.equal(m[:n].cpu(), R.dropout_mask(seed, n, p)) and bool((m[n:] == 9).all())


@pytest.mark.parametrize("code", CODES)
def test_mul_slope(code):
    n = 8 * 9001
    g = _gen(3)
    t, a = quant(torch.randn(n, generator=g), code), quant(torch.randn(n, generator=g), code)
    a[::7] = 0.0     # zero is on the 0.2 side
    out = torch.full((n + 8,), SENT, dtype=tdt(code), device="cuda")
    _call(B.lib().gi_debug_mul_slope(B.get_ctx(), code, B.ptr(_dev(t, tdt(code))), B.ptr(_dev(a, tdt(code))), B.ptr(out), n))
    _sync()
    check("mul_slope", out[:n], R.mul_slope(t, a), _tol(code))
    assert bool((out[n:] == SENT).all())


@pytest.mark.parametrize("code", CODES)
@pytest.mark.parametrize("pixels", [33, 2048])
def test_bn_tangent_inject(code, pixels):
    c = 64
    g = _gen(pixels)
    x = quant(torch.randn(pixels, c, generator=g) * 1.2 + 0.3, code)
    dta, tx = (quant(torch.randn(pixels, c, generator=g), code) for _ in range(2))
    y = quant(torch.randn(pixels, c, generator=g), code)
    y = torch.where(y.abs() < KINK, torch.full_like(y, -2 * KINK), y)
    gamma = torch.rand(c, generator=g) + 0.5
    mean = x.double().mean(0).float()
    inv = (1.0 / torch.sqrt(x.double().var(0, unbiased=False) + 1e-5)).float()
    pre = quant(torch.randn(pixels, c, generator=g), code)
    pre_g = torch.randn(c, generator=g)
    dxp, dgamma = _dev(pre, tdt(code)), _dev(pre_g)
    partials = torch.full(((pixels // 32 + 8) * 5 * c,), float("nan"), device="cuda")
    sums = torch.full((5 * c,), float("nan"), device="cuda")
    _call(B.lib().gi_debug_bn_tangent_inject(B.get_ctx(), code, B.ptr(_dev(dta, tdt(code))), B.ptr(_dev(y, tdt(code))), B.ptr(_dev(tx, tdt(code))),
                                             B.ptr(_dev(x, tdt(code))), B.ptr(dxp), pixels, c, B.ptr(_dev(gamma)), B.ptr(_dev(mean)), B.ptr(_dev(inv)),
                                             B.ptr(dgamma), 0.375, B.ptr(partials), B.ptr(sums)))
    _sync()
    inj, dg = R.bn_tangent_inject(dta, y, tx, x, gamma, mean, inv)
    check(f"bn_tangent_inject p={pixels} dxp", dxp, pre.double() + inj, _tol(code))
    # A = sum(a * u) with u = tx - m1 - xhat * m2: the addends of dgamma
    a = dta.double() * R.lrelu_slope(y)
    xh = (x.double() - mean.double()) * inv.double()
    u = tx.double() - tx.double().mean(0) - xh * (tx.double() * xh).mean(0)
    terms = (a.abs() * (tx.double().abs() + tx.double().mean(0).abs() + xh.abs() * (tx.double() * xh).mean(0).abs())).sum(0)
    assert float(((a * u).sum(0) * inv.double() - dg).abs().max()) < 1e-9
    check_sum(f"bn_tangent_inject p={pixels} dgamma", dgamma, pre_g.double() + 0.375 * dg, pre_g.abs().double() + 0.375 * terms * inv.double())


@pytest.mark.parametrize("hw", [1, 255, 65536])
def test_gp_direction(hw):
    n, lam = 5, 10.0
    g = torch.randn(n, hw, generator=_gen(hw)) * (3.0 / math.sqrt(hw)) * torch.tensor([0.2, 0.5, 1.0, 2.0, 4.0])[:, None]
    gd = _dev(g)
    sumsq, amax = torch.full((n,), float("nan"), device="cuda"), torch.full((n,), float("nan"), device="cuda")
    v = torch.full((n, hw), float("nan"), device="cuda")
    pen, sc = torch.full((1,), float("nan"), device="cuda"), torch.full((2,), float("nan"), device="cuda")
    _call(B.lib().gi_debug_gp_direction(B.get_ctx(), B.ptr(gd), n, hw, lam, B.ptr(sumsq), B.ptr(amax), B.ptr(v), B.ptr(pen), B.ptr(sc)))
    _sync()
    vref, sref, pref = R.gp_direction(g, lam)
    s, inv_s = float(sc[0]), float(sc[1])
    assert s > 0 and math.frexp(s)[0] == 0.5 and s * inv_s == 1.0, f"the scale {s} is not a power of two with its exact inverse"
    vmax = float(v.abs().max())
    assert 1.0 <= vmax < 2.0, f"max|v| = {vmax} outside [1, 2)"
    check(f"gp_direction hw={hw} v * sc[1]", v.double().cpu() * inv_s, vref, 2e-5)
    check(f"gp_direction hw={hw} sumsq", sumsq, (g.double() ** 2).sum(1), 2e-5)
    assert torch.equal(amax.cpu(), g.abs().max(1).values), "amax is a maximum: exact"
    check(f"gp_direction hw={hw} penalty", pen, torch.tensor([pref], dtype=F64), 2e-5)


def test_gp_unscale_add():
    n = 70001
    g = _gen(8)
    src, pre = torch.randn(n, generator=g), torch.randn(n, generator=g)
    dst = torch.full((n + 8,), SENT, device="cuda")
    dst[:n] = pre.cuda()
    sc = torch.tensor([64.0, 1.0 / 64.0], device="cuda")
    _call(B.lib().gi_debug_gp_unscale_add(B.get_ctx(), B.ptr(_dev(src)), B.ptr(sc), B.ptr(dst), n))
    _sync()
    assert torch.equal(dst[:n].cpu(), pre + src / 64.0), "gp_unscale_add: a power-of-two scale and one add are exact in fp32 rounding"
    assert bool((dst[n:] == SENT).all())
