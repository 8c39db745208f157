"""GPU tier: the public entry points of csrc/elementwise.hip ONE OP AT A TIME through the C-ABI, against the restatement of
tests/elementwise_ref.py (proved against torch in float64 by tests/test_elementwise_ref_cpu.py).

  bit-exact  the mask pipeline, gi_mul, gi_clamp, the conversions and both weight packs (gi_pack_weights and, through the
             gi_debug_pack_weights_batch seam, the two kernels that re-pack a network after every update): the device bits equal the
             restatement's.
  exact      the reconstruction losses on integer-valued inputs, whose partial sums are all exact in fp32: the value EQUALS
             float32(reference), so a dropped or doubled element shows whatever the tolerance.
  bounded    gi_add, gi_interpolate, the float-valued losses and their gradients, the optimizer moments: per element
             |got - E| <= (roundings + 1) * 2^-24 * (magnitudes), elementwise_ref.bound; parameters after an update: the rule of
             tests/test_losses_gpu.py (1e-6 of the value or 1e-3 of one move) per element; adversarial losses: 2e-6 per element.

Sizes reach past every grid cap (2048 workgroups of the grid-stride loops, 1024 of the loss partials, 64 on x of gi_interpolate).
Inputs stand in NaN padding and are compared with a snapshot afterwards, outputs stand in a sentinel that must survive. Every test
prints its worst ratio.

Found by this file: mask_composite_kernel, whose comment promises the two roundings of the reference's masked + gen * mask_c,
compiled to one fused multiply-add: with a fractional mask_c every test_mask_composite[fractional-*] case failed, on as many
elements as the inputs make sensitive to fusing (a third of them at the large counts, one ulp each). The kernel now runs under
`#pragma clang fp contract(off)` (__fmul_rn / __fadd_rn are plain operators to this compiler and contract as well); binary masks,
the only ones the training path produces, gave and give the same bits. The masked losses' a m - b m passed as compiled (where a == b
under a fractional mask a fused product would leave a residue instead of 0); masked_diff now keeps it so by the same pragma. And the
BCE loss took log(1 - p) from the fp32 difference 1.f - p, which is 1 for p < 2^-25: test_bce_saturation read a loss of 0 where the float64
reference has p = 2^-30. It now takes log1p(-p); the gradient was and is within 2e-6 of its reference on every element."""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import elementwise_ref as R  # noqa: E402
from gpu_util import B  # noqa: E402

COUNTS = (1, 7, 255, 256, 257, 1023, 4099, 2 ** 20 + 5, 2 ** 21 + 3)
PAD = 4          # elements in front of and behind every view
SENT = 12344.0     # representable in fp16 too
NAN = float("nan")
VAL_TOL = GRAD_TOL = 2e-6          # tests/test_losses_gpu.py
_GUARDS = []


@pytest.fixture(autouse=True)
def _release_device_buffers():
    yield
    _GUARDS.clear()


def _call(status):
    if status != 0 and b"->" in (B.lib().gi_last_error() or b""):     # a HIP error, not a rejected argument: nothing may follow it
        pytest.exit("HIP error: " + B.lib().gi_last_error().decode(errors="replace"), returncode=3)
    B.check(status)


def _rejected(status):
    """the call was refused on the host, before any launch"""
    why = B.lib().gi_last_error() or b""
    if status != 0 and b"->" in why:
        pytest.exit("HIP error: " + why.decode(errors="replace"), returncode=3)
    return status != 0 and bool(why)


def _sync():
    try:
        torch.cuda.synchronize()
    except RuntimeError as e:     # a fault of the device: the session ends here, no further launch
        pytest.exit(f"device error: {e}", returncode=3)


def _raw(t):
    return t.view({1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}[t.element_size()])


def _buf(values, off, fill, out):
    """a device allocation of PAD + off + n + PAD elements with `values` at offset PAD + off and `fill` elsewhere. It lives until the
    test ends (it is handed over as a bare pointer) and _check_guards compares it with the snapshot taken here."""
    v = torch.from_numpy(np.ascontiguousarray(values).reshape(-1))
    buf = torch.full((PAD + off + v.numel() + PAD,), fill, dtype=v.dtype, device="cuda")
    assert buf.data_ptr() % 16 == 0
    view = buf[PAD + off: PAD + off + v.numel()]
    view.copy_(v)
    _GUARDS.append((buf, buf.clone(), PAD + off, PAD + off + v.numel(), out))
    return view


def _in(values, off=0):
    """an input the kernel may only read: NaN (or -1 for integers) all round"""
    return _buf(values, off, NAN if np.asarray(values).dtype.kind == "f" else -1, False)


def _out(n, off=0, dtype=np.float32):
    """an output of n elements holding the sentinel, and the sentinel all round"""
    return _buf(np.full(n, SENT, dtype=dtype), off, SENT, True)


def _inout(values, off=0):
    return _buf(values, off, SENT, True)


def _check_guards(what=""):
    """after the op: every input is bit-identical to its snapshot, and so is the padding of every output"""
    _sync()
    for buf, before, lo, hi, out in _GUARDS:
        a, b = _raw(buf), _raw(before)
        if out:
            assert torch.equal(a[:lo], b[:lo]) and torch.equal(a[hi:], b[hi:]), f"{what}: elements outside an output's range were written"
        else:
            assert torch.equal(a, b), f"{what}: an input was modified"
    _GUARDS.clear()


def _np(view):
    return view.cpu().numpy()


def _untouched(view):
    return bool((view == SENT).all())


def _assert_bits(what, got, ref):
    assert R.same_bits(got, ref), f"{what}: {R.first_diff(got, ref)}"


def _assert_ratio(what, got, E, bnd):
    ratio = R.worst_ratio(got, E, bnd)
    assert ratio <= 1.0, f"{what}: |got - E| is {ratio:.3f} of the bound; {R.first_bad(got, E, bnd)}"
    return ratio


def _rng(*seed):
    return np.random.default_rng(list(seed))


def _wide(r, n, lo=-3, hi=4):
    """float32 values of magnitudes 1e-3 .. 1e3, both signs"""
    return (r.standard_normal(n) * 10.0 ** r.integers(lo, hi, n)).astype(np.float32)


def _lib():
    return B.lib(), B.get_ctx()


# =====================================================================================================================================
# mask pipeline, gi_mul: bit-exact
# =====================================================================================================================================
MASK_VALUES = np.array([0.0, 1.0, 0.3, 0.75, 1e-30, 2.0 ** -140, 0.999], dtype=np.float32)     # the tiny ones: ceil gives 1


@pytest.mark.parametrize("count", COUNTS)
def test_mask_apply(count):
    lib, ctx = _lib()
    r = _rng(1, count)
    ground, mask = _wide(r, count), r.choice(MASK_VALUES, count)
    for flags in (0, 1, 2, 3):
        ref_c, ref_m = R.mask_apply(ground, mask, flags)
        for with_c in (True, False):
            g, m = _in(ground, 1), _in(mask)
            mc, masked = (_out(count) if with_c else None), _out(count, 1)
            _call(lib.gi_mask_apply(ctx, B.ptr(g), B.ptr(m), B.ptr(mc), B.ptr(masked), count, flags))
            _sync()
            _assert_bits(f"mask_apply flags {flags} masked", _np(masked), ref_m)
            if with_c:
                _assert_bits(f"mask_apply flags {flags} mask_c", _np(mc), ref_c)
            _check_guards("mask_apply")
    print(f"mask_apply count {count}: flags 0..3, mask_c given and null: bit-exact")


def _composite_inputs(count, fractional):
    """fractional: from a pool of candidates, those whose fused and unfused evaluation differ come first, so that every count has
    its share of them"""
    r = _rng(2, count, int(fractional))
    pool = 2 * count + 64
    masked, gen = _wide(r, pool, -1, 2), _wide(r, pool, -1, 2)
    if not fractional:
        mc = r.integers(0, 2, pool).astype(np.float32)
        return masked[:count], gen[:count], mc[:count]
    mc = r.uniform(0.05, 0.95, pool).astype(np.float32)
    differ = R.mask_composite(masked, gen, mc).view(np.uint32) != R.mask_composite_fused(masked, gen, mc).view(np.uint32)
    order = np.argsort(~differ, kind="stable")[:count]
    order = order[r.permutation(count)]
    return masked[order], gen[order], mc[order]


@pytest.mark.parametrize("count", COUNTS)
@pytest.mark.parametrize("kind", ["binary", "fractional"])
def test_mask_composite(kind, count):
    lib, ctx = _lib()
    masked, gen, mc = _composite_inputs(count, kind == "fractional")
    ref = R.mask_composite(masked, gen, mc)
    share = float(np.mean(ref.view(np.uint32) != R.mask_composite_fused(masked, gen, mc).view(np.uint32)))
    if kind == "fractional":
        assert share >= 0.10, f"only {share:.1%} of the elements tell a fused evaluation from two roundings"
    else:
        assert share == 0.0
    out = _out(count, 1)
    _call(lib.gi_mask_composite(ctx, B.ptr(_in(masked)), B.ptr(_in(gen, 1)), B.ptr(_in(mc)), B.ptr(out), count))
    _sync()
    got = _np(out)
    print(f"mask_composite {kind} count {count}: {share:.1%} of the elements sensitive to fusing; "
          f"{int(np.count_nonzero(got.view(np.uint32) != ref.view(np.uint32)))} differ from masked + gen * mask_c in two roundings")
    _assert_bits(f"mask_composite {kind}", got, ref)
    _check_guards("mask_composite")


@pytest.mark.parametrize("count", COUNTS)
def test_mul(count):
    lib, ctx = _lib()
    r = _rng(3, count)
    a, b = _wide(r, count), np.where(r.random(count) < 0.5, r.choice(MASK_VALUES, count), _wide(r, count)).astype(np.float32)
    out = _out(count)
    _call(lib.gi_mul(ctx, B.ptr(_in(a, 1)), B.ptr(_in(b)), B.ptr(out), count))
    _sync()
    _assert_bits("mul", _np(out), R.mul(a, b))
    _check_guards("mul")
    print(f"mul count {count}: bit-exact")


# =====================================================================================================================================
# gi_add, gi_interpolate: bounded
# =====================================================================================================================================
@pytest.mark.parametrize("count", COUNTS)
def test_add(count):
    lib, ctx = _lib()
    r = _rng(4, count)
    a, b = _wide(r, count), _wide(r, count)
    worst = 0.0
    for alpha in (1.0, -1.0, 0.25, 1e-3):
        out = _out(count, 1)
        _call(lib.gi_add(ctx, B.ptr(_in(a)), B.ptr(_in(b, 1)), B.ptr(out), count, alpha))
        _sync()
        E, bd = R.add(a, b, alpha)
        worst = max(worst, _assert_ratio(f"add alpha {alpha}", _np(out), E, bd))
        _check_guards("add")
    print(f"add count {count}: worst |out - E| / bound over the alphas = {worst:.3f}")


@pytest.mark.parametrize("hw", [1, 255, 16384 + 3])
@pytest.mark.parametrize("n", [1, 3, 5])
def test_interpolate(n, hw):
    lib, ctx = _lib()
    r = _rng(5, n, hw)
    real, fake = _wide(r, n * hw).reshape(n, hw), _wide(r, n * hw).reshape(n, hw)
    worst = 0.0
    for name, eps in (("0", np.zeros(n, np.float32)), ("1", np.ones(n, np.float32)), ("random", r.random(n).astype(np.float32))):
        out = _out(n * hw, 1)
        _call(lib.gi_interpolate(ctx, B.ptr(_in(real)), B.ptr(_in(fake, 1)), B.ptr(_in(eps)), n, hw, B.ptr(out)))
        _sync()
        got = _np(out).reshape(n, hw)
        E, bd = R.interpolate(real, fake, eps)
        worst = max(worst, _assert_ratio(f"interpolate eps {name}", got, E, bd))
        if name == "0":
            _assert_bits("interpolate eps 0 returns fake", got, fake)
        if name == "1":
            _assert_bits("interpolate eps 1 returns real", got, real)
        _check_guards("interpolate")
    print(f"interpolate n {n} hw {hw}: worst |out - E| / bound = {worst:.3f}")


# =====================================================================================================================================
# reconstruction losses
# =====================================================================================================================================
LOSS_OPS = ("l1", "mse", "rmse", "local0", "local1", "local2")
GSCALES = (1.0, 0.5, -3.0)
EPS_RMSE = 1e-12            # gi_loss_rmse takes its eps as an argument; gi_loss_local kind 2 uses 1e-16


def _loss_kind(op):
    return {"l1": "l1", "mse": "mse", "rmse": "rmse", "local0": "l1", "local1": "mse", "local2": "rmse"}[op]


def _loss_eps(op):
    return EPS_RMSE if op == "rmse" else 1e-16


def _run_loss(op, a, b, m, gscale, with_grad, scratch=True):
    """one call; returns (status, loss_out view, grad view or None)"""
    lib, ctx = _lib()
    n = a.size
    da, db = _in(a), _in(b, 1)
    lo = _out(1)
    grad = _out(n, 1) if with_grad else None
    scr = _buf(np.full(4096, NAN, dtype=np.float32), 0, SENT, True) if scratch else None
    if op.startswith("local"):
        st = lib.gi_loss_local(ctx, B.ptr(da), B.ptr(db), B.ptr(_in(m)), n, int(op[-1]), B.ptr(lo), B.ptr(grad), gscale, B.ptr(scr))
    elif op == "rmse":
        st = lib.gi_loss_rmse(ctx, B.ptr(da), B.ptr(db), n, EPS_RMSE, B.ptr(lo), B.ptr(grad), gscale, B.ptr(scr))
    else:
        st = getattr(lib, "gi_loss_" + op)(ctx, B.ptr(da), B.ptr(db), n, B.ptr(lo), B.ptr(grad), gscale, B.ptr(scr))
    return st, lo, grad


def _judge_loss(what, op, a, b, m, exact_value):
    """all gradient scales, with and without a gradient, against one evaluation of the reference (value, gradient and bound are
    linear in gscale). Returns the worst ratios (value, gradient)."""
    ref = R.loss(_loss_kind(op), a, b, m if op.startswith("local") else None, _loss_eps(op), 1.0)
    wv = wg = 0.0
    for gs in GSCALES:
        for with_grad in (True, False):
            if not with_grad and gs != 1.0:
                continue
            st, lo, grad = _run_loss(op, a, b, m, gs, with_grad)
            _call(st)
            _sync()
            v = _np(lo)[0]
            if exact_value:
                assert v == np.float32(ref["value"]), f"{what} {op}: value {v!r} is not float32({ref['value']!r})"
            else:
                wv = max(wv, _assert_ratio(f"{what} {op} value", v, ref["value"], ref["value_bound"]))
            if with_grad:
                wg = max(wg, _assert_ratio(f"{what} {op} gscale {gs} gradient", _np(grad), ref["grad"] * gs, ref["grad_bound"] * abs(gs)))
            _check_guards(f"{what} {op}")
    return wv, wg


@pytest.mark.parametrize("count", COUNTS)
def test_losses_exact_on_integers(count):
    """a - b integer-valued in [-3, 3], masks 0 / 1: every partial sum is exact in fp32 and so is the count of live elements"""
    r = _rng(6, count)
    b = r.integers(-8, 9, count).astype(np.float32)
    a = (b + r.integers(-3, 4, count)).astype(np.float32)
    m = r.integers(0, 2, count).astype(np.float32)
    m[0] = 1.0
    worst = 0.0
    for op in LOSS_OPS:
        worst = max(worst, _judge_loss(f"exact count {count}", op, a, b, m, True)[1])
    print(f"losses, exact integers, count {count}: every value equals float32(reference); worst gradient ratio {worst:.3f}")


@functools.lru_cache(maxsize=2)
def _float_loss_inputs(count, l1):
    """magnitudes 1e-3 .. 1e3. l1: every |a - b| - after the mask multiply for the masked form - is exactly 0 or at least 2^-6, so
    that the sign the gradient takes is never in doubt (asserted); a tenth of the elements have a == b, under fractional masks too."""
    r = _rng(7, count, int(l1))
    b = _wide(r, count)
    if l1:
        m = r.choice(np.array([0.0, 1.0, 0.3, 0.75], dtype=np.float32), count)
        m[0] = 0.75          # at least one live element, set before the precondition is asserted
        d = (0.25 + np.abs(_wide(r, count))) * np.where(r.random(count) < 0.5, -1.0, 1.0)
        d[r.random(count) < 0.1] = 0.0
        a = (b.astype(np.float64) + d).astype(np.float32)
        for mask in (np.ones(count, np.float32), m):
            exact = np.abs((a.astype(np.float64) - b.astype(np.float64)) * mask)
            f32 = np.abs((a * mask).astype(np.float32).astype(np.float64) - (b * mask).astype(np.float32).astype(np.float64))
            assert bool(((exact == 0) | ((exact >= 2.0 ** -6) & (f32 >= 2.0 ** -6))).all()), "an |a - b| within 2^-6 of zero survived"
            assert bool((f32[exact == 0] == 0).all())
    else:
        m = r.choice(np.array([0.0, 1.0, 0.3, 0.75, 1e-3], dtype=np.float32), count)
        m[0] = 0.75
        a = _wide(r, count)
        same = r.random(count) < 0.1
        a[same] = b[same]
    return a, b, m


@pytest.mark.parametrize("count", COUNTS)
def test_losses_float(count):
    wv = wg = 0.0
    for op in LOSS_OPS:
        a, b, m = _float_loss_inputs(count, _loss_kind(op) == "l1")
        v, g = _judge_loss(f"float count {count}", op, a, b, m, False)
        wv, wg = max(wv, v), max(wg, g)
        print(f"  {op} count {count}: value ratio {v:.3f}, gradient ratio {g:.3f}")
    print(f"losses, float inputs, count {count}: worst value ratio {wv:.3f}, worst gradient ratio {wg:.3f}")


@pytest.mark.parametrize("count", [7, 4099])
def test_rmse_of_equal_inputs_is_sqrt_eps(count):
    r = _rng(8, count)
    a = _wide(r, count)
    m = r.choice(np.array([1.0, 0.3, 0.75, 1e-3], dtype=np.float32), count)
    for op in ("rmse", "local2"):
        st, lo, grad = _run_loss(op, a, a.copy(), m, -3.0, True)
        _call(st)
        _sync()
        expect = np.float32(np.sqrt(np.float64(np.float32(_loss_eps(op)))))
        v, g = _np(lo)[0], _np(grad)
        assert v == expect, f"{op}: {v!r} for equal inputs, sqrt(eps) = {expect!r}"
        assert not g.any(), f"{op}: gradient of equal inputs: {R.first_diff(g, np.zeros_like(g))}"
        _check_guards(op)
        print(f"{op} of equal inputs, count {count}: value {v!r} = sqrt(eps), 0 ulp; largest |gradient| {float(np.abs(g).max())!r}")


def test_loss_without_scratch_is_rejected():
    a = np.ones(300, np.float32)
    for op in LOSS_OPS:
        st, lo, grad = _run_loss(op, a, a, a, 1.0, True, scratch=False)
        assert _rejected(st), op
        _sync()
        assert _untouched(lo) and _untouched(grad), f"{op}: something was written without scratch"
        _check_guards(op)
    print(f"losses without scratch: {len(LOSS_OPS)} calls refused, 0 elements written")


# =====================================================================================================================================
# adversarial losses
# =====================================================================================================================================
ADV_N = (1, 63, 64, 65, 255, 256, 257, 1000)


def _adv_pred(kind, n, seed):
    r = _rng(9, kind, n, seed)
    return (r.standard_normal(n) * 2).astype(np.float32) if kind == 2 else r.uniform(0.01, 0.99, n).astype(np.float32)


def _adv(pred_view, n, kind, target, gscale, with_grad):
    lib, ctx = _lib()
    lo = _out(1)
    grad = _out(n, 1) if with_grad else None
    _call(lib.gi_loss_adv(ctx, B.ptr(pred_view), n, kind, target, B.ptr(lo), B.ptr(grad), gscale))
    _sync()
    return _np(lo)[0], (_np(grad) if with_grad else None)


def _judge_adv(what, v, g, pred, kind, target, gscale):
    val, gref = R.adv_loss(kind, pred, target, gscale)
    ev = abs(float(v) - val) / (abs(val) + 1e-6)
    assert ev <= VAL_TOL, f"{what}: value {v!r} reference {val!r} ({ev:.2e})"
    eg = 0.0
    if g is not None:
        err = np.abs(g.astype(np.float64) - gref)
        bad = np.flatnonzero(err > GRAD_TOL * np.abs(gref))
        assert bad.size == 0, f"{what}: gradient element {bad[0]}: got {g[bad[0]]!r} reference {gref[bad[0]]!r}"
        eg = float(np.max(err / np.maximum(np.abs(gref), 1e-300)))
    return ev, eg


@pytest.mark.parametrize("n", ADV_N)
@pytest.mark.parametrize("kind", [0, 1, 2])
def test_adv_loss(kind, n):
    wv = wg = 0.0
    for target in (0.0, 1.0):
        pred = _adv_pred(kind, n, int(target))
        for gscale, with_grad in ((1.0, True), (-0.5, True), (1.0, False)):
            v, g = _adv(_in(pred, 1), n, kind, target, gscale, with_grad)
            ev, eg = _judge_adv(f"adv kind {kind} n {n} target {target}", v, g, pred, kind, target, gscale)
            wv, wg = max(wv, ev), max(wg, eg)
            _check_guards("adv")
    print(f"adv kind {kind} n {n}: worst value error {wv:.2e}, worst per-element gradient error {wg:.2e} (relative)")


def test_bce_saturation():
    pred = np.array([0.0, 1.0, 2.0 ** -149, 1.0 - 2.0 ** -24, 2.0 ** -30], dtype=np.float32)
    for target in (0.0, 1.0):
        for k in range(pred.size):         # one at a time, so that a clamped 100 does not hide the others in the mean
            v, g = _adv(_in(pred[k:k + 1]), 1, 0, target, 1.0, True)
            assert np.isfinite(v) and np.isfinite(g).all(), (target, pred[k], v, g)
            _judge_adv(f"bce p = {pred[k]!r} target {target}", v, g, pred[k:k + 1], 0, target, 1.0)
        v, g = _adv(_in(pred, 1), pred.size, 0, target, -2.0, True)
        ev, eg = _judge_adv(f"bce saturation target {target}", v, g, pred, 0, target, -2.0)
        print(f"bce saturation target {target}: value {v!r}, value error {ev:.2e}, gradient error {eg:.2e}")
        _check_guards("bce")


@pytest.mark.parametrize("n_each", [1, 63, 255, 1001])
@pytest.mark.parametrize("kind", [0, 1, 2])
def test_adv_pair_equals_two_single_calls(kind, n_each):
    """n_each is odd: the second half starts at an odd float offset"""
    lib, ctx = _lib()
    pred = _adv_pred(kind, 2 * n_each, 5)
    ta, tb, ga, gb = 1.0, 0.0, 0.5, -3.0
    for with_grad in (True, False):
        p = _in(pred)
        la, lb = _out(1), _out(1)
        grad = _out(2 * n_each) if with_grad else None
        _call(lib.gi_loss_adv_pair(ctx, B.ptr(p), n_each, kind, ta, tb, B.ptr(la), B.ptr(lb), B.ptr(grad), ga, gb))
        _sync()
        va, g1 = _adv(p[:n_each], n_each, kind, ta, ga, with_grad)
        vb, g2 = _adv(p[n_each:], n_each, kind, tb, gb, with_grad)
        _assert_bits("pair: first loss", _np(la), np.array([va]))
        _assert_bits("pair: second loss", _np(lb), np.array([vb]))
        if with_grad:
            _assert_bits("pair: gradients", _np(grad), np.concatenate([g1, g2]))
        ev, eg = _judge_adv("pair second half", vb, g2, pred[n_each:], kind, tb, gb)
        _check_guards("adv pair")
        print(f"adv pair kind {kind} n_each {n_each} grad {with_grad}: 0 ulp from two single calls; second half against the reference: "
              f"value {ev:.2e}, gradient {eg:.2e} (relative)")


# =====================================================================================================================================
# optimizers
# =====================================================================================================================================
LR_ADAM, B1, B2, EPS_OPT = 0.0002, 0.5, 0.999, 1e-8
LR_RMS, ALPHA = 0.00005, 0.99


def _opt_inputs(count, seed, steps=3, gs=1.0):
    """parameters, `steps` gradients with |g * gs| in 1e-6 .. 1e3 (asserted) and the same tenth of the elements exactly 0 in all"""
    r = _rng(10, count, seed)
    p = (r.standard_normal(count) * 0.02).astype(np.float32)
    zero = r.random(count) < 0.1
    grads = []
    for _ in range(steps):
        g = (10.0 ** r.uniform(-5.5, 2.5, count) * np.where(r.random(count) < 0.5, -1.0, 1.0)).astype(np.float32)
        g[zero] = 0.0
        live = np.abs(g[~zero].astype(np.float64) * np.float32(gs))
        assert live.size == 0 or (live.min() >= 1e-6 and live.max() <= 1e3)
        grads.append(g)
    return p, grads, zero


def _judge_p(what, got, ref):
    bd = R.p_bound(ref["p"], ref["move"])
    return _assert_ratio(what + " p", got, ref["p"], bd)


@pytest.mark.parametrize("count", COUNTS)
def test_adam_three_steps(count):
    lib, ctx = _lib()
    p0, grads, zero = _opt_inputs(count, 0, gs=0.5)
    p, m, v = _inout(p0, 1), _inout(np.zeros(count, np.float32)), _inout(np.zeros(count, np.float32), 1)
    wm = wv = wp = 0.0
    for t, g in enumerate(grads, 1):
        before = [_np(x) for x in (p, m, v)]
        _call(lib.gi_adam_step(ctx, B.ptr(p), B.ptr(_in(g)), B.ptr(m), B.ptr(v), count, LR_ADAM, B1, B2, EPS_OPT, t, 0.5))
        _sync()
        ref = R.adam_step(before[0], g, before[1], before[2], LR_ADAM, B1, B2, EPS_OPT, t, 0.5)
        gp, gm, gv = _np(p), _np(m), _np(v)
        wm = max(wm, _assert_ratio(f"adam step {t} m", gm, ref["m"], ref["m_bound"]))
        wv = max(wv, _assert_ratio(f"adam step {t} v", gv, ref["v"], ref["v_bound"]))
        wp = max(wp, _judge_p(f"adam step {t}", gp, ref))
        assert not gm[zero].any() and not gv[zero].any() and R.same_bits(gp[zero], p0[zero]), "a zero gradient on zero moments moved something"
    _check_guards("adam")
    print(f"adam count {count}, three steps: worst ratio m {wm:.3f}, v {wv:.3f}, p (1e-6 |p| + 1e-3 move) {wp:.3f}")


ADAM_PATHS = [(t, path, d) for t in (1, 2, 10, 1000, 100000) for path, d in (("host", 0), ("device", 0), ("device", 3))] + [(5, "device", 3)]


@pytest.mark.parametrize("step,path,skipped", ADAM_PATHS)
def test_adam_bias_correction_paths(step, path, skipped):
    """host: guard null, the corrections come as arguments; device: guard and skipped_seen >= 0, formed by the kernel from
    step - (guard[0] - seen), at least 1 (step 1 and 2 with three skipped updates behave as step 1)"""
    lib, ctx = _lib()
    count = 4099
    p0, (g,), _ = _opt_inputs(count, step, steps=1)
    r = _rng(11, step)
    m0, v0 = (_wide(r, count, -4, 1) * 0.1).astype(np.float32), (np.abs(_wide(r, count, -4, 1)) * 0.01).astype(np.float32)
    p, m, v = _inout(p0), _inout(m0, 1), _inout(v0)
    if path == "host":
        _call(lib.gi_adam_step(ctx, B.ptr(p), B.ptr(_in(g)), B.ptr(m), B.ptr(v), count, LR_ADAM, B1, B2, EPS_OPT, step, 1.0))
    else:
        guard = _in(np.array([7, 0, 0, 0], dtype=np.int32))
        _call(lib.gi_adam_step_scan(ctx, B.ptr(p), B.ptr(_in(g)), B.ptr(m), B.ptr(v), count, LR_ADAM, B1, B2, EPS_OPT, step, 7 - skipped, 1.0,
                                    B.ptr(guard), 0, 0))
    _sync()
    eff = max(step - skipped, 1)
    ref = R.adam_step(p0, g, m0, v0, LR_ADAM, B1, B2, EPS_OPT, eff, 1.0)
    wm = _assert_ratio("adam m", _np(m), ref["m"], ref["m_bound"])
    wv = _assert_ratio("adam v", _np(v), ref["v"], ref["v_bound"])
    wp = _judge_p(f"adam step {step} {path} skipped {skipped} (effective step {eff})", _np(p), ref)
    _check_guards("adam paths")
    print(f"adam step {step} {path} path, {skipped} skipped: ratio m {wm:.3f}, v {wv:.3f}, p {wp:.3f}")


@pytest.mark.parametrize("count", COUNTS)
@pytest.mark.parametrize("clampv", [0.0, 0.01])
def test_rmsprop_three_steps(clampv, count):
    lib, ctx = _lib()
    p0, grads, zero = _opt_inputs(count, 1)
    p, sq = _inout(p0, 1), _inout(np.zeros(count, np.float32))
    p4, sq4 = _inout(p0), _inout(np.zeros(count, np.float32), 1)      # the same with 4 g and grad_scale 0.25
    ws = wp = 0.0
    for t, g in enumerate(grads, 1):
        before = [_np(x) for x in (p, sq)]
        _call(lib.gi_rmsprop_step(ctx, B.ptr(p), B.ptr(_in(g)), B.ptr(sq), count, LR_RMS, ALPHA, EPS_OPT, clampv, 1.0))
        _call(lib.gi_rmsprop_step(ctx, B.ptr(p4), B.ptr(_in(g * np.float32(4.0), 1)), B.ptr(sq4), count, LR_RMS, ALPHA, EPS_OPT, clampv, 0.25))
        _sync()
        ref = R.rmsprop_step(before[0], g, before[1], LR_RMS, ALPHA, EPS_OPT, clampv, 1.0)
        gp, gs = _np(p), _np(sq)
        ws = max(ws, _assert_ratio(f"rmsprop step {t} sq", gs, ref["sq"], ref["sq_bound"]))
        wp = max(wp, _judge_p(f"rmsprop step {t} clamp {clampv}", gp, ref))      # clip is a contraction: the bound holds clipped or not
        if clampv > 0:
            assert float(np.abs(gp).max()) <= np.float32(clampv), "a parameter beyond the clamp"
        assert not gs[zero].any()
        _assert_bits("grad_scale 0.25 with 4 g: p", _np(p4), gp)
        _assert_bits("grad_scale 0.25 with 4 g: sq", _np(sq4), gs)
    if clampv > 0 and count >= 255:
        assert float(np.abs(p0).max()) > clampv, "no parameter started beyond the clamp"
    _check_guards("rmsprop")
    print(f"rmsprop count {count} clamp {clampv}, three steps: worst ratio sq {ws:.3f}, p {wp:.3f}")


def _opt_call(kind, p, g, s1, s2, count, guard, word, finish):
    lib, ctx = _lib()
    if kind == "adam":
        return lib.gi_adam_step_scan(ctx, B.ptr(p), B.ptr(g), B.ptr(s1), B.ptr(s2), count, LR_ADAM, B1, B2, EPS_OPT, 3, -1, 1.0, B.ptr(guard), word, finish)
    return lib.gi_rmsprop_step_scan(ctx, B.ptr(p), B.ptr(g), B.ptr(s1), count, LR_RMS, ALPHA, EPS_OPT, 0.0, 1.0, B.ptr(guard), word, finish)


GUARD_TABLE = [
    # flags before, word, finish, applied, flags after
    ([5, 0, 1, 7], 2, 1, False, [6, 1, 1, 0]),     # a set scan word, first kernel of the update: recorded, the other word cleared
    ([5, 0, 9, 1], 3, 1, False, [6, 1, 0, 1]),
    ([5, 0, 1, 7], 2, 0, False, [5, 0, 1, 7]),     # a later kernel of the same update: skipped as well, nothing recorded
    ([5, 1, 0, 0], 0, 0, False, [5, 1, 0, 0]),     # word 0: the verdict is flag4[1]
    ([5, 1, 0, 0], 0, 1, False, [5, 1, 0, 0]),
    ([5, 0, 1, 1], 0, 0, True, [5, 0, 1, 1]),
    ([5, 1, 0, 9], 2, 1, True, [5, 0, 0, 0]),      # a clean word: applied, the stale verdict and the other word cleared
    ([5, 1, 9, 0], 3, 1, True, [5, 0, 0, 0]),
    ([5, 1, 0, 9], 2, 0, True, [5, 1, 0, 9]),
]


@pytest.mark.parametrize("kind", ["adam", "rmsprop"])
def test_guard_truth_table(kind):
    count = 4099                                   # five workgroups: every one of them reads the word
    p0, (g,), _ = _opt_inputs(count, 2, steps=1)
    r = _rng(12)
    s1_0, s2_0 = (_wide(r, count, -4, 1) * 0.1).astype(np.float32), (np.abs(_wide(r, count, -4, 1)) * 0.01).astype(np.float32)
    if kind == "rmsprop":
        s1_0 = np.abs(s1_0)
    ref = R.adam_step(p0, g, s1_0, s2_0, LR_ADAM, B1, B2, EPS_OPT, 3) if kind == "adam" else R.rmsprop_step(p0, g, s1_0, LR_RMS, ALPHA, EPS_OPT)
    wp = w1 = w2 = 0.0
    for before, word, finish, applied, after in GUARD_TABLE:
        p, s1, s2, gd = _inout(p0, 1), _inout(s1_0), _inout(s2_0, 1), _in(g)
        guard = _inout(np.array(before, dtype=np.int32))
        _call(_opt_call(kind, p, gd, s1, s2, count, guard, word, finish))
        _sync()
        what = f"{kind} flags {before} word {word} finish {finish}"
        assert _np(guard).tolist() == after, f"{what}: flags became {_np(guard).tolist()}, expected {after}"
        if applied:
            wp = max(wp, _judge_p(what, _np(p), ref))
            w1 = max(w1, _assert_ratio(what + " first moment", _np(s1), ref["m" if kind == "adam" else "sq"], ref["m_bound" if kind == "adam" else "sq_bound"]))
            if kind == "adam":
                w2 = max(w2, _assert_ratio(what + " v", _np(s2), ref["v"], ref["v_bound"]))
        else:
            _assert_bits(what + ": p of a skipped update", _np(p), p0)
            _assert_bits(what + ": first moment of a skipped update", _np(s1), s1_0)
        if kind == "rmsprop" or not applied:
            _assert_bits(what + ": second state", _np(s2), s2_0)
        _check_guards(what)
    # a word outside {0, 2, 3}, or a scan word without a guard
    p, s1, s2, gd = _inout(p0), _inout(s1_0), _inout(s2_0), _in(g)
    guard = _inout(np.array([5, 0, 0, 0], dtype=np.int32))
    for word, gptr in ((1, guard), (4, guard), (-1, guard), (2, None), (3, None)):
        assert _rejected(_opt_call(kind, p, gd, s1, s2, count, gptr, word, 1)), f"{kind}: word {word} guard {gptr is not None} was accepted"
    _sync()
    _assert_bits("rejected call: p", _np(p), p0)
    assert _np(guard).tolist() == [5, 0, 0, 0]
    _check_guards(kind)
    print(f"guard truth table {kind}: {len(GUARD_TABLE)} rows, skipped updates 0 ulp from their inputs; applied ones: worst ratio p {wp:.3f}, "
          f"{'m' if kind == 'adam' else 'sq'} {w1:.3f}" + (f", v {w2:.3f}" if kind == "adam" else "") + "; 5 bad words refused")


# =====================================================================================================================================
# finite check
# =====================================================================================================================================
FINITE = np.array([0.0, -0.0, 2.0 ** -149, -2.0 ** -130, 1.17549421e-38, 3.4028234663852886e38, -3.4028234663852886e38, 1.0, -1.0], dtype=np.float32)
BAD_BITS = {"+inf": 0x7F800000, "-inf": 0xFF800000, "quiet NaN": 0x7FC00000, "NaN with a payload": 0xFF800001}


def _bad_positions(count, aligned):
    """0 and 1, the last 16-byte chunk boundary +- 1, the last element, and both sides of one and two grid strides (the stride of
    the launcher, restated in elementwise_ref.check_finite_stride: workgroups x 256 chunks of four floats)"""
    stride = R.check_finite_stride(count) * 4
    last_chunk = ((count - 1) // 4) * 4          # where the last, possibly partial, chunk begins
    cand = [0, 1, last_chunk - 1, last_chunk, last_chunk + 1, count - 1, stride - 1, stride, 2 * stride - 1, 2 * stride]
    return sorted({c for c in cand if 0 <= c < count})


@pytest.mark.parametrize("count", [1, 2, 3, 5, 2048, 2049, 2052, 2 ** 22 + 4099])
@pytest.mark.parametrize("off", [0, 1], ids=["aligned", "offset-by-one-float"])
def test_check_finite_scan_word(off, count):
    """off 1: the pointer is not 16-byte aligned and every element goes through the scalar loop"""
    lib, ctx = _lib()
    g = _inout(np.resize(FINITE, count), off)
    assert (g.data_ptr() % 16 == 0) == (off == 0)
    gi = _raw(g)
    flags = torch.tensor([7, 5, 0, 0], dtype=torch.int32, device="cuda")
    for word in (2, 3):
        _call(lib.gi_check_finite_scan_word(ctx, B.ptr(g), count, B.ptr(flags), word))
    assert flags.tolist() == [7, 5, 0, 0], f"finite values (zeros, denormals, +-FLT_MAX) were flagged: {flags.tolist()}"
    launches = 0
    for pos in _bad_positions(count, off == 0):
        keep = int(gi[pos])
        for k, (name, bits) in enumerate(BAD_BITS.items()):
            word = 2 + (k + pos) % 2
            gi[pos] = bits - (1 << 32) if bits >= 1 << 31 else bits
            flags.copy_(torch.tensor([7, 5, 0, 0], dtype=torch.int32))
            _call(lib.gi_check_finite_scan_word(ctx, B.ptr(g), count, B.ptr(flags), word))
            expect = [7, 5, 0, 0]
            expect[word] = 1
            got = flags.tolist()
            assert got == expect, f"count {count} {name} at {pos}, word {word}: flags {got}, expected {expect}"
            launches += 1
        gi[pos] = keep
    # gi_check_finite: scan into word 2, then the finish launch: {count + verdict, verdict, 0}
    f3 = torch.tensor([3, 9, 0, 77], dtype=torch.int32, device="cuda")
    _call(lib.gi_check_finite(ctx, B.ptr(g), count, B.ptr(f3)))
    assert f3.tolist() == [3, 0, 0, 77]
    gi[count - 1] = 0x7F800000
    _call(lib.gi_check_finite(ctx, B.ptr(g), count, B.ptr(f3)))
    assert f3.tolist() == [4, 1, 0, 77]
    _check_guards("check_finite")
    print(f"check_finite count {count} offset {off}: {launches} single bad values found, one launch each; finite extremes not flagged")


def test_check_finite_rejects_bad_arguments():
    lib, ctx = _lib()
    g = _in(np.ones(8, np.float32))
    flags = _inout(np.zeros(4, np.int32))
    for count, word, gp, fp in ((8, 0, g, flags), (8, 1, g, flags), (8, 4, g, flags), (0, 2, g, flags), (8, 2, None, flags), (8, 2, g, None)):
        assert _rejected(lib.gi_check_finite_scan_word(ctx, B.ptr(gp), count, B.ptr(fp), word))
    _check_guards("check_finite arguments")
    assert not _np(flags).any()
    print("check_finite: 6 bad argument sets refused, the flags untouched")


# =====================================================================================================================================
# gi_clamp, gi_grad_absmean
# =====================================================================================================================================
@pytest.mark.parametrize("count", COUNTS)
def test_clamp(count):
    lib, ctx = _lib()
    r = _rng(13, count)
    x = (_wide(r, count) * 0.01).astype(np.float32)
    x[r.random(count) < 0.1] = np.float32(0.01)
    x[r.random(count) < 0.1] = np.float32(-0.01)
    x[r.random(count) < 0.05] = np.float32(3.4028234663852886e38)
    x[r.random(count) < 0.05] = np.float32(-0.0)
    for lo, hi in ((-0.01, 0.01), (1e-3, 1.0), (-3.4028234663852886e38, -1e-3)):
        p = _inout(x, 1)
        _call(lib.gi_clamp(ctx, B.ptr(p), count, lo, hi))
        _sync()
        _assert_bits(f"clamp [{lo}, {hi}]", _np(p), R.clamp(x, lo, hi))
        _check_guards("clamp")
    print(f"clamp count {count}: bit-exact against numpy.clip")


SEG_LENGTHS = (1, 31, 8191, 8193, 100003)


@pytest.mark.parametrize("nseg", [1, 3, 256])
def test_grad_absmean(nseg):
    lib, ctx = _lib()
    r = _rng(14, nseg)
    lens = [SEG_LENGTHS[(k + nseg) % 5] for k in range(nseg)]
    offs, pos = [], 1
    for n in lens:
        offs.append(pos)
        pos += n + 2 * int(r.integers(0, 3)) + (2 if (pos + n) % 2 else 1)       # a gap of NaN, the next offset odd again
    assert all(o % 2 == 1 for o in offs)
    g = np.full(pos, NAN, dtype=np.float32)
    for k, (o, n) in enumerate(zip(offs, lens)):
        g[o:o + n] = 0.0 if k % 4 == 2 else _wide(r, n)
    ref = R.grad_absmean(g, offs, lens)
    gd, od, ld = _in(g), _in(np.array(offs, dtype=np.int64)), _in(np.array(lens, dtype=np.int64))
    outs = []
    for _ in range(2):
        out = _out(nseg)
        _call(lib.gi_grad_absmean(ctx, B.ptr(gd), B.ptr(od), B.ptr(ld), nseg, B.ptr(out)))
        _sync()
        outs.append(_np(out))
    ulps = R.ulp_distance(outs[0], ref)
    assert np.isfinite(outs[0]).all() and int(ulps.max()) <= 1, f"segment {int(ulps.argmax())}: {outs[0][ulps.argmax()]!r} against {ref[ulps.argmax()]!r}"
    zero = [k for k in range(nseg) if k % 4 == 2]
    assert all(outs[0][k] == 0.0 for k in zero), "an all-zero segment did not give exactly 0"
    _assert_bits("two calls", outs[1], outs[0])
    _check_guards("grad_absmean")
    print(f"grad_absmean nseg {nseg}: worst distance from float32(fp64 mean) {int(ulps.max())} ulp; two calls bit-identical")


def test_grad_absmean_rejects_257_segments():
    lib, ctx = _lib()
    g, o, n = _in(np.ones(300, np.float32)), _in(np.arange(257, dtype=np.int64)), _in(np.ones(257, dtype=np.int64))
    out = _out(257)
    assert _rejected(lib.gi_grad_absmean(ctx, B.ptr(g), B.ptr(o), B.ptr(n), 257, B.ptr(out)))
    assert _rejected(lib.gi_grad_absmean(ctx, B.ptr(g), B.ptr(o), B.ptr(n), 0, B.ptr(out)))
    _sync()
    assert _untouched(out)
    _check_guards("grad_absmean arguments")
    print("grad_absmean: 257 and 0 segments refused, 0 elements written")


# =====================================================================================================================================
# conversions and weight packing: bit-exact
# =====================================================================================================================================
CODES = [pytest.param(B.GI_F32, id="fp32"), pytest.param(B.GI_F16, id="fp16")]
HALF_EDGES = np.array([0.0, -0.0, 65504.0, 65520.0, -65520.0, 65519.996, 1.0 + 2.0 ** -11, 1.0 + 3 * 2.0 ** -11, 1.0 + 2.0 ** -11 + 2.0 ** -20,
                       2.0 ** -24, 2.0 ** -25, 2.0 ** -25 + 2.0 ** -40, 3 * 2.0 ** -25, 2.0 ** -14, 2.0 ** -14 - 2.0 ** -25, -2.0 ** -24, 1e-30, 2049.0, 2051.0],
                      dtype=np.float32)     # ties to even, fp16 denormals, the largest finite value, the first one that rounds to inf


def _tdtype(code):
    return np.float16 if code == B.GI_F16 else np.float32


@pytest.mark.parametrize("code", CODES)
@pytest.mark.parametrize("count", COUNTS)
def test_convert_and_back(count, code):
    lib, ctx = _lib()
    r = _rng(15, count)
    src = _wide(r, count, -8, 5)
    k = min(count, HALF_EDGES.size)
    src[:k] = HALF_EDGES[:k] if count >= HALF_EDGES.size else r.choice(HALF_EDGES, k)
    half = code == B.GI_F16
    dst = _out(count, 1, _tdtype(code))
    _call(lib.gi_convert(ctx, code, B.ptr(_in(src)), B.ptr(dst), count))
    _sync()
    ref = R.convert(src, half)
    _assert_bits("convert", _np(dst), ref)
    back = _out(count)
    _call(lib.gi_convert_back(ctx, code, B.ptr(_in(ref, 1)), B.ptr(back), count))
    _sync()
    _assert_bits("convert_back", _np(back), R.convert_back(ref))
    _check_guards("convert")
    print(f"convert / convert_back count {count}: bit-exact against numpy astype")


PACK_SHAPES = [(1, 64), (64, 1), (3, 5), (33, 31), (96, 32), (64, 64), (128, 64), (64, 192)]


def _pack_case(ca, cb, code, scale_mode, seed, packed=True, phase=True):
    """device buffers of one job and the restatement's two copies"""
    r = _rng(16, ca, cb, seed)
    w = _wide(r, ca * 16 * cb, -2, 2)
    scale = None if scale_mode is None else r.uniform(0.25, 4.0, cb if scale_mode == "b" else ca).astype(np.float32)
    T = _tdtype(code)
    job = {"w": _in(w), "scale": None if scale is None else _in(scale), "on_b": int(scale_mode == "b"), "ca": ca, "cb": cb,
           "packed": _out(ca * 16 * cb, 0, T), "phase": _out(ca * 16 * cb, 0, T), "use": (packed, phase)}
    job["ref"] = R.pack(w, ca, cb, code == B.GI_F16, scale, scale_mode == "b")
    return job


def _run_batch(jobs, code):
    lib, ctx = _lib()
    arr = (B.PackJob * len(jobs))()
    for a, j in zip(arr, jobs):
        a.w, a.packed, a.phase = B.ptr(j["w"]), B.ptr(j["packed"]) if j["use"][0] else None, B.ptr(j["phase"]) if j["use"][1] else None
        a.ca, a.cb, a.scale_on_b, a.scale = j["ca"], j["cb"], j["on_b"], B.ptr(j["scale"])
    return lib.gi_debug_pack_weights_batch(ctx, code, arr, len(jobs))


def _check_jobs(what, jobs):
    for k, j in enumerate(jobs):
        for name, used, ref in (("packed", j["use"][0], j["ref"][0]), ("phase", j["use"][1], j["ref"][1])):
            if used:
                _assert_bits(f"{what} job {k} ({j['ca']}, {j['cb']}) {name}", _np(j[name]), ref.reshape(-1))
            else:
                assert _untouched(j[name]), f"{what} job {k}: the {name} copy was not asked for and was written"
    _check_guards(what)


@pytest.mark.parametrize("code", CODES)
@pytest.mark.parametrize("ca,cb", PACK_SHAPES)
def test_pack_weights(ca, cb, code):
    lib, ctx = _lib()
    for packed, phase in ((True, True), (True, False), (False, True)):
        j = _pack_case(ca, cb, code, None, 0, packed, phase)
        _call(lib.gi_pack_weights(ctx, code, B.ptr(j["w"]), ca, cb, B.ptr(j["packed"]) if packed else None, B.ptr(j["phase"]) if phase else None))
        _sync()
        _check_jobs("pack_weights", [j])
    print(f"pack_weights ({ca}, {cb}): both copies bit-exact")


@pytest.mark.parametrize("code", CODES)
@pytest.mark.parametrize("ca,cb", PACK_SHAPES)
def test_pack_batch_single_job(ca, cb, code):
    """multiples of 64 on both sides take pack_batch64_kernel, every other shape pack_batch_kernel"""
    for scale_mode in (None, "a", "b"):
        for packed, phase in ((True, True), (True, False), (False, True)):
            j = _pack_case(ca, cb, code, scale_mode, 1, packed, phase)
            _call(_run_batch([j], code))
            _sync()
            _check_jobs(f"pack_batch scale {scale_mode}", [j])
    print(f"pack_batch ({ca}, {cb}) {'64' if ca % 64 == 0 and cb % 64 == 0 else '32'}-tile kernel: scale none / per a / per b, either copy missing: bit-exact")


@pytest.mark.parametrize("code", CODES)
def test_pack_batch_many_jobs(code):
    modes = (None, "a", "b")
    uses = ((True, True), (True, True), (False, True), (True, False))
    mixed = [_pack_case(*PACK_SHAPES[k % 8], code, modes[k % 3], 10 + k, *uses[k % 4]) for k in range(16)]
    _call(_run_batch(mixed, code))
    _sync()
    _check_jobs("16 mixed jobs (32-tile kernel)", mixed)
    all64 = [_pack_case(ca, cb, code, modes[k % 3], 30 + k, *uses[k % 4]) for k, (ca, cb) in enumerate([(64, 64), (128, 64), (64, 192), (64, 64), (128, 128)])]
    _call(_run_batch(all64, code))
    _sync()
    _check_jobs("5 jobs, multiples of 64 (64-tile kernel)", all64)
    print("pack_batch: 16 mixed jobs and 5 all-64 jobs in one launch each: every element of both copies bit-exact")


def test_pack_batch_rejects_bad_arguments():
    lib, ctx = _lib()
    jobs = [_pack_case(3, 5, B.GI_F32, None, 50 + k) for k in range(17)]
    assert _rejected(_run_batch(jobs, B.GI_F32)), "17 jobs were accepted"
    one = jobs[:1]
    arr = (B.PackJob * 1)()
    assert _rejected(lib.gi_debug_pack_weights_batch(ctx, B.GI_F32, arr, 0))
    assert _rejected(lib.gi_debug_pack_weights_batch(ctx, B.GI_F32, None, 1))
    assert _rejected(lib.gi_debug_pack_weights_batch(ctx, B.GI_F32, arr, 1)), "a job without weights was accepted"
    assert _rejected(_run_batch(one, 7)), "dtype 7 was accepted"
    one[0]["ca"] = 0
    assert _rejected(_run_batch(one, B.GI_F32))
    one[0]["ca"] = 3
    # the 64-tile kernel moves 16-byte chunks: a master that is off by one float is refused, not launched
    j = _pack_case(64, 64, B.GI_F32, None, 70)
    j["w"] = _in(_np(j["w"]), 1)
    assert _rejected(_run_batch([j], B.GI_F32)), "a misaligned master was accepted by the 64-tile path"
    _sync()
    assert all(_untouched(x["packed"]) and _untouched(x["phase"]) for x in jobs + [j])
    _check_guards("pack_batch arguments")
    print("pack_batch: 17 jobs, 0 jobs, null jobs, null weights, a bad dtype, ca = 0 and a misaligned 64-tile master refused; 0 elements written")
