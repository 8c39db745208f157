"""numpy restatement of the public entry points of csrc/elementwise.hip, one function per op, and the bounds their tests use
(tests/test_elementwise_ops_gpu.py; proved against torch in float64 by tests/test_elementwise_ref_cpu.py).

Two kinds of op:

  bit-exact   mask_apply, mask_composite, mul, clamp, convert, convert_back, pack_weights / pack_batch: the restatement works in
              numpy float32 / float16 with every rounding where the kernel's comment or the header puts it, and the device result
              must equal it bit for bit.
  bounded     add, interpolate, the losses and their gradients, the optimizer moments: the restatement returns the float64 value E
              formed from the float32 operands, and a per-element bound
                  (k + 1) * u * (sum of the magnitudes of the rounded terms) + 2^-149,        u = 2^-24,
              k the number of fp32 roundings on the kernel's path (stated per op). A rounding is at most u relative to the term it
              rounds, so k of them stay below k * u * (sum); the "+ 1" is margin for second-order terms and for the float64
              accumulations (n * 2^-53), 2^-149 for results below the normal range. A multiply-add evaluated fused has one rounding
              fewer than the count, so both forms fit.

Nothing here imports torch, the package or the oracle."""
import numpy as np

U = 2.0 ** -24
TINY = 2.0 ** -149
F32, F64 = np.float32, np.float64


def _f32(x):
    return np.asarray(x, dtype=F32)


def _f64(x):
    return np.asarray(x, dtype=F32).astype(F64)


def _state(x):
    """optimizer state and gradients: float32 as the device holds them, or float64 as given (the CPU proof carries the recurrence
    in float64 next to torch.optim on double parameters)"""
    x = np.asarray(x)
    return x if x.dtype == F64 else x.astype(F32).astype(F64)


def bound(k, magnitude):
    """(k + 1) * u * magnitude + 2^-149"""
    return (k + 1) * U * np.asarray(magnitude, dtype=F64) + TINY


def worst_ratio(got, exact, bnd):
    """max over the elements of |got - E| / bound: at most 1 when `got` is within the bound"""
    err = np.abs(np.asarray(got).astype(F64) - np.asarray(exact, dtype=F64))
    return float(np.max(err / np.asarray(bnd, dtype=F64))) if err.size else 0.0


def first_bad(got, exact, bnd):
    """index and figures of the first element outside its bound, for a failure message"""
    got, exact, bnd = (np.atleast_1d(np.asarray(v).astype(F64)).ravel() for v in (got, exact, bnd))
    bad = np.flatnonzero(np.abs(got - exact) > bnd)
    if bad.size == 0:
        return "none"
    i = int(bad[0])
    return f"element {i}: got {got[i]!r} E {exact[i]!r} bound {bnd[i]:.3e} ({bad.size} of {got.size} outside)"


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def first_diff(a, b):
    a, b = np.ascontiguousarray(a).ravel(), np.ascontiguousarray(b).ravel()
    w = {2: np.uint16, 4: np.uint32}[a.dtype.itemsize]
    d = np.flatnonzero(a.view(w) != b.view(w))
    if d.size == 0:
        return "none"
    i = int(d[0])
    return f"element {i}: got {a[i]!r} (0x{int(a.view(w)[i]):x}) expected {b[i]!r} (0x{int(b.view(w)[i]):x}), {d.size} of {a.size} differ"


# ---- mask pipeline (bit-exact) ------------------------------------------------------------------------------------------------------
def mask_apply(ground, mask, flags):
    """mask_c = ceil(mask) if flags & 1 else mask; flags & 2: mask_c = 1 - mask_c; masked = ground * (1 - mask_c). Every operation
    rounds to fp32 on its own (a subtraction feeding a product cannot fuse)."""
    ground, m = _f32(ground), _f32(mask)
    if flags & 1:
        m = np.ceil(m).astype(F32)
    if flags & 2:
        m = (F32(1.0) - m).astype(F32)
    return m, (ground * (F32(1.0) - m).astype(F32)).astype(F32)


def mask_composite(masked, gen, mask_c):
    """inpainted = masked + gen * mask_c: two roundings, the product first"""
    prod = (_f32(gen) * _f32(mask_c)).astype(F32)
    return (_f32(masked) + prod).astype(F32)


def mask_composite_fused(masked, gen, mask_c):
    """the same with ONE rounding (what a fused multiply-add gives): the product is exact in float64 and the sum of a 48-bit product
    and a 24-bit addend is rounded to 53 bits before it is rounded to 24, which can differ from the fused instruction only in rare
    double-rounding cases. Used to show that a test's inputs tell the two evaluations apart."""
    return (_f64(gen) * _f64(mask_c) + _f64(masked)).astype(F32)


def mul(a, b):
    return (_f32(a) * _f32(b)).astype(F32)


def clamp(p, lo, hi):
    return np.clip(_f32(p), F32(lo), F32(hi)).astype(F32)


# ---- add / interpolate (bounded) ----------------------------------------------------------------------------------------------------
def add(a, b, alpha):
    """out = a + alpha * b. Roundings: the product, the sum = 2 (fused: 1)."""
    al = F64(F32(alpha))
    E = _f64(a) + al * _f64(b)
    return E, bound(2, np.abs(_f64(a)) + np.abs(al * _f64(b)))


def interpolate(real, fake, eps):
    """out[n, :] = eps[n] * real[n, :] + (1 - eps[n]) * fake[n, :], real / fake (n, hw). Roundings: 1 - eps, the two products,
    the sum = 4 (fused: 3)."""
    e = _f64(eps)[:, None]
    r, f = _f64(real), _f64(fake)
    E = e * r + (1.0 - e) * f
    return E, bound(4, np.abs(e * r) + np.abs((1.0 - e) * f))


# ---- reconstruction losses (bounded; exact on integer inputs) -----------------------------------------------------------------------
# Kernel path (loss_partial_kernel, loss_final_kernel, loss_grad_kernel):
#   d        unmasked a - b: 1 rounding of |a - b|. Masked a * m - b * m: the two products and the difference, 3 roundings of terms of
#            magnitude at most |a m| + |b m| (the difference cancels, the bound must not)
#   value    sum of |d| or d * d in float64 per workgroup, stored as fp32 (1), the partials added in float64, divided, [sqrt], stored as
#            fp32 (1). A squared d carries d's roundings twice.
#   gradient from d: [2 *] d / den (1), or d / (den * l) (2, and l's own error), * m (1), * gscale (1). den is a count below 2^24: exact.
RMSE_EPS = 1e-16


def _diff(a, b, m):
    """(D, kd, Td): the exact a - b or (a - b) m, the roundings of the kernel's d and the magnitude they act on"""
    a, b = _f64(a), _f64(b)
    if m is None:
        return a - b, 1, np.abs(a - b)
    m = _f64(m)
    return (a - b) * m, 3, np.abs(a * m) + np.abs(b * m)


def loss(kind, a, b, m=None, eps=RMSE_EPS, gscale=1.0):
    """kind 'l1' | 'mse' | 'rmse'; m None: mean over all elements (gi_loss_l1 / _mse / _rmse); m given: the masked form of
    gi_loss_local, sum(base(a m - b m)) / count(m != 0) [rmse: sqrt(. + eps)]. Gradient with respect to a, times gscale.
    Returns a dict: value, value_bound, den, grad, grad_bound (float64)."""
    D, kd, Td = _diff(a, b, m)
    mm = np.ones_like(D) if m is None else _f64(m)
    den = F64(D.size) if m is None else F64(np.count_nonzero(mm))
    gs = F64(F32(gscale))
    e = F64(F32(eps))
    if kind == "l1":
        value = np.abs(D).sum() / den
        vb = bound(kd + 2, Td.sum() / den)                       # d, the partial, the result
        grad = np.sign(D) * mm * gs / den
        gb = bound(3, np.abs(grad))                              # the division, * m, * gscale (the sign itself is decided by the test's inputs)
    else:
        mse = (D * D).sum() / den
        T2 = (Td * Td).sum() / den
        if kind == "mse":
            value = mse
            vb = bound(2 * kd + 2, T2)                           # d twice, the partial, the result
            grad = 2.0 * D * mm * gs / den
            gb = bound(kd + 3, 2.0 * Td * np.abs(mm * gs) / den)  # d, the division, * m, * gscale
        else:
            value = np.sqrt(mse + e)
            vb = bound(2 * kd + 2, T2 / value + value)           # d sqrt(x) = dx / (2 sqrt(x)): the sum's roundings over l, the result's on l
            grad = D * mm * gs / (den * value)
            T = Td * np.abs(mm * gs) / (den * value)
            gb = bound(kd + 4, T) + np.abs(grad) * (vb / value)  # d, den * l, the division, * m, * gscale; and l's own error
    return {"value": F64(value), "value_bound": F64(vb), "den": den, "grad": grad, "grad_bound": gb}


# ---- adversarial losses -----------------------------------------------------------------------------------------------------------
def adv_loss(kind, pred, target, gscale=1.0):
    """kind 0: nn.BCELoss against a constant target, the logarithms clamped at -100 and the backward's p (1 - p) at 1e-12;
    1: mean (p - t)^2; 2: mean p. Returns (value, grad) in float64; grad = d value / d pred * gscale."""
    p = _f64(pred)
    n = p.size
    t, gs = F64(F32(target)), F64(F32(gscale))
    if kind == 0:
        with np.errstate(divide="ignore"):
            lp, l1p = np.maximum(np.log(p), -100.0), np.maximum(np.log(1.0 - p), -100.0)
        l = -(t * lp + (1.0 - t) * l1p)
        g = (p - t) / np.maximum(p * (1.0 - p), F64(F32(1e-12)))     # the clamp is a float constant in torch and in the kernel
    elif kind == 1:
        l = (p - t) ** 2
        g = 2.0 * (p - t)
    else:
        l = p
        g = np.ones_like(p)
    return F64(l.sum() / n), g / n * gs


# ---- optimizers ---------------------------------------------------------------------------------------------------------------------
def py_float(x):
    """the decimal a C float hyper-parameter was written as (7 significant digits), as a double: what the host recovers before it
    forms 1 - beta and lr / bias_correction in double, as torch.optim does with its Python floats"""
    return float("%.7g" % float(F32(x)))


def adam_constants(lr, beta1, beta2, step):
    b1d, b2d, lrd = py_float(beta1), py_float(beta2), py_float(lr)
    st = max(int(step), 1)
    return {"step_size": F64(F32(lrd / (1.0 - b1d ** st))), "sqrt_bc2": F64(F32(np.sqrt(1.0 - b2d ** st))),
            "b1": F64(F32(beta1)), "b2": F64(F32(beta2)), "omb1": F64(F32(1.0 - b1d)), "omb2": F64(F32(1.0 - b2d))}


def adam_step(p, g, m, v, lr, beta1, beta2, eps, step, grad_scale=1.0):
    """One step of adam_kernel from fp32 (or float64) state, in float64 with the kernel's fp32 constants. `step` is the effective
    step (after the skipped updates are taken off; below 1 counts as 1).
      gg = g * gs                      1 rounding
      m' = b1 * m + omb1 * gg          gg, the two products, the sum = 4 roundings (fused: 3)
      v' = b2 * v + omb2 * gg * gg     gg twice, omb2 * gg, * gg, b2 * v, the sum = 6 (fused: 5)
      p' = p - step_size * (m' / (sqrt(v') / sqrt_bc2 + eps))
    Returns a dict: m, m_bound, v, v_bound, p, move (|p' - p| of the reference)."""
    c = adam_constants(lr, beta1, beta2, step)
    p, g, m, v = _state(p), _state(g), _state(m), _state(v)
    gg = g * F64(F32(grad_scale))
    mm = c["b1"] * m + c["omb1"] * gg
    vv = c["b2"] * v + c["omb2"] * gg * gg
    move = c["step_size"] * (mm / (np.sqrt(vv) / c["sqrt_bc2"] + F64(F32(eps))))
    return {"m": mm, "m_bound": bound(4, np.abs(c["b1"] * m) + np.abs(c["omb1"] * gg)),
            "v": vv, "v_bound": bound(6, np.abs(c["b2"] * v) + c["omb2"] * gg * gg),
            "p": p - move, "move": np.abs(move)}


def rmsprop_step(p, g, sq, lr, alpha, eps, clampv=0.0, grad_scale=1.0):
    """One step of rmsprop_kernel:
      gg = g * gs ; sq' = alpha * sq + oma * gg * gg     6 roundings as Adam's v (fused: 5), oma = float(1 - the decimal alpha)
      p' = clip(p - lr * (gg / (sqrt(sq') + eps)), -clamp, clamp) when clamp > 0
    Returns a dict: sq, sq_bound, p, move (|unclipped p' - p|)."""
    p, g, sq = _state(p), _state(g), _state(sq)
    al, oma = F64(F32(alpha)), F64(F32(1.0 - py_float(alpha)))
    gg = g * F64(F32(grad_scale))
    s = al * sq + oma * gg * gg
    move = F64(F32(lr)) * (gg / (np.sqrt(s) + F64(F32(eps))))
    w = p - move
    if clampv > 0:
        w = np.clip(w, -F64(F32(clampv)), F64(F32(clampv)))
    return {"sq": s, "sq_bound": bound(6, np.abs(al * sq) + oma * gg * gg), "p": w, "move": np.abs(move)}


def p_bound(ref_p, move):
    """the project's rule for a parameter after one update (tests/test_losses_gpu.py, applied per element here): 1e-6 of the value or
    1e-3 of one move"""
    return 1e-6 * np.abs(ref_p) + 1e-3 * np.abs(move) + TINY


# ---- finite check -------------------------------------------------------------------------------------------------------------------
MAX_BLOCKS = 2048


def nblocks(count, per_thread=4):
    """the grid-size rule of the launchers: 256 threads, per_thread elements each, at most 2048 workgroups"""
    return int(min(max((count + 256 * per_thread - 1) // (256 * per_thread), 1), MAX_BLOCKS))


def check_finite_stride(count):
    """the scan's grid stride in 16-byte chunks: workgroups x 256, two chunks per thread and round"""
    return nblocks((count + 3) // 4, 2) * 256


# ---- gradient statistics ------------------------------------------------------------------------------------------------------------
def grad_absmean(g, off, length):
    """float32(mean |g|) per segment, the sum in float64; exactly 0 for an all-zero segment"""
    g = _f64(g)
    return np.array([F32(np.abs(g[o:o + n]).sum() / n) for o, n in zip(off, length)], dtype=F32)


def ulp_distance(a, b):
    """distance in units of the last place between two float32 arrays of the same sign pattern (finite values)"""
    ia, ib = (np.ascontiguousarray(_f32(x)).view(np.int32).astype(np.int64) for x in (a, b))
    ia, ib = (np.where(i < 0, -(i & 0x7FFFFFFF), i) for i in (ia, ib))
    return np.abs(ia - ib)


# ---- conversions and weight packing (bit-exact) -------------------------------------------------------------------------------------
def convert(src, half):
    with np.errstate(over="ignore"):     # 65520 and above round to inf: that is the result, not a warning
        return _f32(src).astype(np.float16) if half else _f32(src).copy()


def convert_back(src):
    return np.asarray(src).astype(F32)


def phase_taps(ph, t):
    """tap t = (ty, tx) of sub-pixel phase ph = (py, px) of a 4 x 4, stride 2, padding 1 transposed convolution is the kernel
    element (ky, kx) = (1 - py + 2 ty, 1 - px + 2 tx)"""
    py, px, ty, tx = ph >> 1, ph & 1, t >> 1, t & 1
    return 1 - py + 2 * ty, 1 - px + 2 * tx


def pack(w, ca, cb, half, scale=None, scale_on_b=False):
    """w: the fp32 master [ca][16][cb] (k = ky * 4 + kx). Returns (packed [ca][16][cb], phase [4][cb][4][ca]) of the compute type:
    (w * scale) in float32 - one product, nothing to fuse - then converted; scale per a or per b, or None."""
    w = _f32(w).reshape(ca, 16, cb)
    if scale is not None:
        s = _f32(scale)
        w = (w * (s[None, None, :] if scale_on_b else s[:, None, None])).astype(F32)
    T = np.float16 if half else F32
    phase = np.empty((4, cb, 4, ca), dtype=T)
    for ph in range(4):
        for t in range(4):
            ky, kx = phase_taps(ph, t)
            phase[ph, :, t, :] = w[:, ky * 4 + kx, :].T.astype(T)
    return w.astype(T), phase
