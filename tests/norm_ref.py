"""Plain fp64 restatement of the normalisation and activation-backward passes of csrc/norm.hip, written from the
semantics csrc/common.h documents (the ActBnBwdArgs block, the BatchNorm2d / InstanceNorm2d rules), the fixed-point rules of
csrc/stat_acc.h and the dropout hash of csrc/bn_acc.h. No kernel arithmetic is copied: no chunks, no partial rows, no fp32.
tests/test_norm_ref_cpu.py proves it against torch in fp64; tests/test_norm_ops_gpu.py compares the kernels with it.

Layout: tensors are (pixels, c) torch.float64, vectors (c,)."""
import math

import torch

ACT_NONE, ACT_RELU, ACT_LRELU = 0, 1, 2
F64 = torch.float64


def neg_slope(act):
    return {ACT_NONE: 1.0, ACT_RELU: 0.0, ACT_LRELU: 0.2}[act]


def act_fwd(t, act):
    if act == ACT_NONE:
        return t
    return torch.where(t > 0, t, t * neg_slope(act))


# ---- BatchNorm2d -------------------------------------------------------------------------------------------------------
def col_sums(x):
    """column sum and sum of squares of a (pixels, c) tensor"""
    x = x.to(F64)
    return x.sum(0), (x * x).sum(0)


def bn_from_sums(s, q, count, gamma, beta, rmean, rvar, train=True, momentum=0.1, eps=1e-5):
    """One population. -> dict(scale, shift, mean, inv, rmean, rvar): biased variance for normalisation, unbiased for
    running_var (count 1: the biased one), eval mode normalises with the running statistics and leaves them."""
    gamma, beta, rmean, rvar = (t.to(F64) for t in (gamma, beta, rmean, rvar))
    if train:
        mean = s.to(F64) / count
        var = (q.to(F64) / count - mean * mean).clamp_min(0.0)
        if count == 1:
            var = torch.zeros_like(var)        # one sample has no spread, whatever rounding the sum of squares carries
        unbiased = var * count / (count - 1.0) if count > 1 else var
        rmean = (1.0 - momentum) * rmean + momentum * mean
        rvar = (1.0 - momentum) * rvar + momentum * unbiased
    else:
        mean, var = rmean, rvar
    inv = 1.0 / torch.sqrt(var + eps)
    scale = gamma * inv
    return dict(scale=scale, shift=beta - mean * scale, mean=mean, inv=inv, rmean=rmean, rvar=rvar)


def bn_from_sums_groups(sums, count, gamma, beta, rmean, rvar, train=True, momentum=0.1, eps=1e-5):
    """sums: [(s, q)] per population, handled in call order (the running statistics move population by population)."""
    out = []
    for s, q in sums:
        r = bn_from_sums(s, q, count, gamma, beta, rmean, rvar, train, momentum, eps)
        rmean, rvar = r["rmean"], r["rvar"]
        out.append(r)
    return out


def bn_apply(x, scales, shifts, act, drop=None, drop_scale=1.0, pg=0):
    """y = drop(act(x * scale + shift)); scales / shifts: one vector, or a list of two with pixels >= pg taking the second"""
    x = x.to(F64)
    if isinstance(scales, (list, tuple)) and len(scales) == 2 and 0 < pg < x.shape[0]:
        t = torch.cat([x[:pg] * scales[0] + shifts[0], x[pg:] * scales[1] + shifts[1]], 0)
    else:
        sc, sh = (scales[0], shifts[0]) if isinstance(scales, (list, tuple)) else (scales, shifts)
        t = x * sc + sh
    y = act_fwd(t, act)
    if drop is not None:
        y = torch.where(drop.bool(), y * drop_scale, torch.zeros_like(y))
    return y


def dz_of(g1, g2, sgn, act, drop_scale=1.0):
    """dz = (g1 + g2 * [s > 0]) * (s > 0 ? 1 : slope(act)) * drop_scale. sgn: anything with the sign of the activation's input
    (the saved output y or the pre-activation value); None when nothing needs it."""
    ref = g1 if g1 is not None else g2
    pos = (sgn.to(F64) > 0) if sgn is not None else torch.ones_like(ref, dtype=torch.bool)
    g = torch.zeros_like(ref, dtype=F64)
    if g1 is not None:
        g = g + g1.to(F64)
    if g2 is not None:
        g = g + torch.where(pos, g2.to(F64), torch.zeros_like(g))
    sl = torch.where(pos, torch.ones_like(g), torch.full_like(g, neg_slope(act)))
    return g * sl * drop_scale


def act_bn_bwd(dz, x, gamma, means, invs, groups=1, eval_bn=False, sums=None):
    """dz, x (pixels, c); means / invs: list per population. -> dx, dbeta, dgamma, and the sums of the absolute addends of
    dbeta / dgamma (the scale of their rounding error). Populations are consecutive halves of the pixels. sums: [(sum dz,
    sum dz * xhat)] per population when the caller supplies them (ActBnBwdArgs::reduce_done) instead of the tensors' own."""
    dz, x, gamma = dz.to(F64), x.to(F64), gamma.to(F64)
    P = dz.shape[0]
    pg = P // groups
    dx = torch.empty_like(dz)
    dbeta = torch.zeros(dz.shape[1], dtype=F64)
    dgamma = torch.zeros_like(dbeta)
    abs_b = torch.zeros_like(dbeta)
    abs_g = torch.zeros_like(dbeta)
    for j in range(groups):
        sl = slice(j * pg, (j + 1) * pg)
        mean, inv = means[j].to(F64), invs[j].to(F64)
        xhat = (x[sl] - mean) * inv
        if eval_bn:
            dx[sl] = gamma * inv * dz[sl]
            continue
        s1, s2 = (dz[sl].sum(0), (dz[sl] * xhat).sum(0)) if sums is None else (sums[j][0].to(F64), sums[j][1].to(F64))
        dx[sl] = gamma * inv * (dz[sl] - s1 / pg - xhat * (s2 / pg))
        dbeta += s1
        dgamma += s2
        abs_b += dz[sl].abs().sum(0)
        abs_g += (dz[sl] * xhat).abs().sum(0)
    return dx, dbeta, dgamma, abs_b, abs_g


# ---- InstanceNorm2d(affine=False, track_running_stats=False) -------------------------------------------------------------
def in_forward(x, n, hw, act, drop=None, drop_scale=1.0, eps=1e-5):
    """x (n * hw, c) -> y, mean (n, c), inv (n, c)"""
    x3 = x.to(F64).reshape(n, hw, -1)
    mean = x3.mean(1)
    var = ((x3 - mean[:, None]) ** 2).mean(1)
    inv = 1.0 / torch.sqrt(var + eps)
    y = act_fwd((x3 - mean[:, None]) * inv[:, None], act).reshape(n * hw, -1)
    if drop is not None:
        y = torch.where(drop.bool(), y * drop_scale, torch.zeros_like(y))
    return y, mean, inv


def act_in_bwd(dz, x, n, hw, mean, inv):
    """dx = inv * (dz - mean_p dz - xhat * mean_p(dz * xhat)), the means over the pixels of one (image, channel)"""
    dz3, x3 = dz.to(F64).reshape(n, hw, -1), x.to(F64).reshape(n, hw, -1)
    mean, inv = mean.to(F64)[:, None], inv.to(F64)[:, None]
    xhat = (x3 - mean) * inv
    dx = inv * (dz3 - dz3.mean(1, keepdim=True) - xhat * (dz3 * xhat).mean(1, keepdim=True))
    return dx.reshape(n * hw, -1)


# ---- dropout: splitmix64 of a counter (csrc/bn_acc.h), Python integers ----------------------------------------------------
_M64 = (1 << 64) - 1
_GOLDEN = 0x9E3779B97F4A7C15


def mix64(z):
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & _M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & _M64
    return z ^ (z >> 31)


def dropout_thresh(p):
    """keep when the 32-bit draw >= thresh; p is an fp32 value"""
    t = float(torch.tensor(p, dtype=torch.float32)) * 4294967296.0
    thresh = 0xFFFFFFFF if t >= 4294967295.0 else int(t)
    return thresh if thresh else 1


def dropout_mask(seed, count, p):
    """uint8 keep-mask of elements 0 .. count - 1 (1 with probability 1 - p)"""
    th = dropout_thresh(p)
    return torch.tensor([1 if (mix64((seed + _GOLDEN * (i + 1)) & _M64) >> 32) >= th else 0 for i in range(count)], dtype=torch.uint8)


# ---- exact accumulators (csrc/stat_acc.h) ---------------------------------------------------------------------------------
def stat_acc_total(addends):
    """What reads back after the fp32 values `addends` (any order, any replicas) were added to one accumulator: every addend is
    cut toward -inf to a multiple of 2^-40, the integer total is exact, the read-out forms hi * 2^32 + lo in double. An addend
    that is not below 2^40 in magnitude (inf and NaN included) poisons the total: NaN."""
    hi = lo = 0
    for a in addends:
        a = float(a)
        if not abs(a) < 2.0 ** 40:
            return float("nan")
        units = math.floor(a * 2.0 ** 40)      # exact: a power-of-two scale of an fp32 value, then an integer
        hi += units >> 32                      # floor division: negative values borrow, as two's complement does
        lo += units & 0xFFFFFFFF
    return (float(hi) * 4294967296.0 + float(lo)) * 2.0 ** -40


# ---- small ops ------------------------------------------------------------------------------------------------------------
def tanh_bwd(dy, y, scale):
    return dy.to(F64) * (1.0 - y.to(F64) ** 2) * scale


def mask_layout(src, n, c, hw, to_nhwc):
    return src.reshape(n, c, hw).permute(0, 2, 1).contiguous() if to_nhwc else src.reshape(n, hw, c).permute(0, 2, 1).contiguous()


def lrelu_slope(y):
    """1 where y > 0, else 0.2 (fp64: a bare torch.where(cond, 1.0, 0.2) would be fp32)"""
    y = y.to(F64)
    return torch.where(y > 0, torch.ones_like(y), torch.full_like(y, 0.2))


def mul_slope(t, a):
    return t.to(F64) * lrelu_slope(a)


def bn_tangent_inject(dta, y, tx, x, gamma, mean, inv):
    """BatchNorm (train mode) tangent map tz = gamma * inv * (tx - mean(tx) - xhat * mean(xhat * tx)). With a = slope(y) * dta the
    gradient w.r.t. tz, the scalar sum(a * tz) depends on the PRIMAL x through inv and xhat. -> (d/dx of it, d/dgamma of it)."""
    dta, y, tx, x, gamma, mean, inv = (t.to(F64) for t in (dta, y, tx, x, gamma, mean, inv))
    M = x.shape[0]
    a = dta * lrelu_slope(y)
    xh = (x - mean) * inv
    m1, m2 = tx.mean(0), (tx * xh).mean(0)
    u = tx - m1 - xh * m2
    A = (a * u).sum(0)

    def proj(w):
        return inv * (w - w.mean(0) - xh * (w * xh).mean(0))
    inj = -(gamma * inv * inv) * (xh / M) * A - gamma * inv * (m2 * proj(a) + (a * xh).mean(0) * proj(tx))
    return inj, A * inv


def gp_direction(g, lam):
    """g (n, hw). -> v = d(lam * mean_n (||g_n|| - 1)^2) / dg, the power of two s with max|v * s| in [1, 2) (1 when v is zero),
    the penalty"""
    g = g.to(F64)
    n = g.shape[0]
    norm = g.norm(dim=1)
    coef = torch.where(norm > 0, lam / n * 2.0 * (norm - 1.0) / norm.clamp_min(1e-300), torch.zeros_like(norm))
    v = coef[:, None] * g
    vmax = float(v.abs().max())
    s = 2.0 ** (-math.floor(math.log2(vmax))) if vmax > 0 and math.isfinite(vmax) else 1.0
    return v, s, float(lam * ((norm - 1.0) ** 2).mean())
