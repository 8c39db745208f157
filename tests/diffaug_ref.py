"""Numpy restatement of the differentiable augmentation, independent of the product: Python integers for the
draws, fp64 for the transform and its adjoint, a second pair (fwd32 / bwd32) that follows the device's fp32 operation order
given a mean, and the per-element error bounds that follow from that arithmetic. Shares no code with gan_inpainting_amd."""
import numpy as np

M64 = (1 << 64) - 1
G = 0x9E3779B97F4A7C15
SALT = 0x4449464641554721          # "DIFFAUG!": seed' = seed ^ SALT
COLOUR, TRANSLATION, CUTOUT = 1, 2, 4
NAMES = {"color": COLOUR, "translation": TRANSLATION, "cutout": CUTOUT}
U = 2.0 ** -24                     # unit roundoff of fp32


def mix(z):
    z &= M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return z ^ (z >> 31)


def stream_of(seed, key):
    return mix(seed + G * ((key & M64) + 1))


def draw(stream, k):
    return mix(stream + G * (k + 1)) >> 32


def uni(stream, k, lo, hi):
    return lo + ((draw(stream, k) * (hi - lo + 1)) >> 32)


def policy_bits(policy):
    """'color,translation,cutout' (any non-empty subset) -> bits."""
    bits = 0
    for name in policy.split(","):
        bits |= NAMES[name.strip()]
    return bits


def key_of(step, call, rank, n, i):
    return ((step * 4 + call) << 32) | (rank * n + i)


def params(bits, seed, key, H, W):
    """(b, c, ty, tx, y0, x0, ch, cw) of one sample: the device table's row, the window unclipped. b and c are Python floats
    that fp32 holds exactly."""
    st = stream_of((seed ^ SALT) & M64, key)
    b, c, ty, tx, y0, x0, ch, cw = 0.0, 1.0, 0, 0, 0, 0, 0, 0
    if bits & COLOUR:
        b = (draw(st, 0) >> 8) * 2.0 ** -24 - 0.5
        c = 0.5 + (draw(st, 1) >> 9) * 2.0 ** -23
    if bits & TRANSLATION:
        ty = uni(st, 2, -(H // 8), H // 8)
        tx = uni(st, 3, -(W // 8), W // 8)
    if bits & CUTOUT:
        ch, cw = H // 2, W // 2
        y0 = uni(st, 4, 0, H) - ch // 2
        x0 = uni(st, 5, 0, W) - cw // 2
    return b, c, ty, tx, y0, x0, ch, cw


def table(bits, seed, key0, n, H, W):
    """(n, 8) uint32: the device table, b and c as their fp32 bit patterns."""
    out = np.zeros((n, 8), np.uint32)
    for i in range(n):
        p = params(bits, seed, key0 + i, H, W)
        out[i, :2] = np.array(p[:2], np.float32).view(np.uint32)
        out[i, 2:] = np.array(p[2:], np.int64).astype(np.int32).view(np.uint32)
    return out


def table_row(b, c, ty, tx, y0, x0, ch, cw):
    out = np.zeros(8, np.uint32)
    out[:2] = np.array([b, c], np.float32).view(np.uint32)
    out[2:] = np.array([ty, tx, y0, x0, ch, cw], np.int64).astype(np.int32).view(np.uint32)
    return out


def unpack_row(row):
    row = np.ascontiguousarray(row, np.uint32)
    b, c = (float(v) for v in row[:2].view(np.float32))
    return (b, c) + tuple(int(v) for v in row[2:].view(np.int32))


def keep_mask(p, H, W):
    """(H, W) bool over OUTPUT positions q: True where y[q] = v[q - t] (q - t inside the image, q outside the window)."""
    _, _, ty, tx, y0, x0, ch, cw = p
    qy, qx = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    inside = (qy - ty >= 0) & (qy - ty < H) & (qx - tx >= 0) & (qx - tx < W)
    window = (qy >= y0) & (qy < y0 + ch) & (qx >= x0) & (qx < x0 + cw)
    return inside & ~window


def _shift(v, p, H, W, keep):
    """y[q] = v[q - t] where keep, else 0 (same dtype, values moved untouched)."""
    ty, tx = p[2], p[3]
    y = np.zeros_like(v)
    qy, qx = np.nonzero(keep)
    y[qy, qx] = v[qy - ty, qx - tx]
    return y


def _unshift(dy, p, H, W, keep):
    """dv[p] = dy[p + t] where keep(p + t), else 0."""
    ty, tx = p[2], p[3]
    dv = np.zeros_like(dy)
    qy, qx = np.nonzero(keep)
    dv[qy - ty, qx - tx] = dy[qy, qx]
    return dv


def fwd(x, p, colour):
    """fp64 forward of one (H, W) image."""
    x = np.asarray(x, np.float64)
    H, W = x.shape
    v = x
    if colour:
        m = x.mean()
        v = p[1] * (x - m) + (m + p[0])
    return _shift(v, p, H, W, keep_mask(p, H, W))


def bwd(dy, p, colour):
    """fp64 adjoint of one (H, W) image."""
    dy = np.asarray(dy, np.float64)
    H, W = dy.shape
    dv = _unshift(dy, p, H, W, keep_mask(p, H, W))
    if colour:
        return p[1] * dv + (1.0 - p[1]) * dv.mean()
    return dv


def move(x, p):
    """Translation and cutout alone on the raw values (any dtype: used on uint32 views for the bit-exact tests)."""
    H, W = x.shape
    return _shift(x, p, H, W, keep_mask(p, H, W))


def move_adjoint(dy, p):
    H, W = dy.shape
    return _unshift(dy, p, H, W, keep_mask(p, H, W))


def fwd32(x, p, m):
    """The device's fp32 arithmetic given the mean m (fp32): y = fl(fl(c * fl(x - m)) + fl(m + b)) on kept positions."""
    x = np.asarray(x, np.float32)
    H, W = x.shape
    b, c, m = np.float32(p[0]), np.float32(p[1]), np.float32(m)
    v = (c * (x - m)).astype(np.float32) + np.float32(m + b)
    return _shift(v.astype(np.float32), p, H, W, keep_mask(p, H, W))


def bwd32(dy, p, mean_dv):
    """dx = fl(fl(c * dv) + fl(fl(1 - c) * mean)) at every position."""
    dy = np.asarray(dy, np.float32)
    H, W = dy.shape
    c, mean_dv = np.float32(p[1]), np.float32(mean_dv)
    dv = _unshift(dy, p, H, W, keep_mask(p, H, W))
    k = np.float32(np.float32(np.float32(1.0) - c) * mean_dv)
    return ((c * dv).astype(np.float32) + k).astype(np.float32)


# ---- error bounds -------------------------------------------------------------------------------------------------------------
# The mean. The device adds the N = H W fp32 values of a sample in fp64 in some fixed order, divides by N in fp64 and rounds to
# fp32. Any order of N - 1 fp64 additions has |s - S| <= (N - 1) 2^-53 sum|x| (1 + o(1)); the division and the rounding to fp32
# add 2^-53 and 2^-24 relative to the result. Hence, with A = mean|x| and M the exact mean,
#     |m - M| <= 2^-24 |M| + N 2^-53 A + (tiny second-order terms, covered by the factor SAFE below).
SAFE = 1.01


def mean_bound(values):
    """Bound on |device mean - exact mean| for the values that enter the sum (fp64 array)."""
    values = np.asarray(values, np.float64)
    n = values.size
    return SAFE * (U * abs(values.mean()) + n * 2.0 ** -53 * np.abs(values).mean())


def fwd_bound(x, p):
    """Per-element bound on |device forward - fwd| with colour on. With m the device mean and dm = |m - M|:
    fl(x - m), the product with c, fl(m + b) and the final sum round once each (relative 2^-24), so
        |y - [c (x - m) + (m + b)]| <= u (3 |c| |x - m| + 2 |m + b|)        (first order; SAFE covers the rest)
    and replacing m by M moves the exact value by |1 - c| dm and the magnitudes above by at most (|c| + 1) dm."""
    x = np.asarray(x, np.float64)
    H, W = x.shape
    b, c = p[0], p[1]
    M = x.mean()
    dm = mean_bound(x)
    e = U * (3 * abs(c) * (np.abs(x - M) + dm) + 2 * (abs(M + b) + dm)) + abs(1 - c) * dm
    return SAFE * _shift(e, p, H, W, keep_mask(p, H, W))


def bwd_bound(dy, p):
    """Per-element bound on |device adjoint - bwd| with colour on. 1 - c is exact in fp32 (c is a multiple of 2^-23 in [0.5, 1.5));
    k = fl((1 - c) mean), fl(c dv) and the sum round once each:
        |dx - DX| <= u (2 |c dv| + 2 |(1 - c) MEAN|) + |1 - c| dmean (1 + 2u)."""
    dy = np.asarray(dy, np.float64)
    H, W = dy.shape
    c = p[1]
    dv = _unshift(dy, p, H, W, keep_mask(p, H, W))
    dmean = mean_bound(dv)
    return SAFE * (U * (2 * np.abs(c * dv) + 2 * abs((1 - c) * dv.mean())) + abs(1 - c) * dmean * (1 + 2 * U))


def adjoint_bound(x, dy, p, colour):
    """Bound on |<y_dev, dy> - <x, dx_dev>| evaluated in fp64 on device outputs: the identity is exact for (fwd, bwd), each device
    output is within its per-element bound (zero with colour off: the values are moved), and the fp64 dot products of N terms
    add N 2^-53 sum|terms|."""
    x, dy = np.asarray(x, np.float64), np.asarray(dy, np.float64)
    n = x.size
    y, dx = fwd(x, p, colour), bwd(dy, p, colour)
    eps = n * 2.0 ** -53 * (np.abs(y * dy).sum() + np.abs(x * dx).sum())
    if not colour:
        return SAFE * eps
    return SAFE * ((np.abs(dy) * fwd_bound(x, p)).sum() + (np.abs(x) * bwd_bound(dy, p)).sum() + eps)
