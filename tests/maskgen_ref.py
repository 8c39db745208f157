"""Numpy restatement of the device mask generator's definition, independent of the product: Python integers
for the draws, every pixel tested against every segment by brute force in int64. Shares no code with gan_inpainting_amd."""
import numpy as np

M64 = (1 << 64) - 1
G = 0x9E3779B97F4A7C15


def mix(z):
    """The splitmix64 finaliser (the dropout hash of the library)."""
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


def rect_params(seed, key, H, W):
    st = stream_of(seed, key)
    h = uni(st, 0, H // 8, H // 2)
    w = uni(st, 1, W // 8, W // 2)
    y0 = uni(st, 2, 0, H - h)
    x0 = uni(st, 3, 0, W - w)
    return h, w, y0, x0


def _clamp(v, lo, hi):
    return max(lo, min(hi, v))


def freeform_segments(seed, key, H, W):
    """[(ax, ay, bx, by, r)] of the image, stroke after stroke."""
    st = stream_of(seed, key)
    S = min(H, W)
    L = max(2, S // 8)
    rmin = max(1, S // 48)
    rmax = max(rmin, S // 16)
    segs = []
    for s in range(uni(st, 0, 2, 5)):
        b = 64 * (s + 1)
        nv = uni(st, b, 4, 12)
        r = uni(st, b + 1, rmin, rmax)
        x, y = uni(st, b + 2, 0, W - 1), uni(st, b + 3, 0, H - 1)
        vx, vy = uni(st, b + 4, -L, L), uni(st, b + 5, -L, L)
        for j in range(1, nv):
            nx, ny = x + vx, y + vy
            if not 0 <= nx <= W - 1:
                nx, vx = _clamp(nx, 0, W - 1), -vx
            if not 0 <= ny <= H - 1:
                ny, vy = _clamp(ny, 0, H - 1), -vy
            segs.append((x, y, nx, ny, r))
            x, y = nx, ny
            vx = _clamp(vx + uni(st, b + 4 + 2 * j, -(L // 2), L // 2), -L, L)
            vy = _clamp(vy + uni(st, b + 5 + 2 * j, -(L // 2), L // 2), -L, L)
    return segs


def mask(kind, seed, key, H, W):
    """(H, W) uint8 of {0, 1}; kind 'rect' or 'freeform'."""
    if kind == "rect":
        h, w, y0, x0 = rect_params(seed, key, H, W)
        m = np.zeros((H, W), np.uint8)
        m[y0:y0 + h, x0:x0 + w] = 1
        return m
    assert kind == "freeform"
    py, px = np.meshgrid(np.arange(H, dtype=np.int64), np.arange(W, dtype=np.int64), indexing="ij")
    m = np.zeros((H, W), bool)
    for ax, ay, bx, by, r in freeform_segments(seed, key, H, W):
        dx, dy = bx - ax, by - ay
        qx, qy = px - ax, py - ay
        t = qx * dx + qy * dy
        L2 = dx * dx + dy * dy
        r2 = r * r
        near_a = qx * qx + qy * qy <= r2
        near_b = (px - bx) ** 2 + (py - by) ** 2 <= r2
        cross = qx * dy - qy * dx
        side = cross * cross <= r2 * L2
        m |= np.where(t <= 0, near_a, np.where(t >= L2, near_b, side))
    return m.astype(np.uint8)


def masks(kind, seed, keys, H, W):
    """(n, 1, H, W) float32, like the device entry."""
    return np.stack([mask(kind, seed, int(k), H, W) for k in keys]).astype(np.float32)[:, None]
