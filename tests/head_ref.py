"""fp64 references of the PatchGAN critic head (csrc/head.hip), the magnitudes their error bounds need, the bounds, the inputs of
tests/test_head_gpu.py and a numpy emulation of each path's rounding points (tests/test_head_ref_cpu.py keeps all of this honest
without a GPU). Plain torch / numpy on the CPU, written from the definitions in the kernel comments and the header:

  forward   h[i,py,px] = sum_{ky,kx,ch} x[i,py+ky,px+kx,ch] * w5[ky*4+kx][ch];   out[i] = [sigmoid](bl + sum_p wl[p] * h[i,p])
  affine    x = fp16(lrelu(fma(a4, scale[g], shift[g]))), g = i / n_per_group (the raw-a4 forms); else x = a4
  backward  dz[i] = dy[i] * (sigmoid ? out[i] * (1 - out[i]) : 1);   dh[i,p] = dz[i] * wl[p]
            da4[i,y,x,ch] = T(loss_scale * sum_tap dh[i,y-ky,x-kx] * w5[tap][ch])   (positions inside the Ph x Pw map)
            dw5[tap][ch] += sum_{i,p} dh[i,p] * x[i,p+tap,ch];   dwl[p] += sum_i dz[i] * h[i,p];   dbl += sum_i dz[i]
  bn sums   s0[g][ch] = sum dzz, s1[g][ch] = sum dzz * xhat over the pixels of population g, dzz = da4 * (fma(x, scale, shift) > 0 ? 1 :
            slope), xhat = (x - mean) * inv, da4 the STORED (rounded) gradient

Features are NHWC. Every reference returns, next to the value, A = the sum of the absolute values of the terms of each element.
Rounding points that are single deterministic operations are restated: the fp16 c = 512 forward rounds w5 to fp16 (every other
kernel reads the fp32 w5); the affine map is one fp32 fma, the LeakyReLU one fp32 product, the result rounded to fp16."""
import numpy as np
import torch

from c1_ref import SLOPE, U16, U32, ints, uni, worst_ratio  # noqa: F401  (worst_ratio: for the tests)

_D = torch.float64
SEED = 40
SIGMOID_ALLOWANCE = 2.0 ** -22      # 1 / (1 + expf(-z)) against the fp64 sigmoid: 4 ulp of a value below 1.0
ACC_UNIT = 2.0 ** -40               # every addend of an exact accumulator is cut toward -inf to a multiple of this (stat_acc.h)
FP16_SUBNORMAL_HALF = 2.0 ** -25     # rounding error of an fp16 result in the subnormal range
TAPS = [(t >> 2, t & 3) for t in range(16)]


def bands(n, npx):
    """row bands per image of the fp16 c = 512 backward: about 256 workgroups, at least 32 pixels each"""
    b = 1
    while n * b < 256 and npx // (b * 2) >= 32:
        b *= 2
    return b


def band_ranges(n, npx):
    nb = bands(n, npx)
    ppb = (npx + nb - 1) // nb
    return [(b * ppb, min(npx, (b + 1) * ppb)) for b in range(nb)]


def slices(n, npx):
    """workgroups per image of the sliced fp16 c = 512 forward: about 256 of them, at least 256 pixels each"""
    s = 1
    while n * s < 256 and npx // (s * 2) >= 256:
        s *= 2
    return s


# ---- the references ---------------------------------------------------------------------------------------------------------------
def affine_x(a4, aff, swap=False):
    """aff = (scale (G, c), shift (G, c), n_per_group) or None. The fma is evaluated in fp64 and rounded once to fp32, the slope
    product likewise, then one rounding to fp16. swap (a deliberately wrong form): every image takes population 0's vectors."""
    if aff is None:
        return a4.to(_D)
    sc, sh, npg = aff
    g = torch.arange(a4.shape[0]) // npg
    if swap:
        g = torch.zeros_like(g)
    t = (a4.to(_D) * sc.to(_D)[g][:, None, None, :] + sh.to(_D)[g][:, None, None, :]).to(torch.float32)
    y = torch.where(t > 0, t, (t.to(_D) * SLOPE).to(torch.float32))
    return y.to(torch.float16).to(_D)


def forward_ref(a4, w5, wl, bl, sigmoid=0, fast=False, aff=None):
    """a4 (n, Hh, Wh, c), w5 (16, c), wl (P), bl (1) -> dict: h, A_h (n, P), out, A_out (n), pre (out before the sigmoid)"""
    x = affine_x(a4, aff)
    w = (w5.to(torch.float16) if fast else w5).to(_D)
    n, Hh, Wh, c = x.shape
    Ph, Pw = Hh - 3, Wh - 3
    h = torch.zeros(n, Ph, Pw, dtype=_D)
    A = torch.zeros_like(h)
    for t, (ky, kx) in enumerate(TAPS):
        win = x[:, ky:ky + Ph, kx:kx + Pw, :]
        h += (win * w[t]).sum(-1)
        A += (win.abs() * w[t].abs()).sum(-1)
    h, A = h.reshape(n, -1), A.reshape(n, -1)
    b = float(bl.reshape(-1)[0])
    pre = b + h @ wl.to(_D)
    A_out = abs(b) + A @ wl.to(_D).abs()
    return dict(h=h, A_h=A, pre=pre, out=torch.sigmoid(pre) if sigmoid else pre, A_out=A_out)


def dz_ref(dy, out, sigmoid):
    o = out.to(_D)
    return dy.to(_D) * (o * (1 - o) if sigmoid else 1.0)


def backward_ref(a4, Hh, Wh, w5, wl, h, out, dy, sigmoid=0, loss_scale=1.0, aff=None, pre=None, want_w=True):
    """The whole backward. a4 (n, Hh, Wh, c) or None with want_w = False. -> dict name -> (value, A)"""
    w = w5.to(_D)
    c = w.shape[1]
    n = h.shape[0]
    Ph, Pw = Hh - 3, Wh - 3
    dz = dz_ref(dy, out, sigmoid)
    dh = dz[:, None] * wl.to(_D)[None, :]
    dh3 = dh.reshape(n, Ph, Pw)
    da4 = torch.zeros(n, Hh, Wh, c, dtype=_D)
    Aa = torch.zeros_like(da4)
    for t, (ky, kx) in enumerate(TAPS):
        da4[:, ky:ky + Ph, kx:kx + Pw, :] += dh3[..., None] * w[t]
        Aa[:, ky:ky + Ph, kx:kx + Pw, :] += dh3.abs()[..., None] * w[t].abs()
    r = dict(dh=(dh, dh.abs()), da4=(da4 * loss_scale, Aa * abs(loss_scale)))
    if want_w:
        x = affine_x(a4, aff)
        dw5 = torch.zeros(16, c, dtype=_D)
        Aw = torch.zeros_like(dw5)
        for t, (ky, kx) in enumerate(TAPS):
            win = x[:, ky:ky + Ph, kx:kx + Pw, :]
            dw5[t] = torch.einsum("nyx,nyxc->c", dh3, win)
            Aw[t] = torch.einsum("nyx,nyxc->c", dh3.abs(), win.abs())
        dwl, Al = dz @ h.to(_D), dz.abs() @ h.to(_D).abs()
        dbl, Ab = dz.sum().reshape(1), dz.abs().sum().reshape(1)
        if pre is not None:
            p5, pl, pb = (p.to(_D) for p in pre)
            dw5, Aw, dwl, Al, dbl, Ab = dw5 + p5, Aw + p5.abs(), dwl + pl, Al + pl.abs(), dbl + pb, Ab + pb.abs()
        r.update(dw5=(dw5, Aw), dwl=(dwl, Al), dbl=(dbl, Ab))
    return r


def bn_sums_ref(da4_stored, x, scale, shift, mean, inv, npg, slope=SLOPE, swap=False):
    """da4_stored, x (n, Hh, Wh, c); vectors (G, c) fp32 -> s (G, 2, c), A (G, 2, c). swap (wrong on purpose): population 1's
    pixels take population 0's vectors."""
    n, c = x.shape[0], x.shape[-1]
    G = n // npg
    s, A = torch.zeros(G, 2, c, dtype=_D), torch.zeros(G, 2, c, dtype=_D)
    for g in range(G):
        v = 0 if swap else g
        xs, ds = x[g * npg:(g + 1) * npg].to(_D).reshape(-1, c), da4_stored[g * npg:(g + 1) * npg].to(_D).reshape(-1, c)
        pos = xs * scale[v].to(_D) + shift[v].to(_D) > 0
        dzz = ds * torch.where(pos, torch.ones_like(xs), torch.full_like(xs, float(np.float32(slope))))
        t1 = dzz * ((xs - mean[v].to(_D)) * inv[v].to(_D))
        s[g, 0], s[g, 1], A[g, 0], A[g, 1] = dzz.sum(0), t1.sum(0), dzz.abs().sum(0), t1.abs().sum(0)
    return s, A


# ---- the bounds (derived, not tuned; DESIGN.md "parity of the head kernels") ------------------------------------------------------
# A sum of K terms accumulated in fp32 in ANY order errs by at most K * U32 * A (A = sum |terms|); a factor that every term shares
# and that took r fp32 roundings adds r * U32 * A; a result stored in fp16 adds U16 * |ref|.
def bound_h(c, A):
    """16 c products (exact in fp32: both factors have at most 24 bits between them in fp16, and the bound covers the fp32 ones)"""
    return 16 * c * U32 * A


def bound_out(c, P, A_out, sigmoid):
    """P + 1 more terms on top of h's own 16 c; the sigmoid is 1/4-Lipschitz, plus the allowance for expf and the division"""
    b = (16 * c + P + 1) * U32 * A_out
    return 0.25 * b + SIGMOID_ALLOWANCE if sigmoid else b


DZ_ROUNDINGS = 4      # 1 - out, out * that, dy * that, * loss_scale


def bound_dh(ref):
    """dz's roundings and the product with wl; every count below carries one spare rounding for the second-order terms"""
    return (DZ_ROUNDINGS + 2) * U32 * ref.abs()


def bound_da4(fp16, ref, A):
    """at most 16 terms; every term carries dz's roundings, the product dz * wl and the loss scale (one more when it is applied
    to the sum) and one spare: 16 + DZ_ROUNDINGS + 3; one rounding to the compute type, which for an fp16 result below 2^-14 (subnormal: spacing
    2^-24) is half that spacing, not a fraction of the value"""
    store = torch.clamp(U16 * ref.abs(), min=FP16_SUBNORMAL_HALF) if fp16 else 0.0
    return store + (16 + DZ_ROUNDINGS + 3) * U32 * A


def bound_dw5(n, P, A):
    """n * P terms and the value already there, in any order (bands, waves, partials, atomics); dz's roundings and dz * wl"""
    return (n * P + 1 + DZ_ROUNDINGS + 2) * U32 * A


def bound_dwl(n, A):
    """n terms and the value already there; dz's roundings and a product dz * h that need not be fused into the sum"""
    return (n + 1 + DZ_ROUNDINGS + 2) * U32 * A


def bound_bn_sums(pixels, adds, A):
    """A (G, 2, c). pixels terms per channel and population; the slope product, and for quantity 1 the two roundings of xhat;
    `adds` accumulator additions, each cut by less than ACC_UNIT"""
    k = torch.tensor([pixels + 1.0, pixels + 3.0], dtype=_D)[None, :, None]
    return k * U32 * A + adds * ACC_UNIT


# ---- inputs -----------------------------------------------------------------------------------------------------------------------
def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _choice(vals, shape, seed):
    return torch.tensor(vals, dtype=torch.float32)[torch.randint(0, len(vals), shape, generator=_gen(seed))]


def inputs(exact, fp16, n, Hh, Wh, c, seed=SEED, groups=0, sigmoid=0):
    """-> dict: a4 (n, Hh, Wh, c), w5 (16, c), wl (P), bl (1), dy (n), h (n, P), out (n) (the last two: what a backward is GIVEN as
    the saved forward results - independent values, so a backward test does not depend on the forward), pre = (dw5_0, dwl_0, dbl_0),
    and with groups > 0 aff = (scale (groups, c), shift (groups, c), n / groups): then a4 is the RAW tensor.
    Exact: a4 in {-2 .. 3} (raw: {-5, 0, 1, 2, 3}, scale in {1, 2}, shift in {0, 5}: every negative fma result is a multiple of 5,
    whose product with the fp32 constant 0.2f rounds to an integer, so the LeakyReLU branch is exact too), w5 in {-1, 0, 1}, wl and dy
    in {-2, -1, 1, 2} (no image without a gradient), h small integers: every product and every partial sum is an integer below 2^24.
    Rounding: zero-mean uniform values already rounded to the compute type; w5 is NOT rounded to fp16 (the fast forward does)."""
    P = (Hh - 3) * (Wh - 3)
    d = {}
    if exact:
        d["a4"] = _choice([-5, 0, 1, 2, 3], (n, Hh, Wh, c), seed) if groups else torch.randint(-2, 4, (n, Hh, Wh, c), generator=_gen(seed)).float()
        d["w5"], d["wl"], d["bl"] = ints((16, c), seed + 1, 1), _choice([-2, -1, 1, 2], (P,), seed + 2), ints((1,), seed + 3)
        d["dy"], d["h"], d["out"] = _choice([-2, -1, 1, 2], (n,), seed + 4), ints((n, P), seed + 5, 3), ints((n,), seed + 6)
        d["pre"] = (ints((16, c), seed + 7, 4), ints((P,), seed + 8, 4), ints((1,), seed + 9, 4))
        if groups:
            d["aff"] = (_choice([1, 2], (groups, c), seed + 10), _choice([0, 5], (groups, c), seed + 11), n // groups)
    else:
        d["a4"] = uni((n, Hh, Wh, c), seed, fp16=fp16)
        d["w5"], d["wl"], d["bl"] = uni((16, c), seed + 1, fp16=False) / 8, uni((P,), seed + 2, fp16=False) / 4, uni((1,), seed + 3, fp16=False)
        d["dy"], d["h"] = uni((n,), seed + 4, fp16=False), uni((n, P), seed + 5, -4.0, 4.0, fp16=False)
        d["out"] = uni((n,), seed + 6, 0.05, 0.95, fp16=False) if sigmoid else uni((n,), seed + 6, fp16=False)
        d["pre"] = (uni((16, c), seed + 7, fp16=False), uni((P,), seed + 8, fp16=False), uni((1,), seed + 9, fp16=False))
        if groups:
            d["aff"] = (uni((groups, c), seed + 10, 0.5, 1.5, False), uni((groups, c), seed + 11, -0.25, 0.25, False), n // groups)
    d.setdefault("aff", None)
    return d


def bn_bwd_inputs(n, Hh, Wh, c, groups, seed=SEED):
    """-> x (n, Hh, Wh, c) fp16 values, scale, shift, mean, inv (groups, c) fp32"""
    return (uni((n, Hh, Wh, c), seed + 20), uni((groups, c), seed + 21, 0.5, 1.5, False), uni((groups, c), seed + 22, -0.25, 0.25, False),
            uni((groups, c), seed + 23, -0.25, 0.25, False), uni((groups, c), seed + 24, 0.5, 2.0, False))


# ---- the cases of tests/test_head_gpu.py (tests/test_head_ref_cpu.py checks that the integer inputs are exact at every one) ------------
# (n, Hh, Wh, tbuf, kernel): what each reaches is in the comment
FAST_FWD = [
    (3, 4, 4, None, "head_fwd512"),            # P = 1, one tile, 15 idle waves
    (2, 5, 7, None, "head_fwd512"),            # 35 pixels: ragged last tile, clamped loads, rectangular
    (2, 7, 5, None, "head_fwd512"),
    (2, 16, 16, None, "head_fwd512"),          # the 256^2 critic: exactly one tile per wave
    (2, 17, 17, "ok", "head_fwd512"),          # 19 tiles unsliced (tbuf offered, one slice): three waves take a second tile, ragged
    (2, 23, 23, "ok", "head_fwd512_sliced"),   # 2 slices of 17 tiles each, then head_h512_kernel
    (1, 32, 32, "ok", "head_fwd512_sliced"),   # 4 slices (the 512^2 critic)
    (1, 32, 32, None, "head_fwd512"),          # unsliced, about 88 KiB of dynamic LDS: the attribute path
    (1, 32, 32, "short", "head_fwd512"),       # tbuf one float too small: unsliced as well
]
# the fused conv4 BatchNorm + LeakyReLU with the vectors given: (n, populations) on two maps
AFF_CASES = [(n, g, Hh, Wh) for (n, g) in [(3, 1), (4, 2)] for (Hh, Wh) in [(5, 7), (16, 16)]]
# (n, Hh, Wh): bands and what they reach
FAST_BWD = [
    (1, 4, 4), (9, 4, 4), (17, 4, 4), (24, 4, 4),      # one band; nb odd and even, below and above 16: the paired partial loop and its tail
    (3, 5, 7),                                         # one band of 35 pixels
    (2, 13, 9),                                        # 2 bands of 59 and 58 pixels
    (2, 16, 16),                                       # 8 bands of 32
    (1, 17, 17),                                       # 8 bands of 37, the last one 30
    (1, 32, 32),                                       # 32 bands
    (300, 4, 4),                                       # nb = 300: the batch loop of the Linear's gradients runs twice
]
RAW_CASES = [(2, g, Hh, Wh) for g in (1, 2) for (Hh, Wh) in [(13, 9), (16, 16)]]
# (id, fp16, c, GI_HEAD_FAST off)
GENERIC = [("f32-c512", False, 512, False), ("f32-c24", False, 24, False), ("f16-c64", True, 64, False), ("f16-c8", True, 8, False),
           ("f16-c512-fast_off", True, 512, True)]
GEN_MAPS = [(4, 4), (6, 11), (12, 12)]      # P = 1; Ph < 8: one weight-gradient band; Ph = 9: two bands of 5 and 4 rows


# ---- numpy emulation of the kernels' rounding points ------------------------------------------------------------------------------
def _f32(a):
    return np.asarray(a, dtype=np.float64).astype(np.float32)


def _fma32(acc, a, b):
    """fp32(acc + a * b), the product exact (fp64 holds the 48 bits of two fp32 factors)"""
    return (acc.astype(np.float64) + np.asarray(a, np.float64) * np.asarray(b, np.float64)).astype(np.float32)


def emulate_forward(a4, w5, wl, bl, sigmoid=0, fast=False, aff=None, wrong=None):
    """-> h (n, P), out (n) as fp64 tensors. fast: w5 rounded to fp16, one chain per (pixel, tap) over the channels, then the
    taps in order; generic: one chain over (tap, channel). wrong: 'edge_tap' (tap (0, 3) of the last output column reads one
    pixel to the left), 'pop_swap' (population 1 takes population 0's vectors)."""
    x = affine_x(a4, aff, swap=wrong == "pop_swap").numpy()
    w = (w5.to(torch.float16) if fast else w5).double().numpy()
    n, Hh, Wh, c = x.shape
    Ph, Pw = Hh - 3, Wh - 3
    wins = []
    for t, (ky, kx) in enumerate(TAPS):
        win = x[:, ky:ky + Ph, kx:kx + Pw, :].copy()
        if wrong == "edge_tap" and t == 3:
            win[:, :, Pw - 1, :] = x[:, ky:ky + Ph, Pw - 1 + kx - 1, :]
        wins.append(win)
    h = np.zeros((n, Ph, Pw), np.float32)
    for t in range(16):
        if fast:
            tt = np.zeros((n, Ph, Pw), np.float32)
            for ch in range(c):
                tt = _fma32(tt, wins[t][..., ch], w[t, ch])
            h = h + tt
        else:
            for ch in range(c):
                h = _fma32(h, wins[t][..., ch], w[t, ch])
    h = h.reshape(n, -1)
    z = np.zeros(n, np.float32)
    wln = _f32(wl.numpy())
    for p in range(h.shape[1]):
        z = _fma32(z, h[:, p], wln[p])
    z = z + _f32(bl.numpy())[0]
    if sigmoid:
        z = (1.0 / (1.0 + np.exp(-z.astype(np.float64)))).astype(np.float32)
    return torch.from_numpy(h.astype(np.float64)), torch.from_numpy(z.astype(np.float64))


def _dz32(dy, out, sigmoid, scale=None):
    dy, o = _f32(dy.numpy()), _f32(out.numpy())
    dz = dy * (o * (np.float32(1) - o)) if sigmoid else dy
    return dz * np.float32(scale) if scale is not None else dz


def emulate_backward(a4, Hh, Wh, w5, wl, h, out, dy, fp16, sigmoid=0, loss_scale=1.0, aff=None, pre=None, fast=True, want_w=True, wrong=None):
    """-> dict name -> fp64 tensor. fast: the loss scale rides in dz (da4 role), the weight gradient is summed pixel by pixel within
    a row band, the bands' partials in order, then onto the value there; generic: dh = dz * wl stored, the loss scale applied to the
    sum, the weight gradient one chain per image then the images in order. wrong: 'edge_tap' (da4: tap (0, 3) of the last output
    column comes from one position to the left), 'band_drop' (the last pixel of the first band of every image: its da4 is not
    stored and its share of dw5 is missing), 'pop_swap', 'partial_omit' (the last partial is not added), 'image_omit' (dwl, dbl
    without the last image)."""
    w = _f32(w5.numpy())
    wln = _f32(wl.numpy())
    n, c = h.shape[0], w.shape[1]
    Ph, Pw, npx = Hh - 3, Wh - 3, Hh * Wh
    dzw = _dz32(dy, out, sigmoid)
    dza = _dz32(dy, out, sigmoid, loss_scale) if fast else dzw
    ga = (dza[:, None] * wln[None, :]).reshape(n, Ph, Pw)      # fp32 products
    gw = (dzw[:, None] * wln[None, :]).reshape(n, Ph, Pw)
    r = {"dh": torch.from_numpy(gw.reshape(n, -1).astype(np.float64))}
    da4 = np.zeros((n, Hh, Wh, c), np.float32)
    for t, (ky, kx) in enumerate(TAPS):
        g = ga.copy()
        if wrong == "edge_tap" and t == 3 and Pw > 1:
            g[:, :, Pw - 1] = ga[:, :, Pw - 2]
        da4[:, ky:ky + Ph, kx:kx + Pw, :] = _fma32(da4[:, ky:ky + Ph, kx:kx + Pw, :], g[..., None], w[t])
    if not fast:
        da4 = da4 * np.float32(loss_scale)
    ranges = band_ranges(n, npx) if fast else [(0, npx)]
    if wrong == "band_drop":
        q = ranges[0][1] - 1
        da4[:, q // Wh, q % Wh, :] = 0
    r["da4"] = torch.from_numpy((da4.astype(np.float16) if fp16 else da4).astype(np.float64))
    if not want_w:
        return r
    x = affine_x(a4, aff, swap=wrong == "pop_swap").numpy()
    gpad = np.zeros((n, Ph + 6, Pw + 6), np.float32)
    gpad[:, 3:3 + Ph, 3:3 + Pw] = gw
    parts = []
    for i in range(n):
        for bi, (q0, q1) in enumerate(ranges):
            acc = np.zeros((16, c), np.float32)
            for q in range(q0, q1):
                if wrong == "band_drop" and bi == 0 and q == q1 - 1:
                    continue
                y, xx = divmod(q, Wh)
                g = np.array([gpad[i, y + 3 - ky, xx + 3 - kx] for ky, kx in TAPS], np.float32)
                acc = _fma32(acc, g[:, None], x[i, y, xx][None, :])
            parts.append(acc)
    if wrong == "partial_omit":
        parts = parts[:-1]
    s = np.zeros((16, c), np.float32)
    for p in parts:
        s = s + p
    p5, pl, pb = (_f32(p.numpy()) for p in pre) if pre is not None else (np.float32(0), np.float32(0), np.float32(0))
    r["dw5"] = torch.from_numpy((p5 + s).astype(np.float64))
    hn = _f32(h.numpy())
    m = n - 1 if wrong == "image_omit" else n
    gl, gb = np.zeros(hn.shape[1], np.float32), np.float32(0)
    for i in range(m):
        gl = _fma32(gl, dzw[i], hn[i])
        gb = np.float32(gb + dzw[i])
    r["dwl"] = torch.from_numpy(np.asarray(pl + gl, np.float64).reshape(-1))
    r["dbl"] = torch.from_numpy(np.asarray(pb + gb, np.float64).reshape(1))
    return r


def emulate_bn_sums(da4_stored, x, scale, shift, mean, inv, npg, slope=SLOPE, wrong=None):
    """fp32 chains over the pixels of every (image, band), each band's sum cut to the accumulator's unit; 'pop_swap' as above"""
    n, Hh, Wh, c = x.shape
    G = n // npg
    xs, ds = _f32(x.numpy()).reshape(n, -1, c), _f32(da4_stored.numpy()).reshape(n, -1, c)
    sc, sh, mu, iv = (_f32(v.numpy()) for v in (scale, shift, mean, inv))
    out = np.zeros((G, 2, c), np.float64)
    for i in range(n):
        g = i // npg
        v = 0 if wrong == "pop_swap" else g
        for q0, q1 in band_ranges(n, Hh * Wh):
            b0, b1 = np.zeros(c, np.float32), np.zeros(c, np.float32)
            for q in range(q0, q1):
                pos = _fma32(sh[v], xs[i, q], sc[v]) > 0
                dzz = np.where(pos, ds[i, q], ds[i, q] * np.float32(slope))
                b0 = b0 + dzz
                b1 = _fma32(b1, dzz, (xs[i, q] - mu[v]) * iv[v])
            out[g, 0] += np.floor(b0.astype(np.float64) / ACC_UNIT) * ACC_UNIT
            out[g, 1] += np.floor(b1.astype(np.float64) / ACC_UNIT) * ACC_UNIT
    return torch.from_numpy(out)
