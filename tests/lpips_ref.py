"""fp64 restatement of LPIPS (Zhang et al. 2018; `lpips` v0.1, net='vgg', normalize=True, spatial=False) from its THREE-CHANNEL
definition, for grey images repeated over the channels - what csrc/lpips.hip is tested against:

    x3 = repeat(x, 3);  s = (2 x3 - 1 - shift) / scale;  13 convolutions 3x3 / s1 / ZERO padding of s, ReLU, 2x2 max pools;
    taps relu1_2, relu2_2, relu3_3, relu4_3, relu5_3;  d_l = mean_p sum_c lin_lc (fa / (|fa| + 1e-10) - fb / (|fb| + 1e-10))^2;  d = sum_l d_l

The `lpips` package is not installed here and nothing is compared with it: this file restates its arithmetic from the paper and the
package's documented behaviour; the weights are stand-ins (make_params). Also here: the two-plane form of the first layer the kernel uses,
fp32 emulations of the kernels (what they compute, rounding for rounding, up to summation order) and per-element bounds derived from
that arithmetic, as c1_ref.py / norm_ref.py do.
"""
import numpy as np
import torch
import torch.nn.functional as F

CONV_IDX = (0, 2, 5, 7, 10, 12, 14, 17, 19, 21, 24, 26, 28)
CHANNELS = (64, 64, 128, 128, 256, 256, 256, 512, 512, 512, 512, 512, 512)
TAP_AFTER = (-1, 0, -1, 1, -1, -1, 2, -1, -1, 3, -1, -1, 4)      # a pool follows every tap but the last
TAP_CHANNELS = (64, 128, 256, 512, 512)
SHIFT = (-.030, -.088, -.188)
SCALE = (.458, .448, .450)
U16, U32, ETA16 = 2.0 ** -11, 2.0 ** -24, 2.0 ** -25             # unit roundoffs; half the spacing of fp16's subnormals


def make_params(seed):
    """Machine-independent stand-in weights (numpy PCG64): He-scaled convolutions, small biases, lin >= 0 around 1/C, the published
    scaling constants. Keys: torchvision's `features.<i>.*` plus the package's `lin<k>.model.1.weight` and `scaling_layer.*`."""
    rng = np.random.Generator(np.random.PCG64(seed))
    P, cin = {}, 3
    for i, cout in zip(CONV_IDX, CHANNELS):
        P[f"features.{i}.weight"] = (rng.standard_normal((cout, cin, 3, 3)) * np.sqrt(2.0 / (9 * cin))).astype(np.float32)
        P[f"features.{i}.bias"] = (0.05 * rng.standard_normal(cout)).astype(np.float32)
        cin = cout
    for k, c in enumerate(TAP_CHANNELS):
        P[f"lin{k}.model.1.weight"] = (rng.random((1, c, 1, 1)) * 2.0 / c).astype(np.float32)
    P["scaling_layer.shift"] = np.asarray(SHIFT, np.float32).reshape(1, 3, 1, 1)
    P["scaling_layer.scale"] = np.asarray(SCALE, np.float32).reshape(1, 3, 1, 1)
    return P


def full_lpips_state_dict(P):
    """The same tensors under the keys of one full LPIPS state dict (`net.slice<k>.<i>.*`: the package's vgg16 wrapper keeps torchvision's
    indices; slices end at the taps)."""
    out = {}
    for i in CONV_IDX:
        k = 1 + sum(1 for e in (3, 8, 15, 22) if i > e)
        for s in ("weight", "bias"):
            out[f"net.slice{k}.{i}.{s}"] = P[f"features.{i}.{s}"]
    for k in range(5):
        out[f"lin{k}.model.1.weight"] = P[f"lin{k}.model.1.weight"]
        out[f"lins.{k}.model.1.weight"] = P[f"lin{k}.model.1.weight"]
    out["scaling_layer.shift"], out["scaling_layer.scale"] = P["scaling_layer.shift"], P["scaling_layer.scale"]
    return out


def make_images(seed, n, H, W):
    """Smooth-ish images in [0,1] (a random field plus a ramp), float32."""
    rng = np.random.Generator(np.random.PCG64(seed))
    coarse = rng.random((n, 1, (H + 3) // 4, (W + 3) // 4))
    x = np.kron(coarse, np.ones((1, 1, 4, 4)))[:, :, :H, :W] * 0.7 + 0.3 * rng.random((n, 1, H, W))
    return np.clip(x, 0.0, 1.0).astype(np.float32)


def _t(a):
    return torch.from_numpy(np.asarray(a)).double()


def _r16(t):
    return t.to(torch.float16).double()


def taps(P, x, fp16=False):
    """The five tap maps [(n,C,h,w) float64] of grey images x (n,1,H,W) from the three-channel definition. fp16: the project's yardstick
    (b) - the same fp64 arithmetic with the weights, the input image and every layer's output rounded to fp16 (the storage roundings of the
    HIP path; its accumulation order and its folded first layer differ)."""
    rnd = _r16 if fp16 else (lambda t: t)
    x = rnd(_t(x))
    h = (2.0 * x.repeat(1, 3, 1, 1) - 1.0 - _t(P["scaling_layer.shift"])) / _t(P["scaling_layer.scale"])
    out = []
    for i, tap in zip(CONV_IDX, TAP_AFTER):
        h = rnd(F.relu(F.conv2d(h, rnd(_t(P[f"features.{i}.weight"])), _t(P[f"features.{i}.bias"]), padding=1)))
        if tap >= 0:
            out.append(h)
            if tap < 4:
                h = F.max_pool2d(h, 2)
    return out


def tap_distance(fa, fb, lin):
    """d_l per image (float64) of two maps (n,C,h,w) and lin (C,)."""
    fa, fb, lin = _t(fa), _t(fb), _t(lin).reshape(1, -1, 1, 1)
    na = fa / (fa.pow(2).sum(1, keepdim=True).sqrt() + 1e-10)
    nb = fb / (fb.pow(2).sum(1, keepdim=True).sqrt() + 1e-10)
    return (lin * (na - nb).pow(2)).sum(1).mean((1, 2))


def distance(P, a, b, fp16=False):
    """(d (n,), per_layer (5,n)) float64."""
    ta, tb = taps(P, a, fp16), taps(P, b, fp16)
    per = torch.stack([tap_distance(fa, fb, P[f"lin{k}.model.1.weight"].reshape(-1)) for k, (fa, fb) in enumerate(zip(ta, tb))])
    return per.sum(0), per


# ---- the first layer ------------------------------------------------------------------------------------------------------------
def conv1_three_channel(w, bias, shift, scale, x):
    """relu(conv(zero-padded scaled input)) (n,64,H,W), float64."""
    h = (2.0 * _t(x).repeat(1, 3, 1, 1) - 1.0 - _t(shift).reshape(1, 3, 1, 1)) / _t(scale).reshape(1, 3, 1, 1)
    return F.relu(F.conv2d(h, _t(w), _t(bias), padding=1))


def fold(w, shift, scale):
    """wA[o][tap] = sum_c w alpha_c, wB[o][tap] = sum_c w beta_c, alpha = 2 / scale, beta = (-1 - shift) / scale; float64 (64,9) each."""
    w, shift, scale = _t(w), _t(shift).reshape(3), _t(scale).reshape(3)
    alpha, beta = 2.0 / scale, (-1.0 - shift) / scale
    return (w * alpha.view(1, 3, 1, 1)).sum(1).reshape(64, 9), (w * beta.view(1, 3, 1, 1)).sum(1).reshape(64, 9)


def fold_bound(w, shift, scale):
    """|fp32 kernel - fold()| per element: alpha carries one rounding, beta two, the three-term fma chain three: 6 u32 sum_c |w coef|."""
    w, shift, scale = _t(w), _t(shift).reshape(3), _t(scale).reshape(3)
    alpha, beta = (2.0 / scale).abs(), ((-1.0 - shift) / scale).abs()
    return (6 * U32 * (w.abs() * alpha.view(1, 3, 1, 1)).sum(1).reshape(64, 9), 6 * U32 * (w.abs() * beta.view(1, 3, 1, 1)).sum(1).reshape(64, 9))


def _planes(x):
    x = _t(x)
    return x, torch.ones_like(x)


def conv1_two_plane(wA, wB, bias, x, pre_relu=False):
    """The kernel's form: a convolution over (x, inside-indicator); zero padding of BOTH planes. float64."""
    x, ind = _planes(x)
    y = F.conv2d(x, _t(wA).reshape(64, 1, 3, 3), _t(bias), padding=1) + F.conv2d(ind, _t(wB).reshape(64, 1, 3, 3), None, padding=1)
    return y if pre_relu else F.relu(y)


def conv1_beta_in_bias(wA, wB, bias, x):
    """The tempting WRONG form: beta folded into the bias (as if the padding were applied to x, not to the scaled input)."""
    return F.relu(F.conv2d(_t(x), _t(wA).reshape(64, 1, 3, 3), _t(bias) + _t(wB).sum(1), padding=1))


def ring_mask(H, W):
    m = torch.zeros(H, W, dtype=torch.bool)
    m[0], m[-1], m[:, 0], m[:, -1] = True, True, True, True
    return m


def conv1_emulate(wA, wB, bias, x):
    """What lpips_conv1_mfma_kernel computes: x rounded to fp16, wA and wB as an fp16 head plus an fp16 remainder (both products are exact
    in fp32), fp32 accumulation from the bias, ReLU, fp16 output (as float64)."""
    def hl(w):
        w = _t(w).float()
        hi = w.half().float()
        return hi + (w - hi).half().float()
    x16, wA16, wB16 = _t(x).half().float(), hl(wA), hl(wB)
    y = F.conv2d(x16, wA16.reshape(64, 1, 3, 3), _t(bias).float(), padding=1) + F.conv2d(torch.ones_like(x16), wB16.reshape(64, 1, 3, 3), None, padding=1)
    return F.relu(y).half().double()


def conv1_bound(wA, wB, bias, x):
    """Per-element bound on |kernel - conv1_two_plane| (n,64,H,W). A weight is an fp16 head plus the fp16 of its remainder: the remainder is
    at most u16 |w| and is itself rounded, dw = u16^2 |w| + eta; dx = u16 |x| + eta (0 for the exact indicator): a product errs by
    dw (|x| + dx) + |w| dx; 64 fp32 accumulation steps (two MFMAs of K = 32, any order) by 64 u32 S, S = |b| + sum |w| |x|; the fp16 store
    by u16 (|ref| + E) + eta. ReLU is 1-Lipschitz."""
    x, ind = _planes(x)
    aA, aB = _t(wA).abs().reshape(64, 1, 3, 3), _t(wB).abs().reshape(64, 1, 3, 3)
    dA, dB = U16 * U16 * aA + ETA16, U16 * U16 * aB + ETA16
    ax, dx = x.abs(), U16 * x.abs() + ETA16
    conv = lambda t, k: F.conv2d(t, k, None, padding=1)      # noqa: E731
    e_prod = conv(ax + dx, dA) + conv(dx, aA) + conv(ind, dB)
    S = _t(bias).abs().view(1, 64, 1, 1) + conv(ax, aA) + conv(ind, aB)
    E = e_prod + 64 * U32 * (S + e_prod)
    ref = conv1_two_plane(wA, wB, bias, x)
    return E + U16 * (ref + E) + ETA16


# ---- the tap kernel --------------------------------------------------------------------------------------------------------------
def tap_emulate(fa, fb, lin):
    """What lpips_tap_kernel computes per pixel in fp32 (channel sums in torch's order), then the fp64 spatial mean rounded to fp32."""
    fa, fb, lin = _t(fa).float(), _t(fb).float(), _t(lin).float().reshape(1, -1, 1, 1)
    ia = 1.0 / (fa.pow(2).sum(1, keepdim=True).sqrt() + torch.tensor(1e-10, dtype=torch.float32))
    ib = 1.0 / (fb.pow(2).sum(1, keepdim=True).sqrt() + torch.tensor(1e-10, dtype=torch.float32))
    d = fa * ia - fb * ib
    v = ((lin * d) * d).sum(1)
    return v.double().mean((1, 2)).float().double()


def tap_five_sum(fa, fb, lin):
    """The expanded form the kernel must NOT use, in fp32: sum w a^2 / |a|^2 - 2 sum w a b / (|a| |b|) + sum w b^2 / |b|^2."""
    fa, fb, lin = _t(fa).float(), _t(fb).float(), _t(lin).float().reshape(1, -1, 1, 1)
    ia = 1.0 / (fa.pow(2).sum(1, keepdim=True).sqrt() + torch.tensor(1e-10, dtype=torch.float32))
    ib = 1.0 / (fb.pow(2).sum(1, keepdim=True).sqrt() + torch.tensor(1e-10, dtype=torch.float32))
    v = (lin * fa * fa).sum(1, keepdim=True) * ia * ia - 2 * (lin * fa * fb).sum(1, keepdim=True) * ia * ib + (lin * fb * fb).sum(1, keepdim=True) * ib * ib
    return v[:, 0].double().mean((1, 2)).float().double()


def near_identical(fa, seed):
    """fa with one element in sixteen moved by one fp16 step: the halves nearly agree, the distance is tiny and cancellation is total."""
    rng = np.random.Generator(np.random.PCG64(seed))
    fb = np.asarray(fa, np.float16).copy()
    pick = (rng.random(fb.shape) < 1 / 16) & (fb > 0)
    fb[pick] = np.nextafter(fb[pick], np.float16(np.inf))
    return fb


def tap_bound(fa, fb, lin):
    """Per-image bound on |kernel - tap_distance| (n,). C channels, u = u32. The kernel adds C non-negative terms as a chain of 8 per lane
    and a butterfly over the C / 8 lanes: every term passes D = 8 + log2(C / 8) additions, so such a sum errs by D u of itself (a pairwise
    or blocked sum of the same depth likewise). A normalised value carries rho = (D / 2 + 4) u relative error (the sum of squares D u,
    halved by the root; the root, + eps, the reciprocal and the product one rounding each). d_c = fl(a^ - b^) errs by delta_c =
    rho (|a-|_c + |b-|_c) + u |d_c|; a term w d^2 by w (2 |d| delta + delta^2) + 2 u w d^2; their sum by D u of itself. Where the two
    vectors nearly agree d and delta are both tiny, so the bound is sharp in absolute terms: the expanded five-sum form, whose error is
    of the order u sum_c w (a-^2 + b-^2) whatever d is, does not pass it. The spatial sum is fp64; the result is rounded to fp32 once."""
    fa, fb, lin = _t(fa), _t(fb), _t(lin).abs().reshape(1, -1, 1, 1)
    C = fa.shape[1]
    D = 8 + int(np.log2(C // 8))
    na = fa / (fa.pow(2).sum(1, keepdim=True).sqrt() + 1e-10)
    nb = fb / (fb.pow(2).sum(1, keepdim=True).sqrt() + 1e-10)
    d = (na - nb).abs()
    rho = (D / 2 + 4) * U32
    delta = rho * (na.abs() + nb.abs()) + U32 * d
    pix = (lin * (2 * d * delta + delta ** 2)).sum(1) + (D + 2) * U32 * (lin * (d + delta) ** 2).sum(1)
    ref = (lin * d ** 2).sum(1).mean((1, 2))
    return pix.mean((1, 2)) + 2 * U32 * ref
