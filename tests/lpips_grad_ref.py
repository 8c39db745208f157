"""Differentiable fp64 restatement of LPIPS for the backward of csrc/lpips.hip: tests/lpips_ref.py's arithmetic as torch
autograd, with the GUARDED norm the kernels use, the closed-form seed, fp32 emulations of the new kernels and per-element bounds derived
from that arithmetic.

The guard. d_l = mean_p sum_c w_c (a_c / (|a| + 1e-10) - b^_c)^2. At a = 0 torch autograd gives NaN (the root's derivative is infinite and
meets a zero), and the one-sided derivative would be the meaningless 1e10 w b^. The kernels - and this file - put seed = 0 at such a
pixel: a post-ReLU vector is zero only where every channel's pre-activation is <= 0, so the ReLU mask below removes every channel of that
seed whatever it is, and the image gradient is the same (test_lpips_grad_ref_cpu.py proves both statements). Values are unchanged.
"""
import numpy as np
import torch
import torch.nn.functional as F

import lpips_ref as R

U16, U32, ETA16 = R.U16, R.U32, R.ETA16


def _t(a):
    return a.double() if torch.is_tensor(a) else torch.from_numpy(np.asarray(a)).double()


def _ste16(t):
    """fp16 storage with a straight-through gradient: the value is rounded, the derivative is that of the identity."""
    return t + (t.detach().to(torch.float16).double() - t.detach())


def taps(P, x, fp16=False):
    """lpips_ref.taps on a torch tensor x (n,1,H,W) float64, differentiable. fp16: yardstick (b) - weights, input and every layer's output
    rounded to fp16 - with straight-through rounding."""
    rnd = _ste16 if fp16 else (lambda t: t)
    w16 = (lambda t: t.to(torch.float16).double()) if fp16 else (lambda t: t)
    x = rnd(x)
    h = (2.0 * x.repeat(1, 3, 1, 1) - 1.0 - _t(P["scaling_layer.shift"])) / _t(P["scaling_layer.scale"])
    out = []
    for i, tap in zip(R.CONV_IDX, R.TAP_AFTER):
        h = rnd(F.relu(F.conv2d(h, w16(_t(P[f"features.{i}.weight"])), _t(P[f"features.{i}.bias"]), padding=1)))
        if tap >= 0:
            out.append(h)
            if tap < 4:
                h = F.max_pool2d(h, 2)
    return out


def unit(f, guarded=True):
    """f / (|f| + 1e-10) over the channels (dim 1). guarded: exactly 0, with a zero derivative, where the vector is zero."""
    ss = f.pow(2).sum(1, keepdim=True)
    if not guarded:
        return f / (ss.sqrt() + 1e-10)
    live = ss > 0
    r = torch.where(live, ss, torch.ones_like(ss)).sqrt()
    return torch.where(live, f / (r + 1e-10), torch.zeros_like(f))


def tap_distance(fa, fb, lin, guarded=True):
    """d_l per image (n,) float64, differentiable w.r.t. fa."""
    lin = _t(lin).reshape(1, -1, 1, 1)
    return (lin * (unit(fa, guarded) - unit(fb, guarded)).pow(2)).sum(1).mean((1, 2))


def distance(P, a, b, fp16=False, keep=None):
    """(d (n,), per_layer (5,n)) float64 of torch tensors a (differentiable), b. keep: a list that receives a's five tap maps."""
    ta = taps(P, a, fp16)
    with torch.no_grad():
        tb = taps(P, b, fp16)
    if keep is not None:
        keep.extend(ta)
    per = torch.stack([tap_distance(fa, fb, P[f"lin{k}.model.1.weight"].reshape(-1)) for k, (fa, fb) in enumerate(zip(ta, tb))])
    return per.sum(0), per


def grad(P, a, b, fp16=False, with_taps=False):
    """(d (n,), grad (n,1,H,W)[, tap gradients x 5]) float64: grad[i] = d d[i] / d a[i] (image i's distance depends on a[i] alone, so the
    gradient of the sum is the stack of the per-image gradients). Tap gradients: w.r.t. the post-ReLU tap maps of a."""
    x = _t(a).clone().requires_grad_(True)
    keep = []
    d, _ = distance(P, x, _t(b), fp16, keep)
    gs = torch.autograd.grad(d.sum(), [x] + keep)
    if with_taps:
        return d.detach(), gs[0], list(gs[1:])
    return d.detach(), gs[0]


def rel_l2(x, ref):
    x, ref = _t(x), _t(ref)
    return float((x - ref).norm() / ref.norm())


def cosine(x, ref):
    x, ref = _t(x).reshape(-1), _t(ref).reshape(-1)
    return float((x @ ref) / (x.norm() * ref.norm()))


# ---- the seed ----------------------------------------------------------------------------------------------------------------------
def seed_closed(fa, fb, lin):
    """Closed form of d d_l / d fa (n,C,h,w) float64: (2 / HW) ia (w_k delta_k - q a_k / ra), q = sum_c w_c delta_c a^_c; 0 where ra = 0."""
    fa, fb, w = _t(fa), _t(fb), _t(lin).reshape(1, -1, 1, 1)
    hw = fa.shape[2] * fa.shape[3]
    ra, rb = fa.pow(2).sum(1, keepdim=True).sqrt(), fb.pow(2).sum(1, keepdim=True).sqrt()
    ia, ib = 1.0 / (ra + 1e-10), 1.0 / (rb + 1e-10)
    ah = fa * ia
    delta = ah - fb * ib
    q = (w * delta * ah).sum(1, keepdim=True)
    live = ra > 0
    t = torch.where(live, fa / torch.where(live, ra, torch.ones_like(ra)), torch.zeros_like(fa))
    return torch.where(live, (2.0 / hw) * ia * (w * delta - q * t), torch.zeros_like(fa))


def seed_emulate(fa, fb, lin):
    """What lpips_seed_kernel computes per element in fp32 (channel sums in torch's order), unscaled, as float64."""
    f32 = lambda v: torch.tensor(v, dtype=torch.float32)       # noqa: E731
    fa, fb, w = _t(fa).float(), _t(fb).float(), _t(lin).float().reshape(1, -1, 1, 1)
    hw = fa.shape[2] * fa.shape[3]
    ra, rb = fa.pow(2).sum(1, keepdim=True).sqrt(), fb.pow(2).sum(1, keepdim=True).sqrt()
    ia, ib = 1.0 / (ra + f32(1e-10)), 1.0 / (rb + f32(1e-10))
    pa = fa * ia
    wd = w * (pa - fb * ib)
    q = (wd * pa).sum(1, keepdim=True)
    live = ra > 0
    ir = torch.where(live, 1.0 / torch.where(live, ra, torch.ones_like(ra)), torch.zeros_like(ra))
    k = torch.where(live, f32(2.0 / hw) * ia, torch.zeros_like(ra))
    return (k * (wd - q * (fa * ir))).double()


def seed_bound(fa, fb, lin):
    """Per-element bound on |fp32 kernel - seed_closed| (n,C,h,w), unscaled, before the fp16 store. u = u32, D = 8 + log2(C / 8) the depth
    of a channel sum (a chain of 8 per lane, a butterfly over C / 8 lanes; lpips_ref.tap_bound), a sum of non-negative terms errs by D u of
    itself, a general one by D u of the sum of magnitudes.
      a^, b^:      rho = (D / 2 + 4) u relative (the sum of squares D u, halved by the root; root, + eps, reciprocal, product: 1 each)
      delta_c:     e_c = rho (|a^_c| + |b^_c|) + u |delta_c|
      wd_c:        w_c e_c + u w_c |delta_c|
      q:           per term the factors' errors, (w_c e_c + u w_c |delta_c|) |a^_c| + rho w_c |delta_c| |a^_c|, plus the sum's
                   D u sum_c w_c |delta_c| |a^_c|                                                                        =: dq
      t_k = a_k/ra: tau = (D / 2 + 3) u relative (the root (D / 2 + 1) u, the reciprocal and the product 1 each)
      inner_k = wd_k - q t_k: E_k = w_k e_k + u w_k |delta_k| + dq |t_k| + (tau + u) |q| |t_k| + u (|w_k delta_k| + |q t_k|)
      k = c2 ia:   kappa = (D / 2 + 5) u relative (c2 rounded to fp32: u; ia (D / 2 + 3) u; the product u)
      seed_k:      k E_k + (kappa + u) |seed_k|
    First-order terms only: the neglected products of two errors are below 2^-10 of the bound for C <= 512 (C u < 2^-15); the factor 1.01
    covers them."""
    fa, fb, w = _t(fa), _t(fb), _t(lin).abs().reshape(1, -1, 1, 1)
    C, hw = fa.shape[1], fa.shape[2] * fa.shape[3]
    D = 8 + int(np.log2(C // 8))
    u = U32
    rho, tau, kappa = (D / 2 + 4) * u, (D / 2 + 3) * u, (D / 2 + 5) * u
    ra, rb = fa.pow(2).sum(1, keepdim=True).sqrt(), fb.pow(2).sum(1, keepdim=True).sqrt()
    ia, ib = 1.0 / (ra + 1e-10), 1.0 / (rb + 1e-10)
    ah, bh = (fa * ia).abs(), (fb * ib).abs()
    delta = (fa * ia - fb * ib).abs()
    e = rho * (ah + bh) + u * delta
    dq = ((w * e + u * w * delta) * ah + rho * w * delta * ah).sum(1, keepdim=True) + D * u * (w * delta * ah).sum(1, keepdim=True)
    q = (w * (fa * ia - fb * ib) * (fa * ia)).sum(1, keepdim=True).abs()
    live = ra > 0
    t = torch.where(live, fa.abs() / torch.where(live, ra, torch.ones_like(ra)), torch.zeros_like(fa))
    E = w * e + u * w * delta + dq * t + (tau + u) * q * t + u * (w * delta + q * t)
    k = (2.0 / hw) * ia
    return torch.where(live, 1.01 * (k * E + (kappa + u) * seed_closed(fa, fb, lin).abs()), torch.zeros_like(fa))


def stored_seed_bound(fa, fb, lin, s):
    """Per-element bound on |fp16 store of s * seed - s * seed_closed|, s (n,) powers of two: s E + u16 (|s seed| + s E) + eta16."""
    s = _t(s).reshape(-1, 1, 1, 1)
    E = s * seed_bound(fa, fb, lin)
    return E + U16 * (s * seed_closed(fa, fb, lin).abs() + E) + ETA16


def pow2_scale(m, exp=-2):
    """The power of two that puts m > 0 into [2^(exp-1), 2^exp); 1 for m == 0 (vggtrunk.hip's seed_scale_kernel)."""
    if not m > 0 or not np.isfinite(m):
        return 1.0
    return float(2.0 ** (exp - np.frexp(float(m))[1]))


# ---- activation backward -----------------------------------------------------------------------------------------------------------
def act_bwd_emulate(g, act, seed, pool, relu=True):
    """vggtrunk.hip's act_bwd_kernel bit for bit, NCHW float16 tensors in, float16 out: one fp16 rounding of [act > 0] (routed g + seed) in fp32.
    pool: g is (n,C,H/2,W/2) and goes to the first maximum of each 2x2 window of act in row-major order."""
    act = act.float()
    n, C, H, W = act.shape
    tot = torch.zeros_like(act)
    if g is not None:
        if pool:
            win = act.reshape(n, C, H // 2, 2, W // 2, 2).permute(0, 1, 2, 4, 3, 5).reshape(n, C, H // 2, W // 2, 4)
            # first maximum: the smallest index among the maxima
            ismax = win == win.max(-1, keepdim=True).values
            first = ismax.float().argmax(-1, keepdim=True)           # argmax returns the first of equal values
            route = torch.zeros_like(win).scatter_(-1, first, g.float().unsqueeze(-1))
            tot = route.reshape(n, C, H // 2, W // 2, 2, 2).permute(0, 1, 2, 4, 3, 5).reshape(n, C, H, W)
        else:
            tot = g.float().clone()
    if seed is not None:
        tot = tot + seed.float()
    if relu:
        tot = torch.where(act > 0, tot, torch.zeros_like(tot))
    return tot.half()


# ---- the first-layer adjoint -------------------------------------------------------------------------------------------------------
def conv1_adjoint(wA, D, mul):
    """dx (n,1,H,W) float64 = mul_i sum_o sum_tap wA[o][tap] D[o][p - tap]: the transpose of the 1 -> 64 convolution (the indicator plane is
    constant and contributes nothing). D (n,64,H,W), mul (n,)."""
    return F.conv_transpose2d(_t(D), _t(wA).reshape(64, 1, 3, 3), padding=1) * _t(mul).reshape(-1, 1, 1, 1)


def adjoint_bound(wA, D, mul):
    """Per-element bound on |fp32 kernel - conv1_adjoint|: D (fp16) and wA (fp32) enter exactly; nine chains of 64 fmas (64 u of the sum of
    magnitudes), eight additions of the nine sums (8 u), the product gscale / s_i (u; exact where both are powers of two) and the final
    product (u): 74 u |mul| sum |wA| |D|."""
    return 74 * U32 * F.conv_transpose2d(_t(D).abs(), _t(wA).abs().reshape(64, 1, 3, 3), padding=1) * _t(mul).abs().reshape(-1, 1, 1, 1)


def conv1_adjoint_emulate(wA, D, mul):
    """The same in fp32 (torch's order of summation)."""
    return (F.conv_transpose2d(_t(D).float(), _t(wA).float().reshape(64, 1, 3, 3), padding=1) * _t(mul).float().reshape(-1, 1, 1, 1)).double()


def pack_t(w):
    """[cout][cin][3][3] float32 -> float16 [cin][8 - tap][cout] (vggtrunk.hip's pack3x3_t_kernel)."""
    w = np.asarray(w, np.float32)
    cout, cin = w.shape[:2]
    return np.ascontiguousarray(w.reshape(cout, cin, 9)[:, :, ::-1].transpose(1, 2, 0)).astype(np.float16)
