"""CPU helper for the differentiable VGG-19 perceptual / style tests: the two terms of oracle.torch_ref.perceptual_and_style_loss
WITHOUT no_grad, so autograd (fp64) gives the gradient the reference never takes. The feature stack restates
oracle.torch_ref.vgg19_tap_features (test_vgg_grad_cpu.py pins the two to each other) with three additions:

  * store: oracle.torch_ref.store_fp16 after every activation and pooled map (value and arriving gradient rounded to fp16, as an
    engine that keeps both in fp16 does) and on the weights in the forward direction only;
  * scale: the loss is multiplied by it before backward and the gradients divided by it afterwards (a power of two moves the
    fp16 rounding of `store` to where the engine's scaled backward has it, and changes nothing else);
  * keep: the post-ReLU maps of the 13 convolutions with retain_grad, for a per-layer comparison.

The analytic seeds (the derivatives of both terms w.r.t. a tap's feature map) are restated here as the kernels implement them.
"""
import torch
import torch.nn.functional as F

from oracle import params as op
from oracle import torch_ref as orc

TAP_LAYERS = (0, 2, 4, 8, 12)          # convolution index (0..12) of relu1_1, relu2_1, relu3_1, relu4_1, relu5_1


def features(P, x, store=None, keep=None):
    """The five tap maps of the grey batch x. keep (a list): receives the 13 post-ReLU maps, each with retain_grad."""
    h = x.repeat(1, 3, 1, 1)
    taps, i, layer = [], 0, 0
    for v in op.VGG19_CFG:
        if v == "M":
            h = F.max_pool2d(h, 2, 2)
            if store is not None:
                h = store(h)
            i += 1
        else:
            w = P[f"features.{i}.weight"]
            if store is not None:
                w = store(w, True, False)
            h = F.relu(F.conv2d(h, w, P[f"features.{i}.bias"], padding=1))
            if keep is not None:
                if h.requires_grad:
                    h.retain_grad()
                keep.append(h)
            if store is not None:
                h = store(h)
            if i + 1 in orc.VGG_TAPS:
                taps.append(h)
            i += 2
            layer += 1
        if i > 29:
            break
    return taps


def terms(fo, ft):
    p_terms = [torch.mean(torch.pow(a - b, 2)) for a, b in zip(fo, ft)]
    s_terms = [torch.mean(torch.pow(orc.gram_matrix(a) - orc.gram_matrix(b), 2)) for a, b in zip(fo, ft)]
    return p_terms, s_terms


def loss(P, out, tgt, wp, ws, store=None, keep=None):
    """(wp * sum of perceptual terms, ws * sum of style terms), differentiable w.r.t. `out`; `tgt` is a constant."""
    fo = features(P, out, store, keep)
    with torch.no_grad():
        ft = features(P, tgt.detach(), store)
    p_terms, s_terms = terms(fo, ft)
    return wp * sum(p_terms), ws * sum(s_terms)


def grad(P, out, tgt, wp, ws, store=None, scale=1.0, layers=False, dtype=torch.float64):
    """d(p + s)/d(out) by autograd in `dtype`; with layers=True also the 13 gradients w.r.t. the post-ReLU maps."""
    Pd = {k: v.to(dtype) for k, v in P.items()}
    x = out.detach().to(dtype).requires_grad_(True)
    keep = [] if layers else None
    p, s = loss(Pd, x, tgt.to(dtype), wp, ws, store, keep)
    ((p + s) * scale).backward()
    g = x.grad / scale
    if layers:
        return g, [k.grad / scale for k in keep]
    return g


def pow2_scale_for(g, target_exp=-3):
    """The power of two that puts max |g| into [2^(target_exp - 1), 2^target_exp)."""
    m = float(g.abs().max())
    if m == 0.0:
        return 1.0
    _, e = torch.frexp(torch.tensor(m, dtype=torch.float64))
    return 2.0 ** (target_exp - int(e))


def seeds(fo, ft, wp, ws):
    """Analytic d(wp P + ws S)/dF_o per tap:  wp 2 (F_o - F_t)/(n C H W)  +  ws 4/(n C^2 HW C) (G_o - G_t) F_o."""
    out = []
    for a, b in zip(fo, ft):
        n, C, H, W = a.shape
        dG = orc.gram_matrix(a) - orc.gram_matrix(b)
        sty = torch.bmm(dG, a.reshape(n, C, -1)).reshape(a.shape) * (4.0 / (n * C * C * H * W * C))
        out.append(wp * 2.0 * (a - b) / (n * C * H * W) + ws * sty)
    return out


def rel_l2(a, b):
    a, b = a.double().reshape(-1), b.double().reshape(-1)
    return float((a - b).norm() / b.norm())


def cosine(a, b):
    a, b = a.double().reshape(-1), b.double().reshape(-1)
    return float(torch.dot(a, b) / (a.norm() * b.norm()))
