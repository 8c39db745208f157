"""CPU helper for the FID tests: the FID variant of Inception-V3 up to the 2048-wide pool3 features, restated from the public
architecture (Szegedy et al. 2015, "Rethinking the Inception Architecture"; the layer names are those of the published
`pt_inception-2015-12-05` state dict).

  * keys_and_shapes(): every tensor the published file holds for the feature extractor (no `fc.*`, no `num_batches_tracked`);
  * make_params(seed): machine-independent stand-in weights (numpy PCG64): He-scaled zero-sum convolutions, BatchNorm statistics near
    identity with running variances well above the 0.001 eps;
  * forward(T, x, ...): functional forward in any torch dtype: bilinear resize to 299x299 (align_corners=False), 2x - 1,
    BasicConv2d = conv (no bias) + BatchNorm(eps 0.001, running statistics) + ReLU, average pools that leave the padding out
    of the divisor in Mixed_5b..5d / 6b..6e / 7b, a max pool in Mixed_7c, global average. `round_fn` (e.g. a round trip
    through fp16) is applied to the folded weights and to every layer's output: the rounding points of the fp16 engine.
"""
import numpy as np
import torch
import torch.nn.functional as F

BN_EPS = 0.001

# (name, cin, cout, (kh, kw), stride, (ph, pw))
_STEM = [
    ("Conv2d_1a_3x3", 3, 32, (3, 3), 2, (0, 0)),
    ("Conv2d_2a_3x3", 32, 32, (3, 3), 1, (0, 0)),
    ("Conv2d_2b_3x3", 32, 64, (3, 3), 1, (1, 1)),
    ("Conv2d_3b_1x1", 64, 80, (1, 1), 1, (0, 0)),
    ("Conv2d_4a_3x3", 80, 192, (3, 3), 1, (0, 0)),
]


def _block_a(n, c, pf):
    return [(f"{n}.branch1x1", c, 64, (1, 1), 1, (0, 0)),
            (f"{n}.branch5x5_1", c, 48, (1, 1), 1, (0, 0)),
            (f"{n}.branch5x5_2", 48, 64, (5, 5), 1, (2, 2)),
            (f"{n}.branch3x3dbl_1", c, 64, (1, 1), 1, (0, 0)),
            (f"{n}.branch3x3dbl_2", 64, 96, (3, 3), 1, (1, 1)),
            (f"{n}.branch3x3dbl_3", 96, 96, (3, 3), 1, (1, 1)),
            (f"{n}.branch_pool", c, pf, (1, 1), 1, (0, 0))]


def _block_b(n, c):
    return [(f"{n}.branch3x3", c, 384, (3, 3), 2, (0, 0)),
            (f"{n}.branch3x3dbl_1", c, 64, (1, 1), 1, (0, 0)),
            (f"{n}.branch3x3dbl_2", 64, 96, (3, 3), 1, (1, 1)),
            (f"{n}.branch3x3dbl_3", 96, 96, (3, 3), 2, (0, 0))]


def _block_c(n, c, c7):
    return [(f"{n}.branch1x1", c, 192, (1, 1), 1, (0, 0)),
            (f"{n}.branch7x7_1", c, c7, (1, 1), 1, (0, 0)),
            (f"{n}.branch7x7_2", c7, c7, (1, 7), 1, (0, 3)),
            (f"{n}.branch7x7_3", c7, 192, (7, 1), 1, (3, 0)),
            (f"{n}.branch7x7dbl_1", c, c7, (1, 1), 1, (0, 0)),
            (f"{n}.branch7x7dbl_2", c7, c7, (7, 1), 1, (3, 0)),
            (f"{n}.branch7x7dbl_3", c7, c7, (1, 7), 1, (0, 3)),
            (f"{n}.branch7x7dbl_4", c7, c7, (7, 1), 1, (3, 0)),
            (f"{n}.branch7x7dbl_5", c7, 192, (1, 7), 1, (0, 3)),
            (f"{n}.branch_pool", c, 192, (1, 1), 1, (0, 0))]


def _block_d(n, c):
    return [(f"{n}.branch3x3_1", c, 192, (1, 1), 1, (0, 0)),
            (f"{n}.branch3x3_2", 192, 320, (3, 3), 2, (0, 0)),
            (f"{n}.branch7x7x3_1", c, 192, (1, 1), 1, (0, 0)),
            (f"{n}.branch7x7x3_2", 192, 192, (1, 7), 1, (0, 3)),
            (f"{n}.branch7x7x3_3", 192, 192, (7, 1), 1, (3, 0)),
            (f"{n}.branch7x7x3_4", 192, 192, (3, 3), 2, (0, 0))]


def _block_e(n, c):
    return [(f"{n}.branch1x1", c, 320, (1, 1), 1, (0, 0)),
            (f"{n}.branch3x3_1", c, 384, (1, 1), 1, (0, 0)),
            (f"{n}.branch3x3_2a", 384, 384, (1, 3), 1, (0, 1)),
            (f"{n}.branch3x3_2b", 384, 384, (3, 1), 1, (1, 0)),
            (f"{n}.branch3x3dbl_1", c, 448, (1, 1), 1, (0, 0)),
            (f"{n}.branch3x3dbl_2", 448, 384, (3, 3), 1, (1, 1)),
            (f"{n}.branch3x3dbl_3a", 384, 384, (1, 3), 1, (0, 1)),
            (f"{n}.branch3x3dbl_3b", 384, 384, (3, 1), 1, (1, 0)),
            (f"{n}.branch_pool", c, 192, (1, 1), 1, (0, 0))]


CONVS = (_STEM + _block_a("Mixed_5b", 192, 32) + _block_a("Mixed_5c", 256, 64) + _block_a("Mixed_5d", 288, 64)
         + _block_b("Mixed_6a", 288)
         + _block_c("Mixed_6b", 768, 128) + _block_c("Mixed_6c", 768, 160) + _block_c("Mixed_6d", 768, 160) + _block_c("Mixed_6e", 768, 192)
         + _block_d("Mixed_7a", 768) + _block_e("Mixed_7b", 1280) + _block_e("Mixed_7c", 2048))
CONV_BY_NAME = {c[0]: c for c in CONVS}
BN_SUFFIXES = ("bn.weight", "bn.bias", "bn.running_mean", "bn.running_var")


def keys_and_shapes():
    out = []
    for name, cin, cout, (kh, kw), _, _ in CONVS:
        out.append((f"{name}.conv.weight", (cout, cin, kh, kw)))
        for s in BN_SUFFIXES:
            out.append((f"{name}.{s}", (cout,)))
    return out


def param_count():
    return sum(int(np.prod(s)) for _, s in keys_and_shapes())


def make_params(seed):
    rng = np.random.Generator(np.random.PCG64(seed))
    P = {}
    for name, cin, cout, (kh, kw), _, _ in CONVS:
        std = np.sqrt(2.0 / (cin * kh * kw))
        w = rng.standard_normal((cout, cin, kh, kw)) * std
        # zero-sum filters: the inputs of every layer but the first are non-negative with a large common mode; a filter with a
        # random sum would be switched on or off by that mode alone and a tenth of the features would be dead (constant 0)
        w -= w.mean(axis=(1, 2, 3), keepdims=True)
        P[f"{name}.conv.weight"] = w.astype(np.float32)
        P[f"{name}.bn.weight"] = rng.uniform(0.8, 1.2, cout).astype(np.float32)
        P[f"{name}.bn.bias"] = rng.uniform(0.2, 0.5, cout).astype(np.float32)
        P[f"{name}.bn.running_mean"] = rng.uniform(-0.1, 0.1, cout).astype(np.float32)
        P[f"{name}.bn.running_var"] = rng.uniform(0.5, 1.5, cout).astype(np.float32)
    return P


def make_images(seed, n, c, hw):
    """Smooth random images in [0, 1] (a few random plane waves per channel), fp32 (n, c, hw, hw)."""
    rng = np.random.Generator(np.random.PCG64(seed))
    yy, xx = np.meshgrid(np.arange(hw) / hw, np.arange(hw) / hw, indexing="ij")
    out = np.zeros((n, c, hw, hw), np.float64)
    for i in range(n):
        for ch in range(c):
            for _ in range(6):
                fy, fx = rng.uniform(-6, 6, 2)
                out[i, ch] += rng.uniform(0.2, 1.0) * np.sin(2 * np.pi * (fy * yy + fx * xx) + rng.uniform(0, 2 * np.pi))
            out[i, ch] += 0.3 * rng.standard_normal((hw, hw))
    out = (out - out.min(axis=(2, 3), keepdims=True)) / (out.max(axis=(2, 3), keepdims=True) - out.min(axis=(2, 3), keepdims=True))
    return out.astype(np.float32)


# Frechet-distance cases: name -> (seed, dimensions, samples). The covariance pairs are regenerated from the seed (PCG64 streams are
# machine-independent; a 256- or 2048-wide pair is far beyond what a committed fixture may hold), the fixture holds the values.
FRECHET_CASES = {"d64": (701, 64, 2000), "d256": (702, 256, 3000), "d256_n100": (703, 256, 100), "d2048_n300": (704, 2048, 300)}


def gaussian_stats(rng, d, n):
    """(mu, sigma) of n correlated Gaussian samples in d dimensions (np.mean / np.cov in fp64)."""
    mix = rng.standard_normal((d, d)) / np.sqrt(d) + np.eye(d) * rng.uniform(0.5, 1.0)
    x = rng.standard_normal((n, d)) @ mix + rng.uniform(-0.5, 0.5, d)
    return np.mean(x, axis=0), np.cov(x, rowvar=False)


def frechet_case(name):
    """(mu1, sigma1, mu2, sigma2) of a FRECHET_CASES entry."""
    seed, d, n = FRECHET_CASES[name]
    rng = np.random.Generator(np.random.PCG64(seed))
    return gaussian_stats(rng, d, n) + gaussian_stats(rng, d, n)


def to_torch(P, dtype=torch.float64):
    return {k: torch.from_numpy(np.asarray(v)).to(dtype) for k, v in P.items()}


def round_fp16(t):
    return t.to(torch.float16).to(t.dtype)


def forward(T, x, round_fn=None, blocks=None):
    """T: dict of tensors of one dtype; x: (n, 1 or 3, H, W) in [0, 1], same dtype. Returns (n, 2048).
    round_fn: applied to folded weights and to every layer's output (BatchNorm is then folded in fp32 first, as the engine does).
    blocks: a dict that receives the outputs of Mixed_5d, Mixed_6e and Mixed_7c."""
    rf = round_fn if round_fn is not None else (lambda t: t)

    def conv(name, a):
        _, _, _, _, stride, pad = CONV_BY_NAME[name]
        w, g, b = T[f"{name}.conv.weight"], T[f"{name}.bn.weight"], T[f"{name}.bn.bias"]
        m, v = T[f"{name}.bn.running_mean"], T[f"{name}.bn.running_var"]
        if round_fn is None:
            z = F.conv2d(a, w, None, stride=stride, padding=pad)
            z = (z - m[None, :, None, None]) / torch.sqrt(v[None, :, None, None] + BN_EPS) * g[None, :, None, None] + b[None, :, None, None]
        else:
            s32 = g.float() / torch.sqrt(v.float() + BN_EPS)
            wf = rf((w.float() * s32[:, None, None, None]).to(w.dtype))
            bf = (b.float() - m.float() * s32).to(w.dtype)
            z = F.conv2d(a, wf, bf, stride=stride, padding=pad)
        return rf(F.relu(z))

    def avg(a):
        return rf(F.avg_pool2d(a, 3, 1, 1, count_include_pad=False))

    if x.shape[1] == 1:
        x = x.expand(-1, 3, -1, -1)
    a = F.interpolate(x, size=(299, 299), mode="bilinear", align_corners=False)
    a = rf(2 * a - 1)
    a = conv("Conv2d_1a_3x3", a)
    a = conv("Conv2d_2a_3x3", a)
    a = conv("Conv2d_2b_3x3", a)
    a = F.max_pool2d(a, 3, 2)
    a = conv("Conv2d_3b_1x1", a)
    a = conv("Conv2d_4a_3x3", a)
    a = F.max_pool2d(a, 3, 2)
    for n in ("Mixed_5b", "Mixed_5c", "Mixed_5d"):
        b5 = conv(f"{n}.branch5x5_2", conv(f"{n}.branch5x5_1", a))
        b3 = conv(f"{n}.branch3x3dbl_3", conv(f"{n}.branch3x3dbl_2", conv(f"{n}.branch3x3dbl_1", a)))
        a = torch.cat([conv(f"{n}.branch1x1", a), b5, b3, conv(f"{n}.branch_pool", avg(a))], 1)
    if blocks is not None:
        blocks["Mixed_5d"] = a
    n = "Mixed_6a"
    b3 = conv(f"{n}.branch3x3dbl_3", conv(f"{n}.branch3x3dbl_2", conv(f"{n}.branch3x3dbl_1", a)))
    a = torch.cat([conv(f"{n}.branch3x3", a), b3, F.max_pool2d(a, 3, 2)], 1)
    for n in ("Mixed_6b", "Mixed_6c", "Mixed_6d", "Mixed_6e"):
        b7 = a
        for s in ("1", "2", "3"):
            b7 = conv(f"{n}.branch7x7_{s}", b7)
        bd = a
        for s in ("1", "2", "3", "4", "5"):
            bd = conv(f"{n}.branch7x7dbl_{s}", bd)
        a = torch.cat([conv(f"{n}.branch1x1", a), b7, bd, conv(f"{n}.branch_pool", avg(a))], 1)
    if blocks is not None:
        blocks["Mixed_6e"] = a
    n = "Mixed_7a"
    b3 = conv(f"{n}.branch3x3_2", conv(f"{n}.branch3x3_1", a))
    b7 = a
    for s in ("1", "2", "3", "4"):
        b7 = conv(f"{n}.branch7x7x3_{s}", b7)
    a = torch.cat([b3, b7, F.max_pool2d(a, 3, 2)], 1)
    for n in ("Mixed_7b", "Mixed_7c"):
        t = conv(f"{n}.branch3x3_1", a)
        b3 = torch.cat([conv(f"{n}.branch3x3_2a", t), conv(f"{n}.branch3x3_2b", t)], 1)
        t = conv(f"{n}.branch3x3dbl_2", conv(f"{n}.branch3x3dbl_1", a))
        bd = torch.cat([conv(f"{n}.branch3x3dbl_3a", t), conv(f"{n}.branch3x3dbl_3b", t)], 1)
        p = avg(a) if n == "Mixed_7b" else F.max_pool2d(a, 3, 1, 1)
        a = torch.cat([conv(f"{n}.branch1x1", a), b3, bd, conv(f"{n}.branch_pool", p)], 1)
    if blocks is not None:
        blocks["Mixed_7c"] = a
    return a.mean(dim=(2, 3))
