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


# ---- the step-level tier ---------------------------------------------------------------------------------------------------------
# The engine runs the network as a program of 107 steps (94 convolutions, 13 pools) over four activation buffers: 0 / 1 hold a
# block's input and its concatenated output in turn, 2 / 3 are branch temporaries; a branch's last convolution writes at its channel
# offset of the block's output rows, so no concatenation pass exists. steps() restates that program from the public architecture.
U32 = 2.0 ** -24          # unit roundoff of fp32


def make_params_exact_fold(seed):
    """make_params(seed) with every convolution weight rounded to fp16 (exact in both compute types), bn.weight = 1 and
    bn.running_var = float32(0.999): fl32(0.999f + 0.001f) == 1.0f, so the folded scale is exactly 1, the folded weight is the weight
    itself and the folded bias is fl32(beta - mean) however the expression is contracted."""
    P = make_params(seed)
    for name, *_ in CONVS:
        w = P[f"{name}.conv.weight"]
        P[f"{name}.conv.weight"] = w.astype(np.float16).astype(np.float32)
        P[f"{name}.bn.weight"] = np.ones_like(P[f"{name}.bn.weight"])
        P[f"{name}.bn.running_var"] = np.full_like(P[f"{name}.bn.running_var"], np.float32(0.999))
    return P


def steps():
    """The 107-step program: dicts with kind ("conv", "max_s2", "avg_s1", "max_s1"), name / conv (the convolution and its index in
    CONVS, or None / -1), src (-1: the resized 8-channel input) / dst buffer, in_chw / out_chw (the views), ldout (channels of a
    destination row) and coffout (where the output view starts in it)."""
    out, hw = [], {-1: (299, 299)}
    index = {c[0]: i for i, c in enumerate(CONVS)}

    def conv(name, src, dst, ldout=None, coffout=0):
        _, cin, cout, (kh, kw), st, (ph, pw) = CONV_BY_NAME[name]
        h, w = hw[src]
        ho, wo = (h + 2 * ph - kh) // st + 1, (w + 2 * pw - kw) // st + 1
        out.append(dict(kind="conv", name=name, conv=index[name], src=src, dst=dst, in_chw=(8 if src < 0 else cin, h, w),
                        out_chw=(cout, ho, wo), ldout=cout if ldout is None else ldout, coffout=coffout))
        hw[dst] = (ho, wo)

    def pool(kind, src, c, dst, ldout=None, coffout=0):
        h, w = hw[src]
        ho, wo = ((h - 3) // 2 + 1, (w - 3) // 2 + 1) if kind == "max_s2" else (h, w)
        out.append(dict(kind=kind, name=None, conv=-1, src=src, dst=dst, in_chw=(c, h, w), out_chw=(c, ho, wo),
                        ldout=c if ldout is None else ldout, coffout=coffout))
        hw[dst] = (ho, wo)

    conv("Conv2d_1a_3x3", -1, 0)
    conv("Conv2d_2a_3x3", 0, 1)
    conv("Conv2d_2b_3x3", 1, 0)
    pool("max_s2", 0, 64, 1)
    conv("Conv2d_3b_1x1", 1, 0)
    conv("Conv2d_4a_3x3", 0, 1)
    pool("max_s2", 1, 192, 0)
    x = 0
    for n, c, pf in (("Mixed_5b", 192, 32), ("Mixed_5c", 256, 64), ("Mixed_5d", 288, 64)):
        y, ld = x ^ 1, 224 + pf
        conv(f"{n}.branch1x1", x, y, ld, 0)
        conv(f"{n}.branch5x5_1", x, 2)
        conv(f"{n}.branch5x5_2", 2, y, ld, 64)
        conv(f"{n}.branch3x3dbl_1", x, 2)
        conv(f"{n}.branch3x3dbl_2", 2, 3)
        conv(f"{n}.branch3x3dbl_3", 3, y, ld, 128)
        pool("avg_s1", x, c, 2)
        conv(f"{n}.branch_pool", 2, y, ld, 224)
        x = y
    n, y = "Mixed_6a", x ^ 1
    conv(f"{n}.branch3x3", x, y, 768, 0)
    conv(f"{n}.branch3x3dbl_1", x, 2)
    conv(f"{n}.branch3x3dbl_2", 2, 3)
    conv(f"{n}.branch3x3dbl_3", 3, y, 768, 384)
    pool("max_s2", x, 288, y, 768, 480)
    x = y
    for n in ("Mixed_6b", "Mixed_6c", "Mixed_6d", "Mixed_6e"):
        y = x ^ 1
        conv(f"{n}.branch1x1", x, y, 768, 0)
        conv(f"{n}.branch7x7_1", x, 2)
        conv(f"{n}.branch7x7_2", 2, 3)
        conv(f"{n}.branch7x7_3", 3, y, 768, 192)
        conv(f"{n}.branch7x7dbl_1", x, 2)
        conv(f"{n}.branch7x7dbl_2", 2, 3)
        conv(f"{n}.branch7x7dbl_3", 3, 2)
        conv(f"{n}.branch7x7dbl_4", 2, 3)
        conv(f"{n}.branch7x7dbl_5", 3, y, 768, 384)
        pool("avg_s1", x, 768, 2)
        conv(f"{n}.branch_pool", 2, y, 768, 576)
        x = y
    n, y = "Mixed_7a", x ^ 1
    conv(f"{n}.branch3x3_1", x, 2)
    conv(f"{n}.branch3x3_2", 2, y, 1280, 0)
    conv(f"{n}.branch7x7x3_1", x, 2)
    conv(f"{n}.branch7x7x3_2", 2, 3)
    conv(f"{n}.branch7x7x3_3", 3, 2)
    conv(f"{n}.branch7x7x3_4", 2, y, 1280, 320)
    pool("max_s2", x, 768, y, 1280, 512)
    x = y
    for n, c in (("Mixed_7b", 1280), ("Mixed_7c", 2048)):
        y = x ^ 1
        conv(f"{n}.branch1x1", x, y, 2048, 0)
        conv(f"{n}.branch3x3_1", x, 2)
        conv(f"{n}.branch3x3_2a", 2, y, 2048, 320)
        conv(f"{n}.branch3x3_2b", 2, y, 2048, 704)
        conv(f"{n}.branch3x3dbl_1", x, 2)
        conv(f"{n}.branch3x3dbl_2", 2, 3)
        conv(f"{n}.branch3x3dbl_3a", 3, y, 2048, 1088)
        conv(f"{n}.branch3x3dbl_3b", 3, y, 2048, 1472)
        pool("avg_s1" if n == "Mixed_7b" else "max_s1", x, c, 2)
        conv(f"{n}.branch_pool", 2, y, 2048, 1856)
        x = y
    return out


STEPS = steps()


def block_writers():
    """{Mixed block: the steps that write a branch into the block's concatenated rows, in program order}; the last is the block's last."""
    out, cur = {}, None
    for i, s in enumerate(STEPS):
        if s["name"] and s["name"].startswith("Mixed"):
            cur = s["name"].split(".")[0]
        if cur and s["ldout"] != s["out_chw"][0]:
            out.setdefault(cur, []).append(i)
    return out


def step_label(step):
    s = STEPS[step]
    return s["name"] if s["name"] else f"{s['kind']} after step {step - 1}"


def _gamma(m):
    return m * U32 / (1.0 - m * U32)


def _fp16_rounding(ref):
    """One rounding of a result to fp16: half an ulp, relative 2^-11 in the normal range, 2^-25 absolute below it."""
    return 2.0 ** -11 * ref.abs() + 2.0 ** -25


def exact_fold_bias(T, name):
    """fl32(beta - mean) in T's dtype."""
    return (T[f"{name}.bn.bias"].float() - T[f"{name}.bn.running_mean"].float()).to(T[f"{name}.bn.bias"].dtype)


def step_apply(step, a, T, round_fn=None):
    """One step in a's dtype on exact-fold parameters T (scale 1): the engine's stand-in when a is fp32 (round_fn = round_fp16 for the
    fp16 engine). a: the step's input view (step 0: 8 channels, 3 of them used)."""
    s = STEPS[step]
    rf = round_fn if round_fn is not None else (lambda t: t)
    if s["kind"] == "conv":
        name, cin, _, _, stride, pad = CONV_BY_NAME[s["name"]]
        return rf(F.relu(F.conv2d(a[:, :cin], T[f"{name}.conv.weight"], exact_fold_bias(T, name), stride=stride, padding=pad)))
    if s["kind"] == "max_s2":
        return F.max_pool2d(a, 3, 2)
    if s["kind"] == "max_s1":
        return F.max_pool2d(a, 3, 1, 1)
    return rf(F.avg_pool2d(a, 3, 1, 1, count_include_pad=False))


def step_reference(step, a, T, dtype="fp32"):
    """(ref, tol) in fp64 of one step on the input view `a` as the engine held it. T: exact-fold parameters in fp64. dtype: the engine's
    compute type. With u = 2^-24 and gamma(m) = m u / (1 - m u):
      convolution   tol = gamma(K + 2) S + 1e-30, S = conv(|a|, |W|) + |b|, K = kh kw cinp: the worst case of an fp32-accumulated dot
                    product of K terms in any order plus the bias; fp16 x fp16 products are exact in fp32, fp32 x fp16 ones round once
                    (within gamma(K)); 1e-30 covers flushed denormal products (< 4032 terms below 2^-126); ReLU is 1-Lipschitz
      average pool  tol = 10 u avg|a|: at most 8 additions and one division
      max pools     tol = 0
    fp16 adds the one rounding of the output."""
    s = STEPS[step]
    a = a.double()
    if s["kind"] == "conv":
        name, cin, _, (kh, kw), stride, pad = CONV_BY_NAME[s["name"]]
        w, b = T[f"{name}.conv.weight"].double(), exact_fold_bias(T, name).double()
        ref = F.relu(F.conv2d(a[:, :cin], w, b, stride=stride, padding=pad))
        S = F.conv2d(a[:, :cin].abs(), w.abs(), b.abs(), stride=stride, padding=pad)
        K = kh * kw * ((cin + 7) // 8 * 8)
        tol = _gamma(K + 2) * S + 1e-30
    elif s["kind"] == "avg_s1":
        ref = F.avg_pool2d(a, 3, 1, 1, count_include_pad=False)
        tol = 10 * U32 * F.avg_pool2d(a.abs(), 3, 1, 1, count_include_pad=False)
    else:
        ref = F.max_pool2d(a, 3, 2) if s["kind"] == "max_s2" else F.max_pool2d(a, 3, 1, 1)
        return ref, torch.zeros_like(ref)
    if dtype == "fp16":
        tol = tol + _fp16_rounding(ref)
    return ref, tol


def gap_reference(a):
    """(ref, tol) of the global average of the last step's output: 64 pixels added in fp32 and one division."""
    a = a.double()
    return a.mean(dim=(2, 3)), 65 * U32 * a.abs().mean(dim=(2, 3))


def input_reference(x, dtype="fp32"):
    """(ref, tol) in fp64, (n, 3, 299, 299), of the input kernel on x (n, 1 or 3, H, W) fp32 in [0, 1]: bilinear resize
    (align_corners = False), 2 r - 1. Per pixel tol = 4 (ulp32(H) + ulp32(W)) D + 16 u: the source coordinate is formed in fp32 (the
    scale H / 299, a product and a difference of magnitude <= H: within 2 ulp32(H), contracted into an fma or not), a coordinate error
    d moves r by at most d D, D the largest difference among the pixel's four source neighbours, and 2 r - 1 doubles it; 16 u covers
    the two lerps and the affine map on values in [-1, 1]. fp16 storage adds its one rounding."""
    n, c, H, W = x.shape
    xd = x.double()
    if c == 1:
        xd = xd.expand(-1, 3, -1, -1)
    ref = 2 * F.interpolate(xd, size=(299, 299), mode="bilinear", align_corners=False) - 1

    def cells(size):
        f = np.maximum(size / 299.0 * (np.arange(299) + 0.5) - 0.5, 0.0)
        i0 = np.minimum(np.floor(f).astype(np.int64), size - 1)
        return torch.from_numpy(i0), torch.from_numpy(np.minimum(i0 + 1, size - 1))
    y0, y1 = cells(H)
    x0, x1 = cells(W)
    nb = torch.stack([xd[:, :, yy][:, :, :, xx] for yy in (y0, y1) for xx in (x0, x1)])
    D = nb.max(dim=0).values - nb.min(dim=0).values
    tol = 4 * (float(np.spacing(np.float32(H))) + float(np.spacing(np.float32(W)))) * D + 16 * U32
    if dtype == "fp16":
        tol = tol + _fp16_rounding(ref)
    return ref, tol


def run_program(T, x, round_fn=None, hook=None, keep=False):
    """The stand-in engine: the 107 steps in fp32 over the four buffers, as the device routes them. x: (n, 1 or 3, H, W) fp32.
    hook(step, a, out) may return a replacement for a step's output (fault injection). Returns (features, records), records (if keep)
    a list of (input view, output view) per step."""
    rf = round_fn if round_fn is not None else (lambda t: t)
    n = x.shape[0]
    x3 = x.expand(-1, 3, -1, -1) if x.shape[1] == 1 else x
    a = rf(2 * F.interpolate(x3, size=(299, 299), mode="bilinear", align_corners=False) - 1)
    buf = {-1: torch.cat([a, torch.zeros(n, 5, 299, 299, dtype=a.dtype)], 1)}
    rec = []
    for i, s in enumerate(STEPS):
        src = buf[s["src"]][:, :s["in_chw"][0]]
        out = step_apply(i, src, T, round_fn)
        if hook is not None:
            r = hook(i, src, out)
            out = out if r is None else r
        d = buf.get(s["dst"])
        if d is None or tuple(d.shape[1:]) != (s["ldout"],) + tuple(s["out_chw"][1:]):
            d = buf[s["dst"]] = torch.zeros(n, s["ldout"], *s["out_chw"][1:], dtype=a.dtype)
        d[:, s["coffout"]:s["coffout"] + s["out_chw"][0]] = out
        if keep:
            rec.append((src.clone(), out.clone()))
    last = buf[STEPS[-1]["dst"]]
    return last.mean(dim=(2, 3)), rec


def worst_ratio(got, ref, tol):
    """(largest error / tol, its index): 0 where the error is 0 (also at tol = 0), inf where tol = 0 is missed or got is not finite."""
    err = (got.double() - ref).abs()
    r = torch.where(err == 0, torch.zeros_like(err), err / tol)
    r = torch.where(torch.isfinite(got.double()) & ~torch.isnan(r), r, torch.full_like(r, float("inf")))
    j = int(r.argmax())
    return float(r.reshape(-1)[j]), tuple(int(v) for v in np.unravel_index(j, r.shape))
