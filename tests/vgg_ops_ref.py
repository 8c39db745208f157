"""fp64 restatements of the VGG-19 loss path's kernels (csrc/vgg.hip, csrc/vggtrunk.hip and the 3x3 mode of the implicit GEMMs), one op each, on exactly
the operands the kernel sees: fp16-quantised maps (NHWC), fp32 master weights rounded as the pack kernels round them. Plain torch on
the CPU; tests/test_vgg_ops_ref_cpu.py proves every one against torch's own operators, autograd and the pinned loss functions of
oracle.torch_ref, tests/test_vgg_ops_gpu.py holds the kernels to them through the gi_debug_vgg_* entries."""
import math

import torch
import torch.nn.functional as F

F64 = torch.float64
SEED_EXP = -2            # kSeedExp (csrc/vggtrunk.hip)
SEED_SAMPLE_ALL = 8      # kSeedSampleAll: maps of more 256-pixel blocks are sampled by the maximum pass


# The convolution cases of tests/test_vgg_ops_gpu.py: (expected kernel, options, (n, Hs, Ws, cin, cout) of the GEMM, directions,
# extras). Direction "F": the forward of a VGG layer cin -> cout (bias + ReLU); "T": the input gradient of a layer cout -> cin
# (transposed weights). Only channel pairs VGG-19 has in that direction. Extras: "pool" - also with the pooled store offered;
# "mask" - also with mask + add and with mask alone. tests/test_vgg_ops_ref_cpu.py asks the plan function for every row.
I8, I5, I3 = {"GI_IGEMM8": 2}, {"GI_IGEMM8": 0}, {}
CONV_CASES = [
    ("igemm8<2>", I8, (2, 16, 64, 64, 128), "F", ("pool",)),
    ("igemm8<2>", I8, (2, 16, 64, 256, 256), "FT", ("pool", "mask")),
    ("igemm8<2,64>", I8, (2, 16, 64, 64, 64), "FT", ("pool", "mask")),
    ("igemm8<2,64>", I8, (2, 16, 64, 128, 64), "T", ("mask",)),
    ("igemm5<2,128>", I5, (2, 16, 64, 128, 128), "FT", ("pool", "mask")),
    ("igemm5<2,128>", I5, (2, 16, 16, 128, 256), "F", ()),
    ("igemm5<2,128>", I5, (1, 32, 8, 256, 256), "FT", ()),
    ("igemm5<2,64>", I5, (2, 16, 16, 128, 64), "T", ("mask",)),
    ("igemm3<2,128>", I3, (3, 12, 20, 256, 128), "T", ("mask",)),
    ("igemm3<2,128>", I3, (3, 3, 5, 512, 512), "FT", ()),
    ("igemm3<2,128>", I3, (2, 1, 1, 512, 512), "FT", ()),
    ("igemm3<2,128>", I3, (2, 8, 8, 256, 256), "FT", ()),
    ("igemm3<2,64>", I3, (3, 24, 40, 128, 64), "T", ()),
    ("igemm3<2,64>", I3, (3, 48, 80, 64, 64), "FT", ()),
]


def conv_variants():
    """every launch of the table: (kernel, opts, shape, direction, epilogue, pool_applied, mask_applied) with epilogue one of
    "plain", "pool", "mask+add", "mask". The forward takes the pooled store, the input gradient the mask."""
    out = []
    for kernel, opts, shape, dirs, extras in CONV_CASES:
        halo = not kernel.startswith("igemm3")
        for d in dirs:
            out.append((kernel, opts, shape, d, "plain", 0, 0))
            if "pool" in extras and d == "F":
                out.append((kernel, opts, shape, d, "pool", 1 if kernel.startswith("igemm8") else 0, 0))
            if "mask" in extras and d == "T":
                out.append((kernel, opts, shape, d, "mask+add", 0, 1 if halo else 0))
                out.append((kernel, opts, shape, d, "mask", 0, 1 if halo else 0))
    return out


def q16(t):
    """rounded to fp16, as fp64"""
    return t.to(torch.float16).to(F64)


def nchw(x):
    return x.permute(0, 3, 1, 2)


def nhwc(x):
    return x.permute(0, 2, 3, 1).contiguous()


# ---- 3x3 / s1 / p1 convolutions ----------------------------------------------------------------------------------------------
def conv3x3(x, w, bias=None, relu=False):
    """x (n,H,W,cin), w [cout][cin][3][3] (values already rounded to fp16) -> (n,H,W,cout)"""
    y = F.conv2d(nchw(x.to(F64)), w.to(F64), None if bias is None else bias.to(F64), padding=1)
    return nhwc(torch.relu(y) if relu else y)


def transposed_weights(w):
    """what pack3x3_t_kernel packs, as a weight tensor of an ordinary convolution: [cin][cout][3][3] with the taps reversed"""
    return w.transpose(0, 1).flip(2, 3).contiguous()


def conv3x3_input_grad(g, w):
    """g (n,H,W,cout) -> the gradient w.r.t. the input of conv3x3(., w): the convolution with the transposed weights"""
    return conv3x3(g, transposed_weights(w))


def mask_add(y, mask, add=None):
    """the mode-2 halo kernels' epilogue with slope 0: [mask > 0] * (y + add)"""
    y = y.to(F64) if add is None else y.to(F64) + add.to(F64)
    return torch.where(mask > 0, y, torch.zeros_like(y))


# ---- conv1_1 on the replicated grey image ------------------------------------------------------------------------------------
def w1_of(w):
    """sum_cin_kernel: [64][3][3][3] fp32 -> [64][9] fp32, the input channels added in ascending order in fp32"""
    w = w.float()
    s = torch.zeros(w.shape[0], 9, dtype=torch.float32)
    for c in range(w.shape[1]):
        s = s + w[:, c].reshape(w.shape[0], 9)
    return s


def conv1(xa, xb, w1, bias):
    """xa, xb (n,H,W) fp32, w1 [64][9] fp32 -> (relu(b + conv) as (2n,H,W,64), sum |w1 x| + |b| per element): image and weights
    rounded to fp16, as the matrix-core kernel rounds them"""
    x = q16(torch.cat([xa, xb]).float())[:, None]
    wq = q16(w1).reshape(64, 1, 3, 3)
    y = F.conv2d(x, wq, bias.to(F64), padding=1)
    mag = F.conv2d(x.abs(), wq.abs(), bias.to(F64).abs(), padding=1)
    return nhwc(torch.relu(y)), nhwc(mag)


def conv1_adjoint(D, w1, mul):
    """D (n,H,W,64) fp16 values, w1 [64][9] fp32 -> (dimg (n,H,W), sum |w1 D| per pixel):
    dimg[y][x] = mul * sum_{ky,kx,o} w1[o][ky][kx] * D[y+1-ky][x+1-kx][o]"""
    n, H, W, _ = D.shape
    Dp = F.pad(nchw(D.to(F64)), (1, 1, 1, 1))
    w = w1.to(F64).reshape(64, 3, 3)
    out = torch.zeros(n, H, W, dtype=F64)
    mag = torch.zeros(n, H, W, dtype=F64)
    for ky in range(3):
        for kx in range(3):
            sl = Dp[:, :, 2 - ky:2 - ky + H, 2 - kx:2 - kx + W]          # D[y + 1 - ky][x + 1 - kx], zero outside
            out += (sl * w[:, ky, kx][None, :, None, None]).sum(1)
            mag += (sl * w[:, ky, kx][None, :, None, None]).abs().sum(1)
    return out * mul, mag


# ---- pooling ---------------------------------------------------------------------------------------------------------------
def _windows(x):
    """(n,H,W,C) -> (n,H/2,W/2,4,C), the window positions in row-major order (0,0) (0,1) (1,0) (1,1)"""
    n, H, W, C = x.shape
    return x.reshape(n, H // 2, 2, W // 2, 2, C).permute(0, 1, 3, 2, 4, 5).reshape(n, H // 2, W // 2, 4, C)


def _unwindows(w):
    n, Ho, Wo, _, C = w.shape
    return w.reshape(n, Ho, Wo, 2, 2, C).permute(0, 1, 3, 2, 4, 5).reshape(n, 2 * Ho, 2 * Wo, C)


def maxpool2(x):
    return _windows(x).amax(3)


def pool_bwd(g, act, relu):
    """vggtrunk.hip's act_bwd_kernel<true> with no seed: g (n,H/2,W/2,C) goes to the FIRST maximum of every window of act, times [max > 0] when relu"""
    wa = _windows(act.to(F64))
    m = wa.amax(3, keepdim=True)
    first = (wa == m).to(torch.int8).argmax(3, keepdim=True)              # argmax of a 0/1 tensor: the first 1
    val = g.to(F64)[:, :, :, None]
    if relu:
        val = torch.where(m > 0, val, torch.zeros_like(val))
    out = torch.zeros_like(wa).scatter_(3, first, val)
    return _unwindows(out)


def act_bwd(g, act, seed, relu):
    """vggtrunk.hip's act_bwd_kernel<false>: [act > 0 or not relu] * fp16(fp32(g) + fp32(seed)); g / seed None: zeros"""
    z = torch.zeros(act.shape, dtype=torch.float32)
    s = ((z if g is None else g.float()) + (z if seed is None else seed.float())).to(torch.float16).to(F64)
    return torch.where(act > 0, s, torch.zeros_like(s)) if relu else s


# ---- Gram matrices and the two terms of a tap -----------------------------------------------------------------------------------
def gram(Fm):
    """Fm (m,HW,C) -> (m,C,C): F^T F / (HW C)"""
    Fm = Fm.to(F64)
    return torch.bmm(Fm.transpose(1, 2), Fm) / (Fm.shape[1] * Fm.shape[2])


def tap_terms(Fm, n):
    """Fm (2n,HW,C): output maps then target maps -> (perceptual term, style term, dG (n,C,C))"""
    Fo, Ft = Fm[:n].to(F64), Fm[n:].to(F64)
    dG = gram(Fo) - gram(Ft)
    return ((Fo - Ft) ** 2).mean(), (dG ** 2).mean(), dG


# ---- seeds -----------------------------------------------------------------------------------------------------------------
def seed_coefficients(n, HW, C, wp, ws):
    """vgg_seeds: the two coefficients as the host rounds them to fp32"""
    cp = torch.tensor(wp * 2.0 / (float(n) * C * HW), dtype=F64).float().item()
    cs = torch.tensor(ws * 4.0 / (float(n) * C * C * float(HW) * C), dtype=F64).float().item()
    return cp, cs


def seed(Fo, Ft, dG, dmax, n, wp, ws):
    """vgg_seed_kernel: Fo, Ft (n,HW,C) fp16 values, dG (n,C,C) fp32 values, dmax = fp32 max |dG| ->
    (seed (n,HW,C) = cs' sum_k dGq[c][k] Fo[p][k] + cp (Fo - Ft), cs' sum_k |dGq[c][k] Fo[p][k]|, cs'):
    dGq = fp16(dG 2^-ex) with dmax = m 2^ex, m in [0.5, 1); cs' = fp32(cs 2^ex)"""
    _, HW, C = Fo.shape
    cp, cs = seed_coefficients(n, HW, C, wp, ws)
    ex = math.frexp(float(dmax))[1] if dmax > 0 else 0
    dGq = q16(dG.to(F64) * 2.0 ** -ex)
    cs1 = torch.tensor(cs * 2.0 ** ex, dtype=F64).float().item()
    Fo, Ft = Fo.to(F64), Ft.to(F64)
    sty = torch.bmm(Fo, dGq.transpose(1, 2))
    mag = torch.bmm(Fo.abs(), dGq.abs().transpose(1, 2))
    return cs1 * sty + cp * (Fo - Ft), cs1 * mag, cs1


def sampled_blocks(nb):
    """the 256-pixel blocks the maximum pass reads: all up to SEED_SAMPLE_ALL, else block 8 j + (3 j mod 8), clamped to 8 j"""
    if nb <= SEED_SAMPLE_ALL:
        return list(range(nb))
    out = []
    for j in range((nb + 7) // 8):
        pb = 8 * j + (3 * j) % 8
        out.append(pb if pb < nb else 8 * j)
    return out


def sampled_mask(HW):
    """bool (HW,): the pixels of the sampled blocks"""
    m = torch.zeros(HW, dtype=torch.bool)
    for pb in sampled_blocks((HW + 255) // 256):
        m[pb * 256:(pb + 1) * 256] = True
    return m


def scale(am):
    """vggtrunk.hip's seed_scale_kernel with n = 1: s = 2^(SEED_EXP - e), max |seed| = m 2^e; zero, inf, NaN: 1; the exponent clamped to +-100"""
    if not (am > 0.0 and am < math.inf):
        return 1.0
    k = SEED_EXP - math.frexp(am)[1]
    return 2.0 ** max(-100, min(100, k))
