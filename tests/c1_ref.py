"""fp64 references of the single-channel layer operations (csrc/c1.hip), the magnitudes their error bounds need, the bounds, the
inputs of tests/test_c1_gpu.py and a numpy emulation of each kernel's rounding points (tests/test_c1_ref_cpu.py keeps all of
this honest without a GPU). Plain torch / numpy on the CPU, written from the definitions in the kernel comments:

  gather   out[n,y,x,ch] = act(bias[ch] + sum_tap img[n, 2y-1+ky, 2x-1+kx] * in_scale * w[ch][ky*4+kx])
  scatter  img[n,Y,X]    = post(bias + sum_{ch,tap} relu?(X[n,y,x,ch]) * w[ch][tap]) * out_scale,  Y = 2y-1+ky, X = 2x-1+kx
  wgrad    dW[ch][tap]  += scale * sum_{n,y,x} relu?(X[n,y,x,ch]) * img[n, 2y-1+ky, 2x-1+kx] * img_scale
  reduce   dW[i]        += sum_b part[b][i]
  head4    the scatter with 4 output channels (w [c][tap][o], tanh) and its input gradient

Zero padding outside the image. Features are NHWC here as in the kernels. Every reference returns, next to the value, A = the
sum of the absolute values of the terms of each output element (what a rounding error of a sum is relative to)."""
import numpy as np
import torch
import torch.nn.functional as F

U16 = 2.0 ** -11      # unit roundoff of fp16
U32 = 2.0 ** -24      # ... of fp32
TANH_ALLOWANCE = 2.0 ** -22   # tanhf against fp64 tanh: 4 ulp of a value below 1.0
SLOPE = float(np.float32(0.2))    # the kernels' LeakyReLU slope is the fp32 constant 0.2f
ACT_NONE, ACT_RELU, ACT_LRELU = 0, 1, 2    # GI_ACT_*

_D = torch.float64
SEED = 20     # of the rounding tests' inputs


def _act(v, act):
    if act == ACT_RELU:
        return v.clamp(min=0)
    if act == ACT_LRELU:
        return torch.where(v > 0, v, SLOPE * v)
    return v


def _wk(w):
    """[c][16] -> conv weight (c, 1, 4, 4)"""
    return w.to(_D).reshape(-1, 1, 4, 4)


def gather_ref(img, w, bias=None, act=ACT_NONE, in_scale=1.0):
    """img (n, 2Hs, 2Ws), w (c, 16), bias (c) or None -> value, A, both (n, Hs, Ws, c) fp64"""
    x = (img.to(_D) * in_scale)[:, None]
    b = None if bias is None else bias.to(_D)
    v = F.conv2d(x, _wk(w), b, stride=2, padding=1)
    a = F.conv2d(x.abs(), _wk(w).abs(), None if b is None else b.abs(), stride=2, padding=1)
    return _act(v, act).permute(0, 2, 3, 1).contiguous(), a.permute(0, 2, 3, 1).contiguous()


def affine_x(X, aff):
    """The affine form's input: channels [c/2, c) of X replaced by relu(fma(x2, scale2, shift2)) rounded to fp16.
    aff = (x2 (n, Hs, Ws, c/2), scale2 (c/2), shift2 (c/2)) or None. The fma is evaluated in fp64 and rounded once to fp32."""
    X = X.to(_D)
    if aff is None:
        return X
    x2, sc, sh = aff
    t = (x2.to(_D) * sc.to(_D) + sh.to(_D)).to(torch.float32).clamp(min=0).to(torch.float16).to(_D)
    return torch.cat([X[..., : X.shape[-1] // 2], t], dim=-1)


_OA = torch.eye(16, dtype=_D).reshape(16, 1, 4, 4)     # overlap-add of the 16 taps as a transposed convolution


def overlap_add(col):
    """col (n, Hs, Ws, 16) -> (n, 2Hs, 2Ws): out[2y-1+ky, 2x-1+kx] += col[y, x, ky*4+kx]"""
    return F.conv_transpose2d(col.permute(0, 3, 1, 2), _OA, stride=2, padding=1)[:, 0]


def scatter_ref(X, w, bias=None, relu_in=0, post=0, out_scale=1.0, aff=None):
    """X (n, Hs, Ws, c), w (c, 16), bias (1) or None -> dict: value (n, 2Hs, 2Ws) fp64, pre (before post and out_scale), A,
    col (n, Hs, Ws, 16) fp64 and S4 = the overlap-add of |col| (the at most 4 col values an output element sums)"""
    x = affine_x(X, aff)
    if relu_in:
        x = x.clamp(min=0)
    wd = w.to(_D)
    col = x @ wd
    b = 0.0 if bias is None else float(bias.to(_D).reshape(-1)[0])
    pre = overlap_add(col) + b
    A = overlap_add(x.abs() @ wd.abs()) + abs(b)
    v = torch.tanh(pre) if post == 1 else pre
    return dict(value=v * out_scale, pre=pre, A=A, col=col, S4=overlap_add(col.abs()))


def patches(img):
    """img (n, 2Hs, 2Ws) -> (n, Hs, Ws, 16): the 16 taps under every small-grid pixel, zero padded"""
    n, H, W = img.shape
    p = F.unfold(img.to(_D)[:, None], 4, padding=1, stride=2)      # (n, 16, Hs*Ws)
    return p.reshape(n, 16, H // 2, W // 2).permute(0, 2, 3, 1).contiguous()


def wgrad_ref(X, img, relu_in=0, scale=1.0, img_scale=1.0, aff=None):
    """-> value, A, both (c, 16) fp64: what the call adds onto dW"""
    x = affine_x(X, aff)
    if relu_in:
        x = x.clamp(min=0)
    p = patches(img) * img_scale
    c = x.shape[-1]
    v = x.reshape(-1, c).t() @ p.reshape(-1, 16)
    a = x.abs().reshape(-1, c).t() @ p.abs().reshape(-1, 16)
    return v * scale, a * abs(scale)


def reduce_ref(part, dW0):
    """part (blocks, count), dW0 (count) -> value, A = sum |part| (count): rows added in order in fp64"""
    s = torch.zeros(part.shape[1], dtype=_D)
    for b in range(part.shape[0]):
        s = s + part[b].to(_D)
    return dW0.to(_D) + s, part.to(_D).abs().sum(0)


def head4_forward_ref(X, w4, bias=None, relu_in=0):
    """X (n, Hs, Ws, c), w4 (c, 16, 4) -> dict per scatter_ref with a channel axis: value (n, 4, 2Hs, 2Ws) = tanh(pre)"""
    outs = [scatter_ref(X, w4[:, :, o], None if bias is None else bias[o:o + 1], relu_in, 1, 1.0) for o in range(4)]
    return {k: torch.stack([r[k] for r in outs], 1) for k in ("value", "pre", "A", "S4")}


def head4_dgrad_ref(g, w4):
    """g (n, 4, 2Hs, 2Ws), w4 (c, 16, 4) -> value, A (n, Hs, Ws, c): out[p][ch] = sum_{o,tap} g[o][tap of p] * w4[ch][tap][o]"""
    v = a = 0.0
    for o in range(4):
        vo, ao = gather_ref(g[:, o], w4[:, :, o])
        v, a = v + vo, a + ao
    return v, a


# ---- the bounds (derived, not tuned; DESIGN.md "parity of the single-channel kernels") -----------------------------------------
def bound_fp32(K, A):
    """a sum of K terms accumulated in fp32 in any order"""
    return K * U32 * A


def bound_gather(fp16, ref, A, K=16):
    """fp16: inputs exact in fp16, fp32 accumulation, one rounding of the output"""
    return U16 * ref.abs() + K * U32 * A if fp16 else K * U32 * A


def bound_scatter(kind, r, c, post, out_scale):
    """kind 'col': col stored in fp16, overlap-add and output in fp32; 'fp32': the scalar kernel of either type. tanh is
    1-Lipschitz: the pre-activation bound plus the allowance for tanhf itself."""
    b = U16 * r["S4"] + (c + 4) * U32 * r["A"] if kind == "col" else 4 * c * U32 * r["A"]
    if post == 1:
        b = b + TANH_ALLOWANCE
    return b * abs(out_scale)


def worst_ratio(err, bound):
    """max err / bound over every element; an element with bound 0 must have err 0"""
    err, bound = err.double().abs(), bound.double()
    assert bool(((bound > 0) | (err == 0)).all()), "error where the bound is zero"
    return float((err / bound.clamp(min=1e-300)).max())


# ---- inputs ---------------------------------------------------------------------------------------------------------------------
def _gen(seed):
    return torch.Generator().manual_seed(seed)


def ints(shape, seed, r=2):
    """asymmetric small integers in [-r, r] (fp32)"""
    return torch.randint(-r, r + 1, shape, generator=_gen(seed)).float()


def uni(shape, seed, lo=-1.0, hi=1.0, fp16=True):
    """uniform in [lo, hi), rounded to fp16 when the kernel under test computes in it (gpu_util.quant)"""
    t = torch.rand(shape, generator=_gen(seed)) * (hi - lo) + lo
    return t.half().float() if fp16 else t


def pow2(shape, seed, exps=(-1, 0, 1), signed=True):
    g = _gen(seed)
    e = torch.tensor(exps, dtype=torch.float32)[torch.randint(0, len(exps), shape, generator=g)]
    s = (torch.randint(0, 2, shape, generator=g) * 2 - 1).float() if signed else 1.0
    return s * torch.exp2(e)


def gather_inputs(exact, fp16, n, Hs, Ws, c, bias, seed):
    """-> img (n, 2Hs, 2Ws), w (c, 16), bias (c) or None"""
    if exact:
        return ints((n, 2 * Hs, 2 * Ws), seed), ints((c, 16), seed + 1), (ints((c,), seed + 2) if bias else None)
    return (uni((n, 2 * Hs, 2 * Ws), seed, fp16=fp16), uni((c, 16), seed + 1, fp16=fp16), (uni((c,), seed + 2, fp16=fp16) if bias else None))


def scatter_inputs(exact, fp16, n, Hs, Ws, c, bias, seed, affine=False):
    """-> X (n, Hs, Ws, c), w (c, 16), bias (1) or None, aff or None. Exact: integers; the affine half is integers too (scale2 in
    {+-1, +-2}, shift2 in [-1, 1]), so fused and unfused multiply-adds agree and |col| <= 64*2*2 + 64*5*2 = 896 at c = 128.
    Rounding: X uniform in [-0.25, 1) (relu_in still has something to do), w in [0, 1/c) (pre-activations around 1: inside
    tanh's interesting range): most terms have one sign, the hardest case for a sum in a fixed precision (the error of zero-mean
    terms falls with the square root of their number and would leave the bound untested)."""
    if exact:
        X, w, b = ints((n, Hs, Ws, c), seed), ints((c, 16), seed + 1), (ints((1,), seed + 2) if bias else None)
        aff = (ints((n, Hs, Ws, c // 2), seed + 3), pow2((c // 2,), seed + 4, (0, 1)), ints((c // 2,), seed + 5, 1)) if affine else None
    else:
        X, w, b = uni((n, Hs, Ws, c), seed, -0.25, 1.0, fp16), uni((c, 16), seed + 1, 0.0, 1.0 / c, fp16), (uni((1,), seed + 2, fp16=False) if bias else None)
        aff = (uni((n, Hs, Ws, c // 2), seed + 3), uni((c // 2,), seed + 4, 0.5, 1.5, False), uni((c // 2,), seed + 5, -0.25, 0.25, False)) if affine else None
    return X, w, b, aff


def wgrad_inputs(exact, fp16, n, Hs, Ws, c, seed, affine=False, r=2):
    """-> X (n, Hs, Ws, c), img (n, 2Hs, 2Ws), aff or None; rounding: one-signed terms as in scatter_inputs (X in [-0.25, 1) so
    that relu_in still has something to do)"""
    if exact:
        X, img = ints((n, Hs, Ws, c), seed, r), ints((n, 2 * Hs, 2 * Ws), seed + 1, r)
        aff = (ints((n, Hs, Ws, c // 2), seed + 3), pow2((c // 2,), seed + 4, (0, 1)), ints((c // 2,), seed + 5, 1)) if affine else None
    else:
        X, img = uni((n, Hs, Ws, c), seed, -0.25, 1.0, fp16), uni((n, 2 * Hs, 2 * Ws), seed + 1, 0.0, 1.0, fp16)
        aff = (uni((n, Hs, Ws, c // 2), seed + 3), uni((c // 2,), seed + 4, 0.5, 1.5, False), uni((c // 2,), seed + 5, -0.25, 0.25, False)) if affine else None
    return X, img, aff


def reduce_inputs(exact, count, blocks, seed):
    """-> part (blocks, count), dW0 (count)"""
    if exact:
        return ints((blocks, count), seed, 8), ints((count,), seed + 1, 8)
    # rows of different magnitude, as the partial sums of workgroups with different shares of the image are
    return uni((blocks, count), seed, 0.0, 1.0, False) * pow2((blocks, 1), seed + 2, (-8, -6, -4, -2, 0), False), torch.zeros(count)


def head4_inputs(exact, n, Hs, Ws, seed, c=128):
    """-> X (n, Hs, Ws, c), w4 (c, 16, 4), bias (4), g (n, 4, 2Hs, 2Ws). Exact: integers times a power of two, so that the
    pre-activations stay exact and inside tanh's interesting range."""
    if exact:
        return ints((n, Hs, Ws, c), seed) / 8, ints((c, 16, 4), seed + 1) / 16, ints((4,), seed + 2) / 4, ints((n, 4, 2 * Hs, 2 * Ws), seed + 3)
    return uni((n, Hs, Ws, c), seed), uni((c, 16, 4), seed + 1, -0.125, 0.125), uni((4,), seed + 2, fp16=False), uni((n, 4, 2 * Hs, 2 * Ws), seed + 3)


# ---- the cases of the rounding tests: (id, arguments). tests/test_c1_gpu.py runs them on the device, tests/test_c1_ref_cpu.py
# puts the emulation below through the same inputs and bounds -----------------------------------------------------------------------
# gather: (fp16, n, Hs, Ws, c, bias, act, in_scale, kernel)
GATHER_ROUNDING = [
    ("mfma64-1group", (True, 2, 3, 16, 64, False, ACT_LRELU, 1.0, "c1_gather_mfma<4>")),
    ("mfma128-gpr3", (True, 3, 5, 48, 128, False, ACT_RELU, 0.5, "c1_gather_mfma<8>")),
    ("mfma64-gpr3", (True, 3, 5, 48, 64, False, ACT_NONE, 1.0, "c1_gather_mfma<4>")),
    ("strip32-f32-64", (False, 2, 3, 32, 64, False, ACT_LRELU, 1.0, "c1_gather_strip")),
    ("strip96-f32-64-bias", (False, 1, 3, 96, 64, True, ACT_NONE, 0.5, "c1_gather_strip")),
    ("strip-f16-64-bias", (True, 2, 3, 32, 64, True, ACT_LRELU, 1.0, "c1_gather_strip")),
    ("strip-f16-32", (True, 2, 3, 64, 32, False, ACT_RELU, 1.0, "c1_gather_strip")),
    ("strip-f16-256", (True, 2, 3, 16, 256, False, ACT_NONE, 1.0, "c1_gather_strip")),
    ("generic24-f32", (False, 2, 3, 24, 64, True, ACT_LRELU, 1.0, "c1_gather")),
    ("generic20-f32", (False, 2, 5, 20, 128, False, ACT_NONE, 0.5, "c1_gather")),
    ("generic24-f16", (True, 2, 3, 24, 64, False, ACT_RELU, 1.0, "c1_gather")),
    ("generic20-f16-bias", (True, 2, 5, 20, 128, True, ACT_LRELU, 1.0, "c1_gather")),
    ("generic1x1-f16", (True, 3, 1, 1, 64, True, ACT_NONE, 1.0, "c1_gather")),
    ("generic1x1-f32", (False, 3, 1, 1, 64, False, ACT_NONE, 1.0, "c1_gather")),
]
# scatter: (fp16, n, Hs, Ws, c, bias, relu_in, post, out_scale, affine, col_scratch, fused option, kind of bound, kernel)
SCATTER_ROUNDING = [
    ("fused2-1row", (True, 2, 1, 16, 64, True, 0, 0, 1.0, False, True, 1, "col", "c1_scatter_fused<2>")),
    ("fused4-2bands", (True, 2, 24, 64, 128, False, 1, 1, 1.0, False, True, 1, "col", "c1_scatter_fused<4>")),
    ("fused2-3bands", (True, 1, 10, 256, 64, True, 0, 0, 1.0 / 1024, False, True, 1, "col", "c1_scatter_fused<2>")),
    ("fused4-th21", (True, 3, 7, 48, 128, True, 1, 0, 1.0, False, True, 1, "col", "c1_scatter_fused<4>")),
    ("fused2-affine", (True, 2, 3, 32, 64, True, 0, 1, 1.0, True, True, 1, "col", "c1_scatter_fused<2>")),
    ("fused4-affine", (True, 1, 5, 64, 128, False, 0, 0, 1.0, True, True, 1, "col", "c1_scatter_fused<4>")),
    ("col2-ws24", (True, 1, 5, 24, 64, True, 1, 0, 1.0, False, True, 1, "col", "c1_col+col2im<2>")),
    ("col4-ws24", (True, 3, 3, 24, 128, False, 0, 1, 1.0, False, True, 1, "col", "c1_col+col2im<4>")),
    ("col2-ws512", (True, 1, 2, 512, 64, True, 0, 0, 1.0, False, True, 1, "col", "c1_col+col2im<2>")),
    ("col4-unfused-affine", (True, 2, 3, 32, 128, True, 0, 0, 1.0, True, True, 0, "col", "c1_col+col2im<4>")),
    ("scalar-f32-16", (False, 2, 9, 13, 16, True, 1, 0, 1.0, False, False, 1, "fp32", "c1_scatter")),
    ("scalar-f32-16-tanh", (False, 2, 19, 27, 16, False, 0, 1, 0.5, False, False, 1, "fp32", "c1_scatter")),
    ("scalar-f16-32", (True, 3, 19, 27, 32, True, 0, 0, 1.0, False, False, 1, "fp32", "c1_scatter")),
]
# wgrad: (fp16, n, Hs, Ws, c, relu_in, scale, img_scale, affine, scratch, kernel)
WGRAD_ROUNDING = [
    ("mfma64-1tile", (True, 1, 1, 32, 64, 0, 1.0, 1.0, False, True, "c1_wgrad_mfma")),
    ("mfma128-1tile-atomics", (True, 1, 1, 32, 128, 1, 0.25, 0.5, False, False, "c1_wgrad_mfma,atomics")),
    ("mfma128-rows", (True, 1, 3, 32, 128, 1, 1.0, 1.0, False, True, "c1_wgrad_mfma")),
    ("mfma64-affine", (True, 1, 2, 32, 64, 0, 1.0, 1.0, True, True, "c1_wgrad_mfma")),
    ("scalar-f16-ws24", (True, 1, 3, 24, 64, 1, 1.0, 1.0, False, True, "c1_wgrad")),
    ("scalar-f32-ws24-atomics", (False, 1, 3, 24, 64, 0, 0.25, 0.5, False, False, "c1_wgrad,atomics")),
    ("scalar-f32-1x1", (False, 3, 1, 1, 16, 0, 1.0, 1.0, False, True, "c1_wgrad")),
]
# reduce: (count, blocks, scratch)
REDUCE_ROUNDING = [(f"{c}x{b}{'+scratch' if s else ''}", (c, b, s)) for c, b, s in
                   [(1024, 15, False), (2048, 16, True), (20, 17, False), (20, 15, True), (1024, 17, True), (2048, 256, True)]]
# head4: (n, Hs, Ws)
HEAD4_MAPS = [("2x4x16", (2, 4, 16)), ("1x9x48", (1, 9, 48))]


# ---- numpy emulation of the kernels' rounding points ------------------------------------------------------------------------------
def _f32(a):
    return np.asarray(a, dtype=np.float64).astype(np.float32)


def seq_sum32(terms, order, start=None):
    """fp32 accumulation of terms[..., K] (fp64, each product exact there) along the last axis in the given order: every step
    rounds the exact sum of the accumulator and one term to fp32 (an fma)"""
    acc = np.zeros(terms.shape[:-1], np.float32) if start is None else _f32(start)
    for k in order:
        acc = (acc.astype(np.float64) + terms[..., k]).astype(np.float32)
    return acc


def _np_act(v, act):
    if act == ACT_RELU:
        return np.maximum(v, np.float32(0))
    if act == ACT_LRELU:
        return np.where(v > 0, v, (v.astype(np.float64) * SLOPE).astype(np.float32))
    return v


def emulate_gather(fp16, img, w, bias, act, in_scale, seed=0):
    p = patches(img).numpy() * in_scale                          # (n, Hs, Ws, 16)
    terms = p[..., None, :] * w.double().numpy()                 # (n, Hs, Ws, c, 16)
    start = None if bias is None else np.broadcast_to(bias.numpy(), terms.shape[:-1])
    v = _np_act(seq_sum32(terms, np.random.default_rng(seed).permutation(16), start), act)
    return torch.from_numpy(v.astype(np.float16).astype(np.float64) if fp16 else v.astype(np.float64))


def _np_overlap_add32(col, order):
    n, Hs, Ws, _ = col.shape
    out = np.zeros((n, 2 * Hs + 2, 2 * Ws + 2), np.float32)       # one pixel of padding on every side, cut off below
    for t in order:
        ky, kx = divmod(int(t), 4)
        view = out[:, ky:ky + 2 * Hs:2, kx:kx + 2 * Ws:2]
        view[...] = (view.astype(np.float64) + col[..., t]).astype(np.float32)
    return out[:, 1:-1, 1:-1]


def emulate_scatter(kind, X, w, bias, relu_in, post, out_scale, aff, seed=0):
    """kind 'col': the channel sums in fp32, stored in fp16, then the overlap-add in fp32; 'fp32': every output element one
    chain of multiply-adds over its (tap, channel) terms; both: bias, tanh (correctly rounded), out_scale in fp32"""
    rng = np.random.default_rng(seed)
    x = affine_x(X, aff)
    x = (x.clamp(min=0) if relu_in else x).numpy()
    wn = w.double().numpy()
    n, Hs, Ws, c = x.shape
    if kind == "col":
        col = np.zeros((n, Hs, Ws, 16), np.float32)
        for ch in rng.permutation(c):
            col = (col.astype(np.float64) + x[..., ch, None] * wn[ch]).astype(np.float32)
        o = _np_overlap_add32(col.astype(np.float16).astype(np.float64), rng.permutation(16))
    else:
        pad = np.zeros((n, 2 * Hs + 2, 2 * Ws + 2), np.float32)
        for k in rng.permutation(16 * c):
            (ky, kx), ch = divmod(int(k) % 16, 4), int(k) // 16
            view = pad[:, ky:ky + 2 * Hs:2, kx:kx + 2 * Ws:2]
            view[...] = (view.astype(np.float64) + x[..., ch] * wn[ch, ky * 4 + kx]).astype(np.float32)
        o = pad[:, 1:-1, 1:-1]
    if bias is not None:
        o = (o.astype(np.float64) + float(bias.reshape(-1)[0])).astype(np.float32)
    if post == 1:
        o = np.tanh(o.astype(np.float64)).astype(np.float32)
    return torch.from_numpy((o.astype(np.float64) * out_scale).astype(np.float32).astype(np.float64))


def emulate_wgrad(X, img, relu_in, scale, img_scale, aff, seed=0):
    x = affine_x(X, aff)
    x = (x.clamp(min=0) if relu_in else x).numpy().reshape(-1, X.shape[-1])
    p = (patches(img).numpy() * img_scale).reshape(-1, 16)
    acc = np.zeros((x.shape[1], 16), np.float32)
    for i in np.random.default_rng(seed).permutation(x.shape[0]):
        acc = (acc.astype(np.float64) + x[i][:, None] * p[i][None, :]).astype(np.float32)
    return torch.from_numpy((acc.astype(np.float64) * scale).astype(np.float32).astype(np.float64))


def emulate_reduce(part, dW0, seed=0):
    acc = np.zeros(part.shape[1], np.float32)
    pn = part.numpy().astype(np.float32)
    for b in np.random.default_rng(seed).permutation(part.shape[0]):
        acc = acc + pn[b]
    return torch.from_numpy((dW0.numpy().astype(np.float32) + acc).astype(np.float64))


def emulate_head4_dgrad(g, w4, seed=0):
    n, _, H, W = g.shape
    p = np.stack([patches(g[:, o]).numpy() for o in range(4)], -1)         # (n, Hs, Ws, 16, 4)
    terms = p[..., None, :, :] * w4.double().numpy()                     # (n, Hs, Ws, c, 16, 4)
    terms = terms.reshape(terms.shape[:-2] + (64,))
    return torch.from_numpy(seq_sum32(terms, np.random.default_rng(seed).permutation(64)).astype(np.float16).astype(np.float64))
