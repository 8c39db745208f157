"""TEST INFRASTRUCTURE: numpy restatement of the image-output entries (csrc/imageout.hip, include/ganinpaint.h) and of the chain
lib/inpaint.py runs around the generator. Written from the definitions, not from the kernels: the box count is a sum of shifted
copies, not a running sum; the bounding box comes from np.nonzero. The two resizes go through oracle.resize_ref."""
import math

import numpy as np

from oracle import resize_ref as rr


def quantize(x):
    """(uint8) rint(min(max(x, 0), 1) * 255) in fp32, NaN -> 0; np.rint rounds halves to even like rintf."""
    x = np.asarray(x, np.float32)
    with np.errstate(invalid="ignore"):
        c = np.where(x > 0, x, np.float32(0))          # NaN and -0 -> 0
        c = np.where(c < 1, c, np.float32(1))
    return np.rint(c.astype(np.float32) * np.float32(255.0)).astype(np.uint8)


def panel(cols, gutter):
    """cols: list of (n,1,H,W) fp32 -> (n*(H+g)+g, ncol*(W+g)+g) uint8, white gutters."""
    n, _, H, W = cols[0].shape
    g = gutter
    canvas = np.full((n * (H + g) + g, len(cols) * (W + g) + g), 255, np.uint8)
    for c, col in enumerate(cols):
        for i in range(n):
            y, x = g + i * (H + g), g + c * (W + g)
            canvas[y:y + H, x:x + W] = quantize(col[i, 0])
    return canvas


def bbox(mask):
    """(H,W) uint8 -> (y0, x0, y1, x1) inclusive of the nonzero bytes; (H, W, -1, -1) when there are none."""
    ys, xs = np.nonzero(mask)
    if ys.size == 0:
        return (mask.shape[0], mask.shape[1], -1, -1)
    return (int(ys.min()), int(xs.min()), int(ys.max()), int(xs.max()))


def crop(src, window, binarize=False):
    wy, wx, wh, ww = window
    out = src[wy:wy + wh, wx:wx + ww].copy()
    return np.where(out != 0, 255, 0).astype(np.uint8) if binarize else out


def box_count(hole, r):
    """a(p) = number of true pixels of `hole` in the (2r+1)^2 box around p; outside the array counts as 0."""
    h, w = hole.shape
    pad = np.zeros((h + 2 * r, w + 2 * r), np.int64)
    pad[r:r + h, r:r + w] = hole != 0
    a = np.zeros((h, w), np.int64)
    for dy in range(2 * r + 1):
        for dx in range(2 * r + 1):
            a += pad[dy:dy + h, dx:dx + w]
    return a


def feather_alpha(hole, r):
    """alpha in units of 1 / A, A = (2r+1)^2: A on the hole, else min(A, 2 a)."""
    A = (2 * r + 1) ** 2
    a = box_count(hole, r)
    return np.where(hole != 0, A, np.minimum(A, 2 * a)), A


def feather_paste(orig, mask, window, patch, r):
    """A copy of orig whose window is (alpha * patch + (A - alpha) * orig + A // 2) // A; the hole and its count are the window's."""
    wy, wx, wh, ww = window
    alpha, A = feather_alpha(mask[wy:wy + wh, wx:wx + ww], r)
    o = orig[wy:wy + wh, wx:wx + ww].astype(np.int64)
    out = orig.copy()
    out[wy:wy + wh, wx:wx + ww] = ((alpha * patch.astype(np.int64) + (A - alpha) * o + A // 2) // A).astype(np.uint8)
    return out


def plan_window(H, W, box, S, context, feather):
    y0, x0, y1, x1 = box
    m = max(y1 - y0 + 1, x1 - x0 + 1)
    side = max(S, math.ceil(context * m), m + 2 * (feather + 1))
    wh, ww = min(H, side), min(W, side)
    cy, cx = (y0 + y1 + 1) // 2, (x0 + x1 + 1) // 2
    return (min(max(cy - wh // 2, 0), H - wh), min(max(cx - ww // 2, 0), W - ww), wh, ww)


def model_input(img, mask, window, S):
    """The generator's input for one window: (masked, m) fp32 (S,S). ToTensor's / 255 on the resized bytes, ceil on the mask."""
    g = rr.resize_bilinear_u8(crop(img, window), S, S).astype(np.float32) / np.float32(255.0)
    m = np.ceil(rr.resize_bilinear_u8(crop(mask, window, binarize=True), S, S).astype(np.float32) / np.float32(255.0))
    return (g * (np.float32(1.0) - m)).astype(np.float32), m.astype(np.float32)


def enlarged_patch(masked, m, gen_out, window):
    """quantize(masked + gen_out * m) at S x S, resized to the window's size."""
    comp = (masked + gen_out.astype(np.float32) * m).astype(np.float32)
    return rr.resize_bilinear_u8(quantize(comp), window[2], window[3])


def inpaint_given_generator_output(img, mask, S, context, feather, gen_out):
    """The whole chain of lib.inpaint.Inpainter for one image around a SUPPLIED generator output gen_out (S,S) fp32 (what the
    generator returned for model_input(...)[0]). Returns (result, window)."""
    box = bbox(mask)
    if box[2] < 0:
        return img.copy(), None
    window = plan_window(img.shape[0], img.shape[1], box, S, context, feather)
    masked, m = model_input(img, mask, window, S)
    return feather_paste(img, mask, window, enlarged_patch(masked, m, gen_out, window), feather), window
