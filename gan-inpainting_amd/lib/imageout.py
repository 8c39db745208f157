"""Image output on the device (csrc/imageout.hip): fp32 tensors back to 8-bit pictures, sample panels, and the
byte-level steps of pasting a repaired window into a photograph of any size. Thin wrappers: torch tensors are containers, every
operation is one library entry, and each is exact (tests/imageout_ref.py restates them in numpy). Not in the reference, whose only
pictures are the matplotlib panels of evaluate.py."""
import ctypes as C
import os

import torch

from .. import backend as B

MAX_PANEL_COLS = 8
MAX_FEATHER = 63


def _need(t, dtype, what):
    if not torch.is_tensor(t) or t.dtype != dtype or not t.is_cuda:
        raise B.BackendError(f"{what} takes {str(dtype).replace('torch.', '')} tensors on the gfx950 device")
    return t.contiguous()


def quantize(x):
    """fp32 tensor of any shape -> uint8 of the same shape: rint(clamp(x, 0, 1) * 255), NaN -> 0. Round to nearest even: every
    byte v comes back from v / 255 (lib.fid.fid_score.quantize8 keeps the reference's truncation for the FID path)."""
    x = _need(x, torch.float32, "imageout.quantize")
    out = torch.empty(x.shape, dtype=torch.uint8, device=x.device)
    if x.numel():
        B.check(B.lib().gi_image_quantize(B.get_ctx(x.device), B.ptr(x), x.numel(), B.ptr(out)))
    return out


def panel_shape(ncol, n, H, W, gutter):
    return n * (H + gutter) + gutter, ncol * (W + gutter) + gutter


def assemble_panel(cols, gutter=2):
    """cols: 1 .. 8 fp32 batches (n,1,H,W) of one shape -> the (n*(H+g)+g, ncol*(W+g)+g) uint8 canvas: row i shows sample i of
    every column, quantised as `quantize` does, between white gutters."""
    cols = [_need(c, torch.float32, "imageout.assemble_panel") for c in cols]
    if not 1 <= len(cols) <= MAX_PANEL_COLS:
        raise ValueError(f"a panel has 1 .. {MAX_PANEL_COLS} columns, got {len(cols)}")
    shape = cols[0].shape
    if len(shape) != 4 or shape[1] != 1 or any(c.shape != shape or c.device != cols[0].device for c in cols):
        raise ValueError("panel columns are (n,1,H,W) batches of one shape on one device")
    n, _, H, W = shape
    canvas = torch.empty(panel_shape(len(cols), n, H, W, int(gutter)), dtype=torch.uint8, device=cols[0].device)
    ptrs = (C.c_void_p * len(cols))(*[c.data_ptr() for c in cols])
    B.check(B.lib().gi_panel_assemble(B.get_ctx(canvas.device), C.cast(ptrs, C.c_void_p), len(cols), n, H, W, int(gutter), B.ptr(canvas)))
    return canvas


def mask_bbox(masks):
    """(n,H,W) or (H,W) uint8 -> (n,4) int32 on the device: (y0, x0, y1, x1) inclusive of the bytes != 0; (H, W, -1, -1) when empty."""
    masks = _need(masks, torch.uint8, "imageout.mask_bbox")
    if masks.dim() == 2:
        masks = masks[None]
    n, H, W = masks.shape
    out = torch.empty((n, 4), dtype=torch.int32, device=masks.device)
    B.check(B.lib().gi_mask_bbox(B.get_ctx(masks.device), B.ptr(masks), n, H, W, B.ptr(out)))
    return out


MAX_COMPONENT_CAP = 65536


def mask_components(mask, connectivity=8, cap=256):
    """(H,W) uint8 mask -> (labels, count, table): labels (H,W) int32 on the device, -1 on background and on a hole pixel (byte
    != 0) the smallest linear index of its 4- or 8-connected component; count, the number of components, a host int (the one
    device -> host copy); table (min(count, cap), 6) int32 on the device, a row (label, y0, x0, y1, x1, area) per component in
    label order, the box inclusive (csrc/components.hip)."""
    mask = _need(mask, torch.uint8, "imageout.mask_components")
    if mask.dim() != 2:
        raise ValueError(f"mask_components takes one (H,W) mask, got {tuple(mask.shape)}")
    H, W = mask.shape
    cap = int(cap)
    lib, dev = B.lib(), mask.device
    labels = torch.empty((H, W), dtype=torch.int32, device=dev)
    count = torch.empty(1, dtype=torch.int32, device=dev)
    table = torch.empty((max(cap, 0), 6), dtype=torch.int32, device=dev)
    ws = torch.empty(max(int(lib.gi_mask_components_workspace_bytes(H, W, cap)), 4), dtype=torch.uint8, device=dev)
    B.check(lib.gi_mask_components(B.get_ctx(dev), B.ptr(mask), H, W, int(connectivity), cap, B.ptr(labels), B.ptr(count), B.ptr(table), B.ptr(ws)))
    n = int(count.item())
    return labels, n, table[:min(n, cap)]


def window_crop(src, window, binarize=False, out=None):
    """The (wy, wx, wh, ww) window of a (H,W) uint8 image as a dense (wh, ww) tensor; binarize: nonzero -> 255."""
    src = _need(src, torch.uint8, "imageout.window_crop")
    H, W = src.shape
    wy, wx, wh, ww = (int(v) for v in window)
    if out is None:
        out = torch.empty((max(wh, 0), max(ww, 0)), dtype=torch.uint8, device=src.device)
    B.check(B.lib().gi_window_crop(B.get_ctx(src.device), B.ptr(src), H, W, wy, wx, wh, ww, 1 if binarize else 0, B.ptr(out)))
    return out


def feather_paste(orig, mask, window, patch, r, out=None):
    """A copy of `orig` (H,W) whose window holds the blend of `patch` (wh,ww) and `orig`: all patch on hole pixels (mask != 0), the
    weight 2a / (2r+1)^2 elsewhere, a = the hole pixels in the (2r+1)^2 box inside the window (include/ganinpaint.h). out: a
    (H,W) uint8 tensor that takes the window's bytes instead of a fresh copy (several disjoint windows of one picture paste into
    one copy of it; the entry still reads `orig`)."""
    orig = _need(orig, torch.uint8, "imageout.feather_paste")
    mask = _need(mask, torch.uint8, "imageout.feather_paste")
    patch = _need(patch, torch.uint8, "imageout.feather_paste")
    H, W = orig.shape
    wy, wx, wh, ww = (int(v) for v in window)
    if mask.shape != orig.shape or tuple(patch.shape) != (wh, ww):
        raise ValueError(f"feather_paste: mask {tuple(mask.shape)} / patch {tuple(patch.shape)} do not fit image {(H, W)}, window {(wh, ww)}")
    if out is None:
        dst = orig.clone()
    else:
        dst = out
        if not torch.is_tensor(dst) or dst.dtype != torch.uint8 or dst.device != orig.device or dst.shape != orig.shape or not dst.is_contiguous():
            raise ValueError("feather_paste: out is a contiguous uint8 tensor of the image's shape on its device")
    B.check(B.lib().gi_feather_paste(B.get_ctx(orig.device), B.ptr(orig), B.ptr(mask), H, W, wy, wx, wh, ww, B.ptr(patch), int(r), B.ptr(dst)))
    return dst


def write_png(path, image_u8):
    """A (H,W) uint8 tensor or array as a greyscale 8-bit PNG."""
    from PIL import Image
    a = image_u8.cpu().numpy() if torch.is_tensor(image_u8) else image_u8
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    Image.fromarray(a, mode="L").save(path, format="PNG")
