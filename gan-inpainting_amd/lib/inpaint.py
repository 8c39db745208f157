"""Inpaint a picture of any size with a trained generator (not in the reference, whose eval.py feeds whole images
through the network at their stored size).

One window per image: the hole's bounding box decides a square window around it (`plan_window`), the window is cropped, resized
to the model's S x S with the training pipeline's own resampler, repaired, resized back and blended into a copy of the picture
with a feathered weight (csrc/imageout.hip). Every step around the generator is exact integer or single-rounding arithmetic and
restated in tests/imageout_ref.py. A nonzero mask byte is a hole (minimaxgan_l1.py:113-122).

Opt-in (windows="per-hole"): the mask is split into its connected components on the device
(csrc/components.hip) and `plan_windows` puts one window around every group of holes; each window then takes the same steps."""
import math

import torch

from .. import backend as B
from . import imageout


def plan_window(H, W, bbox, S, context=2.0, feather=8):
    """The (wy, wx, wh, ww) window of a (H, W) image for a hole with the inclusive bounding box (y0, x0, y1, x1): a square of side
    max(S, ceil(context * m), m + 2 * (feather + 1)), m the box's longer side, clipped to the image and centred on the box as far
    as the image allows. It contains the box and leaves feather + 1 pixels around it on every side that is not the image's own edge,
    so the blend weight is zero on every interior window border. Pure host integers (context: a ratio of small integers in practice)."""
    y0, x0, y1, x1 = (int(v) for v in bbox)
    if not (0 <= y0 <= y1 < H and 0 <= x0 <= x1 < W):
        raise ValueError(f"plan_window: box {(y0, x0, y1, x1)} is empty or outside the {H} x {W} image")
    bh, bw = y1 - y0 + 1, x1 - x0 + 1
    m = max(bh, bw)
    side = max(int(S), math.ceil(context * m), m + 2 * (int(feather) + 1))
    wh, ww = min(H, side), min(W, side)
    cy, cx = (y0 + y1 + 1) // 2, (x0 + x1 + 1) // 2
    wy = min(max(cy - wh // 2, 0), H - wh)
    wx = min(max(cx - ww // 2, 0), W - ww)
    return wy, wx, wh, ww


def plan_windows(H, W, boxes, S, context=2.0, feather=8):
    """One window per group of holes. boxes: the components' inclusive (y0, x0, y1, x1) in label order. Every box
    starts as a group with `plan_window`'s window; while two windows share a pixel, the lexicographically first such pair (i, j),
    i < j, becomes one group: i's box grows to the union of both, j is deleted, i's window is planned again. Returns (windows,
    boxes) of the groups that remain: the windows are pairwise disjoint, so every hole pixel lies in exactly one of them and that one
    holds no other group's hole. Host integers; the pair test is one numpy comparison per merge."""
    import numpy as np
    boxes = [tuple(int(v) for v in b) for b in boxes]
    wins = [plan_window(H, W, b, S, context, feather) for b in boxes]
    while len(wins) > 1:
        w = np.asarray(wins, dtype=np.int64)
        y0, x0, y1, x1 = w[:, 0], w[:, 1], w[:, 0] + w[:, 2], w[:, 1] + w[:, 3]
        hit = (y0[:, None] < y1[None, :]) & (y0[None, :] < y1[:, None]) & (x0[:, None] < x1[None, :]) & (x0[None, :] < x1[:, None])
        hit = np.triu(hit, 1).ravel()
        first = int(hit.argmax())                 # row-major: the first pair in lexicographic order
        if not hit[first]:
            break
        i, j = divmod(first, len(wins))
        a, b = boxes[i], boxes[j]
        boxes[i] = (min(a[0], b[0]), min(a[1], b[1]), max(a[2], b[2]), max(a[3], b[3]))
        del boxes[j], wins[j]
        wins[i] = plan_window(H, W, boxes[i], S, context, feather)
    return wins, boxes


class _Resizer:
    """gi_resize_to_tensor for single (h, w) -> (oh, ow) uint8 images, the coefficient tables cached per geometry."""

    def __init__(self):
        self._tables = {}

    def __call__(self, src, oh, ow, out_f32=None, out_u8=None):
        h, w = src.shape
        lib, ctx = B.lib(), B.get_ctx(src.device)
        key = (h, w, oh, ow, src.device.index)
        if key not in self._tables:
            t = torch.empty(lib.gi_resize_table_bytes(h, w, oh, ow), dtype=torch.uint8, device=src.device)
            B.check(lib.gi_resize_build_tables(ctx, h, w, oh, ow, B.ptr(t)))
            self._tables[key] = t
        tmp = torch.empty((h, ow), dtype=torch.uint8, device=src.device)
        B.check(lib.gi_resize_to_tensor(ctx, B.ptr(self._tables[key]), B.ptr(src), 1, h, w, oh, ow, B.ptr(out_f32), B.ptr(out_u8), B.ptr(tmp)))


class Inpainter:
    """Inpainter(generator, imagedim=S)(images, masks): lists of (H_i, W_i) uint8 device tensors of any sizes -> the repaired uint8
    images. The generator is put in eval() (BatchNorm on running statistics, folded into the convolutions; no dropout) and sees
    up to `batch` windows per forward. An image with an empty mask comes back unchanged and costs no forward.

    windows="single" (the default): one window per image around the bounding box of all its holes. windows="per-hole": the mask is
    split into its 8-connected components on the device (imageout.mask_components) and `plan_windows` gives one window per group of
    holes, each repaired at its own scale and pasted into one copy of the picture; an image with more than `max_holes` components
    takes the single window."""

    def __init__(self, generator, imagedim=128, context=2.0, feather=8, batch=16, windows="single", max_holes=256):
        if not 0 <= int(feather) <= imageout.MAX_FEATHER:
            raise ValueError(f"feather = {feather} (0 .. {imageout.MAX_FEATHER})")
        if context < 1.0 or batch < 1 or imagedim < 1:
            raise ValueError("Inpainter: context >= 1, batch >= 1, imagedim >= 1")
        if windows not in ("single", "per-hole"):
            raise ValueError(f"Inpainter: windows = {windows!r} ('single' or 'per-hole')")
        if not 1 <= int(max_holes) <= imageout.MAX_COMPONENT_CAP:
            raise ValueError(f"Inpainter: max_holes = {max_holes} (1 .. {imageout.MAX_COMPONENT_CAP})")
        self.net = generator.eval()
        self.S, self.context, self.feather, self.batch = int(imagedim), float(context), int(feather), int(batch)
        self.windows, self.max_holes = windows, int(max_holes)
        self.forward_calls = 0          # generator forwards so far
        self.holes = []                 # per-hole mode: (components, windows) of every image of the last call
        self.capture = None             # tests: a dict here receives the windows and what went through the generator
        self._resize = _Resizer()
        self._bufs = {}

    def _batch_buffers(self, n, device):
        """(ground, mask, ceil(mask), masked, composite) fp32 (batch,1,S,S), allocated once per device."""
        if device not in self._bufs:
            self._bufs[device] = tuple(torch.empty((self.batch, 1, self.S, self.S), dtype=torch.float32, device=device) for _ in range(5))
        return tuple(b[:n] for b in self._bufs[device])

    @torch.no_grad()
    def __call__(self, images, masks):
        if len(images) != len(masks):
            raise ValueError(f"{len(images)} images, {len(masks)} masks")
        jobs, results = [], []
        self.holes = []
        for i, (img, mk) in enumerate(zip(images, masks)):
            for t in (img, mk):
                if not torch.is_tensor(t) or t.dtype != torch.uint8 or t.dim() != 2 or not t.is_cuda:
                    raise B.BackendError("Inpainter takes (H,W) uint8 tensors on the gfx950 device")
            if img.shape != mk.shape or img.device != mk.device:
                raise ValueError(f"image {tuple(img.shape)} on {img.device}, mask {tuple(mk.shape)} on {mk.device}: one shape, one device")
            img, mk = img.contiguous(), mk.contiguous()
            H, W = img.shape
            if self.windows == "per-hole":
                _, count, table = imageout.mask_components(mk, 8, self.max_holes)
                if count == 0:
                    self.holes.append((0, 0))
                    results.append(img)
                    continue
                if count <= self.max_holes:
                    wins, _ = plan_windows(H, W, table[:, 1:5].tolist(), self.S, self.context, self.feather)
                    self.holes.append((count, len(wins)))
                    results.append(None)
                    jobs.extend((i, img, mk, win) for win in wins)
                    continue
                self.holes.append((count, 1))              # more holes than max_holes: the single window below
            box = imageout.mask_bbox(mk)[0].tolist()       # the one device -> host copy per image
            if box[2] < 0:
                results.append(img)                        # nothing to repair
                continue
            results.append(None)
            jobs.append((i, img, mk, plan_window(H, W, box, self.S, self.context, self.feather)))
        if self.capture is not None:
            self.capture.update(windows=[j[3] for j in jobs], masked=[], mask=[], output=[])
        for k in range(0, len(jobs), self.batch):
            self._run(jobs[k:k + self.batch], results)
        return results

    def _run(self, jobs, results):
        lib, S, n = B.lib(), self.S, len(jobs)
        dev = jobs[0][1].device
        ctx = B.get_ctx(dev)
        ground, mask, m, masked, comp = self._batch_buffers(n, dev)
        for k, (_, img, mk, win) in enumerate(jobs):
            self._resize(imageout.window_crop(img, win), S, S, out_f32=ground[k])                       # ToTensor: / 255
            self._resize(imageout.window_crop(mk, win, binarize=True), S, S, out_f32=mask[k])
        B.check(lib.gi_mask_apply(ctx, B.ptr(ground), B.ptr(mask), B.ptr(m), B.ptr(masked), ground.numel(), 1))   # ceil, as the plugins do
        out = self.net(masked).contiguous()
        self.forward_calls += 1
        B.check(lib.gi_mask_composite(ctx, B.ptr(masked), B.ptr(out), B.ptr(m), B.ptr(comp), comp.numel()))
        patch_s = imageout.quantize(comp)
        for k, (i, img, mk, win) in enumerate(jobs):
            patch = torch.empty((win[2], win[3]), dtype=torch.uint8, device=dev)
            self._resize(patch_s[k, 0], win[2], win[3], out_u8=patch)
            results[i] = imageout.feather_paste(img, mk, win, patch, self.feather, out=results[i])   # (the windows of one image: one copy)
        if self.capture is not None:
            self.capture["masked"].append(masked.clone())
            self.capture["mask"].append(m.clone())
            self.capture["output"].append(out)
