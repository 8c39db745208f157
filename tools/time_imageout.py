#!/usr/bin/env python3
"""Times the image-output kernels (csrc/imageout.hip) and the Inpainter against their byte floors and the host alternative.

    python tools/time_imageout.py [--launches 50] [--out FILE.json]

Per image size (1024 x 1024 and 4096 x 4096, full-image window): HIP events around every single launch after a warm-up, median
and 10th / 90th percentile in microseconds, for gi_feather_paste (r = 8 and r = 63) and gi_panel_assemble (three columns, one
row: what inpaint.py --panel writes). Next to each the bytes the kernel must move (feather: orig + mask + patch read, dst written,
4 HW; panel: 3 fp32 columns read, the canvas written) and the time those bytes take at the rate a device-to-device copy of a
buffer of the image's fp32 size reaches here. Then lib.inpaint.Inpainter end to end for one 1024 x 1024 picture at S = 256 (wall
clock around a device synchronise), next to the generator forward alone; and the host alternative, timed once each after one
warm-up: Pillow crop + two resizes and a numpy blend (box count by cumulative sums) of the same picture. A GPU is required."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def event_times_us(fn, launches, warmup=10):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(launches)]
    for a, b in ev:
        a.record()
        fn()
        b.record()
    torch.cuda.synchronize()
    return sorted(a.elapsed_time(b) * 1e3 for a, b in ev)


def summary(ts):
    return {"median_us": statistics.median(ts), "p10_us": ts[len(ts) // 10], "p90_us": ts[(len(ts) * 9) // 10], "launches": len(ts)}


def host_blend(orig, mask, patch, r):
    """The feathered blend in numpy: box count from a summed-area table, then the integer blend."""
    hole = (mask != 0)
    sat = np.zeros((hole.shape[0] + 1, hole.shape[1] + 1), np.int32)
    sat[1:, 1:] = hole.cumsum(0, dtype=np.int32).cumsum(1, dtype=np.int32)
    H, W = hole.shape
    y0, y1 = np.clip(np.arange(H) - r, 0, H), np.clip(np.arange(H) + r + 1, 0, H)
    x0, x1 = np.clip(np.arange(W) - r, 0, W), np.clip(np.arange(W) + r + 1, 0, W)
    a = sat[y1][:, x1] - sat[y0][:, x1] - sat[y1][:, x0] + sat[y0][:, x0]
    A = (2 * r + 1) ** 2
    alpha = np.where(hole, A, np.minimum(A, 2 * a)).astype(np.int32)
    return ((alpha * patch.astype(np.int32) + (A - alpha) * orig.astype(np.int32) + A // 2) // A).astype(np.uint8)


def host_inpaint(img, mask, window, S, r):
    """Everything lib.inpaint does around the generator, on the host: Pillow crop / resize, numpy mask arithmetic and blend."""
    from PIL import Image
    wy, wx, wh, ww = window
    box = (wx, wy, wx + ww, wy + wh)
    g = np.asarray(Image.fromarray(img).crop(box).resize((S, S), Image.BILINEAR), np.float32) / np.float32(255)
    m = np.ceil(np.asarray(Image.fromarray(np.where(mask != 0, 255, 0).astype(np.uint8)).crop(box).resize((S, S), Image.BILINEAR), np.float32) / 255)
    masked = g * (1 - m)
    comp = np.rint(np.clip(masked + masked * m, 0, 1) * 255).astype(np.uint8)        # (the generator's output is not the host's to make)
    patch = np.asarray(Image.fromarray(comp).resize((ww, wh), Image.BILINEAR))
    out = img.copy()
    out[wy:wy + wh, wx:wx + ww] = host_blend(img[wy:wy + wh, wx:wx + ww], mask[wy:wy + wh, wx:wx + ww], patch, r)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--launches", type=int, default=50)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("time_imageout.py needs the GPU")
    import gan_inpainting_amd  # noqa: F401
    from gan_inpainting_amd import backend as B
    from gan_inpainting_amd.lib import imageout
    from gan_inpainting_amd.lib.inpaint import Inpainter, plan_window
    from gan_inpainting_amd.lib.models import networks
    import ctypes as C

    torch.set_num_threads(16)
    lib, ctx = B.lib(), B.get_ctx()
    res = {"device": torch.cuda.get_device_name(0), "sizes": []}
    rng = np.random.default_rng(0)
    for s in (1024, 4096):
        img = rng.integers(0, 256, (s, s), dtype=np.uint8)
        mask = np.zeros((s, s), np.uint8)
        mask[s // 4:s // 2, s // 3:(2 * s) // 3] = 255
        mask[(5 * s) // 8:(7 * s) // 8, s // 8:s // 4] = 255
        patch = rng.integers(0, 256, (s, s), dtype=np.uint8)
        d_img, d_mask, d_patch = (torch.from_numpy(a).cuda() for a in (img, mask, patch))
        dst = d_img.clone()
        f32 = torch.rand((1, 1, s, s), device="cuda")
        f32b = torch.empty_like(f32)
        copy = summary(event_times_us(lambda: f32b.copy_(f32), args.launches))
        copy_bw = 2 * f32.numel() * 4 / (copy["median_us"] * 1e-6)
        row = {"H": s, "W": s, "copy_bytes_per_s": copy_bw, "copy_median_us": copy["median_us"]}
        for r in (8, 63):
            fn = lambda: B.check(lib.gi_feather_paste(ctx, B.ptr(d_img), B.ptr(d_mask), s, s, 0, 0, s, s, B.ptr(d_patch), r, B.ptr(dst)))  # noqa: E731
            t = summary(event_times_us(fn, args.launches))
            t.update(bytes=4 * s * s, floor_us=4 * s * s / copy_bw * 1e6)
            row[f"feather_r{r}"] = t
            t0 = time.perf_counter()
            ref = host_blend(img, mask, patch, r)
            t["host_numpy_ms"] = (time.perf_counter() - t0) * 1e3
            t["equal_to_host"] = bool(np.array_equal(dst.cpu().numpy(), ref))
            print(f"{s}x{s} feather_paste r={r:2d}: median {t['median_us']:8.1f} us (p10 {t['p10_us']:.1f}, p90 {t['p90_us']:.1f}) | {t['bytes'] / 1e6:.1f} MB, "
                  f"floor {t['floor_us']:.1f} us at {copy_bw / 1e12:.2f} TB/s | numpy {t['host_numpy_ms']:.0f} ms, equal {t['equal_to_host']}")
        cols = [torch.rand((1, 1, s, s), device="cuda") for _ in range(3)]
        Hc, Wc = imageout.panel_shape(3, 1, s, s, 2)
        canvas = torch.empty((Hc, Wc), dtype=torch.uint8, device="cuda")
        ptrs = (C.c_void_p * 3)(*[c.data_ptr() for c in cols])
        fn = lambda: B.check(lib.gi_panel_assemble(ctx, C.cast(ptrs, C.c_void_p), 3, 1, s, s, 2, B.ptr(canvas)))  # noqa: E731
        t = summary(event_times_us(fn, args.launches))
        t.update(bytes=3 * 4 * s * s + Hc * Wc, floor_us=(3 * 4 * s * s + Hc * Wc) / copy_bw * 1e6)
        row["panel_3col"] = t
        print(f"{s}x{s} panel_assemble 3 columns: median {t['median_us']:8.1f} us (p10 {t['p10_us']:.1f}, p90 {t['p90_us']:.1f}) | {t['bytes'] / 1e6:.1f} MB, "
              f"floor {t['floor_us']:.1f} us")
        res["sizes"].append(row)

    # end to end: one 1024 x 1024 picture, S = 256, the hole a 300 x 380 rectangle (window 760 x 760)
    S, s, r = 256, 1024, 8
    torch.manual_seed(0)
    net = networks.get_network("generator", "unet", dtype="fp16").to("cuda:0").eval()
    img = rng.integers(0, 256, (s, s), dtype=np.uint8)
    mask = np.zeros((s, s), np.uint8)
    mask[300:600, 350:730] = 255
    d_img, d_mask = torch.from_numpy(img).cuda(), torch.from_numpy(mask).cuda()
    inp = Inpainter(net, imagedim=S, feather=r)
    for _ in range(3):
        inp([d_img], [d_mask])
    torch.cuda.synchronize()
    wall = []
    for _ in range(20):
        t0 = time.perf_counter()
        inp([d_img], [d_mask])
        torch.cuda.synchronize()
        wall.append((time.perf_counter() - t0) * 1e6)
    x = torch.rand((1, 1, S, S), device="cuda")
    with torch.no_grad():
        fwd = summary(event_times_us(lambda: net(x), args.launches))
        t0 = time.perf_counter()
        for _ in range(20):
            net(x)
        torch.cuda.synchronize()
        fwd_wall = (time.perf_counter() - t0) / 20 * 1e6
    window = plan_window(s, s, (300, 350, 599, 729), S, 2.0, r)
    host_inpaint(img, mask, window, S, r)
    t0 = time.perf_counter()
    host_inpaint(img, mask, window, S, r)
    host_ms = (time.perf_counter() - t0) * 1e3
    e2e = {"image": [s, s], "S": S, "feather": r, "window": list(window), "wall_median_us": statistics.median(wall), "wall_min_us": min(wall),
           "generator_forward_event_us": fwd["median_us"], "generator_forward_wall_us": fwd_wall,
           "host_pillow_numpy_without_generator_ms": host_ms}
    res["end_to_end"] = e2e
    print(f"Inpainter 1024x1024, S=256, window {window}: wall median {e2e['wall_median_us']:.0f} us (min {e2e['wall_min_us']:.0f}); generator forward "
          f"{fwd['median_us']:.0f} us by events, {fwd_wall:.0f} us wall; host Pillow + numpy around the generator {host_ms:.1f} ms")
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
