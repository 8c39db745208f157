#!/usr/bin/env python3
"""Times the device mask generator (csrc/maskgen.hip) against the host path it replaces and against the store floor.

    python tools/maskgen_time.py [--launches 200] [--out FILE.json]

Per configuration (both kinds; n = 32 at 256 x 256 and n = 8 at 512 x 512): HIP events around every single launch after a warm-up,
median and 10th / 90th percentile in microseconds. The store floor is the mask's bytes over the bandwidth a device-to-device copy
of a buffer of the same size reaches here (a copy reads and writes: its bytes per second count both, a mask is written only).
The host path is train.py's SyntheticInpainting: 32 samples' rectangles drawn with torch.Generator calls, stacked, copied to the
device (wall clock around a device synchronise). A GPU is required; nothing falls back."""
import argparse
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def event_times_us(fn, launches, warmup=20):
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--launches", type=int, default=200)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    if args.launches < 100:
        ap.error("--launches must be at least 100")
    if not torch.cuda.is_available():
        sys.exit("maskgen_time.py needs the GPU")
    import gan_inpainting_amd  # noqa: F401
    from gan_inpainting_amd import backend as B
    from gan_inpainting_amd.lib.data.masks import KINDS, mask_key
    from gan_inpainting_amd.train import SyntheticInpainting

    lib, ctx = B.lib(), B.get_ctx()
    res = {"device": torch.cuda.get_device_name(0), "configs": []}
    for n, s in ((32, 256), (8, 512)):
        keys = mask_key("train", 3, torch.arange(n, dtype=torch.int64)).cuda()
        out = torch.empty((n, 1, s, s), dtype=torch.float32, device="cuda")
        cover = torch.empty(n, dtype=torch.int32, device="cuda")
        src = torch.rand_like(out)
        nbytes = out.numel() * 4
        copy = summary(event_times_us(lambda: out.copy_(src), args.launches))
        copy_bw = 2 * nbytes / (copy["median_us"] * 1e-6)           # bytes moved (read + write) per second
        floor_us = nbytes / copy_bw * 1e6
        for kind, code in KINDS.items():
            for with_cover in (False, True):
                fn = lambda: B.check(lib.gi_mask_generate(ctx, code, 0x5EED, B.ptr(keys), n, s, s, B.ptr(out), B.ptr(cover) if with_cover else None))  # noqa: E731
                r = summary(event_times_us(fn, args.launches))
                r.update(kind=kind, n=n, H=s, W=s, coverage_out=with_cover, mask_bytes=nbytes, copy_median_us=copy["median_us"],
                         copy_bytes_per_s=copy_bw, store_floor_us=floor_us, mean_coverage=float(out.mean()))
                res["configs"].append(r)
                print(f"{kind:8s} n={n:2d} {s}x{s} coverage_out={int(with_cover)}: median {r['median_us']:7.2f} us  p10 {r['p10_us']:7.2f}  "
                      f"p90 {r['p90_us']:7.2f}  | store floor {floor_us:5.2f} us ({copy_bw / 1e12:.2f} TB/s copy, {copy['median_us']:.2f} us)")

    # the host path: 32 rectangles at 256 x 256 drawn sample by sample, stacked, copied to the device
    ds = SyntheticInpainting(32, 256, 1)
    g = torch.Generator()
    host = []
    for rep in range(25):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        m = torch.stack([SyntheticInpainting._host_rectangle(256, g.manual_seed(ds.seed + i)) for i in range(32)]).cuda()
        torch.cuda.synchronize()
        host.append((time.perf_counter() - t0) * 1e6)
    host = sorted(host[5:])
    res["host_rectangles_32x256"] = {"median_us": statistics.median(host), "p10_us": host[len(host) // 10], "p90_us": host[(len(host) * 9) // 10],
                                     "repeats": len(host), "what": "32 x SyntheticInpainting rectangle draws + stack + copy to the device"}
    print(f"host path, 32 masks of 256x256 (draw + stack + copy): median {res['host_rectangles_32x256']['median_us']:.0f} us  "
          f"p10 {res['host_rectangles_32x256']['p10_us']:.0f}  p90 {res['host_rectangles_32x256']['p90_us']:.0f}")
    assert tuple(m.shape) == (32, 1, 256, 256)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
