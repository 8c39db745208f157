#!/usr/bin/env python3
"""Times the device dataset cache (lib/data/cache.py, csrc/batchgather.hip) against the per-pass decode it replaces.

    python tools/cache_time.py [--n128 4096] [--n256 2048] [--passes 3] [--launches 200] [--out FILE.json]

Per image size (128 and 256; the PNG files are 5/4 of it, so the Resize runs), on a dataset generated from a seed in a temporary
directory (N grey images - random 8 x 8 blocks plus +-8 of noise - and N rectangle mask files), batch 32:
  (a) the path without the cache: train.py's DataLoader over InpaintingDataset(transform=None) + to_device_images on both items,
      at 0 and at 16 workers;
  (b) the cache build (every file decoded and resized once), at 0 and at 16 workers;
  (c) a pass of the cached loader, plain and with flips.
Each figure is images per second of a full pass that ends in a device synchronise (host clock), after one warm-up pass: the
median of --passes passes with their minimum and maximum. Then the gather launch alone at 32 x 256 x 256 (fp32 out): HIP events
around every launch, median / p10 / p90, and its bytes (one read per pixel, four written) over that time next to the HBM rate a
float4 copy reaches (6.29 TB/s, MI355X) - at 10 MB a launch this mostly measures launch cost, not bandwidth.
A GPU is required; nothing falls back."""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

BATCH = 32
HBM_COPY_BYTES_PER_S = 6.29e12


def write_dataset(root, n, src, seed):
    from PIL import Image
    import pandas as pd
    os.makedirs(os.path.join(root, "csv"))
    os.makedirs(os.path.join(root, "img"))
    rng = np.random.Generator(np.random.PCG64(seed))
    rows = []
    for i in range(n):
        coarse = rng.integers(16, 240, ((src + 7) // 8, (src + 7) // 8)).repeat(8, 0).repeat(8, 1)[:src, :src]
        g = (coarse + rng.integers(-8, 9, (src, src))).astype(np.uint8)
        m = np.zeros((src, src), np.uint8)
        h, w = rng.integers(src // 8, src // 2 + 1, 2)
        y0, x0 = rng.integers(0, src - h + 1), rng.integers(0, src - w + 1)
        m[y0:y0 + h, x0:x0 + w] = 255
        Image.fromarray(g, mode="L").save(os.path.join(root, "img", f"g{i}.png"))
        Image.fromarray(m, mode="L").save(os.path.join(root, "img", f"m{i}.png"))
        rows.append({"groundtruth_source": f"img/g{i}.png", "mask_source": f"img/m{i}.png"})
    pd.DataFrame(rows).to_csv(os.path.join(root, "csv", "train_all_masks.csv"), index=False)


def rate(n_images, seconds):
    s = sorted(seconds)
    return {"images_per_s_median": n_images / statistics.median(s), "images_per_s_min": n_images / s[-1],
            "images_per_s_max": n_images / s[0], "passes": len(s), "images_per_pass": n_images}


def timed(fn, passes, warmup=1):
    for _ in range(warmup):
        fn()
    out = []
    for _ in range(passes):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        out.append(time.perf_counter() - t0)
    return out


def show(name, r):
    print(f"  {name:34s} {r['images_per_s_median']:10.0f} images/s  (min {r['images_per_s_min']:.0f}, max {r['images_per_s_max']:.0f}; "
          f"{r['passes']} passes of {r['images_per_pass']})", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n128", type=int, default=4096)
    ap.add_argument("--n256", type=int, default=2048)
    ap.add_argument("--passes", type=int, default=3)
    ap.add_argument("--launches", type=int, default=200)
    ap.add_argument("--workers", type=int, default=16)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("cache_time.py needs the GPU")
    import pandas as pd
    import gan_inpainting_amd  # noqa: F401
    from gan_inpainting_amd import backend as B
    from gan_inpainting_amd.experiment_list._common import to_device_images
    from gan_inpainting_amd.lib.data.cache import DeviceCachedLoader, DeviceImageCache
    from gan_inpainting_amd.lib.data.dataset import InpaintingDataset

    device = torch.device("cuda", 0)
    res = {"device": torch.cuda.get_device_name(0), "batch": BATCH, "sizes": []}
    for size, n in ((128, args.n128), (256, args.n256)):
        src = size * 5 // 4
        with tempfile.TemporaryDirectory() as root:
            root = os.path.join(root, "data")
            t0 = time.perf_counter()
            write_dataset(root, n, src, seed=size)
            print(f"{size} x {size}: N = {n} images + {n} masks of {src} x {src} written in {time.perf_counter() - t0:.1f} s", flush=True)
            ds = InpaintingDataset(root, dataframe=pd.read_csv(os.path.join(root, "csv", "train_all_masks.csv")), transform=None)
            rec = {"size": size, "source": src, "N": n}
            state = {"imagedim": size}
            per_pass = (n // BATCH) * BATCH
            for workers in (0, args.workers):
                kw = {"num_workers": workers}
                if workers > 0:
                    kw.update(persistent_workers=True, pin_memory=True, prefetch_factor=4)          # train.py's settings
                loader = torch.utils.data.DataLoader(ds, batch_size=BATCH, shuffle=True, drop_last=True, **kw)

                def uncached():
                    for g, m, _ in loader:
                        to_device_images(g, device, state)
                        to_device_images(m, device, state)
                rec[f"a_uncached_workers{workers}"] = rate(per_pass, timed(uncached, args.passes))
                show(f"(a) uncached, {workers} workers", rec[f"a_uncached_workers{workers}"])
                del loader
                cache = None

                def build():
                    nonlocal cache
                    cache = DeviceImageCache.build(ds, size, device, workers=workers)
                rec[f"b_build_workers{workers}"] = rate(n, timed(build, args.passes, warmup=1))
                show(f"(b) cache build, {workers} workers", rec[f"b_build_workers{workers}"])
            rec["cache_bytes"] = cache.nbytes
            cl = DeviceCachedLoader(cache, BATCH, "train", seed=1)

            def cached():
                for _ in cl:
                    pass
            epoch = [0]

            def flipped():
                epoch[0] += 1
                for _ in cl.augmented(epoch[0]):
                    pass
            rec["c_cached"] = rate(per_pass, timed(cached, max(args.passes, 10)))
            show("(c) cached loader", rec["c_cached"])
            rec["c_cached_flips"] = rate(per_pass, timed(flipped, max(args.passes, 10)))
            show("(c) cached loader, --flip", rec["c_cached_flips"])
            if size == 256:
                # the gather launch alone, 32 x 256 x 256, fp32 out, with flip keys
                lib, ctx = B.lib(), B.get_ctx(device)
                rows = torch.randperm(n, device=device)[:BATCH].contiguous()
                keys = rows + (1 << 32)
                out = torch.empty((BATCH, 1, size, size), dtype=torch.float32, device=device)
                store = cache.stores["ground"]
                fn = lambda: B.check(lib.gi_batch_gather(ctx, B.ptr(store), n, size, size, B.ptr(rows), BATCH, B.ptr(keys), 0x5EED, 0, B.ptr(out)))  # noqa: E731
                for _ in range(20):
                    fn()
                torch.cuda.synchronize()
                ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(args.launches)]
                for a, b in ev:
                    a.record()
                    fn()
                    b.record()
                torch.cuda.synchronize()
                ts = sorted(a.elapsed_time(b) * 1e3 for a, b in ev)
                nbytes = BATCH * size * size * 5
                med = statistics.median(ts)
                rec["gather_launch"] = {"median_us": med, "p10_us": ts[len(ts) // 10], "p90_us": ts[(len(ts) * 9) // 10], "launches": len(ts),
                                        "bytes": nbytes, "bytes_per_s": nbytes / (med * 1e-6),
                                        "share_of_hbm_copy_rate": nbytes / (med * 1e-6) / HBM_COPY_BYTES_PER_S}
                g = rec["gather_launch"]
                print(f"  gather launch 32 x {size} x {size} fp32: median {med:.2f} us (p10 {g['p10_us']:.2f}, p90 {g['p90_us']:.2f}; {len(ts)} launches), "
                      f"{nbytes / 1e6:.1f} MB -> {g['bytes_per_s'] / 1e12:.2f} TB/s = {100 * g['share_of_hbm_copy_rate']:.0f} % of the 6.29 TB/s copy rate "
                      f"(launch cost included)", flush=True)
            res["sizes"].append(rec)
            del cache, cl
    if args.out:
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
