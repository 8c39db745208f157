#!/usr/bin/env python3
"""Times gi_mask_components (csrc/components.hip) and Inpainter(windows="per-hole").

    python tools/time_components.py [--launches 50] [--out profiles/components_timing.json]
    python tools/time_components.py --resolution-only [--out FILE.json]         (no GPU: window planning on the host)

Per image size (1024 x 1024 and 4096 x 4096) and mask (a free-form mask of the device mask generator, a random mask of density
0.4, the serpentine of tests/components_ref.py as the worst case): HIP events around every single call after a warm-up, median and
10th / 90th percentile in microseconds, 8-connected, cap 256. Next to each the byte floor - one read of the mask and one write of
the labels, 5 HW bytes - at the rate a device-to-device copy of a buffer of the image's fp32 size reaches in the same run, and the
Python restatement (tests/components_ref.py) on the host, timed once, whose three outputs the device's must equal. Then
lib.inpaint.Inpainter end to end on one 4096 x 4096 picture at S = 256, with a five-stroke free-form mask and with five scattered
scratches, windows="single" against "per-hole": windows, generator forwards and wall clock around a device synchronise.

--resolution-only: the planning evidence. For 16 free-form masks of the mask generator and 16 masks of five short scratches
(tests/components_ref.py) at 2048 x 2048, S = 256: the components, the side of the single window and the sides of the per-hole
windows, and the enlargement (side / S) the hole pixels are repaired at, weighted by area."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import components_ref as CR  # noqa: E402
import maskgen_ref as MG  # noqa: E402


def summary(ts):
    return {"median_us": statistics.median(ts), "p10_us": ts[len(ts) // 10], "p90_us": ts[(len(ts) * 9) // 10], "launches": len(ts)}


def resolution(size=2048, S=256, context=2.0, feather=8, seed=0, keys=range(16)):
    import gan_inpainting_amd  # noqa: F401
    from gan_inpainting_amd.lib.inpaint import plan_window, plan_windows
    out = {"size": size, "S": S, "context": context, "feather": feather, "seed": seed, "families": {}}
    for family in ("freeform", "scratches"):
        rows = []
        for key in keys:
            mask = MG.mask("freeform", seed, key, size, size) if family == "freeform" else CR.scratches(size, size, 1000 * seed + key)
            ys, xs = np.nonzero(mask)
            single = plan_window(size, size, (ys.min(), xs.min(), ys.max(), xs.max()), S, context, feather)
            _, count, table = CR.components(mask, 8, cap=1 << 20)
            wins, groups = plan_windows(size, size, table[:, 1:5].tolist(), S, context, feather)
            area = [int(mask[w[0]:w[0] + w[2], w[1]:w[1] + w[3]].sum()) for w in wins]
            scale = sum(a * max(w[2:]) / S for a, w in zip(area, wins)) / sum(area)
            rows.append({"key": int(key), "components": count, "windows": len(wins), "single_side": max(single[2:]),
                         "per_hole_sides": [max(w[2:]) for w in wins], "single_scale": max(single[2:]) / S, "per_hole_scale_area_weighted": scale})
            print(f"{family} {key:2d}: {count} components -> {len(wins)} windows; single side {rows[-1]['single_side']} "
                  f"(x{rows[-1]['single_scale']:.2f}), per-hole sides {rows[-1]['per_hole_sides']} (area-weighted x{scale:.2f})")
        fam = {"masks": rows, "mean_single_scale": statistics.mean(r["single_scale"] for r in rows),
               "mean_per_hole_scale": statistics.mean(r["per_hole_scale_area_weighted"] for r in rows),
               "masks_with_several_windows": sum(r["windows"] > 1 for r in rows)}
        print(f"{family}: mean enlargement single x{fam['mean_single_scale']:.2f}, per-hole x{fam['mean_per_hole_scale']:.2f}; "
              f"{fam['masks_with_several_windows']} of {len(rows)} masks keep more than one window")
        out["families"][family] = fam
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--launches", type=int, default=50)
    ap.add_argument("--out", default="")
    ap.add_argument("--resolution-only", action="store_true")
    args = ap.parse_args()
    res = {}
    if args.resolution_only:
        res["resolution"] = resolution()
    else:
        import torch
        if not torch.cuda.is_available():
            sys.exit("time_components.py needs the GPU (or --resolution-only)")
        from time_imageout import event_times_us
        import gan_inpainting_amd  # noqa: F401
        from gan_inpainting_amd import backend as B
        from gan_inpainting_amd.lib.data.masks import DeviceMaskGenerator
        from gan_inpainting_amd.lib.inpaint import Inpainter
        from gan_inpainting_amd.lib.models import networks

        torch.set_num_threads(16)
        lib, ctx = B.lib(), B.get_ctx()
        res = {"device": torch.cuda.get_device_name(0), "connectivity": 8, "cap": 256, "sizes": []}
        cap = 256

        def freeform(s, key):
            m = DeviceMaskGenerator("freeform", s, s, 0)(torch.tensor([key], dtype=torch.int64))
            return (m[0, 0] * 255).to(torch.uint8)

        for s in (1024, 4096):
            f32 = torch.rand((1, 1, s, s), device="cuda")
            f32b = torch.empty_like(f32)
            copy = summary(event_times_us(lambda: f32b.copy_(f32), args.launches))
            copy_bw = 2 * f32.numel() * 4 / (copy["median_us"] * 1e-6)
            row = {"H": s, "W": s, "copy_bytes_per_s": copy_bw, "floor_bytes": 5 * s * s, "floor_us": 5 * s * s / copy_bw * 1e6, "masks": {}}
            del f32, f32b
            masks = {"freeform": freeform(s, 2), "random0.4": torch.from_numpy(CR.pattern("random0.4", s, s)).cuda(),
                     "serpentine": torch.from_numpy(CR.serpentine(s, s)).cuda()}
            labels = torch.empty((s, s), dtype=torch.int32, device="cuda")
            count = torch.empty(1, dtype=torch.int32, device="cuda")
            table = torch.empty((cap, 6), dtype=torch.int32, device="cuda")
            ws = torch.empty(int(lib.gi_mask_components_workspace_bytes(s, s, cap)), dtype=torch.uint8, device="cuda")
            for name, m in masks.items():
                fn = lambda: B.check(lib.gi_mask_components(ctx, B.ptr(m), s, s, 8, cap, B.ptr(labels), B.ptr(count), B.ptr(table), B.ptr(ws)))  # noqa: E731
                t = summary(event_times_us(fn, args.launches))
                host = m.cpu().numpy()
                t0 = time.perf_counter()
                r_labels, r_count, r_table = CR.components(host, 8, cap)
                t["host_python_ms"] = (time.perf_counter() - t0) * 1e3
                n = int(count.item())
                t["components"] = n
                t["equal_to_host"] = bool(n == r_count and np.array_equal(labels.cpu().numpy(), r_labels)
                                          and np.array_equal(table[:min(n, cap)].cpu().numpy(), r_table))
                t["times_floor"] = t["median_us"] / row["floor_us"]
                row["masks"][name] = t
                print(f"{s}x{s} {name:10s}: median {t['median_us']:9.1f} us (p10 {t['p10_us']:.1f}, p90 {t['p90_us']:.1f}) | {n} components | floor "
                      f"{row['floor_us']:.1f} us at {copy_bw / 1e12:.2f} TB/s: x{t['times_floor']:.1f} | python {t['host_python_ms']:.0f} ms, equal {t['equal_to_host']}")
            res["sizes"].append(row)

        # end to end: one 4096 x 4096 picture at S = 256, a five-stroke free-form mask and five scattered scratches
        S, s = 256, 4096
        key = next(k for k in range(64) if MG.uni(MG.stream_of(0, k), 0, 2, 5) == 5)
        torch.manual_seed(0)
        net = networks.get_network("generator", "unet", dtype="fp16").to("cuda:0").eval()
        img = torch.from_numpy(np.random.default_rng(0).integers(0, 256, (s, s), dtype=np.uint8)).cuda()
        res["end_to_end"] = {"image": [s, s], "S": S, "freeform_key": key, "masks": {}}
        for name, mask in (("freeform_5_strokes", freeform(s, key)), ("scratches_5", torch.from_numpy(CR.scratches(s, s, 3) * 255).cuda())):
            e2e = {}
            for mode in ("single", "per-hole"):
                inp = Inpainter(net, imagedim=S, windows=mode)
                for _ in range(3):
                    inp([img], [mask])
                torch.cuda.synchronize()
                inp.forward_calls, wall = 0, []
                for _ in range(20):
                    t0 = time.perf_counter()
                    inp([img], [mask])
                    torch.cuda.synchronize()
                    wall.append((time.perf_counter() - t0) * 1e6)
                inp.capture = {}
                inp([img], [mask])
                e2e[mode] = {"wall_median_us": statistics.median(wall), "wall_min_us": min(wall), "windows": [list(w) for w in inp.capture["windows"]],
                             "forwards_per_call": inp.forward_calls // 21, "holes": inp.holes}
                print(f"Inpainter 4096x4096 S=256 {name} {mode:8s}: wall median {e2e[mode]['wall_median_us']:.0f} us (min {e2e[mode]['wall_min_us']:.0f}); "
                      f"{len(e2e[mode]['windows'])} windows {[w[2:] for w in e2e[mode]['windows']]}, {e2e[mode]['forwards_per_call']} forwards, holes {inp.holes}")
            res["end_to_end"]["masks"][name] = e2e
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
