#!/usr/bin/env python3
"""LPIPS timing on one MI355X.

  python tools/time_lpips.py [--size 256] [--n 32] [--reps 100] [--cpu-pairs 4] [--out FILE.json]
      LPIPS.distance on n pairs of size x size images (max_pairs = n: one call of the handle), HIP events, the median of --reps
      after warm-up; then the torch fp32 restatement of the same metric on 16 host threads of the same box.
  GI_LIB_PATH=<another build> python tools/time_lpips.py ...
      the same numbers from another build of the library."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

CHANNELS = (64, 64, 128, 128, 256, 256, 256, 512, 512, 512, 512, 512, 512)
POOL_AFTER = (1, 3, 6, 9)


def conv_flop(size):
    """Convolution FLOP of one image (three input channels counted for the first layer, as the definition has them)."""
    flop, cin, hw = 0.0, 3, size * size
    for i, cout in enumerate(CHANNELS):
        flop += 2.0 * hw * cout * cin * 9
        cin = cout
        if i in POOL_AFTER:
            hw //= 4
    return flop


def _events(fn, reps):
    import torch
    for _ in range(5):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        ts.append(a.elapsed_time(b))
    ts.sort()
    return ts[len(ts) // 2], ts[0], ts[-1]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--n", type=int, default=32)
    ap.add_argument("--reps", type=int, default=100)
    ap.add_argument("--cpu-pairs", type=int, default=4)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    import torch
    import gan_inpainting_amd  # noqa: F401
    import lpips_ref as R
    from gan_inpainting_amd import backend as B
    from gan_inpainting_amd.lib.lpips import LPIPS
    if not torch.cuda.is_available():
        raise SystemExit("time_lpips.py measures on the GPU; none is visible")
    P = R.make_params(20261)
    m = LPIPS(max_pairs=a.n)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in P.items()})
    m = m.cuda()
    x = torch.from_numpy(R.make_images(1, a.n, a.size, a.size)).cuda()
    y = torch.from_numpy(R.make_images(2, a.n, a.size, a.size)).cuda()
    d = m.distance(x, y)
    med, lo, hi = _events(lambda: m.distance(x, y), a.reps)
    flop = 2 * a.n * conv_flop(a.size)
    print(f"library {B.LIB_PATH}")
    print(f"LPIPS.distance {a.n} pairs of {a.size}x{a.size}: median {med:.3f} ms ({lo:.3f}..{hi:.3f}) of {a.reps}, {med / a.n * 1e3:.1f} us per pair, "
          f"{flop / (med * 1e-3) / 1e12:.0f} TFLOP/s convolution-equivalent; mean d {float(d.mean()):.6f}")
    res = dict(lib=B.LIB_PATH, size=a.size, pairs=a.n, reps=a.reps, median_ms=med, min_ms=lo, max_ms=hi, us_per_pair=med / a.n * 1e3,
               conv_flop=flop, tflops=flop / (med * 1e-3) / 1e12, mean_distance=float(d.mean()))
    # the same metric in torch fp32 on 16 host threads: the restatement's arithmetic in float32
    torch.set_num_threads(16)
    T = {k: torch.from_numpy(v) for k, v in P.items()}
    xc, yc = x[:a.cpu_pairs].cpu(), y[:a.cpu_pairs].cpu()

    def cpu_distance(p, q):
        import torch.nn.functional as F
        h = torch.cat([p, q]).repeat(1, 3, 1, 1)
        h = (2 * h - 1 - T["scaling_layer.shift"]) / T["scaling_layer.scale"]
        tot = 0
        for i, tap in zip(R.CONV_IDX, R.TAP_AFTER):
            h = F.relu(F.conv2d(h, T[f"features.{i}.weight"], T[f"features.{i}.bias"], padding=1))
            if tap >= 0:
                f = h / (h.pow(2).sum(1, keepdim=True).sqrt() + 1e-10)
                n = p.shape[0]
                tot = tot + (T[f"lin{tap}.model.1.weight"] * (f[:n] - f[n:]).pow(2)).sum(1).mean((1, 2))
                if tap < 4:
                    h = F.max_pool2d(h, 2)
        return tot
    with torch.no_grad():
        cpu_distance(xc[:1], yc[:1])
        t0 = time.perf_counter()
        dc = cpu_distance(xc, yc)
        dtc = time.perf_counter() - t0
    print(f"host CPU (torch fp32, 16 threads): {a.cpu_pairs} pairs in {dtc:.2f} s = {dtc / a.cpu_pairs * 1e3:.0f} ms per pair; "
          f"max |d_hip - d_cpu| {float((d[:a.cpu_pairs].cpu() - dc).abs().max()):.2e}")
    res["cpu_baseline"] = dict(pairs=a.cpu_pairs, seconds=dtc, ms_per_pair=dtc / a.cpu_pairs * 1e3, threads=16)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        json.dump(res, open(a.out, "w"), indent=1)


if __name__ == "__main__":
    main()
