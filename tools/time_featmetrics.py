#!/usr/bin/env python3
"""KID and precision / recall timing on one MI355X against the same computation on the host.

  python tools/time_featmetrics.py [--sizes 2000,10000] [--dims 2048] [--reps 5] [--host-reps 1] [--out FILE.json]
      per size n (rows in each of the two sets): kernel_inception_distance at its defaults (100 subsets of min(n, 1000) rows) and
      precision_recall with k = 3 on the device - HIP-event medians after warm-up, feature matrices already on the device, the
      host-side index draw and the readback of the result included - and the same two computations in torch fp64 on the host with
      16 threads (one matmul per Gram matrix, torch.kthvalue for the radii): wall time, best of --host-reps. The two sides'
      values are printed side by side. Algorithmic FLOP (2 d per Gram element that the definition needs) and the device's
      rate are reported; no share of a peak is: the fp64 MFMA peak has not been measured here."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

HOST_THREADS = 16


def _events(fn, reps):
    import torch
    for _ in range(2):
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
    return ts[len(ts) // 2]


def host_kid(real, fake, num_subsets=100, max_subset_size=1000, seed=0):
    """tests/featmetrics_ref.kid with torch fp64 matmuls (real, fake: float64 host tensors)."""
    import featmetrics_ref as F
    import torch
    d = real.shape[1]
    m, ir, jf = F.kid_indices(real.shape[0], fake.shape[0], num_subsets, max_subset_size, seed)
    off = ~torch.eye(m, dtype=torch.bool)
    terms = []
    for s in range(ir.shape[0]):
        x, y = real[torch.from_numpy(ir[s])], fake[torch.from_numpy(jf[s])]
        kxx, kyy, kxy = ((a @ b.T / d + 1.0) ** 3 for a, b in ((x, x), (y, y), (x, y)))
        terms.append(float(kxx[off].sum() / (m * (m - 1)) + kyy[off].sum() / (m * (m - 1)) - 2.0 * kxy.sum() / (m * m)))
    return sum(terms) / len(terms)


def host_pr(real, fake, k=3):
    import torch

    def d2(a, b):
        return torch.clamp(((a * a).sum(1)[:, None] + (b * b).sum(1)[None, :]) - 2.0 * (a @ b.T), min=0.0)

    def radii(a):
        D = d2(a, a)
        D.fill_diagonal_(float("inf"))
        return torch.kthvalue(D, k, dim=1).values
    p = (d2(real, fake) <= radii(real)[:, None]).any(dim=0).double().mean()
    r = (d2(fake, real) <= radii(fake)[:, None]).any(dim=0).double().mean()
    return float(p), float(r)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="2000,10000")
    ap.add_argument("--dims", type=int, default=2048)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--host-reps", dest="host_reps", type=int, default=1)
    ap.add_argument("--no-host", dest="host", action="store_false", default=True)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    import torch
    import gan_inpainting_amd  # noqa: F401
    from gan_inpainting_amd.lib.fid import dist_metrics as dm
    if not torch.cuda.is_available():
        raise SystemExit("time_featmetrics.py measures on the GPU; none is visible")
    torch.set_num_threads(HOST_THREADS)
    d = a.dims
    res = {"dims": d, "host_threads": HOST_THREADS, "host": "torch %s fp64" % torch.__version__,
           "note": "flop = 2 d per Gram element of the definition (3 m^2 per KID subset, 4 n^2 for precision / recall); the device "
                   "computes only the tiles on and above the diagonal of the two symmetric KID matrices, so its tflops are algorithmic, "
                   "not executed; no fp64 MFMA peak was measured, no share of peak is claimed",
           "sizes": {}}
    for n in (int(s) for s in a.sizes.split(",")):
        g = torch.Generator().manual_seed(n)
        real = torch.rand((n, d), generator=g)                   # pool3 features are averages of ReLU outputs: non-negative
        fake = torch.rand((n, d), generator=g) * 1.05
        tr, tf = real.cuda(), fake.cuda()
        m = min(n, 1000)
        subsets = 1 if m == n else 100
        kid_flop = subsets * 3 * 2.0 * m * m * d
        pr_flop = 4 * 2.0 * n * n * d
        row = {"kid_subsets_computed": subsets, "kid_subset_size": m, "kid_flop": kid_flop, "pr_flop": pr_flop}
        row["kid_device_ms"] = _events(lambda: dm.kernel_inception_distance(tr, tf), a.reps)
        row["pr_device_ms"] = _events(lambda: dm.precision_recall(tr, tf, k=3), a.reps)
        row["kid_device"] = dm.kernel_inception_distance(tr, tf)
        row["pr_device"] = dm.precision_recall(tr, tf, k=3)
        row["kid_device_tflops"] = kid_flop / (row["kid_device_ms"] * 1e-3) / 1e12
        row["pr_device_tflops"] = pr_flop / (row["pr_device_ms"] * 1e-3) / 1e12
        print(f"n={n} d={d} device: KID {row['kid_device_ms']:.2f} ms ({row['kid_device_tflops']:.2f} TFLOP/s fp64), "
              f"precision/recall {row['pr_device_ms']:.2f} ms ({row['pr_device_tflops']:.2f} TFLOP/s fp64)", flush=True)
        if a.host:
            r64, f64 = real.double(), fake.double()
            for name, fn in (("kid", lambda: host_kid(r64, f64)), ("pr", lambda: host_pr(r64, f64, 3))):
                best = None
                for _ in range(a.host_reps):
                    t0 = time.perf_counter()
                    val = fn()
                    dt = (time.perf_counter() - t0) * 1e3
                    best = dt if best is None else min(best, dt)
                row[name + "_host_ms"], row[name + "_host"] = best, val
                row[name + "_speedup"] = best / row[name + "_device_ms"]
                print(f"n={n} host ({HOST_THREADS} threads, torch fp64): {name} {best:.0f} ms = {row[name + '_speedup']:.1f}x the device time; "
                      f"value {val} (device {row[name + '_device']})", flush=True)
        res["sizes"][str(n)] = row
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        json.dump(res, open(a.out, "w"), indent=1)


if __name__ == "__main__":
    main()
