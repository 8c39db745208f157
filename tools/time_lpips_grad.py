#!/usr/bin/env python3
"""Cost of the LPIPS backward on one MI355X.

  python tools/time_lpips_grad.py [--size 256] [--n 32] [--reps 50] [--out FILE.json]
      LPIPS.distance (the forward-only entry: the yardstick) against LPIPS.distance_and_grad on n pairs of size x size images
      (max_pairs = n: one call of the handle each), ALTERNATING in one process, HIP events, the medians of --reps after warm-up, and
      their ratio; the two workspaces' sizes at this geometry and at 256 x 256 x 16 pairs.
  rocprofv3 --kernel-trace --stats -- python tools/time_lpips_grad.py --trace [--size 256] [--n 32]
      five grad calls and nothing else: the per-kernel table of the profiler."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--n", type=int, default=32)
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--trace", action="store_true")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    import ctypes as C
    import torch
    import gan_inpainting_amd  # noqa: F401
    import lpips_ref as R
    from gan_inpainting_amd import backend as B
    from gan_inpainting_amd.lib.lpips import LPIPS
    if not torch.cuda.is_available():
        raise SystemExit("time_lpips_grad.py measures on the GPU; none is visible")
    P = R.make_params(20261)
    m = LPIPS(max_pairs=a.n, grad=True)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in P.items()})
    m = m.cuda()
    x = torch.from_numpy(R.make_images(1, a.n, a.size, a.size)).cuda()
    y = torch.from_numpy(R.make_images(2, a.n, a.size, a.size)).cuda()
    if a.trace:
        for _ in range(5):
            m.distance_and_grad(x, y)
        torch.cuda.synchronize()
        return
    d0 = m.distance(x, y)
    d1, g = m.distance_and_grad(x, y)
    assert torch.equal(d0, d1) and torch.isfinite(g).all()
    for _ in range(5):
        m.distance(x, y)
        m.distance_and_grad(x, y)
    torch.cuda.synchronize()
    tf, tg = [], []
    for _ in range(a.reps):
        for fn, ts in ((lambda: m.distance(x, y), tf), (lambda: m.distance_and_grad(x, y), tg)):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            torch.cuda.synchronize()
            ts.append(e0.elapsed_time(e1))
    tf.sort()
    tg.sort()
    fwd, grd = tf[len(tf) // 2], tg[len(tg) // 2]

    def ws_bytes(size, pairs):
        lib, hd = B.lib(), C.c_void_p()
        B.check(lib.gi_lpips_create(B.get_ctx(x.device), size, size, pairs, C.byref(hd)))
        out = (int(lib.gi_lpips_workspace_bytes(hd)), int(lib.gi_lpips_grad_workspace_bytes(hd)))
        lib.gi_lpips_destroy(hd)
        return out
    here, ref = ws_bytes(a.size, a.n), ws_bytes(256, 16)
    print(f"library {B.LIB_PATH}")
    print(f"{a.n} pairs of {a.size}x{a.size}, medians of {a.reps}: distance {fwd:.3f} ms ({tf[0]:.3f}..{tf[-1]:.3f}), distance_and_grad {grd:.3f} ms "
          f"({tg[0]:.3f}..{tg[-1]:.3f}), ratio {grd / fwd:.2f}")
    print(f"workspace at this geometry: forward {here[0] / 2 ** 20:.1f} MiB, grad {here[1] / 2 ** 20:.1f} MiB; at 256x256 x 16 pairs: forward "
          f"{ref[0] / 2 ** 20:.1f} MiB, grad {ref[1] / 2 ** 20:.1f} MiB")
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        json.dump(dict(lib=B.LIB_PATH, size=a.size, pairs=a.n, reps=a.reps, distance_ms=fwd, distance_and_grad_ms=grd, ratio=grd / fwd,
                       workspace_bytes=here, workspace_bytes_256x16=ref), open(a.out, "w"), indent=1)


if __name__ == "__main__":
    main()
