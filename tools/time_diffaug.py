#!/usr/bin/env python3
"""Differentiable augmentation on the GPU (HIP events).
kernels: the forward and the adjoint alone (lib.models.augment, the production entries) at 64x1x512x512 and 64x1x256x256, for the
  whole policy (colour on: a partial-sum launch + the apply launch, 3 passes over the images) and for translation,cutout (one
  launch, 2 passes), as microseconds and achieved GB/s next to a torch copy of the same tensor measured in the same process.
batch: the WGAN batch of bench.py's headline configuration (256x256, bs 32, fp16, RMSE, clip 0.01, critic on a side stream,
  inputs resident) with and without the policy, critic-only batches and batches with a generator update apart, the two steps
  alternating in one process so both see the same clocks. Wall time per batch over runs of --batches batches between two
  synchronisations (the overlapped step has no single stream to put events on).
usage: tools/time_diffaug.py [--what kernels|batch|all] [--reps 200] [--batches 40] [--rounds 5] [--policy color,translation,cutout]"""
import argparse
import json
import os
import statistics
import sys
import time

R = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, R)
import torch  # noqa: E402
import gan_inpainting_amd  # noqa: E402,F401
from gan_inpainting_amd import backend as B  # noqa: E402
from gan_inpainting_amd import optim, trainer  # noqa: E402
from gan_inpainting_amd.lib.models import augment, networks  # noqa: E402


def timed(fn, reps, warmup=20):
    """Median / min microseconds of fn() over `reps` single timings."""
    out = []
    for it in range(warmup + reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        if it >= warmup:
            out.append(e0.elapsed_time(e1) * 1e3)
    return statistics.median(out), min(out)


def kernels(a):
    for hw in (512, 256):
        n = 64
        x = torch.rand((n, 1, hw, hw), generator=torch.Generator().manual_seed(1)).cuda()
        y = torch.empty_like(x)
        nbytes = x.numel() * 4
        med, lo = timed(lambda: y.copy_(x), a.reps)
        copy_gbs = 2 * nbytes / med / 1e3
        print(json.dumps({"what": "copy", "shape": [n, 1, hw, hw], "median_us": round(med, 1), "min_us": round(lo, 1),
                          "GBps": round(copy_gbs, 1)}), flush=True)
        for policy in (a.policy, "translation,cutout"):
            aug = augment.DiffAugment(policy, seed=1)
            passes = 3 if aug.bits & 1 else 2        # colour: the images are read twice and written once
            for name, fn in (("forward", aug.into), ("adjoint", aug.adjoint_into)):
                med, lo = timed(lambda: fn(x, y, 3, 0), a.reps)
                print(json.dumps({"what": name, "policy": aug.policy, "shape": [n, 1, hw, hw], "median_us": round(med, 1),
                                  "min_us": round(lo, 1), "passes": passes, "GBps": round(passes * nbytes / med / 1e3, 1),
                                  "of_copy": round(passes * nbytes / med / 1e3 / copy_gbs, 3)}), flush=True)


def make_step(policy, hw, bs, dtype):
    torch.manual_seed(1234)
    G = networks.get_network("generator", "unet", dtype=dtype).cuda()
    torch.manual_seed(4321)
    D = networks.PatchGANDiscriminator(sigmoid=False, image_size=hw, dtype=dtype).cuda()
    kw = {"diffaug": policy} if policy else {}
    step = trainer.WGANStep(G, D, optim.RMSprop(G.parameters(), lr=0.00005), optim.RMSprop(D.parameters(), lr=0.00005), recon="rmse",
                            clip=0.01, overlap=True, **kw)
    step.inputs_resident = True
    return step


def batch(a):
    hw, bs = 256, 32
    gen = torch.Generator().manual_seed(7)
    data = []
    for _ in range(4):
        g = torch.rand((bs, 1, hw, hw), generator=gen)
        m = torch.zeros((bs, 1, hw, hw))
        m[:, :, hw // 4:hw // 2, hw // 4:3 * hw // 4] = 1.0
        data.append((g.cuda(), m.cuda()))
    steps = {"off": make_step(None, hw, bs, "fp16"), "on": make_step(a.policy, hw, bs, "fp16")}
    if not hasattr(B.lib(), "gi_diffaug_apply"):      # a build from before the feature, named through GI_LIB_PATH
        del steps["on"]
    times = {(k, u): [] for k in steps for u in (False, True)}
    for rnd in range(a.rounds + 1):
        for upd in (False, True):
            for k, step in steps.items():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for it in range(a.batches):
                    g, m = data[it % 4]
                    step(g, m, upd)
                torch.cuda.synchronize()
                if rnd > 0:      # the first round warms up
                    times[(k, upd)].append((time.perf_counter() - t0) / a.batches * 1e6)
    for (k, upd), t in times.items():
        print(json.dumps({"what": "wgan batch", "diffaug": a.policy if k == "on" else None, "generator_update": upd, "hw": hw, "bs": bs,
                          "dtype": "fp16", "rounds": len(t), "batches": a.batches, "median_us": round(statistics.median(t), 1),
                          "min_us": round(min(t), 1), "max_us": round(max(t), 1), "library": B.LIB_PATH}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--what", choices=["kernels", "batch", "all"], default="all")
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--batches", type=int, default=40)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--policy", default="color,translation,cutout")
    a = ap.parse_args()
    if a.what in ("kernels", "all"):
        kernels(a)
    if a.what in ("batch", "all"):
        batch(a)


if __name__ == "__main__":
    main()
