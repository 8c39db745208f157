#!/usr/bin/env python3
"""WGAN-GP timing on the GPU (HIP events): the gradient-penalty call alone (PatchGANDiscriminator.gradient_penalty) and the
whole WGAN-GP critic step (trainer.WGANStep, gp_lambda 10, overlap + stacked as the plugins run it), fp16 and fp32 alternated
in one process, at 128x128 bs=16 (BASELINE configs[1]) and 256x256 bs=32.
usage: tools/time_gp.py [--steps 100] [--warmup 10] [--shapes 128x16,256x32] [--dtypes fp16,fp32] [--what gp,step]"""
import argparse
import json
import os
import statistics
import sys

R = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, R)
import torch  # noqa: E402
import gan_inpainting_amd  # noqa: E402,F401
from gan_inpainting_amd import optim, trainer  # noqa: E402
from gan_inpainting_amd.lib.models import networks  # noqa: E402


def batch(n, hw, seed):
    g = torch.Generator().manual_seed(seed)
    ground = torch.rand((n, 1, hw, hw), generator=g)
    mask = torch.zeros((n, 1, hw, hw))
    for i in range(n):
        mask[i, 0, 16 + 3 * i:16 + 3 * i + hw // 3, 24 + 2 * i:24 + 2 * i + hw // 2] = 1.0
    return ground.cuda(), mask.cuda()


def make(kind, dtype, hw, n):
    torch.manual_seed(3)
    D = networks.PatchGANDiscriminator(sigmoid=False, image_size=hw, dtype=dtype).cuda()
    ground, mask = batch(n, hw, 1)
    if kind == "gp":
        fake = (ground * 0.5).contiguous()
        eps = torch.rand(n, device="cuda")
        return lambda: D.gradient_penalty(ground, fake, eps, lam=10.0)
    G = networks.get_network("generator", "unet", dtype=dtype).cuda()
    step = trainer.WGANStep(G, D, optim.RMSprop(G.parameters(), lr=5e-5), optim.RMSprop(D.parameters(), lr=5e-5), recon="l1",
                            gp_lambda=10.0, overlap=True, stacked=True)

    def run():
        step(ground, mask, False)   # critic batch (4 of every 5)
        step.sync_for_logging()
    return run


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--shapes", default="128x16,256x32")
    ap.add_argument("--dtypes", default="fp16,fp32")
    ap.add_argument("--what", default="gp,step")
    a = ap.parse_args()
    shapes = [tuple(int(v) for v in s.split("x")) for s in a.shapes.split(",")]
    dtypes = a.dtypes.split(",")
    for kind in a.what.split(","):
        for hw, n in shapes:
            fns = {dt: make(kind, dt, hw, n) for dt in dtypes}
            times = {dt: [] for dt in dtypes}
            for it in range(a.warmup + a.steps):
                for dt in dtypes:   # alternated: both dtypes see the same clocks / thermal state
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    fns[dt]()
                    e1.record()
                    e1.synchronize()
                    if it >= a.warmup:
                        times[dt].append(e0.elapsed_time(e1) * 1e3)
            for dt in dtypes:
                t = times[dt]
                print(json.dumps({"what": kind, "hw": hw, "n": n, "dtype": dt, "steps": len(t), "median_us": round(statistics.median(t), 1),
                                  "min_us": round(min(t), 1), "max_us": round(max(t), 1)}), flush=True)
            del fns
            torch.cuda.synchronize()


if __name__ == "__main__":
    main()
