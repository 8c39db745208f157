#!/usr/bin/env python3
"""Spectral-norm overhead on the GPU (HIP events): one critic-only batch - the stacked [real | fake] forward with two BatchNorm
populations and its backward with parameter gradients - of a PatchGAN critic with and without spectral_norm=True, alternated in
one process so both see the same clocks. Default: the headline shape, 256x256, stacked n = 64, fp16. With GI_LIB_PATH naming a
build from before the feature only the plain critic runs (A/B of the unchanged path). --only sn|plain: one variant alone, for a
kernel trace (rocprofv3 --kernel-trace --stats -- python tools/time_sn.py --only sn --steps 20).
usage: tools/time_sn.py [--steps 200] [--warmup 20] [--hw 256] [--n 64] [--dtype fp16] [--only sn|plain]"""
import argparse
import json
import os
import statistics
import sys

R = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, R)
import torch  # noqa: E402
import gan_inpainting_amd  # noqa: E402,F401
from gan_inpainting_amd import backend as B  # noqa: E402
from gan_inpainting_amd.lib.models import networks  # noqa: E402


def make(sn, dtype, hw, n):
    torch.manual_seed(3)
    D = networks.PatchGANDiscriminator(sigmoid=False, image_size=hw, dtype=dtype, **({"spectral_norm": True} if sn else {})).cuda().train()
    g = torch.Generator().manual_seed(1)
    x = torch.rand((n, 1, hw, hw), generator=g).cuda()
    dy = torch.cat([torch.full((n // 2, 1), -2.0 / n), torch.full((n // 2, 1), 2.0 / n)]).cuda()

    def run():
        _, slot, gen = D._forward_raw(x, bn_groups=2)
        D._backward_raw(slot, gen, dy, False, True)
    return run


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--hw", type=int, default=256)
    ap.add_argument("--n", type=int, default=64)
    ap.add_argument("--dtype", default="fp16")
    ap.add_argument("--only", choices=["sn", "plain"], default=None)
    a = ap.parse_args()
    kinds = [a.only] if a.only else ["plain", "sn"]
    if not hasattr(B.lib(), "gi_patchgan_create_sn"):
        kinds = [k for k in kinds if k == "plain"]
    fns = {k: make(k == "sn", a.dtype, a.hw, a.n) for k in kinds}
    times = {k: [] for k in kinds}
    for it in range(a.warmup + a.steps):
        for k in kinds:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fns[k]()
            e1.record()
            e1.synchronize()
            if it >= a.warmup:
                times[k].append(e0.elapsed_time(e1) * 1e3)
    for k in kinds:
        t = times[k]
        print(json.dumps({"what": "critic batch", "critic": k, "hw": a.hw, "n": a.n, "dtype": a.dtype, "steps": len(t),
                          "median_us": round(statistics.median(t), 1), "min_us": round(min(t), 1), "max_us": round(max(t), 1),
                          "library": B.LIB_PATH}), flush=True)


if __name__ == "__main__":
    main()
