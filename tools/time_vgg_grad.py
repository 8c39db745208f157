"""Times the VGG-19 perceptual / style call with and without its backward on the device, 512x512 with 8 pairs by default:
the forward-only `perceptual_and_style` (the yardstick: its code path is unchanged by the backward) and `perceptual_and_style_grad`,
alternating in one process; device events around `reps` back-to-back calls per sample, median over the samples.

    python tools/time_vgg_grad.py [--hw 512] [--n 8] [--samples 9] [--reps 5] [--once]

--once: one warmed call of each, no timing - the body for `rocprofv3 --kernel-trace --stats -d DIR -- python tools/time_vgg_grad.py --once`.
--step: instead, the config-5 training step (WGANPerceptualStep, fp16, two streams, random stand-in networks, synthetic resident
batches) with perceptual_grad off and on, a generator update in EVERY batch (the case in which the flag costs most): images/s.
Prints one JSON line."""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import gan_inpainting_amd  # noqa: F401,E402
from gan_inpainting_amd.lib.models import networks  # noqa: E402


def step_rate(a):
    import functools
    from gan_inpainting_amd import optim, trainer
    res = {}
    g = torch.Generator().manual_seed(1)
    ground = torch.rand((a.n, 1, a.hw, a.hw), generator=g).cuda()
    mask = torch.zeros_like(ground)
    mask[:, :, a.hw // 4: a.hw // 2, a.hw // 4: a.hw // 4 * 3] = 1.0
    labels = torch.randint(0, 4, (a.n, a.hw, a.hw), generator=g).cuda()
    steps = {}
    for flag in (False, True):
        torch.manual_seed(7)
        G = networks.get_network("generator", "unet", dtype="fp16").cuda()
        D = networks.PatchGANDiscriminator(sigmoid=False, image_size=a.hw, dtype="fp16").cuda()
        seg = networks.UnetGenerator(1, 4, 7, ngf=32, norm_layer=functools.partial(torch.nn.BatchNorm2d, affine=True, track_running_stats=True),
                                     use_dropout='False', dtype="fp16").cuda()
        vgg = networks.VGG19Wrapper(max_pairs=a.n, grad=flag).cuda()
        st = trainer.WGANPerceptualStep(G, D, optim.RMSprop(G.parameters(), lr=5e-5), optim.RMSprop(D.parameters(), lr=5e-5), vgg=vgg,
                                        segment_model=seg, clip=0.01, overlap=True, perceptual_grad=flag)
        st.inputs_resident = True
        for _ in range(3):
            st(ground, mask, True, segment=labels)
        st.sync_for_logging()
        torch.cuda.synchronize()
        steps[flag] = st
    ms = {False: [], True: []}
    for _ in range(a.samples):
        for flag, st in steps.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(a.reps):
                st(ground, mask, True, segment=labels)
            st.sync_for_logging()
            e1.record()
            e1.synchronize()
            ms[flag].append(e0.elapsed_time(e1) / a.reps)
    for flag in (False, True):
        res["images_per_s_flag_%s" % ("on" if flag else "off")] = round(a.n / (statistics.median(ms[flag]) * 1e-3), 1)
        res["step_ms_flag_%s" % ("on" if flag else "off")] = round(statistics.median(ms[flag]), 2)
    print(json.dumps({"hw": a.hw, "n": a.n, "samples": a.samples, "reps": a.reps, "g_update": "every batch", **res}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--hw", type=int, default=512)
    ap.add_argument("--n", type=int, default=8)
    ap.add_argument("--samples", type=int, default=9)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--once", action="store_true")
    ap.add_argument("--step", action="store_true")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("time_vgg_grad: no GPU - this script measures on the device only")
    if a.step:
        return step_rate(a)
    torch.manual_seed(3)
    out = torch.rand(a.n, 1, a.hw, a.hw, device="cuda")
    tgt = torch.rand(a.n, 1, a.hw, a.hw, device="cuda")
    vgg = networks.VGG19Wrapper(max_pairs=a.n, grad=True).cuda()
    calls = {"forward": lambda: vgg.perceptual_and_style(out, tgt, 0.01, 0.01),
             "forward+backward": lambda: vgg.perceptual_and_style_grad(out, tgt, 0.01, 0.01)}
    for f in calls.values():          # warm-up: code objects, workspaces, packed weights
        for _ in range(2):
            f()
    torch.cuda.synchronize()
    if a.once:
        for f in calls.values():
            f()
        torch.cuda.synchronize()
        return
    ms = {k: [] for k in calls}
    for _ in range(a.samples):
        for k, f in calls.items():    # alternate the two within every sample
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(a.reps):
                f()
            e1.record()
            e1.synchronize()
            ms[k].append(e0.elapsed_time(e1) / a.reps)
    med = {k: statistics.median(v) for k, v in ms.items()}
    print(json.dumps({"hw": a.hw, "n": a.n, "samples": a.samples, "reps": a.reps,
                      "forward_ms": round(med["forward"], 3), "forward_ms_min_max": [round(min(ms["forward"]), 3), round(max(ms["forward"]), 3)],
                      "forward_backward_ms": round(med["forward+backward"], 3),
                      "forward_backward_ms_min_max": [round(min(ms["forward+backward"]), 3), round(max(ms["forward+backward"]), 3)],
                      "ratio": round(med["forward+backward"] / med["forward"], 3),
                      "grad_workspace_MB": round(sum(w[1].numel() for _, w in vgg._handles.values() if isinstance(w, tuple)) / 1e6, 1)}))


if __name__ == "__main__":
    main()
