#!/usr/bin/env python3
"""Times what resumable training and the EMA generator add.

    python tools/time_resume.py [--launches 200] [--out FILE.json]

1. gi_ema_update over the headline generator's 41,822,849 parameters: HIP events around every single launch after a warm-up,
   median and 10th / 90th percentile in microseconds; the same for a device-to-device copy of a buffer of that size. The pass
   moves 12 bytes per element (reads ema and p, writes ema), the copy 8: both are reported as bytes per second, and the pass as
   a fraction of the copy's rate. tools/copy_bw.py measures the copy rate over a range of sizes on the same device.
2. Writing and loading last_state.pt for the headline configuration (wgan_rmse, 256 x 256, batch 32, fp16, RMSprop): one step
   so that every lazily created object exists, then the save and the load of the plugin loop, wall clock around a device
   synchronise, and the file's size. A GPU is required; nothing falls back."""
import argparse
import json
import logging
import os
import statistics
import sys
import tempfile
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from tools.maskgen_time import event_times_us, summary  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--launches", type=int, default=200)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("time_resume.py needs the GPU")
    import gan_inpainting_amd  # noqa: F401
    from gan_inpainting_amd import backend as B
    from gan_inpainting_amd import optim, trainer
    from gan_inpainting_amd.experiment_list import _common as C
    from gan_inpainting_amd.lib.models import networks

    dev = torch.device("cuda", 0)
    res = {"device": torch.cuda.get_device_name(0)}
    count = 41822849
    lib, ctx = B.lib(), B.get_ctx(dev)
    for off_e, off_p in ((0, 0), (1, 1), (0, 1)):
        ema = torch.randn(count + 4, device=dev)[off_e: off_e + count]
        p = torch.randn(count + 4, device=dev)[off_p: off_p + count]
        r = summary(event_times_us(lambda: B.check(lib.gi_ema_update(ctx, B.ptr(ema), B.ptr(p), count, 0.999, None)), args.launches))
        cp = summary(event_times_us(lambda: ema.copy_(p), args.launches))
        r.update(float_offsets=[off_e, off_p], bytes=12 * count, bytes_per_s=12 * count / (r["median_us"] * 1e-6),
                 copy_median_us=cp["median_us"], copy_bytes_per_s=8 * count / (cp["median_us"] * 1e-6))
        r["fraction_of_copy_rate"] = r["bytes_per_s"] / r["copy_bytes_per_s"]
        res.setdefault("ema_update", []).append(r)
        print(f"gi_ema_update {count} floats, float offsets ({off_e},{off_p}): median {r['median_us']:.1f} us  p10 {r['p10_us']:.1f}  p90 {r['p90_us']:.1f}"
              f"  {r['bytes_per_s'] / 1e12:.2f} TB/s | copy {cp['median_us']:.1f} us {r['copy_bytes_per_s'] / 1e12:.2f} TB/s | "
              f"{r['fraction_of_copy_rate']:.2f} of the copy rate")
        del ema, p

    # the headline configuration's training state
    torch.manual_seed(0)
    state = {"imagedim": 256, "batchsize": 32, "dtype": "fp16", "title": "wgan_rmse", "ema_decay": 0.999}
    G, (D,) = C.build_networks(state, dev, n_disc=1, sigmoid=False)
    oG, oD = C.make_optimizers("rmsprop", G, D.parameters())
    step = trainer.WGANStep(G, D, oG, oD, recon="rmse", clip=0.01, overlap=True)
    step.ema_G = optim.EMA(G, 0.999)
    ground = torch.rand(32, 1, 256, 256, device=dev)
    mask = torch.zeros_like(ground)
    mask[:, :, 64:160, 64:160] = 1.0
    step(ground, mask, True)
    logger = logging.getLogger("time_resume")
    with tempfile.TemporaryDirectory() as d:
        path = os.path.join(d, "last_state.pt")
        saves, loads = [], []
        for _ in range(3):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            C._save_training_state(path, state, 1, [], [], {"G_iter_count": 1}, {}, dev, G, [D], step, True)
            saves.append(time.perf_counter() - t0)
            t0 = time.perf_counter()
            C._load_training_state(path, state, logger, {}, {}, dev, G, [D], step)
            torch.cuda.synchronize()
            loads.append(time.perf_counter() - t0)
        res["state"] = {"save_s": statistics.median(saves), "load_s": statistics.median(loads), "file_bytes": os.path.getsize(path),
                        "what": "wgan_rmse 256x256 batch 32 fp16, RMSprop, EMA on: median of 3"}
    print(f"last_state.pt: save {res['state']['save_s']:.2f} s, load {res['state']['load_s']:.2f} s, {res['state']['file_bytes'] / 2 ** 20:.0f} MiB")
    if args.out:
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
