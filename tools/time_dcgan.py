#!/usr/bin/env python3
"""DCGANDiscriminator (-d dcgan) timing on one MI355X, fp16 and fp32.

  python tools/time_dcgan.py [--dtype fp16,fp32] [--reps 10] [--batches 20] [--out FILE.json]
      passes at n = 64 (one stacked bs-32 [real | fake] pair): forward, full backward, frozen backward (dx only);
      one MinimaxStep batch at 128x128, bs = 32, -d dcgan (U-Net generator): ms and images/s; fp16: updates the overflow
      guard skipped in `--batches` batches at the steps' loss scale (64 n).
  python tools/time_dcgan.py --trace kernel_trace.csv
      per layer from a `rocprofv3 --kernel-trace` of the first form: average us and TFLOP/s of every DCGAN GEMM, keyed by
      operation and launch grid (the grid names the layer), and the time-weighted rate of all convolution GEMMs.
Times are HIP-event medians after warm-up."""
import argparse
import csv
import json
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CH = [1, 128, 256, 512, 1024]
HI = [128, 63, 30, 14]
HP = [63, 30, 14, 6]
PEAK_FP16 = 2.5e15


def _events(fn, reps):
    import torch
    for _ in range(3):
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


def conv_flops(n):
    """per pass at n images: forward (all four convolutions), input gradient (convs 1..3 as GEMMs, conv 0's direct kernel
    not counted), weight gradient."""
    fwd = sum(2.0 * n * (2 * HP[l]) ** 2 * CH[l + 1] * 25 * CH[l] for l in range(4))
    dgrad = sum(2.0 * n * HI[l] ** 2 * CH[l] * 25 * CH[l + 1] for l in range(1, 4))
    return fwd, dgrad, fwd


def time_passes(dtype, reps):
    import torch
    import gan_inpainting_amd  # noqa: F401
    from gan_inpainting_amd.lib.models import networks
    torch.manual_seed(0)
    d = networks.DCGANDiscriminator(dtype=dtype).to("cuda").train()
    n = 64
    x = torch.rand(n, 1, 128, 128, device="cuda")
    dy = torch.full((2 * n, 1), 1.0 / (2 * n), device="cuda")
    out = {}
    out["forward_ms"] = _events(lambda: d._forward_raw(x), reps)

    def fb(need_dx, need_w):
        y, s, g = d._forward_raw(x)
        d._backward_raw(s, g, dy, need_dx, need_w)
    out["forward_backward_ms"] = _events(lambda: fb(False, True), reps)
    out["forward_frozen_backward_ms"] = _events(lambda: fb(True, False), reps)
    out["backward_ms"] = out["forward_backward_ms"] - out["forward_ms"]
    out["frozen_backward_ms"] = out["forward_frozen_backward_ms"] - out["forward_ms"]
    f, dg, wg = conv_flops(n)
    out["conv_flop_forward"], out["conv_flop_backward"] = f, dg + wg
    return out


def time_step(dtype, reps, batches):
    import torch
    import gan_inpainting_amd  # noqa: F401
    from gan_inpainting_amd import optim, trainer
    from gan_inpainting_amd.lib.models import networks
    torch.manual_seed(0)
    G = networks.get_network("generator", "unet", dtype=dtype).to("cuda")
    D = networks.get_network("discriminator", "dcgan", dtype=dtype).to("cuda")
    oG = optim.Adam(G.parameters(), lr=2e-4, betas=(0.5, 0.999))
    oD = optim.Adam(D.parameters(), lr=2e-4, betas=(0.5, 0.999))
    step = trainer.MinimaxStep(G, D, oG, oD, recon="l1")
    bs = 32
    g = torch.rand(bs, 1, 128, 128, device="cuda")
    m = (torch.rand(bs, 1, 128, 128, device="cuda") > 0.75).float()
    ms = _events(lambda: step(g, m), reps)
    out = dict(step_ms=ms, images_per_s=bs / (ms * 1e-3), d_loss_scale=D._loss_scale)
    if dtype == "fp16":
        skipped_d = oD.poll_skipped()   # the timing loop's updates
        for i in range(batches):
            gi = torch.rand(bs, 1, 128, 128, device="cuda")
            mi = (torch.rand(bs, 1, 128, 128, device="cuda") > 0.75).float()
            step(gi, mi)
        torch.cuda.synchronize()
        out["overflow_skipped_D"] = oD.poll_skipped() + skipped_d
        out["overflow_skipped_G"] = oG.poll_skipped()
        out["overflow_batches"] = batches + reps + 3
    L = {k: float(v) for k, v in step.L.items()}
    out["last_losses"] = L
    return out


# ---- trace ------------------------------------------------------------------------------------------------------------
def _layer(op, gx, gy):
    """(label, flop per launch) of a dc_gemm_kernel launch from its operation and workgroup grid (64 x 64 tiles)."""
    M = gx * 64
    if op == "ConvFwdOp":
        l = {2: 0, 4: 1, 8: 2, 16: 3}[gy]
        return f"conv{l} forward", 2.0 * M * CH[l + 1] * 25 * CH[l]
    if op == "ConvDgradOp":
        l = {2: 1, 4: 2, 8: 3}[gy]
        return f"conv{l} input gradient", 2.0 * M * CH[l] * 25 * CH[l + 1]
    if op == "ConvWgradOp":
        l = {2: 0, 4: 1, 8: 2, 16: 3}[gx]
        return f"conv{l} weight gradient", None   # K (pixels) is not in the grid: the caller scales by n
    return f"{op} grid {gx}x{gy}", None


def trace(path, n):
    rows = list(csv.DictReader(open(path)))
    agg = {}
    for r in rows:
        name = r["Kernel_Name"]
        dur = (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) * 1e-9
        if "dc_conv0_dgrad_kernel" in name:   # conv 0's input gradient (direct kernel, one output channel)
            imgs = min(n, int(r["Grid_Size_X"]) // (128 * 128))   # one thread per pixel, grid capped at 4096 x 256 (n = 64)
            a = agg.setdefault("conv0 input gradient (direct)", [0, 0.0, 0.0])
            a[0] += 1; a[1] += dur; a[2] += 2.0 * imgs * 128 * 128 * 25 * 128
            continue
        m = re.search(r"dc_(gemm|splitk_reduce)_kernel.*?((?:Conv|Lin)\w*?Op)", name)   # mangled or demangled names
        if not m:
            continue
        kind, op = m.group(1), m.group(2)
        wg = int(r["Workgroup_Size_X"])
        gx, gy = int(r["Grid_Size_X"]) // wg, int(r["Grid_Size_Y"]) // int(r["Workgroup_Size_Y"])
        if kind == "gemm":
            label, flop = _layer(op, gx, gy)
            if op == "ConvWgradOp":
                l = int(label[4])
                flop = 2.0 * n * (2 * HP[l]) ** 2 * CH[l + 1] * 25 * CH[l]
        else:
            label, flop = f"{op} split-K reduce", 0.0
        a = agg.setdefault(label, [0, 0.0, 0.0])
        a[0] += 1
        a[1] += dur
        a[2] += flop or 0.0
    print(f"{'launch':34s} {'calls':>6s} {'avg us':>9s} {'TFLOP/s':>9s}")
    conv_t = conv_f = 0.0
    for k in sorted(agg):
        c, t, f = agg[k]
        print(f"{k:34s} {c:6d} {t / c * 1e6:9.1f} {f / t / 1e12 if f else 0:9.1f}")
        if k.startswith("conv") or "ConvWgradOp" in k:
            conv_t += t
            conv_f += f
    if conv_t:
        r = conv_f / conv_t
        print(f"convolution kernels (GEMMs, their split-K reduction, conv 0's direct input gradient), time-weighted: {r / 1e12:.1f} TFLOP/s "
              f"= {r / PEAK_FP16:.3f} of 2.5 PFLOP/s")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dtype", default="fp16,fp32")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--batches", type=int, default=20)
    ap.add_argument("--out", default="")
    ap.add_argument("--trace", default="")
    ap.add_argument("--n", type=int, default=64, help="--trace: images per pass of the traced run (weight-gradient FLOP)")
    ap.add_argument("--passes-only", action="store_true")
    a = ap.parse_args()
    if a.trace:
        trace(a.trace, a.n)
        return
    res = {}
    for dt in a.dtype.split(","):
        p = time_passes(dt, a.reps)
        f_tot = p["conv_flop_forward"] + p["conv_flop_backward"]
        print(f"{dt} n=64: forward {p['forward_ms']:.2f} ms ({p['conv_flop_forward'] / p['forward_ms'] / 1e9:.0f} TFLOP/s conv-equivalent), "
              f"backward {p['backward_ms']:.2f} ms, frozen backward {p['frozen_backward_ms']:.2f} ms; conv FLOP fwd+bwd {f_tot / 1e12:.2f} T")
        res[dt] = dict(passes_n64=p)
        if not a.passes_only:
            s = time_step(dt, a.reps, a.batches)
            print(f"{dt} MinimaxStep 128x128 bs=32 -d dcgan: {s['step_ms']:.2f} ms/batch, {s['images_per_s']:.0f} images/s"
                  + (f"; overflow-skipped updates D {s['overflow_skipped_D']} / G {s['overflow_skipped_G']} of {s['overflow_batches']} batches "
                     f"(D loss scale {s['d_loss_scale']:g})" if dt == "fp16" else ""))
            res[dt]["minimax_bs32"] = s
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        json.dump(res, open(a.out, "w"), indent=1)


if __name__ == "__main__":
    main()
