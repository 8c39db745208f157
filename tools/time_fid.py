#!/usr/bin/env python3
"""FID path timing on one MI355X.

  python tools/time_fid.py [--dtype fp16,fp32] [--batch 50] [--reps 10] [--out FILE.json] [--cpu-images 8]
      images/s of gi_inception_features at 128x128 inputs (batch 50 = the reference's FID batch), HIP-event medians after warm-up;
      wall time of one calculate_metric pass over the synthetic loader with and without FID;
      the same forward in PyTorch on the host CPU (tests/inception_ref.py in fp32, 16 threads) for comparison.
  rocprofv3 --kernel-trace --output-format csv -d DIR -- python tools/time_fid.py --forwards 12 --dtype fp16
      nothing but 12 forwards of one compute type, to be traced;
  python tools/time_fid.py --trace DIR/.../*_kernel_trace.csv [--batch 50] [--out FILE.json]
      the per-layer table from that trace: the convolution launches of a forward are in program order, so launch i of every
      94 is layer i. Per layer: median and min..max kernel time over the traced forwards (the first two dropped), algorithmic
      FLOP, TFLOP/s and share of the dense fp16 MFMA peak; then the other kernels of the forward by name."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "gan-inpainting_amd"))

PEAK_FP16 = 2.5e15
PEAK_FP32 = 157.3e12


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


def conv_table():
    """[(name, flop per image, output pixels, cout, K)] at the network's fixed 299x299 input."""
    import inception_ref as R
    import torch
    sizes = {}
    # output map of every convolution from a shape-only run of the restatement on the meta device, keyed by the weight tensor
    orig = torch.nn.functional.conv2d
    rows = []
    ident = {}
    T = {k: torch.empty(s, device="meta") for k, s in R.keys_and_shapes()}
    for k, v in T.items():
        ident[id(v)] = k

    def spy2(a, w, b=None, **kw):
        out = orig(a, w, b, **kw)
        sizes[ident[id(w)][:-len(".conv.weight")]] = out.shape[2] * out.shape[3]
        return out
    torch.nn.functional.conv2d = spy2
    try:
        R.forward(T, torch.empty(1, 3, 64, 64, device="meta"))
    finally:
        torch.nn.functional.conv2d = orig
    for name, cin, cout, (kh, kw), _, _ in R.CONVS:
        px = sizes[name]
        rows.append((name, 2.0 * px * cout * cin * kh * kw, px, cout, cin * kh * kw))
    return rows


def trace(path, batch, out):
    import csv
    import re
    rows = sorted(csv.DictReader(open(path)), key=lambda r: int(r["Start_Timestamp"]))
    gemm, other = [], {}
    for r in rows:
        name = r["Kernel_Name"]
        us = (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) * 1e-3
        if "inc_gemm_kernel" in name:
            gemm.append((name, us))
        elif "inc_" in name and "fold_pack" not in name:
            other.setdefault(re.search(r"inc_\w+(<[^>]*>)?", name).group(0), []).append(us)
    table = conv_table()
    nl = len(table)
    assert gemm and len(gemm) % nl == 0, f"{len(gemm)} convolution launches are not a multiple of {nl}"
    fwd = len(gemm) // nl
    drop = 2 if fwd > 4 else 0
    f16 = any(("Float16" in n or "DF16" in n) for n, _ in gemm)
    print(f"{fwd} traced forwards ({drop} dropped as warm-up), batch {batch}, {'fp16' if f16 else 'fp32'}")
    print(f"{'layer':28s} {'M':>8s} {'N':>5s} {'K':>6s} {'median us':>10s} {'min':>8s} {'max':>8s} {'TFLOP/s':>9s} {'of fp16 peak':>13s}")
    layers, tot_us, tot_flop = [], 0.0, 0.0
    for i, (name, flop, px, cout, K) in enumerate(table):
        ts = sorted(gemm[f * nl + i][1] for f in range(drop, fwd))
        med = ts[len(ts) // 2]
        r = flop * batch / (med * 1e-6)
        layers.append(dict(name=name, M=px * batch, N=cout, K=K, median_us=med, min_us=ts[0], max_us=ts[-1], tflops=r / 1e12,
                           share_of_fp16_peak=r / PEAK_FP16))
        tot_us += med
        tot_flop += flop * batch
        print(f"{name:28s} {px * batch:8d} {cout:5d} {K:6d} {med:10.1f} {ts[0]:8.1f} {ts[-1]:8.1f} {r / 1e12:9.1f} {r / PEAK_FP16:13.4f}")
    rate = tot_flop / (tot_us * 1e-6)
    print(f"all {nl} convolution kernels: {tot_us:.0f} us per forward, {rate / 1e12:.1f} TFLOP/s time-weighted = {rate / PEAK_FP16:.4f} of 2.5 PFLOP/s")
    others = {}
    for k, v in sorted(other.items()):
        per_fwd = sum(v) / fwd
        others[k] = dict(launches_per_forward=len(v) / fwd, us_per_forward=per_fwd)
        print(f"{k[:90]:90s} {len(v) / fwd:5.1f} launches, {per_fwd:8.1f} us per forward")
    if out:
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
        json.dump(dict(batch=batch, dtype="fp16" if f16 else "fp32", forwards=fwd, conv_us_per_forward=tot_us, conv_tflops=rate / 1e12,
                       conv_share_of_fp16_peak=rate / PEAK_FP16, layers=layers, other_kernels=others), open(out, "w"), indent=1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dtype", default="fp16,fp32")
    ap.add_argument("--batch", type=int, default=50)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", default="")
    ap.add_argument("--forwards", type=int, default=0, help="run only this many forwards of the first --dtype (for a kernel trace)")
    ap.add_argument("--trace", default="", help="kernel-trace CSV of a --forwards run: print the per-layer table")
    ap.add_argument("--cpu-images", type=int, default=8)
    a = ap.parse_args()
    if a.trace:
        trace(a.trace, a.batch, a.out)
        return
    import torch
    import gan_inpainting_amd  # noqa: F401
    import inception_ref as R
    from gan_inpainting_amd.lib.fid import fid_score
    from gan_inpainting_amd.lib.fid.inception import InceptionV3
    from gan_inpainting_amd.lib.models import evaluate, networks
    if not torch.cuda.is_available():
        raise SystemExit("time_fid.py measures on the GPU; none is visible")
    P = R.make_params(20260)
    sd = {k: torch.from_numpy(v) for k, v in P.items()}
    table = conv_table()
    flop_img = sum(r[1] for r in table)
    if a.forwards:
        dt = a.dtype.split(",")[0]
        m = InceptionV3([3], dtype=dt, max_batch=a.batch)
        m.load_state_dict(sd)
        m = m.cuda()
        xf = torch.rand(a.batch, 1, 128, 128, device="cuda")
        for _ in range(a.forwards):
            m.features(xf)
            torch.cuda.synchronize()
        return
    res = {"flop_per_image": flop_img, "batch": a.batch}
    x = torch.rand(a.batch, 1, 128, 128, device="cuda")
    for dt in a.dtype.split(","):
        m = InceptionV3([3], dtype=dt, max_batch=a.batch)
        m.load_state_dict(sd)
        m = m.cuda()
        ms = _events(lambda: m.features(x), a.reps)
        rate = flop_img * a.batch / (ms * 1e-3)
        peak = PEAK_FP16 if dt == "fp16" else PEAK_FP32
        print(f"{dt}: gi_inception_features batch {a.batch} at 128x128: {ms:.2f} ms, {a.batch / (ms * 1e-3):.0f} images/s, "
              f"{rate / 1e12:.1f} TFLOP/s convolution-equivalent = {rate / peak:.3f} of the {dt} MFMA peak")
        res[dt] = dict(features_ms=ms, images_per_s=a.batch / (ms * 1e-3), tflops=rate / 1e12, share_of_peak=rate / peak)
        if dt == "fp16":
            # one evaluation pass over the synthetic loader (256 images of 128x128, batch 32), with and without FID
            from gan_inpainting_amd.train import SyntheticInpainting
            loader = [b for b in torch.utils.data.DataLoader(SyntheticInpainting(256, 128, 7), batch_size=32)]
            torch.manual_seed(0)
            G = networks.get_network("generator", "unet", dtype="fp16").to("cuda")
            truth = fid_score.calculate_activation_statistics((b[0] for b in loader), m, quantize=True)
            for label, kw in (("without FID", {}), ("with FID", dict(fid_stats=truth, inception_model=m))):
                evaluate.calculate_metric(torch.device("cuda"), loader, G, **kw)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                met = evaluate.calculate_metric(torch.device("cuda"), loader, G, **kw)
                torch.cuda.synchronize()
                dtm = time.perf_counter() - t0
                print(f"calculate_metric over 256 synthetic 128x128 images {label}: {dtm * 1e3:.1f} ms (fid {met['fid']})")
                res[dt]["calculate_metric_ms_" + label.replace(" ", "_")] = dtm * 1e3
        del m
    # the same forward on the host CPU: the restatement in fp32, 16 threads
    torch.set_num_threads(16)
    T = R.to_torch(P, torch.float32)
    xc = x[:a.cpu_images].cpu()
    with torch.no_grad():
        R.forward(T, xc[:1])
        t0 = time.perf_counter()
        R.forward(T, xc)
        dtc = time.perf_counter() - t0
    print(f"host CPU (PyTorch fp32, 16 threads): {a.cpu_images} images in {dtc:.2f} s = {a.cpu_images / dtc:.1f} images/s")
    res["cpu_baseline"] = dict(images=a.cpu_images, seconds=dtc, images_per_s=a.cpu_images / dtc, threads=16)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        json.dump(res, open(a.out, "w"), indent=1)


if __name__ == "__main__":
    main()
