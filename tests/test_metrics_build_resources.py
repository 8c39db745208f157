"""Every kernel of csrc/ssim.hip, csrc/evalmetrics.hip and csrc/auxloss.hip is in the build record (csrc/build/resources.txt) and uses
no scratch. ce_grad_kernel<16> keeps a per-lane v[16] that turns into scratch if one of its unrolls ever fails, seg_count_kernel<16>
keeps 48 counters per lane, and ssim11_kernel runs 320 threads = 5 waves per workgroup and is meant to have several workgroups on a
CU: 102 = floor(512 / 5) registers per lane is the ceiling of the 512-entry file of a SIMD shared by five waves (80 in the record now).
None of this shows in a parity test: a spilling kernel still computes the right numbers."""
import os

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RES = os.path.join(ROOT, "gan-inpainting_amd", "csrc", "build", "resources.txt")
CE_K = (2, 3, 4, 8, 16)
SEG_NU = (4, 8, 16)
EXPECTED = {
    "ssim": ["ssim11_kernel", "ssim_tile_kernelILi16ELi64E", "ssim_tile_kernelILi8ELi32E", "ssim_finish_kernel", "ssim_mean_kernel"],
    "evalmetrics": ["eval_recon_partial_kernel", "eval_recon_final_kernel", "seg_final_kernel"] + [f"seg_count_kernelILi{u}E" for u in SEG_NU],
    "auxloss": ["tv_partial_kernel", "tv_final_kernel", "tv_grad_kernel", "ce_final_kernel"]
               + [f"ce_partial_kernelILi{k}E" for k in CE_K] + [f"ce_grad_kernelILi{k}E" for k in CE_K],
}
SSIM11_VGPR = 102     # 512 VGPRs per SIMD lane / 5 waves


def _record(src):
    assert os.path.exists(RES), "no build record: build() always writes csrc/build/resources.txt, so the build did not run or failed"
    rows = [line.rstrip("\n").split("\t") for line in open(RES)]
    return [(name, dict(x.split("=", 1) for x in kv)) for s, name, *kv in rows if s == src]


def test_every_metric_kernel_is_recorded_without_scratch():
    for src, kernels in EXPECTED.items():
        rec = _record(src)
        assert rec, f"csrc/{src}.hip is missing from the build record"
        for k in kernels:
            hits = [d for name, d in rec if k in name]
            assert len(hits) == 1, f"{src}: {k} is in the record {len(hits)} times: {[n for n, _ in rec]}"
        bad = [(name, d.get("scratch")) for name, d in rec if d.get("scratch") != "0"]
        assert not bad, f"{src}: kernels with scratch: {bad}"
        assert len(rec) == len(kernels), f"{src}: the record has kernels this test does not know: {[n for n, _ in rec]}"


def test_ssim11_stays_within_five_waves_per_simd():
    d = [d for name, d in _record("ssim") if "ssim11_kernel" in name]
    assert len(d) == 1 and int(d[0]["vgpr"]) + int(d[0]["agpr"]) <= SSIM11_VGPR, f"ssim11_kernel over {SSIM11_VGPR} VGPRs: {d}"
