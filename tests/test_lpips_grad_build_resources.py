"""The kernels of the LPIPS backward (csrc/lpips.hip: the seed kernel's eight instances; csrc/vggtrunk.hip: scale, activation backward
with and without un-pool, transposed pack, first-layer adjoint, de-scaling read-back) are in the build record (csrc/build/resources.txt)
and use no scratch."""
import os

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RES = os.path.join(ROOT, "gan-inpainting_amd", "csrc", "build", "resources.txt")
# mangled template arguments: Li<N>E = lanes per pixel (C / 8), Lb1 / Lb0 = the store / the maximum pass; act_bwd: with / without un-pool
INSTANCES = tuple(f"lpips_seed_kernelILi{lpp}ELb{p}E" for lpp in (8, 16, 32, 64) for p in (0, 1))
# moved to the trunk file, each without its lpips_ prefix: lpips_act_bwd_kernel -> act_bwd_kernel, lpips_scale_kernel -> seed_scale_kernel,
# lpips_pack3x3_t_kernel -> pack3x3_t_kernel, lpips_conv1_adjoint_kernel -> conv1_adjoint_kernel, lpips_nhwc_to_nchw_unscale_kernel ->
# nhwc_to_nchw_unscale_kernel
TRUNK = ("act_bwd_kernelILb0E", "act_bwd_kernelILb1E", "seed_scale_kernel", "pack3x3_t_kernel", "conv1_adjoint_kernel",
         "nhwc_to_nchw_unscale_kernel")


def test_lpips_grad_kernels_are_recorded_without_scratch():
    assert os.path.exists(RES), "no build record: build() always writes csrc/build/resources.txt, so the build did not run or failed"
    rows = [line.rstrip("\n").split("\t") for line in open(RES)]
    for src, wanted in (("lpips", INSTANCES), ("vggtrunk", TRUNK)):
        got = [(name, dict(x.split("=", 1) for x in kv)) for s, name, *kv in rows if s == src]
        for k in wanted:
            hit = [d for name, d in got if k in name]
            assert hit, f"{k} missing from the record: {[n for n, _ in got]}"
            assert all(d.get("scratch") == "0" for d in hit), f"{k} uses scratch: {hit}"
