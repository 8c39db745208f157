"""The LPIPS kernels (csrc/lpips.hip: first layer, fold, the tap kernel's eight instances, finish; csrc/vggtrunk.hip: weight packing,
read-back) are in the build record (csrc/build/resources.txt) and use no scratch."""
import os

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RES = os.path.join(ROOT, "gan-inpainting_amd", "csrc", "build", "resources.txt")
# mangled template arguments: Li<N>E = lanes per pixel (C / 8), Lb1 / Lb0 = with / without the fused 2x2 max pool
INSTANCES = tuple(f"lpips_tap_kernelILi{lpp}ELb{p}E" for lpp in (8, 16, 32, 64) for p in (0, 1))
OTHERS = ("lpips_conv1_mfma_kernel", "lpips_fold_kernel", "lpips_finish_kernel")
# moved to the trunk file: lpips_pack3x3_kernel -> pack3x3_kernel, lpips_nhwc_to_nchw_kernel -> nhwc_to_nchw_kernel
TRUNK = ("pack3x3_kernel", "nhwc_to_nchw_kernel")


def test_lpips_kernels_are_recorded_without_scratch():
    assert os.path.exists(RES), "no build record: build() always writes csrc/build/resources.txt, so the build did not run or failed"
    rows = [line.rstrip("\n").split("\t") for line in open(RES)]
    for src, wanted in (("lpips", INSTANCES + OTHERS), ("vggtrunk", TRUNK)):
        got = [(name, dict(x.split("=", 1) for x in kv)) for s, name, *kv in rows if s == src]
        assert got, f"csrc/{src}.hip is missing from the build record"
        for k in wanted:
            assert any(k in name for name, _ in got), f"{k} missing from the record: {[n for n, _ in got]}"
        bad = [(name, d.get("scratch")) for name, d in got if d.get("scratch") != "0"]
        assert not bad, f"kernels with scratch: {bad}"
