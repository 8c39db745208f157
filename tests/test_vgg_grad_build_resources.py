"""The kernels of the VGG-19 backward (csrc/vgg.hip: seeds, dense Gram difference; csrc/vggtrunk.hip: scale, fused activation backward,
first-layer adjoint, transposed weight packing, read-back) are in the build record (csrc/build/resources.txt) and use no scratch."""
import os

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RES = os.path.join(ROOT, "gan-inpainting_amd", "csrc", "build", "resources.txt")
# mangled template arguments: Lb1 / Lb0 = true / false (seed: store / maximum only; activation backward: un-pooling / plain)
INSTANCES = ("vgg_seed_kernelILb0E", "vgg_seed_kernelILb1E")
OTHERS = ("gram_delta_kernel",)
# moved to the trunk file: vgg_act_bwd_kernel -> act_bwd_kernel, vgg_scale_kernel -> seed_scale_kernel, vgg_conv1_adjoint_kernel ->
# conv1_adjoint_kernel; pack3x3_t_kernel and nhwc_to_nchw_unscale_kernel kept their names
TRUNK = ("act_bwd_kernelILb0E", "act_bwd_kernelILb1E", "pack3x3_t_kernel", "seed_scale_kernel", "conv1_adjoint_kernel",
         "nhwc_to_nchw_unscale_kernel")


def test_vgg_grad_kernels_are_recorded_without_scratch():
    assert os.path.exists(RES), "no build record: build() always writes csrc/build/resources.txt, so the build did not run or failed"
    rows = [line.rstrip("\n").split("\t") for line in open(RES)]
    for src, wanted in (("vgg", INSTANCES + OTHERS), ("vggtrunk", TRUNK)):
        got = [(name, dict(x.split("=", 1) for x in kv)) for s, name, *kv in rows if s == src]
        assert got, f"csrc/{src}.hip is missing from the build record"
        for k in wanted:
            assert any(k in name for name, _ in got), f"{k} missing from the record: {[n for n, _ in got]}"
        bad = [(name, d.get("scratch")) for name, d in got if d.get("scratch") != "0"]
        assert not bad, f"kernels with scratch: {bad}"
