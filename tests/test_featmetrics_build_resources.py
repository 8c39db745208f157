"""The distribution-metric kernels (csrc/featmetrics.hip) are in the build record (csrc/build/resources.txt) and use no scratch."""
import os

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RES = os.path.join(ROOT, "gan-inpainting_amd", "csrc", "build", "resources.txt")
KERNELS = ("feat_gram_kernel", "feat_kid_kernel", "feat_kid_final_kernel", "feat_rownorm_kernel", "feat_knn_tile_kernel",
           "feat_knn_merge_kernel", "feat_member_kernel", "feat_count_kernel")


def test_featmetrics_kernels_have_no_scratch():
    assert os.path.exists(RES), "build() always writes csrc/build/resources.txt"
    rows = [line.rstrip("\n").split("\t") for line in open(RES)]
    fm = [(name, dict(x.split("=", 1) for x in kv)) for src, name, *kv in rows if src == "featmetrics"]
    seen = {k for name, _ in fm for k in KERNELS if k in name}
    assert seen == set(KERNELS), f"featmetrics kernels missing from the record: {set(KERNELS) - seen}"
    bad = [(name, d.get("scratch")) for name, d in fm if d.get("scratch") != "0"]
    assert not bad, f"kernels with scratch: {bad}"
    # the MFMA tile kernels keep their 16 fp64 accumulators per lane in registers at 4 waves per SIMD
    for name, d in fm:
        if any(k in name for k in ("feat_gram_kernel", "feat_kid_kernelE", "feat_knn_tile_kernel", "feat_member_kernel")):
            assert int(d["occ"]) >= 4, (name, d)
