"""CPU tier: which implicit-GEMM kernel serves which layer, asked of gi_debug_igemm_plan (the decision function of
csrc/igemm_plan.hip without a launch: no GPU). tests/golden/igemm_dispatch.json is what the library LAUNCHED per row before the
decision was gathered into one function (tools/dispatch_table.py --launch on an MI355X at the commit named in the file: kernel
name, returned fields, output hash); the plan must name the same kernel and return the same fields for every row. The rows the
single-layer entries cannot produce (folded normalisation, the first layer's weight gradient, VGG-19's 3x3 layers) carry the
expectations of the GPU tests that run them inside the networks."""
import importlib.util
import json
import os

import pytest

import gan_inpainting_amd  # noqa: F401
from gan_inpainting_amd import backend as B

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("dispatch_table", os.path.join(ROOT, "tools", "dispatch_table.py"))
DT = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(DT)

GOLDEN = DT.loads(open(os.path.join(ROOT, "tests", "golden", "igemm_dispatch.json")).read())
F16 = B.GI_F16


def test_golden_table_covers_the_generated_cases():
    assert GOLDEN["how"] == "launch" and len(GOLDEN["commit"]) >= 7
    want = sorted(json.dumps(c, sort_keys=True) for c in DT.cases())
    assert sorted(json.dumps(r["case"], sort_keys=True) for r in GOLDEN["rows"]) == want
    assert len(want) >= 300


def test_plan_names_the_kernel_the_parent_launched_for_every_row():
    bad = []
    for r in GOLDEN["rows"]:
        got = DT.plan_row(B, r["case"])
        for f in DT.FIELDS:
            if got[f] != r[f]:
                bad.append(f"{json.dumps(r['case'], sort_keys=True)}: {f} = {got[f]!r}, launched {r[f]!r}")
    assert not bad, f"{len(bad)} differences:\n" + "\n".join(bad[:20])


def test_plan_leaves_the_options_as_it_found_them():
    before = {k: B.get_option(k) for o in DT.OPTION_SETS for k in o}
    DT.plan_row(B, DT._case(0, 32, 8, 8, 512, 512, opts={"GI_IGEMM7": 0, "GI_IGEMM_FIXUP": 0}))
    assert {k: B.get_option(k) for k in before} == before


# the critic's second layer at its own batch (n = 64; the launched table halves it to keep tensors within 64 MiB), with the names
# tests/test_dispatch_gpu.py asserts there: (case, GI_IGEMM8, kernel)
@pytest.mark.parametrize("mode,cin,cout,use8,kernel", [
    (0, 64, 128, 1, "igemm8<0>"), (0, 64, 128, 0, "igemm6<0,128>"), (1, 128, 64, 1, "igemm8<3>"), (1, 128, 64, 0, "igemm6<3,128>")])
def test_critic_conv2_at_n64(mode, cin, cout, use8, kernel):
    got = DT.plan_row(B, DT._case(mode, 64, 64, 64, cin, cout, opts={"GI_IGEMM8": use8}))
    assert got["rc"] == 0 and got["kernel"] == kernel, got


@pytest.mark.parametrize("name,case,kernel", [("d6", (0, 32, 4, 4, 512, 512), "igemm7<0,64>"), ("u7", (1, 32, 2, 2, 512, 512), "igemm7<1,64>")])
def test_folded_normalisation_at_the_headline_shapes(name, case, kernel):
    """tests/test_options_gpu.py::test_folded_normalisation_is_dispatched_at_the_headline_shapes: with GI_BN_FOLD = 1 at least d6 and
    u7 normalise their own output ('+bn' kernels); with the default they do not. The fold needs the statistics in the accumulators."""
    for fold, epi in ((1, "stat"), (0, "stat"), (1, "none")):
        got = DT.plan_row(B, DT._case(*case, epi=epi, opts={"GI_BN_FOLD": fold}), offered=DT.OFFER_FOLD)
        on = fold == 1 and epi == "stat"
        assert got["rc"] == 0 and got["kernel"] == kernel + ("+bn" if on else ""), (name, fold, epi, got["kernel"])
        assert got["_info"].fold_applied == (1 if on else 0) and got["_info"].splitk > 1


def test_first_layer_weight_gradient_rides_on_d2_input_gradient():
    """d2's input gradient at n = 32 with d1's sign words (tests/test_dispatch_gpu.py: igemm8<3> by default, igemm6<3,128> with
    GI_IGEMM8 = 0): only igemm8's dual-px tiles take the words, and with them the first layer's weight gradient (one 64 x 16 block
    of partial sums per workgroup)."""
    case = (1, 32, 64, 64, 128, 64)
    got = DT.plan_row(B, DT._case(*case, epi="mask+bits"), offered=DT.OFFER_C1W)
    info = got["_info"]
    assert got["kernel"] == "igemm8<3>" and got["mask_applied"] == 1 and info.c1w_applied == 1 and info.c1w_blocks == info.grid == 1024
    got = DT.plan_row(B, DT._case(*case, epi="mask"), offered=DT.OFFER_C1W)           # no sign words: nothing to ride on
    assert got["kernel"] == "igemm8<3>" and got["mask_applied"] == 1 and got["_info"].c1w_applied == 0
    got = DT.plan_row(B, DT._case(*case, epi="mask+bits", opts={"GI_IGEMM8": 0}), offered=DT.OFFER_C1W)
    assert got["kernel"] == "igemm6<3,128>" and got["mask_applied"] == 1 and got["_info"].c1w_applied == 0 and got["_info"].c1w_blocks == 0


def _vgg(n_img, hw, cin, cout, pool, opts=None):
    c = DT._case(2, n_img, hw, hw, cin, cout, opts=opts)
    return DT.plan_row(B, c, offered=DT.OFFER_BIAS | (DT.OFFER_POOL2 if pool else 0))


def test_vgg_3x3_layers():
    """VGG-19 at 512 x 512 (two image pairs): the pooled layers conv2_2 / conv3_4 store their max pool from igemm8<2>, conv1_2 (64
    output channels) from igemm8<2,64>; conv4_4 has 256 workgroups there - below igemm8's 512 - and 512 with four pairs; at
    128 x 128 conv3_1 runs on igemm8<2> with GI_IGEMM8 = 2 and on igemm5<2,128> with GI_IGEMM8 = 0
    (tests/test_auxloss_gpu.py::test_vgg_feature_maps_per_3x3_kernel_family)."""
    for hw, cin, cout, kernel in ((512, 64, 64, "igemm8<2,64>"), (256, 128, 128, "igemm8<2>"), (128, 256, 256, "igemm8<2>"), (64, 512, 512, "igemm5<2,128>"), (64, 512, 512, "igemm8<2>")):
        n_img = 8 if (hw, kernel) == (64, "igemm8<2>") else 4
        got = _vgg(n_img, hw, cin, cout, True)
        assert got["rc"] == 0 and got["kernel"] == kernel and got["_info"].pool_applied == (1 if kernel.startswith("igemm8") else 0), (hw, got["kernel"])
        assert _vgg(n_img, hw, cin, cout, False)["_info"].pool_applied == 0
    assert _vgg(4, 32, 128, 256, False, {"GI_IGEMM8": 2})["kernel"] == "igemm8<2>"
    assert _vgg(4, 32, 128, 256, False, {"GI_IGEMM8": 0})["kernel"] == "igemm5<2,128>"
    assert _vgg(4, 32, 128, 256, False, {"GI_IGEMM5": 3})["kernel"] == "igemm3<2,128>"       # the 3x3 halo kernels off
    # a 3x3 shape that no LDS-DMA kernel serves is reported to the caller, never handed to the 4x4 kernels
    got = _vgg(4, 32, 96, 256, False)
    assert got["rc"] == -4, got
