"""CPU tier: the storage-rounded restatement of the oracle (oracle/torch_ref.py: store=...) and the fp16 bound built on it
(oracle/kink.py: yardstick, fp16_parity), checked on the oracle itself: the fp32 oracle plays the implementation under test."""
import pytest
import torch

from oracle import kink
from oracle import torch_ref as orc

CASES = {
    "unet6-64": lambda: kink.unet_case(170, 6, 2, 64),
    "unet7-128": lambda: kink.unet_case(235, 7, 2, 128),
    "instance6-64": lambda: kink.unet_case(4109, 6, 3, 64, "instance"),
    "none6-64": lambda: kink.unet_case(4109, 6, 3, 64, "none"),
    "patchgan128": lambda: kink.patchgan_case(328, 128, 3, True),
    "patchgan128-two-populations": lambda: kink.patchgan_case(1028, 128, 4, False, groups=2),
}
# the absolute fp16 bounds of tests/test_nets_gpu.py, which stay asserted next to the yardstick
OLD_OUT, OLD_GRAD_L2 = 2e-2, 3e-2


def _identity(t, fwd=True, bwd=True):
    return t


def _same(a, b):
    return all(torch.equal(a[k], b[k]) for k in b) and set(a) == set(b)


@pytest.mark.parametrize("name", ["unet6-64", "instance6-64", "patchgan128-two-populations"])
def test_store_none_is_the_oracle_and_an_identity_store_is_the_same_function(name):
    """store=None: today's numbers bit for bit (fp32: output, gradients, dx, running statistics). The restatement's graph with a
    store that rounds nothing (d1 / u1 as unfold + GEMM + fold, BatchNorm written out with the statistics of the unrounded tensor,
    ReLU before the concat) is the oracle's function: fp64 agreement to rounding."""
    torch.set_num_threads(8)
    case = CASES[name]()
    y0, g0, dx0, OP0 = kink.run(case, torch.float32)
    y1, g1, dx1, OP1 = kink.run(case, torch.float32, store=None)
    assert torch.equal(y0, y1) and torch.equal(dx0, dx1) and _same(g0, g1) and _same(kink._running(OP0), kink._running(OP1))
    ta, tb = {}, {}
    ya, ga, dxa, OPa = kink.run(case, torch.float64, ta)
    yb, gb, dxb, OPb = kink.run(case, torch.float64, tb, store=_identity)
    rel = lambda a, b: float((a - b).abs().max() / (b.abs().max() + 1e-300))   # noqa: E731
    assert rel(yb.detach(), ya.detach()) < 1e-12 and rel(dxb, dxa) < 1e-9
    skip = {k for k in ga if case.get("norm") == "instance" and k.endswith(".bias")}   # (exactly cancelling sums: rounding residue only)
    assert max(rel(gb[k], ga[k]) for k in ga if k not in skip) < 1e-9
    assert sorted(ta) == sorted(tb) and max(rel(tb[k].detach().double(), ta[k].detach().double()) for k in ta) < 1e-12
    ra, rb = kink._running(OPa), kink._running(OPb)
    assert all(rel(rb[k], ra[k]) < 1e-12 for k in ra)


@pytest.mark.parametrize("name", sorted(CASES))
def test_restatement_band_and_sign_disagreements(name):
    """With the fp16 store the output differs from the oracle's and stays under the forward bound 2e-2; a kink decision of the
    restatement can differ from the fp64 oracle's only where |z64| <= |z16 - z64| <= eps16; the band min(FP16_BAND max|z64|,
    K eps16) holds at most 5 % of the live units, at most 2e-3 of them decided by the restatement, none outside."""
    torch.set_num_threads(8)
    case = CASES[name]()
    yd = kink.yardstick(case)
    r, f64 = kink.restated(case), kink.forward64(case)
    out_err = yd["err"][("out", "y")]
    print(f"{name}: output error of the restatement {out_err:.3e}")
    assert 0 < out_err < OLD_OUT
    for tap, e in yd["eps16"].items():
        z64, z16 = f64["taps"][tap], r["taps"][tap]
        dis = (z64 > 0) != (z16 > 0)
        assert e > 0
        assert not dis.any() or float(z64.abs()[dis].max()) < e, tap
    rep = yd["rep"]
    share, flipped = rep["at_risk"] / rep["units"], rep["flipped"] / rep["units"]
    print(f"{name}: {share:.2%} of {rep['units']} live units inside the band, {flipped:.2e} decided by the restatement")
    assert share <= kink.BAND_SHARE_CAP and flipped <= kink.FLIP_SHARE_CAP and rep["outside"] == 0
    for tap, s in kink.survey(case, fp16=True).items():      # never wider than the constant it replaces
        assert s["width"] <= kink.FP16_BAND * float(s["z64"].abs().max())


def _stand_in(case):
    """The fp32 oracle as the implementation under test: what the GPU tests read from the HIP network."""
    taps = {}
    y, g, dx, OP = kink.run(case, torch.float32, taps)
    acts = {k: kink.saved_from_tap(case, k, v.detach(), taps.get(k + ".keep")) for k, v in taps.items() if not k.endswith(".keep")}
    return {"y": y, "stats": kink._running(OP), "acts": acts, "grads": dict(g), "dx": dx}


def _old_bounds_hold(case, impl, ref):
    """What tests/test_nets_gpu.py asserted for fp16 before the yardstick: output 2e-2 of max|ref|, every gradient 3e-2 relative
    L2 - and no saved activation compared with anything."""
    y64, g64, dx64 = ref
    ok = kink._rel_max(impl["y"], y64) <= OLD_OUT and kink._rel_l2(impl["dx"], dx64) <= OLD_GRAD_L2
    return ok and all(kink._rel_l2(impl["grads"][k], g64[k]) <= OLD_GRAD_L2 for k in g64)


MUTATIONS = [("patchgan128", "grads", "model.5.weight"), ("patchgan128", "grads", "model.6.bias"),
             ("unet7-128", "grads", "model.model.3.weight"), ("unet7-128", "acts", "d2")]


@pytest.mark.parametrize("name", ["patchgan128", "unet7-128"])
def test_the_yardstick_bound_sees_a_one_percent_error_the_absolute_bound_does_not(name):
    """A 1 % relative error in ONE tensor - a critic weight gradient, a critic BatchNorm bias gradient, the generator's outermost
    decoder weight gradient, the generator's saved d2 activation - fails K x yardstick and passes the absolute bounds; the
    unperturbed stand-in passes both. These tensors' yardsticks are <= 2.1e-3 (printed), so 1e-2 exceeds K x yardstick + floor."""
    torch.set_num_threads(8)
    case = CASES[name]()
    impl = _stand_in(case)
    dec = {k: v > 0 for k, v in impl["acts"].items()}
    y, g, dx, rep = kink.kink_reference(case, dec, fp16=True)
    ref = (y, g, dx)
    records, bad = kink.fp16_parity(case, impl, ref, rep)
    assert not bad, bad
    assert _old_bounds_hold(case, impl, ref)
    assert {r["cls"] for r in records} == {"out", "tap", "grad"} | ({"stat"} if impl["stats"] else set())
    yd = kink.yardstick(case)["err"]
    for cname, group, tensor in MUTATIONS:
        if cname != name:
            continue
        key = ("grad" if group == "grads" else "tap", tensor)
        scale = float(kink.forward64(case)["taps"][tensor].abs().max()) if group == "acts" else 1.0
        print(f"{name} {tensor}: yardstick {yd[key] / scale:.3e} -> bound {(kink.K * yd[key] / scale + kink.FLOOR32):.3e}")
        assert kink.K * yd[key] / scale + kink.FLOOR32 < 1e-2 / 1.2, "pick another shallow tensor: 1 % is not 1.2 x above this bound"
        mutated = dict(impl)
        mutated[group] = dict(impl[group])
        mutated[group][tensor] = impl[group][tensor] * 1.01
        _, bad = kink.fp16_parity(case, mutated, ref, rep)
        assert len(bad) == 1 and tensor in bad[0], bad
        assert _old_bounds_hold(case, mutated, ref)
