"""CPU tier of the step-level FID checks (tests/test_fid_layers_gpu.py): the per-step references and tolerances of
tests/inception_ref.py are satisfiable, their inputs keep every layer alive, and they reject the faults the end-to-end feature
bound lets through or barely catches. The fp32 restatement (inception_ref.run_program, with round_fp16 for the fp16 engine) stands
in for the engine: same rounding points, another summation order.

Measured where this file was written (exact-fold parameters 4242, make_images(77, 2, 1, 128)), worst error / tol of the stand-in:
    fp16: pointwise conv 0.962, tap conv 0.985, average pool 0.998 (one half-ulp rounding to fp16 is nearly the whole tolerance)
    fp32: pointwise conv 0.047, tap conv 0.026, average pool 0 (torch adds the taps in fp64)
    liveness: at least 58.3 % of every step's reference output positive, largest magnitude 5.49
Injected faults, fp16 stand-in: error / tol at the step | end-to-end feature error in yardsticks (b), where the suite's bound is 4
(a clean run is 1.00 by definition):
    padding counted in Mixed_5b's average pool                       1140 | 10.6
    tap 6 of the 1x7 Mixed_6b.branch7x7_2 dropped                    2020 | 64.1
    the 18 rows of the ragged last M tile of Mixed_5b.branch5x5_2    1120 | 11.2
    the last 32 of 448 input channels of Mixed_7b.branch3x3dbl_2      179 | 56.6
    the bottom-right output pixel of Mixed_6b.branch7x7_3 zero       1350 |  3.36   (passes end to end)
    one output element of Mixed_6c.branch7x7dbl_3 off by 10 %         112 |  1.08   (passes end to end)
    one output element of Mixed_7c.branch1x1 off by 8 fp16 ulp       5.44 |  1.00   (invisible end to end)
In fp32 the same faults give 206 .. 9.3e5 at the step; the 8-ulp16 one 9.06.
"""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import inception_ref as R

SEED, IMAGES = 4242, (77, 2, 1, 128)
GEOMETRIES = [(64, 64), (128, 128), (299, 299), (512, 512), (200, 360), (360, 200), (1, 1), (2, 3), (300, 298)]
ROUND = {"fp16": R.round_fp16, "fp32": None}


def _step_of(name):
    return next(i for i, s in enumerate(R.STEPS) if s["name"] == name)


@pytest.fixture(scope="module")
def world():
    P = R.make_params_exact_fold(SEED)
    w = dict(T32=R.to_torch(P, torch.float32), T64=R.to_torch(P, torch.float64), x=torch.from_numpy(R.make_images(*IMAGES)))
    with torch.no_grad():
        for dt in ("fp16", "fp32"):
            w[dt] = R.run_program(w["T32"], w["x"], ROUND[dt], keep=True)
        w["f64"] = R.forward(w["T64"], w["x"].double())
    return w


def test_the_fold_of_the_exact_parameters_is_exact():
    assert np.float32(np.float32(0.999) + np.float32(0.001)) == np.float32(1.0)
    P, G = R.make_params_exact_fold(SEED), R.make_params(SEED)
    for name, *_ in R.CONVS:
        w = P[f"{name}.conv.weight"]
        assert np.array_equal(w.astype(np.float16).astype(np.float32), w)
        assert np.abs(w - G[f"{name}.conv.weight"]).max() <= 2.0 ** -11 * np.abs(w).max()
        s = P[f"{name}.bn.weight"] / np.sqrt(P[f"{name}.bn.running_var"] + np.float32(R.BN_EPS))
        assert s.dtype == np.float32 and np.all(s == 1.0)
        assert np.array_equal(P[f"{name}.bn.bias"], G[f"{name}.bn.bias"]) and np.array_equal(P[f"{name}.bn.running_mean"], G[f"{name}.bn.running_mean"])


def test_program_shape():
    assert len(R.STEPS) == 107 and sum(s["kind"] == "conv" for s in R.STEPS) == 94
    assert [s["name"] for s in R.STEPS if s["kind"] == "conv"] == [c[0] for c in R.CONVS]
    assert [s["kind"] for s in R.STEPS if s["kind"] != "conv"] == ["max_s2"] * 2 + ["avg_s1"] * 3 + ["max_s2"] + ["avg_s1"] * 4 + ["max_s2", "avg_s1", "max_s1"]
    bw = R.block_writers()
    assert len(bw) == 11
    for name, steps in bw.items():
        s = [R.STEPS[i] for i in steps]
        spans = sorted((t["coffout"], t["coffout"] + t["out_chw"][0]) for t in s)
        assert spans[0][0] == 0 and spans[-1][1] == s[0]["ldout"] and all(a[1] == b[0] for a, b in zip(spans, spans[1:])), name
        assert len({(t["dst"], t["ldout"]) for t in s}) == 1
    for s in R.STEPS:                                  # no step works in place, and a step's source is what an earlier one wrote
        assert s["src"] != s["dst"]
    assert R.STEPS[-1]["out_chw"][1:] == (8, 8) and R.STEPS[-1]["ldout"] == 2048


def test_the_routed_stand_in_is_the_functional_restatement(world):
    """run_program (buffers, channel offsets) computes what forward() computes: exact-fold parameters make the fold exact to 1e-8."""
    for dt in ("fp16", "fp32"):
        T = world["T32"]
        with torch.no_grad():
            want = R.forward(T, world["x"], ROUND[dt])
        got = world[dt][0]
        assert float((got - want).abs().max()) <= 1e-4 * float(want.abs().max())


@pytest.mark.parametrize("dt", ["fp16", "fp32"])
def test_the_reference_alone_stays_inside_the_bounds(world, dt):
    feats, rec = world[dt]
    worst = {}
    with torch.no_grad():
        for i, (a, o) in enumerate(rec):
            ref, tol = R.step_reference(i, a, world["T64"], dt)
            s = R.STEPS[i]
            if s["kind"].startswith("max"):
                assert torch.equal(o.double(), ref), (i, R.step_label(i))
                continue
            ratio, _ = R.worst_ratio(o, ref, tol)
            kind = s["kind"] if s["kind"] != "conv" else "pointwise" if R.CONV_BY_NAME[s["name"]][3] == (1, 1) else "taps"
            worst[kind] = max(worst.get(kind, 0.0), ratio)
            assert ratio <= 1.0, (i, R.step_label(i), ratio)
        ref, tol = R.gap_reference(_last_rows(world, dt))
        g, _ = R.worst_ratio(feats, ref, tol)
        assert g <= 1.0
    print(f"stand-in {dt}: worst error / tol {worst}, global average {g:.3f}")


def _last_rows(world, dt):
    """The last block's whole output rows of the stand-in: the four branch outputs of Mixed_7c at their offsets."""
    rec = world[dt][1]
    steps = R.block_writers()["Mixed_7c"]
    out = torch.zeros(rec[-1][1].shape[0], 2048, 8, 8)
    for i in steps:
        s = R.STEPS[i]
        out[:, s["coffout"]:s["coffout"] + s["out_chw"][0]] = rec[i][1]
    return out


def test_the_inputs_keep_every_step_alive(world):
    """A condition on the chosen seed, not a measurement: a dead or saturated layer would make its step test vacuous."""
    lo, hi = 1.0, 0.0
    with torch.no_grad():
        for i, (a, _) in enumerate(world["fp16"][1]):
            ref, _ = R.step_reference(i, a, world["T64"], "fp16")
            pos, mag = float((ref > 0).double().mean()), float(ref.abs().max())
            assert pos >= 0.5 and mag < 1000.0, (i, R.step_label(i), pos, mag)
            lo, hi = min(lo, pos), max(hi, mag)
    print(f"liveness: least positive fraction {lo:.3f}, largest magnitude {hi:.3f}")


# ---- the bounds bite --------------------------------------------------------------------------------------------------------------
def _conv_with(step, a, T, rf, w=None, a2=None):
    name, cin, _, _, stride, pad = R.CONV_BY_NAME[R.STEPS[step]["name"]]
    w = T[f"{name}.conv.weight"] if w is None else w
    a = a if a2 is None else a2
    out = F.relu(F.conv2d(a[:, :cin], w, R.exact_fold_bias(T, name), stride=stride, padding=pad))
    return rf(out) if rf else out


def _f_pad_counted(step, a, out, T, rf):
    o = F.avg_pool2d(a, 3, 1, 1, count_include_pad=True)
    return rf(o) if rf else o


def _f_tap_dropped(step, a, out, T, rf):
    w = T[f"{R.STEPS[step]['name']}.conv.weight"].clone()
    w[:, :, :, 6] = 0
    return _conv_with(step, a, T, rf, w=w)


def _f_ragged_tile_lost(step, a, out, T, rf):
    n, c, h, wd = out.shape
    rows = (n * h * wd) % 64
    assert rows == 18
    o = out.permute(0, 2, 3, 1).reshape(n * h * wd, c).clone()
    o[-rows:] = 0
    return o.reshape(n, h, wd, c).permute(0, 3, 1, 2).contiguous()


def _f_channels_ignored(step, a, out, T, rf):
    a2 = a.clone()
    a2[:, 448 - 32:] = 0
    return _conv_with(step, a, T, rf, a2=a2)


def _f_corner_zero(step, a, out, T, rf):
    o = out.clone()
    o[:, :, -1, -1] = 0
    return o


def _argmax(out):
    return np.unravel_index(int(out.abs().argmax()), out.shape)


def _f_one_element_10_percent(step, a, out, T, rf):
    o, j = out.clone(), _argmax(out)
    o[j] = o[j] * 1.1
    return rf(o) if rf else o


def _f_one_element_8_ulp16(step, a, out, T, rf):
    o, j = out.clone(), _argmax(out)
    o[j] = o[j] + 8 * float(np.spacing(np.float16(float(o[j]))))
    return o


FAULTS = [("padding counted in Mixed_5b's average pool", 13, _f_pad_counted),
          ("tap 6 of the 1x7 Mixed_6b.branch7x7_2 dropped", _step_of("Mixed_6b.branch7x7_2"), _f_tap_dropped),
          ("the 18 rows of the ragged last M tile of Mixed_5b.branch5x5_2 lost", _step_of("Mixed_5b.branch5x5_2"), _f_ragged_tile_lost),
          ("the last 32 of 448 input channels of Mixed_7b.branch3x3dbl_2 ignored", _step_of("Mixed_7b.branch3x3dbl_2"), _f_channels_ignored),
          ("the bottom-right output pixel of the 7x1 Mixed_6b.branch7x7_3 zero", _step_of("Mixed_6b.branch7x7_3"), _f_corner_zero),
          ("one output element of Mixed_6c.branch7x7dbl_3 off by 10 %", _step_of("Mixed_6c.branch7x7dbl_3"), _f_one_element_10_percent),
          ("one output element of Mixed_7c.branch1x1 off by 8 fp16 ulp", _step_of("Mixed_7c.branch1x1"), _f_one_element_8_ulp16)]


@pytest.mark.parametrize("dt", ["fp16", "fp32"])
@pytest.mark.parametrize("fault", FAULTS, ids=[f[0] for f in FAULTS])
def test_the_bounds_bite(world, fault, dt):
    what, step, fn = fault
    assert R.STEPS[13]["kind"] == "avg_s1"
    T, rf = world["T32"], ROUND[dt]
    clean_feats, rec = world[dt]
    a, out = rec[step]
    with torch.no_grad():
        bad = fn(step, a, out, T, rf)
        ref, tol = R.step_reference(step, a, world["T64"], dt)
        ratio, _ = R.worst_ratio(bad, ref, tol)
        # what the end-to-end feature check sees of it: the faulty step inside the whole stand-in, in yardsticks
        feats, _ = R.run_program(T, world["x"], rf, hook=lambda i, aa, oo: fn(i, aa, oo, T, rf) if i == step else None)
    f64 = world["f64"]
    yard = float((clean_feats.double() - f64).abs().max())
    e2e = float((feats.double() - f64).abs().max()) / yard
    print(f"fault [{dt}] {what}: error / tol at the step {ratio:.3g}; end to end {e2e:.2f} yardsticks ({'b' if dt == 'fp16' else 'a'})")
    assert not torch.equal(bad, out)
    assert ratio > 1.0, (what, ratio)


# ---- the input kernel's tolerance ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", [1, 3])
@pytest.mark.parametrize("hw", GEOMETRIES, ids=[f"{h}x{w}" for h, w in GEOMETRIES])
def test_input_tolerance_holds_for_an_fp32_resize(hw, c):
    """torch's own fp32 bilinear resize against its fp64 self on uniform noise (the worst case for D) stays inside the tolerance,
    with and without the rounding to fp16."""
    rng = np.random.Generator(np.random.PCG64(900 + hw[0] * 7 + hw[1] + c))
    x = torch.from_numpy(rng.random((2, c, hw[0], hw[1]), dtype=np.float32))
    x3 = x.expand(-1, 3, -1, -1) if c == 1 else x
    got = 2 * F.interpolate(x3, size=(299, 299), mode="bilinear", align_corners=False) - 1
    for dt in ("fp32", "fp16"):
        ref, tol = R.input_reference(x, dt)
        g = R.round_fp16(got) if dt == "fp16" else got
        ratio, _ = R.worst_ratio(g, ref, tol)
        print(f"input {hw} c={c} {dt}: torch fp32 error / tol {ratio:.3f}")
        assert ratio <= 1.0
    if hw == (299, 299):
        assert torch.equal(got, 2 * x3 - 1)
    # the tolerance is not slack: a resize that is one source pixel off fails it
    if hw[0] > 2:
        shifted = 2 * F.interpolate(torch.roll(x3, 1, 3), size=(299, 299), mode="bilinear", align_corners=False) - 1
        ref, tol = R.input_reference(x, "fp16")
        assert R.worst_ratio(shifted, ref, tol)[0] > 100.0
