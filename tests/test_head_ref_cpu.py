"""CPU tier: tests/head_ref.py is honest. Its fp64 reference equals torch autograd on the module the head stands for; its numpy
emulation of the kernels' rounding points equals the reference on the exact-integer inputs of tests/test_head_gpu.py, stays inside
the derived bounds on the rounding inputs, and one deliberately wrong emulation per output leaves them: a bound that could not
see a shifted tap, a dropped pixel, a population's vectors taken from the other one or a missing partial would be no check."""
import pytest
import torch
import torch.nn as nn

import head_ref as R

LS = 256.0


# ---- the reference against autograd ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Hh,Wh", [(5, 7), (13, 9)])
@pytest.mark.parametrize("sigmoid", [0, 1])
def test_reference_equals_autograd(Hh, Wh, sigmoid):
    n, c = 3, 24
    P = (Hh - 3) * (Wh - 3)
    d = R.inputs(False, False, n, Hh, Wh, c, seed=3)
    layers = [nn.Conv2d(c, 1, 4, 1, 0, bias=False), nn.Flatten(), nn.Linear(P, 1)] + ([nn.Sigmoid()] if sigmoid else [])
    net = nn.Sequential(*layers).double()
    with torch.no_grad():
        net[0].weight.copy_(d["w5"].double().reshape(4, 4, c).permute(2, 0, 1)[None])
        net[2].weight.copy_(d["wl"].double()[None])
        net[2].bias.copy_(d["bl"].double())
    x = d["a4"].double().permute(0, 3, 1, 2).contiguous().requires_grad_(True)
    hmid = net[1](net[0](x))
    y = net(x)
    y.backward(d["dy"].double()[:, None])
    f = R.forward_ref(d["a4"], d["w5"], d["wl"], d["bl"], sigmoid)
    assert torch.allclose(f["h"], hmid.detach(), rtol=1e-12, atol=1e-12) and torch.allclose(f["out"], y.detach()[:, 0], rtol=1e-12, atol=1e-12)
    b = R.backward_ref(d["a4"], Hh, Wh, d["w5"], d["wl"], f["h"], f["out"], d["dy"], sigmoid, LS)
    assert torch.allclose(b["da4"][0], LS * x.grad.permute(0, 2, 3, 1), rtol=1e-12, atol=1e-12)
    assert torch.allclose(b["dw5"][0], net[0].weight.grad[0].permute(1, 2, 0).reshape(16, c), rtol=1e-12, atol=1e-12)
    assert torch.allclose(b["dwl"][0], net[2].weight.grad[0], rtol=1e-12, atol=1e-12)
    assert torch.allclose(b["dbl"][0], net[2].bias.grad, rtol=1e-12, atol=1e-12)
    # A bounds its value, and the preloaded gradients are added
    for k, (v, A) in b.items():
        assert bool((v.abs() <= A * (1 + 1e-12) + 1e-300).all()), k
    b2 = R.backward_ref(d["a4"], Hh, Wh, d["w5"], d["wl"], f["h"], f["out"], d["dy"], sigmoid, LS, pre=d["pre"])
    assert torch.allclose(b2["dw5"][0] - b["dw5"][0], d["pre"][0].double(), atol=1e-12)


def test_affine_restatement():
    """population of image i = i / n_per_group; fp32 fma, fp32 slope product, fp16 result"""
    a4 = torch.tensor([[-5.0, 3.0], [-5.0, 1.0]]).reshape(2, 1, 1, 2)
    sc, sh = torch.tensor([[1.0, 2.0], [2.0, 1.0]]), torch.tensor([[0.0, 5.0], [5.0, 0.0]])
    x = R.affine_x(a4, (sc, sh, 1))
    assert x.reshape(-1).tolist() == [-1.0, 11.0, -1.0, 1.0]
    assert R.affine_x(a4, (sc, sh, 1), swap=True).reshape(-1).tolist() == [-1.0, 11.0, -1.0, 7.0]
    assert R.bands(1, 289) == 8 and R.band_ranges(1, 289)[-1] == (259, 289) and R.bands(2, 117) == 2 and R.bands(300, 16) == 1
    assert R.slices(2, 529) == 2 and R.slices(1, 1024) == 4 and R.slices(2, 289) == 1


# ---- the emulation on the exact inputs -------------------------------------------------------------------------------------------
CPU_SHAPES = [(3, 4, 4), (2, 5, 7), (2, 7, 5), (2, 13, 9)]      # the last one: two bands of 59 and 58 pixels


@pytest.mark.parametrize("n,Hh,Wh", CPU_SHAPES)
@pytest.mark.parametrize("path", ["fast", "fast-affine", "generic-f16", "generic-f32"])
def test_emulation_is_exact_on_integer_inputs(n, Hh, Wh, path):
    fast, fp16 = path.startswith("fast"), path != "generic-f32"
    c = 512 if fast else 24
    groups = 2 if path == "fast-affine" and n % 2 == 0 else (1 if path == "fast-affine" else 0)
    d = R.inputs(True, fp16, n, Hh, Wh, c, groups=groups)
    f = R.forward_ref(d["a4"], d["w5"], d["wl"], d["bl"], 0, fast, d["aff"])
    h, out = R.emulate_forward(d["a4"], d["w5"], d["wl"], d["bl"], 0, fast, d["aff"])
    assert torch.equal(h, f["h"]) and torch.equal(out, f["out"])
    b = R.backward_ref(d["a4"], Hh, Wh, d["w5"], d["wl"], d["h"], d["out"], d["dy"], 0, LS, d["aff"], d["pre"])
    e = R.emulate_backward(d["a4"], Hh, Wh, d["w5"], d["wl"], d["h"], d["out"], d["dy"], fp16, 0, LS, d["aff"], d["pre"], fast)
    for k in ("dh", "da4", "dw5", "dwl", "dbl"):
        assert torch.equal(e[k], b[k][0]), k
    assert float(b["da4"][0].abs().max()) <= 65504 and float(f["h"].abs().max()) < 2 ** 24


def _gpu_exact_shapes():
    s = {(n, Hh, Wh, 512, 0) for n, Hh, Wh, _, _ in R.FAST_FWD} | {(n, Hh, Wh, 512, 0) for n, Hh, Wh in R.FAST_BWD}
    s |= {(n, Hh, Wh, 512, g) for n, g, Hh, Wh in R.AFF_CASES + R.RAW_CASES}
    s |= {(2, Hh, Wh, c, 0) for _, _, c, _ in R.GENERIC for Hh, Wh in R.GEN_MAPS}
    return sorted(s)


@pytest.mark.parametrize("n,Hh,Wh,c,groups", _gpu_exact_shapes())
def test_integer_inputs_are_exact_at_every_gpu_shape(n, Hh, Wh, c, groups):
    """every term is an integer and the sum of the absolute values of an element's terms stays below 2^24, so fp32 sums of them are
    exact in ANY order; da4 is a multiple of the loss scale that fp16 holds exactly"""
    d = R.inputs(True, True, n, Hh, Wh, c, groups=groups)
    x = R.affine_x(d["a4"], d["aff"])
    assert torch.equal(x, x.round()) and (groups == 0 or float(x.min()) < 0), "the affine map must stay on the integers and reach the LeakyReLU branch"
    f = R.forward_ref(d["a4"], d["w5"], d["wl"], d["bl"], 0, True, d["aff"])
    assert float(f["A_h"].max()) < 2 ** 24 and float(f["A_out"].max()) < 2 ** 24
    b = R.backward_ref(d["a4"], Hh, Wh, d["w5"], d["wl"], d["h"], d["out"], d["dy"], 0, LS, d["aff"], d["pre"])
    assert all(float(b[k][1].max()) < 2 ** 24 for k in ("dw5", "dwl", "dbl"))
    k = b["da4"][0] / LS
    assert torch.equal(k, k.round()) and float(b["da4"][1].max()) / LS <= 2048 and float(b["da4"][1].max()) <= 65504
    assert bool((b["dw5"][0] != d["pre"][0]).any()) and bool((b["da4"][0] != 0).any())


# ---- the emulation on the rounding inputs: inside the bounds, and the wrong forms outside -----------------------------------------
def _forward_ratios(n, Hh, Wh, fast, fp16, groups, sigmoid, wrong=None):
    c = 512 if fast else 24
    P = (Hh - 3) * (Wh - 3)
    d = R.inputs(False, fp16, n, Hh, Wh, c, groups=groups, sigmoid=sigmoid)
    f = R.forward_ref(d["a4"], d["w5"], d["wl"], d["bl"], sigmoid, fast, d["aff"])
    h, out = R.emulate_forward(d["a4"], d["w5"], d["wl"], d["bl"], sigmoid, fast, d["aff"], wrong)
    return dict(h=R.worst_ratio(h - f["h"], R.bound_h(c, f["A_h"])), out=R.worst_ratio(out - f["out"], R.bound_out(c, P, f["A_out"], sigmoid)))


def _backward_ratios(n, Hh, Wh, fast, fp16, groups, sigmoid, wrong=None):
    c = 512 if fast else 24
    P = (Hh - 3) * (Wh - 3)
    d = R.inputs(False, fp16, n, Hh, Wh, c, groups=groups, sigmoid=sigmoid)
    b = R.backward_ref(d["a4"], Hh, Wh, d["w5"], d["wl"], d["h"], d["out"], d["dy"], sigmoid, LS, d["aff"], d["pre"])
    e = R.emulate_backward(d["a4"], Hh, Wh, d["w5"], d["wl"], d["h"], d["out"], d["dy"], fp16, sigmoid, LS, d["aff"], d["pre"], fast, wrong=wrong)
    bounds = dict(dh=R.bound_dh(b["dh"][0]), da4=R.bound_da4(fp16, *b["da4"]), dw5=R.bound_dw5(n, P, b["dw5"][1]),
                  dwl=R.bound_dwl(n, b["dwl"][1]), dbl=R.bound_dwl(n, b["dbl"][1]))
    return {k: R.worst_ratio(e[k] - b[k][0], bounds[k]) for k in bounds}


def _bn_ratios(n, Hh, Wh, wrong=None):
    c, G = 512, 2
    d = R.inputs(False, True, n, Hh, Wh, c)
    b = R.backward_ref(None, Hh, Wh, d["w5"], d["wl"], d["h"], d["out"], d["dy"], 0, LS, want_w=False)
    stored = b["da4"][0].to(torch.float32).to(torch.float16).double()
    x, sc, sh, mu, iv = R.bn_bwd_inputs(n, Hh, Wh, c, G)
    s, A = R.bn_sums_ref(stored, x, sc, sh, mu, iv, n // G)
    e = R.emulate_bn_sums(stored, x, sc, sh, mu, iv, n // G, wrong=wrong)
    return R.worst_ratio(e - s, R.bound_bn_sums((n // G) * Hh * Wh, (n // G) * R.bands(n, Hh * Wh), A))


PATHS = [("fast", True, True, 0), ("fast-affine", True, True, 2), ("generic-f16", False, True, 0), ("generic-f32", False, False, 0)]


@pytest.mark.parametrize("path", PATHS, ids=[p[0] for p in PATHS])
def test_emulation_stays_inside_the_bounds(path):
    name, fast, fp16, groups = path
    worst = {}
    for n, Hh, Wh in [(2, 4, 4), (2, 5, 7), (2, 13, 9)]:
        for sigmoid in (0, 1):
            r = dict(_forward_ratios(n, Hh, Wh, fast, fp16, groups, sigmoid), **_backward_ratios(n, Hh, Wh, fast, fp16, groups, sigmoid))
            for k, v in r.items():
                worst[k] = max(worst.get(k, 0.0), v)
    print(f"head emulation {name}: worst err / bound " + " ".join(f"{k}={v:.4f}" for k, v in worst.items()))
    assert all(v <= 1.0 for v in worst.values()), worst


def test_da4_bound_covers_fp16_subnormal_results():
    """n = 17 on a 4 x 4 map behind the sigmoid: some gradients fall below 2^-14, where fp16 rounds to a multiple of 2^-24"""
    d = R.inputs(False, True, 17, 4, 4, 512, sigmoid=1)
    ref = R.backward_ref(None, 4, 4, d["w5"], d["wl"], d["h"], d["out"], d["dy"], 1, LS, want_w=False)["da4"][0]
    assert bool(((ref.abs() < 2.0 ** -14) & (ref != 0)).any())
    r = _backward_ratios(17, 4, 4, True, True, 0, 1)["da4"]
    print(f"head emulation da4 with subnormal results: worst err / bound {r:.4f}")
    assert r <= 1.0


def test_bn_sums_emulation_stays_inside_the_bound():
    r = max(_bn_ratios(4, 13, 9), _bn_ratios(2, 5, 7))
    print(f"head emulation bn sums: worst err / bound {r:.4f}")
    assert r <= 1.0


# (output, wrong form, path, shape): every output has at least one
SHARP = [
    ("h", "edge_tap", PATHS[0], (2, 5, 7)), ("out", "edge_tap", PATHS[0], (2, 4, 4)), ("h", "edge_tap", PATHS[3], (2, 7, 5)),
    ("h", "pop_swap", PATHS[1], (2, 5, 7)), ("out", "pop_swap", PATHS[1], (2, 4, 4)),
    ("da4", "edge_tap", PATHS[0], (2, 5, 7)), ("da4", "band_drop", PATHS[0], (2, 13, 9)), ("da4", "edge_tap", PATHS[2], (2, 5, 7)),
    ("dw5", "band_drop", PATHS[0], (2, 13, 9)), ("dw5", "partial_omit", PATHS[0], (2, 13, 9)), ("dw5", "pop_swap", PATHS[1], (2, 13, 9)),
    ("dw5", "partial_omit", PATHS[3], (2, 5, 7)),
    ("dwl", "image_omit", PATHS[0], (2, 5, 7)), ("dbl", "image_omit", PATHS[0], (2, 5, 7)),
]


@pytest.mark.parametrize("case", SHARP, ids=[f"{c[0]}-{c[1]}-{c[2][0]}" for c in SHARP])
def test_bounds_see_a_wrong_kernel(case):
    out, wrong, (name, fast, fp16, groups), (n, Hh, Wh) = case
    fn = _forward_ratios if out in ("h", "out") else _backward_ratios
    good, bad = fn(n, Hh, Wh, fast, fp16, groups, 0)[out], fn(n, Hh, Wh, fast, fp16, groups, 0, wrong)[out]
    print(f"head sharpness {out} {wrong} {name}: right {good:.4f} wrong {bad:.2f}")
    assert good <= 1.0 < bad


def test_bn_sums_bound_sees_swapped_populations():
    good, bad = _bn_ratios(4, 13, 9), _bn_ratios(4, 13, 9, "pop_swap")
    print(f"head sharpness bn sums pop_swap: right {good:.4f} wrong {bad:.2f}")
    assert good <= 1.0 < bad
