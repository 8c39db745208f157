"""CPU tier: tests/lpips_ref.py against itself - the restatement the HIP kernels of csrc/lpips.hip are held to - and the host side of
lib/lpips.py. The `lpips` package is not installed on the machines this suite runs on, so nothing here (or in test_lpips_gpu.py) is
compared with it; the weights are stand-ins (lpips_ref.make_params)."""
import numpy as np
import pytest
import torch

import lpips_ref as R


@pytest.fixture(scope="module")
def params():
    return R.make_params(11)


def _first(P):
    return P["features.0.weight"], P["features.0.bias"], P["scaling_layer.shift"], P["scaling_layer.scale"]


@pytest.mark.parametrize("shape", [(16, 16), (32, 48)])
def test_two_plane_first_layer_equals_three_channel_border_included(params, shape):
    w, b, shift, scale = _first(params)
    x = R.make_images(3, 2, *shape)
    ref = R.conv1_three_channel(w, b, shift, scale, x)
    wA, wB = R.fold(w, shift, scale)
    got = R.conv1_two_plane(wA, wB, b, x)
    ring = R.ring_mask(*shape)
    tol = 1e-12 * float(ref.abs().max())
    assert float((got - ref).abs()[..., ring].max()) <= tol          # the ring on its own
    assert float((got - ref).abs()[..., ~ring].max()) <= tol
    # the test can see the tempting wrong fold: beta in the bias is right inside and wrong on the ring
    wrong = R.conv1_beta_in_bias(wA, wB, b, x)
    assert float((wrong - ref).abs()[..., ~ring].max()) <= tol
    assert float((wrong - ref).abs()[..., ring].max()) > 1e-2 * float(ref.abs().max())


def test_distance_properties(params):
    a, b = R.make_images(5, 2, 32, 32), R.make_images(6, 2, 32, 32)
    d_aa, per_aa = R.distance(params, a, a)
    assert torch.equal(d_aa, torch.zeros(2, dtype=torch.float64)) and float(per_aa.abs().max()) == 0.0
    d_ab, _ = R.distance(params, a, b)
    d_ba, _ = R.distance(params, b, a)
    assert torch.equal(d_ab, d_ba) and float(d_ab.min()) > 0.0
    # zero channel vectors (common after ReLU) give 0, not NaN; a zero vector against a unit vector gives lin's weight
    z = np.zeros((1, 64, 2, 2))
    lin = params["lin0.model.1.weight"].reshape(-1)
    assert float(R.tap_distance(z, z, lin)) == 0.0
    e = z.copy()
    e[0, 7] = 3.0
    assert abs(float(R.tap_distance(e, z, lin)) - float(lin[7])) <= 1e-9 * float(lin[7])
    assert float(R.tap_emulate(z, z, lin)) == 0.0 and np.isfinite(float(R.tap_emulate(e, z, lin)))


def test_both_state_dict_spellings_load_to_the_same_buffer(params):
    import gan_inpainting_amd  # noqa: F401
    from gan_inpainting_amd.lib.lpips import LPIPS
    tv = {k: torch.from_numpy(v) for k, v in params.items() if k.startswith("features.")}
    tv["classifier.0.weight"] = torch.zeros(4, 4)                                   # ignored
    lin = {k: torch.from_numpy(v) for k, v in params.items() if k.startswith("lin")}
    m1, m2 = LPIPS(), LPIPS()
    assert m1.load_state_dict({**tv, **lin}) == []
    full = {k: torch.from_numpy(v) for k, v in R.full_lpips_state_dict(params).items()}
    full["net.slice1.1.unknown"] = torch.zeros(1)                                   # ignored
    assert m2.load_state_dict(full) == []
    assert torch.equal(m1.flat, m2.flat)
    assert m1.flat.numel() == sum(v.size for v in params.values())
    sd = m1.state_dict()
    for k, v in params.items():
        assert np.array_equal(sd[k].numpy().reshape(v.shape), v), k
    with pytest.raises(RuntimeError, match="missing keys"):
        LPIPS().load_state_dict(tv)                                                 # no lin tensors
    assert len(LPIPS().load_state_dict(tv, strict=False)) == 5
    # defaults: lin = 1 / C, zero bias, the published scaling constants
    d = LPIPS().state_dict()
    assert torch.equal(d["lin2.model.1.weight"], torch.full((1, 256, 1, 1), 1.0 / 256)) and float(d["features.0.bias"].abs().max()) == 0.0
    assert torch.equal(d["scaling_layer.shift"].reshape(3), torch.tensor(R.SHIFT)) and torch.equal(d["scaling_layer.scale"].reshape(3), torch.tensor(R.SCALE))


def test_colour_input_is_refused_with_a_clear_message():
    import gan_inpainting_amd  # noqa: F401
    from gan_inpainting_amd import backend as B
    from gan_inpainting_amd.lib.lpips import LPIPS
    with pytest.raises(B.BackendError, match="grey"):
        LPIPS().distance(torch.zeros(2, 3, 32, 32), torch.zeros(2, 3, 32, 32))


def test_first_layer_bound_holds_for_the_fp32_emulation(params):
    w, b, shift, scale = _first(params)
    wA, wB = R.fold(w, shift, scale)
    wA, wB = wA.float().numpy(), wB.float().numpy()
    for seed, shape in ((1, (16, 16)), (2, (32, 48))):
        x = R.make_images(seed, 2, *shape)
        err = (R.conv1_emulate(wA, wB, b, x) - R.conv1_two_plane(wA, wB, b, x)).abs()
        bound = R.conv1_bound(wA, wB, b, x)
        assert bool((err <= bound).all()), float((err / bound).max())
        assert float(bound.max()) < 1e-2 * float(R.conv1_two_plane(wA, wB, b, x).abs().max())     # and it is not vacuous


def test_fold_bound_holds_for_fp32(params):
    w, _, shift, scale = _first(params)
    wt, sh, sc = torch.from_numpy(w), torch.from_numpy(shift).reshape(3), torch.from_numpy(scale).reshape(3)
    a32, b32 = torch.zeros(64, 9), torch.zeros(64, 9)
    for c in range(3):
        a32 += wt[:, c].reshape(64, 9) * (2.0 / sc[c])
        b32 += wt[:, c].reshape(64, 9) * ((-1.0 - sh[c]) / sc[c])
    wA, wB = R.fold(w, shift, scale)
    bA, bB = R.fold_bound(w, shift, scale)
    assert bool(((a32.double() - wA).abs() <= bA).all()) and bool(((b32.double() - wB).abs() <= bB).all())


@pytest.mark.parametrize("C", [64, 512])
def test_tap_bound_holds_for_the_fp32_emulation(C):
    rng = np.random.Generator(np.random.PCG64(C))
    fa = np.maximum(rng.standard_normal((3, C, 4, 4)), 0).astype(np.float16)
    fb = np.maximum(fa.astype(np.float32) + 0.3 * rng.standard_normal((3, C, 4, 4)), 0).astype(np.float16)
    fb[0, :, 0, 0] = 0
    lin = (rng.random(C) * 2 / C).astype(np.float32)
    ref, bound = R.tap_distance(fa, fb, lin), R.tap_bound(fa, fb, lin)
    err = (R.tap_emulate(fa, fb, lin) - ref).abs()
    assert bool((err <= bound).all()), (err, bound)
    assert float((bound / ref).max()) < 1e-4
    assert float(R.tap_emulate(fa, fa, lin).abs().max()) == 0.0
    # nearly equal halves: the bound is sharp there, the direct form passes it and the expanded five-sum form does not
    fn = R.near_identical(fa, C + 1)
    ref, bound = R.tap_distance(fa, fn, lin), R.tap_bound(fa, fn, lin)
    assert float(ref.min()) > 0.0
    assert bool(((R.tap_emulate(fa, fn, lin) - ref).abs() <= bound).all())
    assert bool(((R.tap_five_sum(fa, fn, lin) - ref).abs() > bound).all())


def test_fp16_yardstick_is_small_and_not_zero(params):
    a, b = R.make_images(8, 1, 32, 32), R.make_images(9, 1, 32, 32)
    d64, _ = R.distance(params, a, b)
    d16, _ = R.distance(params, a, b, fp16=True)
    rel = float((d16 - d64).abs() / d64)
    assert 0.0 < rel < 0.05
