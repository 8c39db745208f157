"""GPU tier: the spectral-normalisation kernels of csrc/specnorm.hip ONE OP AT A TIME through gi_debug_sn_power_iteration and
gi_debug_sn_project_add, against tests/sn_ref.py (fp64, proven against torch.nn.utils.spectral_norm by tests/test_sn_ref_cpu.py)
within the bounds that file derives from the kernels' summation shape. Matrices are handed over in the master layout (cb > 0:
[a][ky][kx][b]) with v in torch's column order, so every comparison also checks the column map."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import gan_inpainting_amd  # noqa: F401,E402
from gan_inpainting_amd import backend as B  # noqa: E402
import sn_ref  # noqa: E402

# (ca, K, cb): 1x1 (W_sn = +-1, adds exactly 0) | Linear(25,1) | ragged | conv1 | conv2 | head conv (one row, eight column chunks) |
# conv4-sized with 256 input channels: more than one row chunk, column tile and column chunk at once
SHAPES = [(1, 1, 0), (1, 25, 0), (3, 5, 0), (64, 16, 1), (128, 1024, 64), (1, 8192, 512), (512, 4096, 256)]
IDS = ["x".join(map(str, s)) for s in SHAPES]


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).cuda()


def _unit(rng, n):
    x = rng.standard_normal(n).astype(np.float32)
    return (x / np.float32(np.linalg.norm(x))).astype(np.float32)


def power_iteration(w_mem, cb, u, v, iters, train):
    ca, K = w_mem.shape
    wd, ud, vd, sig = _dev(w_mem), _dev(u), _dev(v), torch.zeros(1, device="cuda")
    B.check(B.lib().gi_debug_sn_power_iteration(B.get_ctx(), B.ptr(wd), ca, K, cb, B.ptr(ud), B.ptr(vd), iters, int(train), B.ptr(sig)))
    return ud.cpu().numpy(), vd.cpu().numpy(), sig.cpu().numpy()[0]


def project_add(g_mem, weff_mem, u, v, sigma, cb, scale, dst0):
    ca, K = g_mem.shape
    dst = _dev(dst0)
    sc = None if scale is None else _dev(np.array([scale], np.float32))
    gd, wd, ud, vd, sd = _dev(g_mem), _dev(weff_mem), _dev(u), _dev(v), _dev(np.array([sigma], np.float32))   # (kept alive over the call)
    B.check(B.lib().gi_debug_sn_project_add(B.get_ctx(), B.ptr(gd), B.ptr(wd), B.ptr(ud), B.ptr(vd), B.ptr(sd), ca, K, cb, B.ptr(sc), B.ptr(dst)))
    return dst.cpu().numpy()


def _random_case(shape, seed):
    ca, K, cb = shape
    rng = np.random.default_rng(seed)
    w_mem = (rng.standard_normal((ca, K)) * 0.05).astype(np.float32)
    return rng, w_mem, _unit(rng, ca), _unit(rng, K)


@pytest.mark.parametrize("iters", [1, 3])
@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_power_iteration_within_derived_bounds(shape, iters):
    ca, K, cb = shape
    _, w_mem, u0, v0 = _random_case(shape, 11 + ca + K)
    u, v, sigma = power_iteration(w_mem, cb, u0, v0, iters, True)
    b = sn_ref.power_iteration_bounds(sn_ref.to_torch_order(w_mem, cb), u0, v0, iters, True)
    print(f"sn power iteration {shape} iters={iters}: |du|={np.abs(u - b['u']).max():.3e} (bound {b['eu'].max():.3e}) "
          f"|dv|={np.abs(v - b['v']).max():.3e} (bound {b['ev'].max():.3e}) |dsigma|={abs(sigma - b['sigma']):.3e} (bound {b['esigma']:.3e})")
    assert (np.abs(u - b["u"]) <= b["eu"]).all()
    assert (np.abs(v - b["v"]) <= b["ev"]).all()
    assert abs(sigma - b["sigma"]) <= b["esigma"]
    assert b["esigma"] <= 5e-2 * abs(b["sigma"]) and b["ev"].max() <= 5e-2      # the bounds themselves stay far below an O(1) error
    u2, v2, sigma2 = power_iteration(w_mem, cb, u0, v0, iters, True)
    assert np.array_equal(u, u2) and np.array_equal(v, v2) and sigma == sigma2, "two runs differ"
    if shape == (1, 1, 0):
        assert abs(u[0]) == 1.0 and abs(v[0]) == 1.0 and abs(w_mem[0, 0] / sigma) == 1.0 and sigma > 0


@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_eval_mode_reads_u_v_and_leaves_them_bit_identical(shape):
    ca, K, cb = shape
    _, w_mem, u0, v0 = _random_case(shape, 23 + ca + K)
    u, v, sigma = power_iteration(w_mem, cb, u0, v0, 3, False)
    assert np.array_equal(u, u0) and np.array_equal(v, v0)
    b = sn_ref.power_iteration_bounds(sn_ref.to_torch_order(w_mem, cb), u0, v0, 3, False)
    assert abs(sigma - b["sigma"]) <= b["esigma"], (sigma, b["sigma"], b["esigma"])


@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_small_integer_data_is_exact(shape):
    """Integers small enough that every partial sum is exact in fp32 whatever its order: W in {-1, 0, 1}, u with three non-zero
    entries. Train: t = W^T u is exact, |t|^2 <= 36 K < 2^24 is exact, so v must equal fp32(t / sqrt(|t|^2)) bit for bit, in
    torch's column order. Eval with integer u, v: sigma = u . (W v) is an exact integer."""
    ca, K, cb = shape
    rng = np.random.default_rng(5 + ca + K)
    w_mem = rng.integers(-1, 2, size=(ca, K)).astype(np.float32)
    if not w_mem.any():
        w_mem[0, 0] = 1.0
    w_t = sn_ref.to_torch_order(w_mem, cb)
    u0 = np.zeros(ca, np.float32)
    nz = rng.choice(ca, size=min(3, ca), replace=False)
    u0[nz] = rng.choice(np.array([-2.0, -1.0, 1.0, 2.0], np.float32), size=nz.size)
    t = (w_t.astype(np.float64).T @ u0.astype(np.float64))
    if not t.any():          # (1 x 1 with W = 0 cannot happen: w_mem.any() above; a zero t needs cancelling rows)
        u0[:] = 0.0
        u0[nz[0]] = 1.0
        t = (w_t.astype(np.float64).T @ u0.astype(np.float64))
    q = np.float32((t * t).sum())
    assert q < 2 ** 24 and q > 0
    want_v = t.astype(np.float32) / np.sqrt(q)
    _, v, _ = power_iteration(w_mem, cb, u0, np.zeros(K, np.float32), 1, True)
    assert np.array_equal(v, want_v), np.abs(v - want_v).max()
    ue = rng.integers(-1, 2, size=ca).astype(np.float32)
    ve = rng.integers(-2, 3, size=K).astype(np.float32)
    want_sigma = float(ue.astype(np.float64) @ (w_t.astype(np.float64) @ ve.astype(np.float64)))
    assert abs(want_sigma) < 2 ** 24
    _, _, sigma = power_iteration(w_mem, cb, ue, ve, 1, False)
    assert float(sigma) == want_sigma


@pytest.mark.parametrize("scale", [None, 0.25])
@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_project_add_within_derived_bounds(shape, scale):
    """A random G: <G, W_eff> is O(|G| |W_eff|), so the u v^T term is a large part of the result - the network tests cannot pin it
    on the BatchNorm-fed layers, whose G is orthogonal to W_eff."""
    ca, K, cb = shape
    rng, weff_mem, u, v = _random_case(shape, 37 + ca + K)
    g_mem = rng.standard_normal((ca, K)).astype(np.float32)
    dst0 = rng.standard_normal((ca, K)).astype(np.float32)
    sigma = np.float32(1.7)
    got = project_add(g_mem, weff_mem, u, v, sigma, cb, scale, dst0)
    ref_t, bound_t = sn_ref.project_bounds(sn_ref.to_torch_order(g_mem, cb), sn_ref.to_torch_order(weff_mem, cb), u, v, float(sigma),
                                           1.0 if scale is None else scale, sn_ref.to_torch_order(dst0, cb))
    ref, bound = sn_ref.to_memory_order(ref_t, cb), sn_ref.to_memory_order(bound_t, cb)
    err = np.abs(got - ref)
    term = abs(float((g_mem.astype(np.float64) * weff_mem).sum())) * np.abs(np.outer(u, v)).max() / float(sigma)
    print(f"sn project_add {shape} scale={scale}: max err {err.max():.3e}, max bound {bound.max():.3e}, max |c u v^T / sigma| {term:.3e}")
    assert (err <= bound).all(), f"{int((err > bound).sum())} elements outside the bound, worst {(err / bound).max():.2f} x"
    assert bound.max() <= 1e-4 * np.abs(ref).max()
    again = project_add(g_mem, weff_mem, u, v, sigma, cb, scale, dst0)
    assert np.array_equal(got, again), "two runs differ"


def test_one_by_one_adds_exactly_zero():
    """Linear(1,1) (a 64 x 64 critic's head): W_sn = +-1 whatever W, so the gradient is exactly zero."""
    for w in (0.37, -2.5e-3):
        w_mem = np.array([[w]], np.float32)
        u, v, sigma = power_iteration(w_mem, 0, np.array([1.0], np.float32), np.array([-1.0], np.float32), 1, True)
        weff = w_mem / sigma
        assert abs(weff[0, 0]) == 1.0
        dst0 = np.array([[0.123]], np.float32)
        got = project_add(np.array([[3.21]], np.float32), weff, u, v, sigma, 0, None, dst0)
        assert got[0, 0] == dst0[0, 0]


def test_bad_arguments_are_refused():
    x = torch.zeros(64, device="cuda")
    lib, ctx = B.lib(), B.get_ctx()
    assert lib.gi_debug_sn_power_iteration(ctx, B.ptr(x), 0, 4, 0, B.ptr(x), B.ptr(x), 1, 1, B.ptr(x)) != 0
    assert lib.gi_debug_sn_power_iteration(ctx, B.ptr(x), 2, 24, 2, B.ptr(x), B.ptr(x), 1, 1, B.ptr(x)) != 0      # K != 16 cb
    assert lib.gi_debug_sn_power_iteration(ctx, B.ptr(x), 2, 4, 0, B.ptr(x), B.ptr(x), 0, 1, B.ptr(x)) != 0       # iters < 1
    assert lib.gi_debug_sn_project_add(ctx, B.ptr(x), B.ptr(x), B.ptr(x), B.ptr(x), None, 2, 4, 0, None, B.ptr(x)) != 0
