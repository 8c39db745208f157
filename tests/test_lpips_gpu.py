"""GPU tier: csrc/lpips.hip - the first layer, the fold, the tap kernel, the whole metric, its Python surface and the evaluation pass -
against tests/lpips_ref.py (fp64, three-channel definition). The `lpips` package is not installed here: nothing is compared with it, and
the weights are stand-ins (lpips_ref.make_params).

Bounds are not chosen here. Single kernels: the per-element bounds lpips_ref derives from their arithmetic. End to end: 4 x yardstick (b),
the error of the restatement with weights, input and every layer's output rounded to fp16 against its fp64 self, computed in the test
(as tests/test_fid_gpu.py does): max |restatement16 - restatement64| of the checked quantity, per tap map and for the distance. The five
terms of the distance are printed with their own yardsticks and not asserted: a maximum over three images is too noisy a yardstick for
a term (the two cases' differ by 2.5x for the same term). Measured ratios: DESIGN.md section 4.11."""
import os
import pickle

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import lpips_ref as R

pytestmark = pytest.mark.gpu


def _B():
    import gan_inpainting_amd  # noqa: F401
    from gan_inpainting_amd import backend as B
    return B


@pytest.fixture(scope="module")
def params():
    return R.make_params(11)


@pytest.fixture(scope="module")
def model(params):
    import gan_inpainting_amd  # noqa: F401
    from gan_inpainting_amd.lib.lpips import LPIPS
    m = LPIPS(max_pairs=4)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in params.items()})
    return m.cuda()


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).cuda()


def _conv1(xa, xb, wA, wB, bias):
    B = _B()
    n, _, H, W = xa.shape
    out = torch.empty(2 * n, H, W, 64, dtype=torch.float16, device="cuda")
    dxa, dxb, dwA, dwB, db = (_dev(t) for t in (xa, xb, wA, wB, bias))       # held until the call has been enqueued
    B.check(B.lib().gi_debug_lpips_conv1(B.get_ctx(), B.ptr(dxa), B.ptr(dxb), n, H, W, B.ptr(dwA), B.ptr(dwB), B.ptr(db), B.ptr(out)))
    return out.cpu().permute(0, 3, 1, 2).double()


def _tap(fa, fb, lin, pool):
    """fa, fb (n,C,h,w) float16 arrays -> (d (n,) float32 tensor on the CPU, pooled (2n,C,h/2,w/2) float16 or None)."""
    B = _B()
    n, Cc, H, W = fa.shape
    Fd = torch.from_numpy(np.concatenate([fa, fb])).permute(0, 2, 3, 1).contiguous().cuda()
    ws = torch.empty(B.lib().gi_debug_lpips_tap_ws_bytes(n) // 8, dtype=torch.float64, device="cuda")
    d = torch.empty(n, dtype=torch.float32, device="cuda")
    pooled = torch.empty(2 * n, H // 2, W // 2, Cc, dtype=torch.float16, device="cuda") if pool else None
    dlin = _dev(lin)
    B.check(B.lib().gi_debug_lpips_tap(B.get_ctx(), B.ptr(Fd), n, H, W, Cc, B.ptr(dlin), B.ptr(ws), ws.numel() * 8, B.ptr(d), B.ptr(pooled)))
    return d.cpu(), (pooled.cpu().permute(0, 3, 1, 2) if pool else None)


# ---- first layer -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 3])
@pytest.mark.parametrize("shape", [(16, 16), (32, 48)])
def test_first_layer_is_exact_on_exact_data_ring_included(shape, n):
    """Small-integer wA, wB, bias and pixels k / 8: every product and sum is exact in fp16 / fp32, so the kernel equals the fp64 reference."""
    rng = np.random.Generator(np.random.PCG64(100 + n + shape[1]))
    wA, wB = rng.integers(-4, 5, (64, 9)).astype(np.float32), rng.integers(-4, 5, (64, 9)).astype(np.float32)
    bias = rng.integers(-4, 5, 64).astype(np.float32)
    xa, xb = (rng.integers(0, 9, (n, 1) + shape) / 8.0).astype(np.float32), (rng.integers(0, 9, (n, 1) + shape) / 8.0).astype(np.float32)
    got = _conv1(xa, xb, wA, wB, bias)
    ref = R.conv1_two_plane(wA, wB, bias, np.concatenate([xa, xb]))
    ring = R.ring_mask(*shape)
    assert torch.equal(got[..., ring], ref[..., ring])
    assert torch.equal(got, ref)
    assert float(ref.max()) > 8.0
    # the test sees a beta folded into the bias: it differs on the ring
    assert not torch.equal(R.conv1_beta_in_bias(wA, wB, bias, np.concatenate([xa, xb]))[..., ring], ref[..., ring])


@pytest.mark.parametrize("n", [1, 3])
@pytest.mark.parametrize("shape", [(16, 16), (32, 48)])
def test_first_layer_within_its_bound(params, shape, n):
    w, b = params["features.0.weight"], params["features.0.bias"]
    wA, wB = (t.float().numpy() for t in R.fold(w, params["scaling_layer.shift"], params["scaling_layer.scale"]))
    xa, xb = R.make_images(40 + n, n, *shape), R.make_images(50 + n, n, *shape)
    got = _conv1(xa, xb, wA, wB, b)
    x = np.concatenate([xa, xb])
    ref, bound = R.conv1_two_plane(wA, wB, b, x), R.conv1_bound(wA, wB, b, x)
    err = (got - ref).abs()
    print(f"lpips conv1 {shape} n={n}: max err {float(err.max()):.3e}, max err / bound {float((err / bound).max()):.3f}, max|ref| {float(ref.max()):.3f}")
    assert bool((err <= bound).all())
    # and against the three-channel definition the folded weights came from
    ref3 = R.conv1_three_channel(w, b, params["scaling_layer.shift"], params["scaling_layer.scale"], x)
    assert bool(((got - ref3).abs() <= bound + 1e-5).all())


def test_fold_kernel_within_its_bound(params):
    B = _B()
    w, shift, scale = params["features.0.weight"], params["scaling_layer.shift"].reshape(3), params["scaling_layer.scale"].reshape(3)
    wA, wB = torch.empty(64, 9, device="cuda"), torch.empty(64, 9, device="cuda")
    dw, dshift, dscale = _dev(w), _dev(shift), _dev(scale)
    B.check(B.lib().gi_debug_lpips_fold(B.get_ctx(), B.ptr(dw), B.ptr(dshift), B.ptr(dscale), B.ptr(wA), B.ptr(wB)))
    rA, rB = R.fold(w, shift, scale)
    bA, bB = R.fold_bound(w, shift, scale)
    eA, eB = (wA.cpu().double() - rA).abs(), (wB.cpu().double() - rB).abs()
    print(f"lpips fold: max err / bound {float((eA / bA).max()):.3f} (wA), {float((eB / bB).max()):.3f} (wB)")
    assert bool((eA <= bA).all()) and bool((eB <= bB).all())


# ---- tap kernel --------------------------------------------------------------------------------------------------------------------
def _tap_data(Cc, hw, n, seed):
    rng = np.random.Generator(np.random.PCG64(seed))
    fa = np.maximum(rng.standard_normal((n, Cc, hw, hw)), 0).astype(np.float16)
    fb = np.maximum(fa.astype(np.float32) + 0.4 * rng.standard_normal((n, Cc, hw, hw)), 0).astype(np.float16)
    fb[0, :, 0, 0] = 0                                   # a zero channel vector against a live one
    if hw > 1:
        fa[-1, :, 1, 1] = 0                              # both zero
        fb[-1, :, 1, 1] = 0
    lin = (rng.random(Cc) * 2 / Cc).astype(np.float32)
    return fa, fb, lin


@pytest.mark.parametrize("hw", [1, 2, 4, 16])
@pytest.mark.parametrize("Cc", [64, 128, 256, 512])
def test_tap_kernel(Cc, hw):
    for pool in ((False, True) if hw > 1 else (False,)):
        for n in (1, 3):
            fa, fb, lin = _tap_data(Cc, hw, n, 1000 + Cc + hw)
            d, pooled = _tap(fa, fb, lin, pool)
            ref, bound = R.tap_distance(fa, fb, lin), R.tap_bound(fa, fb, lin)
            err = (d.double() - ref).abs()
            print(f"lpips tap C={Cc} {hw}x{hw} n={n} pool={pool}: max err / bound {float((err / bound).max()):.3f}, d {ref.tolist()}")
            assert bool(torch.isfinite(d).all()) and bool((err <= bound).all())
            d2, pooled2 = _tap(fa, fb, lin, pool)
            assert torch.equal(d, d2)                                                   # two runs: the same bits
            same, _ = _tap(fa, fa, lin, pool)
            assert torch.equal(same, torch.zeros(n))                                    # identical halves: exactly 0.0
            zero, _ = _tap(np.zeros_like(fa), np.zeros_like(fa), lin, pool)
            assert torch.equal(zero, torch.zeros(n))                                    # zero vectors: 0, not NaN
            fn = R.near_identical(fa, Cc + hw)                                          # nearly equal halves: the bound is sharp there
            dn, _ = _tap(fa, fn, lin, pool)                                             # (the expanded five-sum form does not pass it)
            refn, boundn = R.tap_distance(fa, fn, lin), R.tap_bound(fa, fn, lin)
            errn = (dn.double() - refn).abs()
            print(f"lpips tap C={Cc} {hw}x{hw} n={n} pool={pool} near-identical: d {refn.tolist()} err {errn.tolist()} bound {boundn.tolist()}")
            assert bool((errn <= boundn).all())
            if pool:
                want = F.max_pool2d(torch.from_numpy(np.concatenate([fa, fb])).float(), 2).half()
                assert torch.equal(pooled, want) and torch.equal(pooled2, want)         # bit-equal to a max pool
            if n == 3:
                for i in range(3):                                                      # image i alone: the same bits as inside n = 3
                    di, _ = _tap(fa[i:i + 1], fb[i:i + 1], lin, pool)
                    assert torch.equal(di, d[i:i + 1]), (i, di, d)


@pytest.mark.parametrize("Cc,hw,pool", [(512, 32, False), (512, 64, True), (64, 70, False), (64, 140, True)])
def test_tap_kernel_grid_stride(Cc, hw, pool):
    """Maps on which a workgroup takes more than one unit per lane group and the grid sits at its cap of 128 workgroups per image:
    C = 512 (4 units per workgroup and pass): 1024 units = two full passes; C = 64 (32 units per workgroup and pass, 4096 per pass):
    4900 units, so the second pass ends inside a wave - the lane groups of one wave take different numbers of units."""
    fa, fb, lin = _tap_data(Cc, hw, 3, 2000 + Cc + hw)
    d, pooled = _tap(fa, fb, lin, pool)
    ref, bound = R.tap_distance(fa, fb, lin), R.tap_bound(fa, fb, lin)
    err = (d.double() - ref).abs()
    print(f"lpips tap grid-stride C={Cc} {hw}x{hw} pool={pool}: max err / bound {float((err / bound).max()):.3f}")
    assert bool((err <= bound).all())
    if pool:
        assert torch.equal(pooled, F.max_pool2d(torch.from_numpy(np.concatenate([fa, fb])).float(), 2).half())
    for i in range(3):                                                                  # image i alone: the same bits as inside n = 3
        di, _ = _tap(fa[i:i + 1], fb[i:i + 1], lin, pool)
        assert torch.equal(di, d[i:i + 1]), (i, di, d)
    same, _ = _tap(fa, fa, lin, pool)
    assert torch.equal(same, torch.zeros(3))
    fn = R.near_identical(fa, Cc + hw)
    dn, _ = _tap(fa, fn, lin, pool)
    assert bool(((dn.double() - R.tap_distance(fa, fn, lin)).abs() <= R.tap_bound(fa, fn, lin)).all())


# ---- end to end --------------------------------------------------------------------------------------------------------------------
_REF = {}


def _reference(params, shape):
    """fp64 taps and distances, and their fp16-rounded restatement, of one seeded case: computed once."""
    if shape not in _REF:
        a, b = R.make_images(70 + shape[0], 3, *shape), R.make_images(80 + shape[0], 3, *shape)
        _REF[shape] = dict(a=a, b=b, taps64=R.taps(params, a), taps16=R.taps(params, a, fp16=True), d64=R.distance(params, a, b),
                           d16=R.distance(params, a, b, fp16=True))
    return _REF[shape]


@pytest.mark.parametrize("shape", [(32, 32), (48, 32)])
def test_features_and_distance_end_to_end(model, params, shape):
    ref = _reference(params, shape)
    a, b = _dev(ref["a"]), _dev(ref["b"])
    for t in range(5):
        got = model.features(a, t).cpu().double()
        yard = float((ref["taps16"][t] - ref["taps64"][t]).abs().max())
        err = float((got - ref["taps64"][t]).abs().max())
        print(f"lpips features {shape} tap {t}: max|err| {err:.3e}, yardstick (b) {yard:.3e}, ratio {err / yard:.3f}, max|ref| {float(ref['taps64'][t].max()):.3f}")
        assert tuple(got.shape) == tuple(ref["taps64"][t].shape) and bool(torch.isfinite(got).all())
        assert err <= 4.0 * yard
    d, per = model.distance(a, b, per_layer=True)
    d, per = d.cpu().double(), per.cpu().double()
    (d64, per64), (d16, per16) = ref["d64"], ref["d16"]
    yard = float((d16 - d64).abs().max())                            # the restatement's own error in the checked quantity
    err = float((d - d64).abs().max())
    print(f"lpips distance {shape}: d {d.tolist()} ref {d64.tolist()} max|err| {err:.3e}, yardstick (b) {yard:.3e}, ratio {err / yard:.3f}")
    print(f"lpips per-layer {shape}: max|err| {(per - per64).abs().max(1).values.tolist()} yardsticks {(per16 - per64).abs().max(1).values.tolist()}")
    assert err <= 4.0 * yard
    assert float((per.sum(0) - d).abs().max()) <= 1e-6 * float(d.max())
    assert torch.equal(model.distance(a, a).cpu(), torch.zeros(3))   # identical inputs: exactly 0.0 through the whole network
    assert torch.equal(model.distance(a, b).cpu().double(), d)       # reproducible


def test_chunking_gives_the_same_bits(params):
    """At 32x32 no layer reaches the grid at which the dispatch changes the implicit-GEMM family, so chunks of 2 and 1 run the same kernels
    and the bits must agree. Across sizes where the family changes with the chunk this is not promised (LPIPS.distance says so)."""
    import gan_inpainting_amd  # noqa: F401
    from gan_inpainting_amd.lib.lpips import LPIPS
    m = LPIPS(max_pairs=2)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in params.items()})
    m = m.cuda()
    a, b = _dev(R.make_images(90, 5, 32, 32)), _dev(R.make_images(91, 5, 32, 32))
    whole = m.distance(a, b)
    single = torch.cat([m.distance(a[i:i + 1], b[i:i + 1]) for i in range(5)])
    assert tuple(whole.shape) == (5,) and torch.equal(whole, single)
    B = _B()
    with pytest.raises(B.BackendError, match="grey"):
        m.distance(a.repeat(1, 3, 1, 1), b.repeat(1, 3, 1, 1))


# ---- the evaluation pass -----------------------------------------------------------------------------------------------------------
class _FixedNet:
    def __init__(self, gens):
        self.gens, self.i = gens, 0

    def __call__(self, masked):
        g = self.gens[self.i]
        self.i += 1
        return g


def _eval_batches():
    batches, gens = [], []
    for bi in range(2):
        rng = np.random.Generator(np.random.PCG64(300 + bi))
        g = R.make_images(310 + bi, 3, 32, 32)
        mk = np.zeros((3, 1, 32, 32), np.float32)
        mk[:, :, 8:20, 4 + bi:24] = 1.0
        batches.append((torch.from_numpy(g), torch.from_numpy(mk), 0))
        gens.append(torch.from_numpy(rng.random((3, 1, 32, 32), dtype=np.float32)).cuda())
    return batches, gens


def test_calculate_metric_with_lpips(model):
    B = _B()
    from gan_inpainting_amd.lib.models import evaluate
    batches, gens = _eval_batches()
    plain = evaluate.calculate_metric(torch.device("cuda"), batches, _FixedNet(gens), epoch=3)
    met = evaluate.calculate_metric(torch.device("cuda"), batches, _FixedNet(gens), epoch=3, lpips_model=model)
    assert "lpips" not in plain and set(met) == set(plain) | {"lpips"}
    for k, v in plain.items():
        assert met[k] == v, k                                         # the other keys: bit for bit what they are without it
    total, dists = None, []
    for (g, mk, _), gen in zip(batches, gens):                        # the pass's own composite: masked + out * m, not quantised
        inp, mask = g.cuda(), mk.cuda()
        m, masked, comp = torch.empty_like(mask), torch.empty_like(inp), torch.empty_like(inp)
        B.check(B.lib().gi_mask_apply(B.get_ctx(), B.ptr(inp), B.ptr(mask), B.ptr(m), B.ptr(masked), inp.numel(), 1))
        B.check(B.lib().gi_mask_composite(B.get_ctx(), B.ptr(masked), B.ptr(gen), B.ptr(m), B.ptr(comp), gen.numel()))
        assert torch.equal(comp.cpu(), (gen.cpu() * torch.ceil(mk) + g * (1 - torch.ceil(mk))))
        d = model.distance(comp, inp)
        dists.append(d)
        total = d.sum() if total is None else total + d.sum()
    assert met["lpips"] == float(total) / 6
    mean = float(torch.cat(dists).double().mean())
    assert np.isfinite(met["lpips"]) and met["lpips"] > 0 and abs(met["lpips"] - mean) <= 1e-6 * mean


def test_plugin_writes_lpips_with_lpips_weights(tmp_path, params):
    import gan_inpainting_amd  # noqa: F401
    from gan_inpainting_amd import train
    tv, lin = str(tmp_path / "vgg16_standin.pth"), str(tmp_path / "lpips_vgg_standin.pth")
    torch.save({k: torch.from_numpy(v) for k, v in params.items() if k.startswith("features.")}, tv)
    torch.save({k: torch.from_numpy(v) for k, v in params.items() if k.startswith("lin")}, lin)
    train.main(["-exp", "minimaxgan_l1", "-ep", "1", "-b", "4", "--imagedim", "64", "--saveevery", "1", "--evalevery", "1",
                "--data", "synthetic", "--samples", "16", "--outdir", str(tmp_path), "--dtype", "fp16", "--lpips-weights", tv, lin])
    with open(os.path.join(str(tmp_path), "model", "minimaxgan_l1", "eval_history.obj"), "rb") as h:
        ev = pickle.load(h)
    assert set(ev[-1]) == {"train", "test"}
    for part in ev[-1].values():
        assert set(part) == {"recon_rmse_global", "recon_l1_global", "recon_rmse_local", "recon_l1_local", "fid", "epoch", "lpips"}
        assert isinstance(part["lpips"], float) and np.isfinite(part["lpips"]) and part["lpips"] > 0.0
