"""GPU tier: the opt-in backward of LPIPS (csrc/lpips.hip) end to end against fp64 autograd over the guarded restatement
(tests/lpips_grad_ref.py), its Python / autograd surface and the WGAN training step with the term. Stand-in weights
(lpips_ref.make_params): the `lpips` package and its weights are not available here.

Bounds are not tuned to the device: every comparison of a gradient uses
    bound = 2 x (relative L2 error of the fp16-storage emulation - the restatement with weights, input and every layer's output rounded
                 to fp16, straight-through - against the fp64 restatement, for that same case and tensor)
and cosine >= 1 - bound^2, as tests/test_vgg_grad_gpu.py does. The factor 2: the device accumulates in fp32, rounds its seeds and
gradients to fp16 and takes its own, independent set of ReLU / pool decisions where the fp16 forward lands on the other side of a kink.
"""
import numpy as np
import pytest
import torch

import lpips_grad_ref as G
import lpips_ref as R

pytestmark = pytest.mark.gpu

CASES = [(5, 2, 32, 32), (7, 3, 48, 32), (9, 2, 64, 64)]
_ref_cache = {}


def _B():
    import gan_inpainting_amd  # noqa: F401
    from gan_inpainting_amd import backend as B
    return B


def _model(P, max_pairs, grad=True):
    import gan_inpainting_amd  # noqa: F401
    from gan_inpainting_amd.lib.lpips import LPIPS
    m = LPIPS(max_pairs=max_pairs, grad=grad)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in P.items()})
    return m.cuda()


def _case(seed, n, h, w):
    """(P, a, b, fp64 (d, grad, tap grads), fp16-emulation (d, grad, tap grads)), computed once per case."""
    key = (seed, n, h, w)
    if key not in _ref_cache:
        P = R.make_params(seed)
        a, b = R.make_images(seed + 1, n, h, w), R.make_images(seed + 2, n, h, w)
        _ref_cache[key] = (P, a, b, G.grad(P, a, b, with_taps=True), G.grad(P, a, b, fp16=True, with_taps=True))
    return _ref_cache[key]


def _check(tag, got, ref, emu):
    bound = 2.0 * G.rel_l2(emu, ref)
    rel, cos = G.rel_l2(got, ref), G.cosine(got, ref)
    print(f"{tag}: device rel L2 {rel:.3e} cos {cos:.7f} | fp16 emulation {bound / 2:.3e} -> bound {bound:.3e}, cos >= {1 - bound * bound:.7f}")
    assert torch.isfinite(got).all(), tag
    assert rel <= bound, f"{tag}: rel L2 {rel:.3e} > {bound:.3e}"
    assert cos >= 1.0 - bound * bound, f"{tag}: cosine {cos:.7f}"


@pytest.mark.parametrize("seed,n,h,w", CASES)
def test_image_gradient_vs_fp64_autograd(seed, n, h, w):
    """Measured on MI355X: relative L2 of the whole image gradient (the fp16-storage emulation's own error; bound = 2 x that), cosine
         seed 5, n 2, 32x32   1.568e-2 (1.595e-2)  0.999877
         seed 7, n 3, 48x32   1.806e-2 (1.619e-2)  0.999837
         seed 9, n 2, 64x64   2.199e-2 (2.183e-2)  0.999758
       i.e. 0.98 - 1.12 x the emulation's own error. The fp64 reference has no zero tap vector (asserted below) and no NaN."""
    P, a, b, ref, emu = _case(seed, n, h, w)
    assert torch.isfinite(ref[1]).all() and all(float(t.pow(2).sum(1).min()) > 0 for t in G.taps(P, G._t(a))), "a zero vector in the reference"
    m = _model(P, n)
    da, db = torch.from_numpy(a).cuda(), torch.from_numpy(b).cuda()
    d, g = m.distance_and_grad(da, db)
    assert g.shape == da.shape and g.dtype == torch.float32
    _check(f"seed {seed} n {n} {h}x{w} image", g.cpu(), ref[1], emu[1])
    # the values are the forward-only entry's and a grad=False model's, bit for bit
    plain = _model(P, n, grad=False)
    assert torch.equal(d, m.distance(da, db)) and torch.equal(d, plain.distance(da, db))


@pytest.mark.parametrize("seed,n,h,w", CASES)
def test_tap_gradients_vs_fp64_autograd(seed, n, h, w):
    """gi_lpips_grad_tap for the five taps, the same rule per tap: a failure names its tap. Measured on MI355X: relu5_3 5.0e-3 - 6.1e-3
    (0.49 of its bound), the four pooled taps 2.5e-2 - 5.9e-2, at most 0.60 of their bounds (tap 1 of the 48x32 case, 5.2e-2 against
    8.7e-2): single ReLU / pool decisions the fp16 forward takes differently from fp64, of the same size in the emulation."""
    P, a, b, ref, emu = _case(seed, n, h, w)
    m = _model(P, n)
    da, db = torch.from_numpy(a).cuda(), torch.from_numpy(b).cuda()
    m.distance_and_grad(da, db)
    failures = []
    for tap in range(4, -1, -1):
        got = m.grad_tap(tap, da).cpu()
        assert got.shape == ref[2][tap].shape
        try:
            _check(f"seed {seed} n {n} {h}x{w} tap {tap}", got, ref[2][tap], emu[2][tap])
        except AssertionError as e:
            failures.append(str(e))
    assert not failures, failures


def test_properties():
    B = _B()
    seed, n, h, w = CASES[0]
    P, a, b, ref, emu = _case(seed, n, h, w)
    m = _model(P, n)
    plain = _model(P, n, grad=False)
    da, db = torch.from_numpy(a).cuda(), torch.from_numpy(b).cuda()
    # the forward-only workspace is what it was: the grad workspace is a second one
    lib = B.lib()
    hd, hp = m._handle(h, w, da.device), plain._handle(h, w, da.device)
    assert lib.gi_lpips_workspace_bytes(hd) == lib.gi_lpips_workspace_bytes(hp) and lib.gi_lpips_grad_workspace_bytes(hd) > 0
    # bit-reproducible
    d1, g1 = m.distance_and_grad(da, db)
    d2, g2 = m.distance_and_grad(da, db)
    assert torch.isfinite(g1).all() and float(g1.abs().max()) > 0
    assert torch.equal(g1, g2) and torch.equal(d1, d2)
    # a == b: exactly zero, no NaN
    d0, g0 = m.distance_and_grad(da, da)
    assert torch.equal(d0, torch.zeros_like(d0)) and torch.equal(g0, torch.zeros_like(g0))
    # gscale: a power of two scales the bits exactly
    for k in (3, -5):
        _, gk = m.distance_and_grad(da, db, gscale=2.0 ** k)
        assert torch.equal(gk, g1 * 2.0 ** k)
    _, g3 = m.distance_and_grad(da, db, gscale=3.0)
    assert G.rel_l2(g3.cpu(), (g1 * 3.0).cpu()) <= 1e-6
    # no grad workspace: a clean error
    with pytest.raises(B.BackendError):
        plain.distance_and_grad(da, db)
    with pytest.raises(B.BackendError):
        plain.grad_tap(0, da)


def test_nearly_identical_pair_and_per_image_scales():
    """b = a + 1e-3 noise (d ~ 1e-7): within the same rule. In one chunk with a very different pair each image keeps the bits of its
    single-pair call: one scale per image, and 32x32 chunks of 1 and 2 pairs run on the same kernels. Measured on MI355X: the near pair
    (d = 6.9e-7) 1.41e-1 against the emulation's 1.42e-1 (the forward's fp16 rounding of nearly equal maps dominates both), the far pair
    (d = 1.6e-2) 1.91e-2 against 1.89e-2."""
    seed, _, h, w = CASES[0]
    P = R.make_params(seed)
    rng = np.random.Generator(np.random.PCG64(77))
    a = R.make_images(seed + 1, 2, h, w)
    b = R.make_images(seed + 2, 2, h, w)
    b[0] = np.clip(a[0] + 1e-3 * rng.standard_normal(a[0].shape), 0.0, 1.0).astype(np.float32)
    dref, gref = G.grad(P, a, b)
    _, gemu = G.grad(P, a, b, fp16=True)
    print("distances", dref.tolist())
    assert float(dref[0]) < 1e-5 < 1e-3 < float(dref[1])
    m = _model(P, 2)
    da, db = torch.from_numpy(a).cuda(), torch.from_numpy(b).cuda()
    d, g = m.distance_and_grad(da, db)
    for i in range(2):
        _check(f"pair {i} (d = {float(dref[i]):.3e})", g[i:i + 1].cpu(), gref[i:i + 1], gemu[i:i + 1])
    for i in range(2):
        di, gi = m.distance_and_grad(da[i:i + 1], db[i:i + 1])
        assert torch.equal(gi, g[i:i + 1]) and torch.equal(di, d[i:i + 1]), i


def test_chunking_equals_single_calls():
    seed, _, h, w = CASES[0]
    P = R.make_params(seed)
    a, b = R.make_images(seed + 11, 5, h, w), R.make_images(seed + 12, 5, h, w)
    m = _model(P, 2)
    da, db = torch.from_numpy(a).cuda(), torch.from_numpy(b).cuda()
    d, g, per = m.distance_and_grad(da, db, per_layer=True)
    assert torch.equal(d, m.distance(da, db)) and torch.allclose(per.sum(0), d, rtol=1e-6, atol=0)
    for i in range(5):
        di, gi = m.distance_and_grad(da[i:i + 1], db[i:i + 1])
        assert torch.equal(gi, g[i:i + 1]) and torch.equal(di, d[i:i + 1]), i


def test_autograd_surface_and_refusals():
    B = _B()
    import gan_inpainting_amd  # noqa: F401
    from gan_inpainting_amd import optim, trainer
    from gan_inpainting_amd.lib.models import loss
    seed, n, h, w = CASES[0]
    P, a, b, ref, emu = _case(seed, n, h, w)
    m = _model(P, n)
    plain = _model(P, n, grad=False)
    da, db = torch.from_numpy(a).cuda(), torch.from_numpy(b).cuda()
    d, g = m.distance_and_grad(da, db)
    x = da.clone().requires_grad_()
    val = loss.lpips_loss(x, db, m, weight=4.0)
    assert val.grad_fn is not None and float(val.detach()) == float(d.mean() * 4.0)
    (2.0 * val).backward()
    _, g8 = m.distance_and_grad(da, db, gscale=4.0 / n)
    assert torch.equal(x.grad, g8 * 2.0)
    # no gradient is taken when the output does not require one; a grad=False model serves that case
    v0 = loss.lpips_loss(da, db, plain, weight=4.0)
    assert v0.grad_fn is None and not v0.requires_grad and float(v0) == float(val.detach())
    with pytest.raises(B.BackendError):
        loss.lpips_loss(da.clone().requires_grad_(), db, plain)
    # the steps: the WGAN step wants a grad model, the others refuse the term
    from test_steps_gpu import build
    Gn, (Dn,) = build(1, [2], False, "fp32")
    oG, oD = optim.RMSprop(Gn.parameters(), lr=5e-5), optim.RMSprop(Dn.parameters(), lr=5e-5)
    with pytest.raises(B.BackendError):
        trainer.WGANStep(Gn, Dn, oG, oD, lpips=plain, lpips_weight=1.0)
    with pytest.raises(B.BackendError):
        trainer.MinimaxStep(Gn, Dn, oG, oD, lpips=m, lpips_weight=1.0)
    with pytest.raises(B.BackendError):
        trainer.DualDStep(Gn, Dn, Dn, oG, oD, lpips=m, lpips_weight=1.0)


# ---- the training step with the term -----------------------------------------------------------------------------------------------
# Weight chosen on the CPU: in the fp32 oracle, at the generator update of the wgan_steps fixture (seed 41, N = 2, 128x128, batch 1), the
# L2 norm of the image gradient of g_adv + recon (L1) is 1.566e-3 and that of mean_i LPIPS (restatement, make_params(seed + 3)) is
# 4.353e-5 per unit weight: STEP_W = 32 gives a ratio of 0.89, inside the 0.3x - 3x window.
STEP_W = 32.0
_oracle_cache = {}


def _oracle_step(weight):
    """The batches of wgan_steps on the oracle (fp32, the fixture's dropout masks) with weight * mean_i d_i from the restatement added to
    the generator's loss."""
    if weight in _oracle_cache:
        return _oracle_cache[weight]
    from oracle import params as op
    from oracle import torch_ref as orc
    from util_golden import load, unpack_masks
    fx = load("wgan_steps")
    seed, N = int(fx["seed"]), int(fx["N"])
    OG, OD = orc.to_torch(op.make_unet_params(seed)), orc.to_torch(op.make_patchgan_params(seed + 1))
    oG, oD = orc.RMSprop(orc.trainable(OG)), orc.RMSprop(orc.trainable(OD))
    P = R.make_params(seed + 3)
    res = {}

    def fn(inpainted, ground, mc):
        d, _ = G.distance(P, inpainted.double(), ground.double())
        term = (weight * d.mean()).to(inpainted.dtype)
        return term, {"lpips_loss": float(term.detach())}
    for it, upd in enumerate(int(v) for v in fx["pattern"]):
        g, mk = op.synth_batch(seed * 100 + it, N, 128, 128)
        o = orc.wgan_step(OG, OD, oG, oD, torch.from_numpy(g), torch.from_numpy(mk), 7, unpack_masks(fx, f"it{it}_"), bool(upd), recon="l1", extra=fn)
        if upd:
            res = dict(absmean=dict(o["g_grad_absmean"]), lpips_loss=o["lpips_loss"], recon=o["recon"], g_adv=o["g_adv"])
            # yardstick (b) of the term's value on this batch: the restatement with fp16 storage against its fp64 self
            with torch.no_grad():
                d16, _ = G.distance(P, o["inpainted"].double(), torch.from_numpy(g).double(), fp16=True)
                d64, _ = G.distance(P, o["inpainted"].double(), torch.from_numpy(g).double())
            res["lpips_yard"] = weight * abs(float(d16.mean() - d64.mean()))
    names = [str(s) for s in fx["g_param_names"]]
    res["stats"] = np.array([float(OG[k].detach().double().abs().sum()) for k in names])
    _oracle_cache[weight] = res
    return res


def test_oracle_step_sees_the_term():
    """Against the oracle alone: with weight 0 the same step lies outside the step test's gradient tolerances for more than half of
    the tensors, so the step test cannot pass without the feature."""
    d, c = _oracle_step(STEP_W), _oracle_step(0.0)
    for tol in (5e-3, 8e-2):
        out = [k for k, v in d["absmean"].items() if abs(c["absmean"][k] - v) > tol * abs(v) + 1e-12]
        print(f"tol {tol}: {len(out)} of {len(d['absmean'])} tensors outside")
        assert len(out) > len(d["absmean"]) // 2


def _device_step(dtype, overlap):
    from gan_inpainting_amd import optim, trainer
    from gan_inpainting_amd.lib.models import util
    from oracle import params as op
    from test_steps_gpu import build
    from util_golden import load, unpack_masks
    fx = load("wgan_steps")
    seed, N = int(fx["seed"]), int(fx["N"])
    Gn, (Dn,) = build(seed, [seed + 1], False, dtype)
    lp = _model(R.make_params(seed + 3), N)
    oG = optim.RMSprop(Gn.parameters(), lr=0.00005)
    oD = optim.RMSprop(Dn.parameters(), lr=0.00005)
    step = trainer.WGANStep(Gn, Dn, oG, oD, recon="l1", clip=0.01, overlap=overlap, lpips=lp, lpips_weight=STEP_W)
    L, gflow = None, None
    for it, upd in enumerate(int(v) for v in fx["pattern"]):
        g, mk = op.synth_batch(seed * 100 + it, N, 128, 128)
        Gn.impose_dropout_masks(unpack_masks(fx, f"it{it}_"))
        L = step(torch.from_numpy(g).cuda(), torch.from_numpy(mk).cuda(), bool(upd))
        step.sync_for_logging()
        torch.cuda.synchronize()
        if upd:
            gflow = util.GradFlow(Gn)
            gflow.measure()
            gflow = gflow.as_dict()
            Lupd = {k: float(v) for k, v in L.items()}
    return Gn, gflow, Lupd, step


@pytest.mark.parametrize("dtype", ["fp32", "fp16"])
def test_step_with_lpips_vs_oracle(dtype):
    """The three batches of wgan_steps (one generator update) at 128x128 with WGANStep(lpips=..., lpips_weight=STEP_W) against
    orc.wgan_step with the restatement's term; tolerances of tests/test_steps_gpu.py and of the VGG-19 step test (per-tensor mean |grad|
    5e-3 / 8e-2, parameter statistics STAT_TOL, losses LOSS_TOL). overlap=True gives bit-identical parameters and gradients; the
    step's state survives a state_dict round trip. Measured on MI355X: worst per-tensor mean |grad| 1.5e-3 (fp32) and 1.2e-2 (fp16),
    parameter statistics 1.5e-5 and 1.2e-4, the term's value 0.065846 / 0.065845 against the oracle's 0.065847."""
    from test_steps_gpu import LOSS_TOL, STAT_TOL, abs_sums
    from util_golden import relerr
    ref = _oracle_step(STEP_W)
    Gn, absmean, L, step = _device_step(dtype, False)
    # the term's value: the generator's own deviation (LOSS_TOL, as for the other losses) plus 4 x yardstick (b) of the distance on this
    # batch, the rule of tests/test_lpips_gpu.py for the fp16-storage forward
    lp_tol = LOSS_TOL[dtype] * ref["lpips_loss"] + 4.0 * ref["lpips_yard"]
    print("lpips_loss", L["lpips_loss"], ref["lpips_loss"], "bound", lp_tol, "recon", L["recon"], ref["recon"])
    assert abs(L["lpips_loss"] - ref["lpips_loss"]) <= lp_tol
    assert abs(L["recon"] - ref["recon"]) <= LOSS_TOL[dtype] * ref["recon"]
    tol = 5e-3 if dtype == "fp32" else 8e-2
    worst = max(abs(v - ref["absmean"][k]) / (abs(ref["absmean"][k]) + 1e-12) for k, v in absmean.items())
    print(f"{dtype}: worst per-tensor mean |grad| rel {worst:.3e} (bound {tol})")
    stat = relerr(abs_sums(Gn), ref["stats"])
    print(f"{dtype}: parameter statistics rel {stat:.3e} (bound {STAT_TOL[dtype]})")
    for k, v in absmean.items():
        assert abs(v - ref["absmean"][k]) <= tol * abs(ref["absmean"][k]) + 1e-12, f"absmean {k}: {v} vs {ref['absmean'][k]}"
    assert stat <= STAT_TOL[dtype]
    # overlap=True: the same gradients and parameters, bit for bit
    G2, _, _, step2 = _device_step(dtype, True)
    assert torch.equal(Gn.flat_params(), G2.flat_params())
    for (k, x), (_, y) in zip(Gn.named_parameters(), G2.named_parameters()):
        assert torch.equal(x.grad, y.grad), k
    # the extra state: on an fp16 generator the term's largest per-pixel gradient was folded into recon_weight once
    st = step.state_dict()
    ex = st["extra"]
    assert "lpips_fold" in ex and ex["recon_weight"] == step.recon_weight
    if dtype == "fp16":
        assert ex["lpips_fold"] > 0 and ex["recon_weight"] == 1.0 + ex["lpips_fold"] and tuple(ex["lpips_scaled_for"]) == (2, 1, 128, 128)
    else:
        assert ex["lpips_fold"] == 0.0 and ex["lpips_scaled_for"] is None
    step2.recon_weight, step2._lpips_fold, step2._lpips_scaled_for = 1.0, 0.0, None
    step2.load_state_dict(st)
    assert step2.recon_weight == step.recon_weight and step2._lpips_fold == step._lpips_fold
    assert step2._lpips_scaled_for == step._lpips_scaled_for
    assert step2.state_dict()["extra"] == ex
