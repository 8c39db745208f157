"""GPU tier: differentiable augmentation inside the per-batch steps (trainer.MinimaxStep / WGANStep with diffaug=...), in the
pattern of test_autograd_surface_matches_fast_path (tests/test_steps_gpu.py): the fused step against reference-style plugin code
that drives a DiffAugment module at the same (seed, step, call) under autograd. Same builders, fixture inputs, imposed dropout
masks and tolerances as that file."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import gan_inpainting_amd  # noqa: F401,E402
from gan_inpainting_amd import backend as B  # noqa: E402
from gan_inpainting_amd import optim, trainer  # noqa: E402
from gan_inpainting_amd.lib.models import augment, loss, networks, util  # noqa: E402
from oracle import params as op  # noqa: E402
from util_golden import load, relerr, unpack_masks  # noqa: E402
from test_steps_gpu import LOSS_TOL, STAT_TOL, abs_sums, build, check_loss  # noqa: E402
import diffaug_ref as R  # noqa: E402

POLICY = "color,translation,cutout"
PARAM_TOL = 1e-4      # what test_autograd_surface_matches_fast_path holds the un-augmented pair to


def adam(net):
    return optim.Adam(net.parameters(), lr=0.0002, betas=(0.5, 0.999))


def rms(net):
    return optim.RMSprop(net.parameters(), lr=0.00005)


def test_minimax_step_matches_plugin_style_autograd():
    fx = load("minimax_steps")
    seed, N = int(fx["seed"]), int(fx["N"])
    g, m = op.synth_batch(seed * 100, N, 128, 128, fractional_edge=True)
    ground, mask_raw = torch.from_numpy(g).cuda(), torch.from_numpy(m).cuda()
    masks = unpack_masks(fx, "it0_")
    G1, (D1,) = build(seed, [seed + 1], True, "fp32")
    s1 = trainer.MinimaxStep(G1, D1, adam(G1), adam(D1), diffaug=POLICY)
    G1.impose_dropout_masks(masks)
    L1 = {k: float(v) for k, v in s1(ground, mask_raw).items()}
    # plugin style (minimaxgan_l1.py:113-173), every critic input through the module
    G2, (D2,) = build(seed, [seed + 1], True, "fp32")
    oG, oD = adam(G2), adam(D2)
    aug = augment.DiffAugment(POLICY)
    bce, l1 = loss.BCELoss(), loss.L1Loss()
    G2.impose_dropout_masks(masks)
    mask = torch.ceil(mask_raw)
    masked = ground * (1 - mask)
    inpainted = masked + G2(masked) * mask
    util.set_requires_grad([D2], True)
    oD.zero_grad()
    pr = D2(aug(ground, 0, 0)).view(-1)
    d_real = bce(pr, torch.ones(len(pr)).cuda())
    d_real.backward()
    pf = D2(aug(inpainted.detach(), 0, 1)).view(-1)
    d_fake = bce(pf, torch.zeros(len(pf)).cuda())
    d_fake.backward()
    oD.step()
    util.set_requires_grad([D2], False)
    oG.zero_grad()
    pf = D2(aug(inpainted, 0, 2)).view(-1)
    g_adv, rec = bce(pf, torch.ones(len(pf)).cuda()), l1(ground, inpainted)
    (g_adv + rec).backward()
    oG.step()
    torch.cuda.synchronize()
    for k, v in (("d_loss_real", d_real), ("d_loss_fake", d_fake), ("g_adv", g_adv), ("recon", rec)):
        check_loss("minimax diffaug", k, L1[k], float(v), "fp32")
    assert relerr(abs_sums(D2), abs_sums(D1)) <= PARAM_TOL
    assert relerr(abs_sums(G2), abs_sums(G1)) <= PARAM_TOL
    # the transform did something: the un-augmented step's critic losses differ
    G3, (D3,) = build(seed, [seed + 1], True, "fp32")
    s3 = trainer.MinimaxStep(G3, D3, adam(G3), adam(D3))
    G3.impose_dropout_masks(masks)
    L3 = {k: float(v) for k, v in s3(ground, mask_raw).items()}
    assert abs(L3["d_loss_real"] - L1["d_loss_real"]) > 1e-4 * abs(L3["d_loss_real"])


def test_wgan_step_matches_plugin_style_autograd():
    """One critic-only batch, then one with a generator update (RMSprop, weight clipping)."""
    fx = load("wgan_steps")
    seed, N = int(fx["seed"]), int(fx["N"])
    G1, (D1,) = build(seed, [seed + 1], False, "fp32")
    s1 = trainer.WGANStep(G1, D1, rms(G1), rms(D1), recon="l1", clip=0.01, diffaug=augment.DiffAugment(POLICY, seed=5))
    G2, (D2,) = build(seed, [seed + 1], False, "fp32")
    oG, oD = rms(G2), rms(D2)
    aug, l1 = augment.DiffAugment(POLICY, seed=5), loss.L1Loss()
    for it, upd in enumerate((False, True)):
        g, m = op.synth_batch(seed * 100 + it, N, 128, 128)
        ground, mask_raw = torch.from_numpy(g).cuda(), torch.from_numpy(m).cuda()
        masks = unpack_masks(fx, f"it{it}_")
        G1.impose_dropout_masks(masks)
        L1 = s1(ground, mask_raw, upd)
        torch.cuda.synchronize()
        L1 = {k: float(v) for k, v in L1.items()}
        G2.impose_dropout_masks(masks)
        mask = torch.ceil(mask_raw)
        masked = ground * (1 - mask)
        inpainted = masked + G2(masked) * mask
        util.set_requires_grad([D2], True)
        oD.zero_grad()
        d_real = D2(aug(ground, it, 0)).view(-1).mean()
        d_fake = D2(aug(inpainted.detach(), it, 1)).view(-1).mean()
        d_real.backward()              # backward(one)
        (-d_fake).backward()           # backward(mone)
        oD.step()
        util.clamp_parameters(D2, -0.01, 0.01)
        ref = {"d_loss_real": d_real, "d_loss_fake": d_fake}
        if upd:
            util.set_requires_grad([D2], False)
            oG.zero_grad()
            g_adv, rec = D2(aug(inpainted, it, 2)).view(-1).mean(), l1(ground, inpainted)
            (g_adv + rec).backward()
            oG.step()
            ref.update(g_adv=g_adv, recon=rec)
        torch.cuda.synchronize()
        for k, v in ref.items():
            check_loss(f"wgan diffaug it{it}", k, L1[k], float(v), "fp32", floor=2e-3)
        assert relerr(abs_sums(D2), abs_sums(D1)) <= PARAM_TOL
        assert relerr(abs_sums(G2), abs_sums(G1)) <= PARAM_TOL
    assert float(D1.flat_params().abs().max()) <= 0.01 + 1e-9


# ---- the smaller geometry of tests/test_streams_gpu.py for everything below ---------------------------------------------------------
def small(seed, dtype="fp32", hw=64, nd=6):
    sd = lambda P: {k: torch.from_numpy(np.array(v)) for k, v in P.items()}   # noqa: E731
    G = networks.UnetGenerator(1, 1, nd, ngf=64, use_dropout="False", dtype=dtype)
    G.load_state_dict(sd(op.make_unet_params(seed, num_downs=nd)))
    D = networks.PatchGANDiscriminator(sigmoid=False, image_size=hw, dtype=dtype)
    D.load_state_dict(sd(op.make_patchgan_params(seed + 1, hw, hw)))
    G, D = G.cuda(), D.cuda()
    G.set_dropout_seed(99)
    return G, D


def batches(k, n=4, hw=64):
    out = []
    for it in range(k):
        g, m = op.synth_batch(6000 + it, n, hw, hw)
        out.append((torch.from_numpy(g).cuda(), torch.from_numpy(m).cuda()))
    return out


def run_wgan(overlap, stacked, diffaug=POLICY, dtype="fp32", n_batches=4, **kw):
    G, D = small(21, dtype)
    args = {} if diffaug is False else {"diffaug": diffaug}
    step = trainer.WGANStep(G, D, rms(G), rms(D), recon="rmse", clip=0.01, overlap=overlap, stacked=stacked, **args, **kw)
    losses = []
    for it, (ground, mask) in enumerate(batches(n_batches)):
        L = step(ground, mask, it % 2 == 1)
        step.sync_for_logging()
        losses.append({k: float(v) for k, v in L.items()})
    torch.cuda.synchronize()
    return G.flat_params().clone(), D.flat_params().clone(), losses, step


def test_overlap_and_stacking_agree_under_augmentation():
    """As tests/test_streams_gpu.py holds the un-augmented step: the overlapped schedule equals the serial one bit for bit.
    Stacked and un-stacked critic passes are the same arithmetic per image in different launches; tests/test_steps_gpu.py holds
    both to one reference within LOSS_TOL / STAT_TOL, which is what they are held to against each other here."""
    runs = {(o, s): run_wgan(o, s) for o in (False, True) for s in (False, True)}
    for s in (False, True):
        g0, d0, l0, _ = runs[(False, s)]
        g1, d1, l1, _ = runs[(True, s)]
        assert torch.equal(d0, d1) and torch.equal(g0, g1), f"stacked={s}: the overlapped schedule differs from the serial one"
        assert l0 == l1
    (ga, da, la, _), (gb, db, lb, _) = runs[(False, False)], runs[(False, True)]
    for a, b in zip(la, lb):
        for k in a:
            assert relerr(a[k], b[k], floor=2e-3) <= LOSS_TOL["fp32"], (k, a[k], b[k])
    assert relerr(float(da.double().abs().sum()), float(db.double().abs().sum())) <= STAT_TOL["fp32"]
    assert relerr(float(ga.double().abs().sum()), float(gb.double().abs().sum())) <= STAT_TOL["fp32"]


@pytest.mark.parametrize("overlap,stacked", [(False, True), (True, True), (False, False)])
def test_gradient_penalty_is_taken_between_the_augmented_halves(overlap, stacked):
    n, hw = 4, 64
    G, D = small(31)
    step = trainer.WGANStep(G, D, rms(G), rms(D), recon="rmse", gp_lambda=10.0, overlap=overlap, stacked=stacked,
                            diffaug=augment.DiffAugment(POLICY, seed=2))
    eps = torch.from_numpy(np.random.default_rng(8).random(n).astype(np.float32)).cuda()
    step.gp_eps = eps
    (ground, mask), = batches(1, n, hw)
    L = step(ground, mask, False)
    step.sync_for_logging()
    torch.cuda.synchronize()
    got = float(L["gp"])
    # by hand: a critic with the weights the step started from, on the reference-augmented halves
    _, D2 = small(31)
    halves = []
    for call, img in ((0, ground), (1, step.inpainted)):
        x = img.cpu().numpy()[:, 0]
        rows = [R.fwd(x[i], R.params(7, 2, R.key_of(0, call, 0, n, i), hw, hw), True) for i in range(n)]
        halves.append(torch.from_numpy(np.stack(rows).astype(np.float32)[:, None]).cuda())
    want = float(D2.gradient_penalty(halves[0], halves[1], eps, 10.0))
    plain = float(small(31)[1].gradient_penalty(ground, step.inpainted, eps, 10.0))
    print(f"gp overlap={overlap} stacked={stacked}: step {got:.6f}, by hand {want:.6f}, un-augmented {plain:.6f}")
    assert abs(got - want) <= 1e-3 * abs(want) + 1e-6        # the bound tests/test_gp_gpu.py holds the penalty to
    assert abs(plain - want) > 1e-2 * abs(want)


def test_step_counter_survives_a_state_dict_round_trip():
    _, _, _, step = run_wgan(False, True, n_batches=3)
    sd = step.state_dict()
    assert sd["extra"]["diffaug_step"] == 3
    G, D = small(21)
    fresh = trainer.WGANStep(G, D, rms(G), rms(D), recon="rmse", clip=0.01, diffaug=POLICY)
    assert fresh._aug_step == 0
    fresh.load_state_dict(sd)
    assert fresh._aug_step == 3
    tables = [s.aug.params(s._aug_step, 1, 4, 64, 64).cpu().numpy() for s in (step, fresh)]
    assert np.array_equal(tables[0], tables[1])
    assert np.array_equal(tables[0].view(np.uint32), R.table(7, 0, R.key_of(3, 1, 0, 4, 0), 4, 64, 64))
    # and the next batch's real half is the same batch (it depends on the critic and on T0(ground) only)
    (ground, mask), = batches(1)
    D.load_state_dict(step.D.state_dict())
    la, lb = step(ground, mask, False), fresh(ground, mask, False)
    torch.cuda.synchronize()
    assert float(la["d_loss_real"]) == float(lb["d_loss_real"])
    assert step._aug_step == fresh._aug_step == 4


def test_dual_d_step_refuses_the_option():
    G, (Dg, Dl) = build(51, [52, 53], True, "fp32")
    oD = optim.Adam(optim.chain(Dl.parameters(), Dg.parameters()), lr=0.0002, betas=(0.5, 0.999))
    with pytest.raises(B.BackendError):
        trainer.DualDStep(G, Dg, Dl, adam(G), oD, diffaug=POLICY)


@pytest.mark.parametrize("overlap", [False, True])
def test_without_the_option_nothing_changes(overlap):
    """diffaug=None equals a step constructed without the argument bit for bit, adds no state key, and never reaches the library's
    gi_diffaug_* entries (counted on the Python wrapper)."""
    before = dict(augment.CALLS)
    g0, d0, l0, s0 = run_wgan(overlap, True, diffaug=False, n_batches=2)
    g1, d1, l1, s1 = run_wgan(overlap, True, diffaug=None, n_batches=2)
    assert torch.equal(g0, g1) and torch.equal(d0, d1) and l0 == l1
    assert augment.CALLS == before, "a step without diffaug called the augmentation entries"
    assert s1.state_dict()["extra"] == {} and not hasattr(s1, "aug_a")
    run_wgan(overlap, True, n_batches=1)
    assert augment.CALLS["gi_diffaug_apply"] == before["gi_diffaug_apply"] + 2


def test_fp16_critic_runs_and_reproduces():
    a = run_wgan(True, True, dtype="fp16", n_batches=3)
    b = run_wgan(True, True, dtype="fp16", n_batches=3)
    assert all(np.isfinite(v) for L in a[2] for v in L.values())
    assert torch.isfinite(a[0]).all() and torch.isfinite(a[1]).all()
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and a[2] == b[2]
