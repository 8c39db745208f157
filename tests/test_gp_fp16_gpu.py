"""GPU tier: the WGAN-GP gradient penalty (an EXTENSION, see tests/test_gp_gpu.py) on fp16 critics.

The reference is the oracle's fp64 double backward (torch.autograd.grad(create_graph=True), as
oracle.torch_ref.gradient_penalty) evaluated with the kink decisions of the penalty's OWN primal forward
(gi_patchgan_gp_saved_activation) on the units within oracle.kink.FP16_BAND of a kink, as the fp16 network parity
tests do (gpu_util.check_grads_vs_kink_reference). Bounds: about 2x the errors measured on MI355X
(profiles/r05_gp_fp16_measured_errors.txt)."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import gan_inpainting_amd  # noqa: F401,E402
from gan_inpainting_amd.lib.models import networks  # noqa: E402
from oracle import kink  # noqa: E402
from oracle import params as op  # noqa: E402
from oracle import torch_ref as orc  # noqa: E402
from gpu_util import rel_l2  # noqa: E402

# relative errors against the fp64 reference, about 2x the worst measured on MI355X (profiles/r05_gp_fp16_measured_errors.txt)
TOL_PENALTY = 3e-4         # measured <= 1.5e-4
TOL_GRAD_L2 = 1e-2         # measured <= 5.3e-3 (model.2.weight at 64x64)
TOL_RUNNING = 2.5e-4       # BatchNorm running statistics after the penalty's forward; measured <= 1.03e-4
# whole stacked critic batch: its D(ground) | D(inpainted) terms are compared WITHOUT the kink correction (their decisions live in
# the step's own slots), and the BatchNorm-4 shift's gradient is a difference of two near-equal population means; measured
# <= 6.8e-2 there (<= 4.7e-2 elsewhere) while the penalty's own share stays <= 5.3e-3 (TOL_GRAD_L2). Bound above the issue's
# proposed 5e-2 for that reason.
TOL_STACKED_PENALTY = 3e-3  # measured <= 1.3e-3
TOL_STACKED_L2 = 0.14


def _sd(P):
    return {k: torch.from_numpy(np.array(v)) for k, v in P.items()}


def _critic(P, HW):
    D = networks.PatchGANDiscriminator(sigmoid=False, image_size=HW, dtype="fp16")
    D.load_state_dict(_sd(P))
    return D.to("cuda").train()


def _inputs(seed, N, HW):
    real, _ = op.synth_batch(seed + 1, N, HW, HW)
    fake, _ = op.synth_batch(seed + 2, N, HW, HW)
    eps = np.random.Generator(np.random.PCG64(seed + 3)).random(N).astype(np.float32)
    return real, fake, eps


def _penalty(D, real, fake, eps, lam):
    D.zero_grad()
    pen = D.gradient_penalty(torch.from_numpy(real).cuda(), torch.from_numpy(fake).cuda(), torch.from_numpy(eps), lam=lam)
    torch.cuda.synchronize()
    return pen, {name: p.grad.detach().cpu().clone() for name, p in D.named_parameters()}


def kink_aware_gp_reference(P, xhat64, lam, decisions):
    """fp64 penalty, parameter gradients and running statistics of the penalty on xhat64 (N,1,H,W), with the HIP forward's
    decisions on the units within FP16_BAND * max|z64| of a kink. -> (penalty, {name: grad}, {name: buffer}, report)."""
    taps = {}
    with torch.no_grad():
        orc.patchgan_forward(orc.to_torch(P, dtype=torch.float64, requires_grad=False), xhat64, sigmoid=False, train=True, taps=taps)
    flips, rep = {}, {"units": 0, "flipped": 0, "outside": 0}
    for name, z64 in taps.items():
        live = z64 != 0
        at_risk = live & (z64.abs() < kink.FP16_BAND * float(z64.abs().max()))
        disagree = (decisions[name] != (z64 > 0)) & live
        rep["units"] += int(live.sum())
        rep["flipped"] += int((disagree & at_risk).sum())
        rep["outside"] += int((disagree & ~at_risk).sum())
        if (disagree & at_risk).any():
            flips[name] = disagree & at_risk
    OP = orc.to_torch(P, dtype=torch.float64)
    x = xhat64.clone().requires_grad_(True)
    d = orc.patchgan_forward(OP, x, sigmoid=False, train=True, flips=flips or None)
    (g,) = torch.autograd.grad(d.sum(), x, create_graph=True)
    gp = lam * ((g.reshape(g.shape[0], -1).norm(2, dim=1) - 1) ** 2).mean()
    gp.backward()
    grads = {k: OP[k].grad for k in orc.named_parameter_keys(P)}
    bufs = {k: OP[k].detach() for k in OP if k.endswith("running_mean") or k.endswith("running_var")}
    return float(gp.detach()), grads, bufs, rep


def _hip_decisions(D, N, HW):
    return {f"c{i}": (D.gp_saved_activation(i, (N, c, HW >> i, HW >> i)) > 0).cpu()
            for i, c in ((1, 64), (2, 128), (3, 256), (4, 512))}


@pytest.mark.parametrize("cfg", [(64, 4), (128, 3), (256, 4)])
def test_fp16_penalty_vs_kink_aware_fp64_double_backward(cfg):
    HW, N = cfg
    seed = 900 + HW
    P = op.make_patchgan_params(seed, HW, HW)
    D = _critic(P, HW)
    real, fake, eps = _inputs(seed, N, HW)
    pen, grads = _penalty(D, real, fake, eps, 10.0)
    e64 = torch.from_numpy(eps).double().view(-1, 1, 1, 1)
    xhat64 = (e64 * torch.from_numpy(real).double() + (1 - e64) * torch.from_numpy(fake).double())
    ref, g64, b64, rep = kink_aware_gp_reference(P, xhat64, 10.0, _hip_decisions(D, N, HW))
    share = rep["flipped"] / max(rep["units"], 1)
    print(f"GPMEASURE penalty{cfg} units={rep['units']} flipped={rep['flipped']} ({share:.2e}) outside={rep['outside']}")
    assert rep["outside"] == 0, f"{rep['outside']} kink decisions of the penalty's forward differ from the oracle's outside the band"
    assert share <= 2e-3, f"{rep['flipped']} of {rep['units']} kink decisions differ from the oracle's"
    perr = abs(float(pen) - ref) / abs(ref)
    print(f"GPMEASURE penalty{cfg} value hip={float(pen):.6g} ref={ref:.6g} rel={perr:.3e}")
    assert perr <= TOL_PENALTY
    bad = []
    for name, g in grads.items():
        if g64[name] is None:   # no path in the penalty's graph: the Linear bias, the last BatchNorm's shift (it moves
            assert float(g.abs().max()) == 0.0, name   # D, not grad_x D, away from the kinks)
            continue
        err = rel_l2(g, g64[name])
        print(f"GPMEASURE penalty{cfg} grad {name} relL2={err:.3e}")
        if not err <= TOL_GRAD_L2:
            bad.append(f"{name}: relL2 {err:.3e} > {TOL_GRAD_L2}")
    assert not bad, "\n".join(bad)
    sd = D.state_dict()
    for k, v in b64.items():
        err = rel_l2(sd[k].cpu(), v)
        print(f"GPMEASURE penalty{cfg} buffer {k} relL2={err:.3e}")
        assert err <= TOL_RUNNING, k


def test_fp16_penalty_gradients_follow_lambda():
    """The tangent scale is derived on the device per call: lam = 1e-6 puts the direction's elements near 2e-9 * |‖g‖ - 1|,
    below fp16's smallest subnormal, where an unscaled tangent forward loses the penalty entirely."""
    HW, N, seed = 256, 4, 1700
    P = op.make_patchgan_params(seed, HW, HW)
    D = _critic(P, HW)
    real, fake, eps = _inputs(seed, N, HW)
    res = {}
    for lam in (10.0, 1e-4, 1e-6):
        pen, grads = _penalty(D, real, fake, eps, lam)
        flat = torch.cat([g.flatten() for g in grads.values()]).double() / lam
        assert torch.isfinite(flat).all() and float(flat.abs().max()) > 0.0, lam
        res[lam] = (float(pen) / lam, flat)
    for lam in (1e-4, 1e-6):
        err = rel_l2(res[lam][1], res[10.0][1])
        print(f"GPMEASURE lambda {lam:g}: grads/lam relL2 vs lam=10: {err:.3e}; penalty/lam {res[lam][0]:.6g} vs {res[10.0][0]:.6g}")
        assert err <= 1e-2, lam
        assert abs(res[lam][0] - res[10.0][0]) <= 1e-5 * abs(res[10.0][0])


def test_fp16_penalty_lambda_zero_is_exactly_zero():
    HW, N, seed = 128, 4, 1800
    D = _critic(op.make_patchgan_params(seed, HW, HW), HW)
    real, fake, eps = _inputs(seed, N, HW)
    pen, grads = _penalty(D, real, fake, eps, 0.0)
    assert float(pen) == 0.0
    for name, g in grads.items():
        assert not torch.isnan(g).any() and float(g.abs().max()) == 0.0, name


def test_fp16_penalty_is_reproducible():
    HW, N, seed = 128, 4, 1900
    D = _critic(op.make_patchgan_params(seed, HW, HW), HW)
    real, fake, eps = _inputs(seed, N, HW)
    p1, g1 = _penalty(D, real, fake, eps, 10.0)
    p2, g2 = _penalty(D, real, fake, eps, 10.0)
    assert torch.equal(p1, p2)
    for name in g1:
        assert torch.equal(g1[name], g2[name]), name


@pytest.mark.parametrize("n,overlap", [(4, False), (3, False), (3, True)])
def test_stacked_wgan_gp_critic_gradients_fp16(n, overlap):
    """fp16 counterpart of test_gp_gpu.py::test_stacked_wgan_gp_critic_gradients_vs_oracle: the critic's gradients of a whole
    WGAN-GP critic batch (stacked D(ground) | D(inpainted) with two BatchNorm populations, the penalty with one) against the
    fp64 oracle on the same inpainted images (the fp16 generator's own output), relative L2 per tensor."""
    from gan_inpainting_amd import optim, trainer
    HW, nd, seed = 64, 6, 2000 + n
    PG, PD = op.make_unet_params(seed, num_downs=nd), op.make_patchgan_params(seed + 1, HW, HW)
    G = networks.UnetGenerator(1, 1, nd, ngf=64, use_dropout="False", dtype="fp16")
    G.load_state_dict(_sd(PG))
    D = networks.PatchGANDiscriminator(sigmoid=False, image_size=HW, dtype="fp16")
    D.load_state_dict(_sd(PD))
    G, D = G.cuda(), D.cuda()
    step = trainer.WGANStep(G, D, optim.RMSprop(G.parameters(), lr=5e-5), optim.RMSprop(D.parameters(), lr=5e-5), gp_lambda=10.0,
                            overlap=overlap, stacked=True)
    g, m = op.synth_batch(seed + 2, n, HW, HW)
    eps = np.random.Generator(np.random.PCG64(seed + 3)).random(n).astype(np.float32)
    step.gp_eps = torch.from_numpy(eps).cuda()
    L = step(torch.from_numpy(g).cuda(), torch.from_numpy(m).cuda(), False)
    step.sync_for_logging()
    torch.cuda.synchronize()
    assert step.poll_overflow() == 0
    inp = step.inpainted.detach().double().cpu()
    OD = orc.to_torch(PD, dtype=torch.float64)
    ground = torch.from_numpy(g).double()
    orc.patchgan_forward(OD, ground, False, True).mean().backward()
    (-orc.patchgan_forward(OD, inp, False, True).mean()).backward()
    gp = orc.gradient_penalty(OD, ground, inp, torch.from_numpy(eps).double().view(-1, 1, 1, 1), lam=10.0)
    gp.backward()
    perr = abs(float(L["gp"]) - float(gp)) / abs(float(gp))
    print(f"GPMEASURE stacked n={n} overlap={overlap} penalty rel={perr:.3e}")
    assert perr <= TOL_STACKED_PENALTY
    bad = []
    for name, p in D.named_parameters():
        ref = OD[name].grad
        if name == "model.13.bias":   # d/db (mean D(real) - mean D(fake)) = 1 - 1; the penalty does not see it
            assert float(p.grad.abs().max()) <= 1e-5, name
            continue
        err = rel_l2(p.grad.detach().cpu(), ref)
        print(f"GPMEASURE stacked n={n} overlap={overlap} grad {name} relL2={err:.3e}")
        if not err <= TOL_STACKED_L2:
            bad.append(f"{name}: relL2 {err:.3e} > {TOL_STACKED_L2}")
    assert not bad, "\n".join(bad)


def _batch(n, hw, seed):
    g = torch.Generator().manual_seed(seed)
    ground = torch.rand((n, 1, hw, hw), generator=g)
    mask = torch.zeros((n, 1, hw, hw))
    for i in range(n):
        y0, x0 = 16 + 3 * i, 24 + 2 * i
        mask[i, 0, y0:y0 + hw // 3, x0:x0 + hw // 2] = 0.5 if i % 2 else 1.0
    return ground.cuda(), mask.cuda()


def test_headline_shape_wgan_gp_step_fp16():
    """256x256 bs=32 fp16, two-stream + stacked critic, with the penalty (lambda 10) in place of the clipping; 6 batches,
    generator update on the fifth."""
    from gan_inpainting_amd import optim, trainer
    torch.manual_seed(12)
    G = networks.get_network("generator", "unet", dtype="fp16").cuda()
    D = networks.PatchGANDiscriminator(sigmoid=False, image_size=256, dtype="fp16").cuda()
    oG, oD = optim.RMSprop(G.parameters(), lr=5e-5), optim.RMSprop(D.parameters(), lr=5e-5)
    step = trainer.WGANStep(G, D, oG, oD, recon="rmse", gp_lambda=10.0, overlap=True, stacked=True)
    g0 = G.flat_params().clone()
    pens = []
    for it in range(6):
        ground, mask = _batch(32, 256, 500 + it)
        d0 = D.flat_params().clone()
        L = step(ground, mask, it == 4)
        step.sync_for_logging()
        torch.cuda.synchronize()
        assert all(torch.isfinite(v).all() for v in L.values())
        pens.append(float(L["gp"]))
        mc = torch.ceil(mask)
        assert torch.equal(step.inpainted[mc == 0], ground[mc == 0])
        assert not torch.equal(D.flat_params(), d0)
        if it < 4:
            assert torch.equal(G.flat_params(), g0)
    assert step.poll_overflow() == 0
    assert min(pens) > 0.0
    assert not torch.equal(G.flat_params(), g0)
    assert float(D.flat_params().abs().max()) > 0.011   # not clipped


def test_plugin_wgan_l1_with_penalty_fp16(tmp_path):
    from gan_inpainting_amd import train
    train.main(["-exp", "wgan_l1", "--gp-lambda", "10", "--dtype", "fp16", "-ep", "1", "-b", "4", "--imagedim", "64",
                "--saveevery", "1", "--evalevery", "1", "--samples", "16", "--outdir", str(tmp_path)])
    ck = os.path.join(str(tmp_path), "model", "wgan_l1", "epoch1_G.pt")
    assert os.path.exists(ck)
    sd = torch.load(ck)
    assert "model.model.0.weight" in sd
    assert all(torch.isfinite(v.float()).all() for v in sd.values())
