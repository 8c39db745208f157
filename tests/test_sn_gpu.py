"""GPU tier: a PatchGAN critic built with spectral_norm=True (gi_patchgan_create_sn) as a whole: the power iteration state and the
effective weights against tests/sn_ref.py, network parity through oracle/kink.py with the HIP effective weights as the oracle's
parameters and the fp64 gradient projected by sn_ref, the gradient penalty, slots, phases, a training step, resume, and a critic
built WITHOUT the keyword against what the library computed before the feature existed.

Scale invariance: model.0/2/5/8 feed a train-mode BatchNorm, so the critic's output does not depend on their
scale and <G, W_eff> is ~0 for them: the network tests pin the projection's u v^T term only on model.11 and model.13; the
single-op test with a random G (tests/test_sn_ops_gpu.py) pins it for every shape."""
import hashlib

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import gan_inpainting_amd  # noqa: F401,E402
from gan_inpainting_amd import backend as B, checkpoint, optim  # noqa: E402
from gan_inpainting_amd.lib.models import networks  # noqa: E402
from oracle import kink, params as op, torch_ref as orc  # noqa: E402
from gpu_util import close_to_either, hip_decisions, rel_l2, report  # noqa: E402
from test_nets_gpu import TOL_GRAD, TOL_GRAD_L2, TOL_OUT  # noqa: E402  (the tolerances of the non-spectral tests of the same cases)
from test_gp_fp16_gpu import TOL_STACKED_L2, TOL_STACKED_PENALTY  # noqa: E402  (fp16: a whole stacked critic batch with the penalty)
import sn_ref  # noqa: E402

LAYERS = (0, 2, 5, 8, 11, 13)
CFGS = [(64, 4), (128, 3)]          # Linear(1,1) and Linear(25,1)
SEEDS = {64: 200, 128: 245}         # chosen on the CPU from the oracle alone: see test_network_parity_through_the_kink_reference


def uv0(seed, mats):
    rng = np.random.default_rng(seed)
    out = {}
    for k, W in mats.items():
        u, v = rng.standard_normal(W.shape[0]), rng.standard_normal(W.shape[1])
        out[k] = ((u / np.linalg.norm(u)).astype(np.float32), (v / np.linalg.norm(v)).astype(np.float32))
    return out


def sn_state_dict(P, uv):
    sd = {}
    for k, v in P.items():
        pre = k[:-len(".weight")]
        sd[k + "_orig" if k.endswith(".weight") and pre in uv else k] = torch.from_numpy(np.array(v))
    for pre, (u, v) in uv.items():
        sd[pre + ".weight_u"], sd[pre + ".weight_v"] = torch.from_numpy(u.copy()), torch.from_numpy(v.copy())
    return sd


def make_sn(P, uv, HW, dtype, iters=1):
    net = networks.get_network("discriminator", "patchgan", sigmoid=False, image_size=HW, dtype=dtype, spectral_norm=True,
                               n_power_iterations=iters)
    net.load_state_dict(sn_state_dict(P, uv), strict=True)
    net.set_loss_scale(1.0)
    return net.to("cuda").train()


def read_uv(net):
    sd = net.state_dict()
    return {f"model.{i}": (sd[f"model.{i}.weight_u"].cpu().numpy().copy(), sd[f"model.{i}.weight_v"].cpu().numpy().copy()) for i in LAYERS}


_BOUNDS = {}


def bounds(HW, mats, uv, iters):
    """sn_ref.power_iteration_bounds per layer (the normalisation is fp32 whatever the compute type: shared by both dtypes)"""
    if (HW, iters) not in _BOUNDS:
        _BOUNDS[(HW, iters)] = {k: sn_ref.power_iteration_bounds(W, uv[k][0], uv[k][1], iters, True) for k, W in mats.items()}
    return _BOUNDS[(HW, iters)]


def check_state(what, net, mats, b):
    uv, sig, eff = read_uv(net), net.spectral_sigmas(), net.effective_parameters()
    for k, W in mats.items():
        r = b[k]
        du, dv, ds = np.abs(uv[k][0] - r["u"]).max(), np.abs(uv[k][1] - r["v"]).max(), abs(sig[k] - r["sigma"])
        print(f"{what} {k}: |du| {du:.2e} (bound {r['eu'].max():.2e}) |dv| {dv:.2e} (bound {r['ev'].max():.2e}) |dsigma| {ds:.2e} (bound {r['esigma']:.2e})")
        assert (np.abs(uv[k][0] - r["u"]) <= r["eu"]).all() and (np.abs(uv[k][1] - r["v"]) <= r["ev"]).all(), f"{what} {k}: u / v"
        assert ds <= r["esigma"], f"{what} {k}: sigma {sig[k]} vs {r['sigma']}"
        e = eff[k + ".weight"].cpu().numpy().reshape(W.shape)
        assert (np.abs(e - W.astype(np.float64) / r["sigma"]) <= sn_ref.effective_bound(W, r["sigma"], r["esigma"])).all(), f"{what} {k}: W / sigma"
    sd = net.state_dict()
    for k, t in eff.items():        # everything that is not normalised is copied
        if k[:-len(".weight")] not in mats or not k.endswith(".weight"):
            assert torch.equal(t.cpu(), sd[k].cpu()), k
    return uv, sig


@pytest.mark.parametrize("dtype", ["fp32", "fp16"])
@pytest.mark.parametrize("cfg", CFGS)
def test_power_iteration_state_and_effective_weights(cfg, dtype):
    HW, N = cfg
    SEED = SEEDS[HW]
    case = kink.patchgan_case(SEED, HW, N, False)
    mats = sn_ref.critic_matrices(case["P"])
    uv = uv0(SEED + 9, mats)
    net = make_sn(case["P"], uv, HW, dtype)
    x = case["x"].cuda()
    with torch.no_grad():
        net(x)
        check_state(f"sn {cfg} {dtype} forward 1", net, mats, bounds(HW, mats, uv, 1))
        net(x)
        uv2, sig2 = check_state(f"sn {cfg} {dtype} forward 2", net, mats, bounds(HW, mats, uv, 2))
        if HW == 64:    # Linear(1,1): W_sn = +-1 exactly
            assert abs(float(net.effective_parameters()["model.13.weight"].abs().item()) - 1.0) == 0.0
        net.eval()
        net(x)
        uv3, sig3 = read_uv(net), net.spectral_sigmas()
        for k in mats:
            assert np.array_equal(uv3[k][0], uv2[k][0]) and np.array_equal(uv3[k][1], uv2[k][1]), f"eval forward moved {k}'s u / v"
            r = sn_ref.power_iteration_bounds(mats[k], uv2[k][0], uv2[k][1], 1, False)
            assert abs(sig3[k] - r["sigma"]) <= r["esigma"], k


def _frob(a):
    return float(np.linalg.norm(np.asarray(a, np.float64)))


@pytest.mark.parametrize("dtype", ["fp32", "fp16"])
@pytest.mark.parametrize("cfg", CFGS)
def test_network_parity_through_the_kink_reference(cfg, dtype):
    """oracle.kink.patchgan_case with the HIP effective weights (read back) as its parameters; the fp64 gradient with respect to
    those, G_ref, projected by sn_ref with the HIP u, v, sigma, against weight_orig.grad:
        |dW - ref|_F <= tau |G_ref|_F (1 + |W_sn|_F) / sigma,   tau = the tolerance tests/test_nets_gpu.py uses for this dtype
    (the error of G enters through G / sigma and through <G, W_sn> u v^T / sigma, |u| = |v| = 1). Output, dx and the BatchNorm /
    bias gradients compare directly at that file's tolerances.
    Not vacuous: for model.11 and (128 x 128) model.13 the reference's own projection term |c u v^T / sigma|_F must be at least
    10 x the bound. With |W_sn|_F = 1 for these one-row tensors that asks |cos(G, W)| >= 20 tau. The seeds meet it for fp32 on
    both tensors (tau = 1e-4), and 245 (the best of 200 .. 299 at 128 x 128 on the CPU oracle, cosine 0.63) meets it for
    model.13 in fp16 (tau = 3e-2: a cosine of 0.6). model.11's 8192-element gradient reaches that on no seed (at most 0.03
    over those hundred: both tensors share c = sum_n R_n (y_n - bias), and |G_11| is two orders above it), so the 10 x condition
    is asserted everywhere but for model.11 in fp16, and BOTH dtypes and both tensors carry a sharper assertion that fails when
    the term is missing or wrong: for a one-row tensor u v^T = W_sn (sigma = |W| > 0), so the projection removes the W_sn
    component of G entirely, <dW, W_sn>_F = (c - c_hat) / sigma, whatever the error of G itself. c_hat is the kernels' fp32 sum:
    |<dW, W_sn>| <= 2 (gamma(depth) + 8 U) sum|G||W_sn| / sigma (depth: sn_ref.dot_depth; 8 U: the elementwise roundings and
    u v^T - W_sn; 2: |G_hip| against |G_ref|). Without the term it would be c / sigma, which must be at least 10 x that tolerance.
    At 64 x 64 the model.13.weight_orig gradient is exactly zero."""
    HW, N = cfg
    SEED = SEEDS[HW]
    case = kink.patchgan_case(SEED, HW, N, False)
    mats = sn_ref.critic_matrices(case["P"])
    net = make_sn(case["P"], uv0(SEED + 9, mats), HW, dtype)
    xd = case["x"].cuda().requires_grad_(True)
    y = net(xd)
    (y * case["R"].cuda()).sum().backward()
    torch.cuda.synchronize()
    what = f"sn patchgan{cfg} {dtype}"
    uv, sig, eff = read_uv(net), net.spectral_sigmas(), net.effective_parameters()
    P2 = type(case["P"])((k, (eff[k].cpu().numpy() if k in eff else np.array(v))) for k, v in case["P"].items())
    case2 = dict(case, P=P2, key=case["key"] + ("spectral", dtype))
    fp16 = dtype == "fp16"
    y64, g64, dx64, rep = kink.kink_reference(case2, hip_decisions(net, case2), fp16=fp16)
    assert rep["outside"] == 0, f"{what}: {rep['outside']} kink decisions differ from the oracle's outside the rounding band"
    assert rep["flipped"] / max(rep["units"], 1) <= (2e-3 if fp16 else 1e-4)
    ok, msg = report(f"{what} out", y.detach().cpu(), y64.float(), TOL_OUT[dtype])
    assert ok, msg
    tau = TOL_GRAD_L2[dtype] if fp16 else TOL_GRAD[dtype]
    bad = []
    for name, p in list(net.named_parameters()) + [("dx", None)]:
        got = (xd.grad if name == "dx" else p.grad).detach().cpu()
        pre = name[:-len(".weight_orig")]
        if not name.endswith(".weight_orig"):
            ref = dx64 if name == "dx" else g64[name]
            err = rel_l2(got, ref) if fp16 else float((got.double() - ref).abs().max() / (ref.abs().max() + 1e-300))
            print(f"{what} {name}: {'relL2' if fp16 else 'max-norm'} {err:.3e} (tol {tau:.1e})")
            if not err <= tau:
                bad.append(f"{name}: {err:.3e} > {tau:.1e}")
            continue
        W = mats[pre]
        G = g64[pre + ".weight"].numpy().reshape(W.shape)
        W_sn = eff[pre + ".weight"].cpu().numpy().reshape(W.shape).astype(np.float64)
        u, v, sigma = uv[pre][0].astype(np.float64), uv[pre][1].astype(np.float64), float(sig[pre])
        ref = sn_ref.project(G, W_sn, u, v, sigma)
        err = _frob(got.numpy().reshape(W.shape) - ref)
        bound = tau * _frob(G) * (1 + _frob(W_sn)) / sigma
        term = abs(float((G * W_sn).sum())) * _frob(np.outer(u, v)) / sigma
        print(f"{what} {name}: |dW - ref|_F {err:.3e} bound {bound:.3e} |ref|_F {_frob(ref):.3e} projection term {term:.3e} ({term / bound:.1f} x bound)")
        if not err <= bound:
            bad.append(f"{name}: |dW - ref|_F {err:.3e} > {bound:.3e}")
        if HW == 64 and pre == "model.13":
            assert float(got.abs().max()) == 0.0, "Linear(1,1): the gradient of weight_orig must be exactly zero"
        elif pre in ("model.11", "model.13"):
            comp = abs(float((got.numpy().reshape(W.shape).astype(np.float64) * W_sn).sum()))
            tol_c = 2 * (sn_ref.gamma(sn_ref.dot_depth(G.size)) + 8 * sn_ref.U) * float((np.abs(G) * np.abs(W_sn)).sum()) / sigma
            print(f"{what} {name}: |<dW, W_sn>| {comp:.3e} tolerance {tol_c:.3e} term {term:.3e} ({term / tol_c:.0f} x tolerance)")
            assert comp <= tol_c, f"{name}: the W_sn component of the gradient {comp:.3e} > {tol_c:.3e}: the u v^T term is missing or wrong"
            assert term >= 10 * tol_c, f"{name}: the projection term {term:.3e} does not stand out of the tolerance {tol_c:.3e}"
            if not fp16 or pre == "model.13":
                assert term >= 10 * bound, f"{name}: the projection term {term:.3e} does not stand out of the bound {bound:.3e}"
    assert not bad, f"{what}:\n" + "\n".join(bad)


def _sn_oracle_params(OP, uv_t, mats, iters=1):
    """One forward call's worth of torch.nn.utils.spectral_norm on the oracle's leaves: the power iteration updates uv_t in place
    under no_grad, the returned dict holds weight = weight_orig / sigma with autograd through sigma."""
    out = dict(OP)
    for pre in mats:
        W = OP[pre + ".weight"]
        Wm = W.reshape(W.shape[0], -1)
        u, v = uv_t[pre]
        with torch.no_grad():
            for _ in range(iters):
                v = torch.nn.functional.normalize(Wm.t() @ u, dim=0, eps=1e-12)
                u = torch.nn.functional.normalize(Wm @ v, dim=0, eps=1e-12)
        uv_t[pre] = (u, v)
        out[pre + ".weight"] = W / torch.dot(u, Wm @ v)
    return out


@pytest.mark.parametrize("dtype", ["fp32", "fp16"])
@pytest.mark.parametrize("cfg", CFGS)
def test_stacked_pass_then_gradient_penalty_vs_oracle(cfg, dtype):
    """D(real) | D(fake) stacked with two BatchNorm populations (ONE power iteration), its backward, then gradient_penalty (one
    more, for its own forward) - against the same sequence in the oracle with autograd through sigma. fp32: tolerance and
    acceptance rule of tests/test_gp_gpu.py. fp16 (the penalty's buffer reaches the projection at tangent scale s != 1, removed
    by scale = 1/s read on the device): relative L2 per tensor and the penalty's value at the tolerances
    tests/test_gp_fp16_gpu.py uses for a whole stacked critic batch, at the loss scale the trainer picks (64 n)."""
    HW, n = cfg
    seed = 700 + HW
    fp16 = dtype == "fp16"
    P = op.make_patchgan_params(seed, HW, HW)
    mats = sn_ref.critic_matrices(P)
    uv = uv0(seed + 9, mats)
    D = make_sn(P, uv, HW, dtype)
    if fp16:
        D.set_loss_scale(64.0 * n)
    real = torch.from_numpy(op.synth_batch(seed + 1, n, HW, HW)[0])
    fake = torch.from_numpy(op.synth_batch(seed + 2, n, HW, HW)[0] * 0.5 + 0.2)
    eps = np.random.Generator(np.random.PCG64(seed + 3)).random(n).astype(np.float32)
    D.zero_grad()
    y, slot, gen = D._forward_raw(torch.cat([real, fake]).cuda(), bn_groups=2)
    sig_pair = D.spectral_sigmas()
    dy = torch.cat([torch.full((n, 1), -1.0 / n), torch.full((n, 1), 1.0 / n)]).cuda()
    D._backward_raw(slot, gen, dy, False, True)
    pen = D.gradient_penalty(real.cuda(), fake.cuda(), torch.from_numpy(eps), lam=10.0)
    torch.cuda.synchronize()
    sig_gp = D.spectral_sigmas("gp")
    res = {}
    for dt in (torch.float32, torch.float64):
        OP = orc.to_torch(P, dtype=dt)
        uv_t = {k: (torch.from_numpy(u).to(dt), torch.from_numpy(v).to(dt)) for k, (u, v) in uv.items()}
        Pa = _sn_oracle_params(OP, uv_t, mats)
        sig_a = {k: float(torch.dot(uv_t[k][0], OP[k + ".weight"].detach().reshape(mats[k].shape) @ uv_t[k][1])) for k in mats}
        (-(orc.patchgan_forward(Pa, real.to(dt), False, True).mean() - orc.patchgan_forward(Pa, fake.to(dt), False, True).mean())).backward()
        Pb = _sn_oracle_params(OP, uv_t, mats)
        sig_b = {k: float(torch.dot(uv_t[k][0], OP[k + ".weight"].detach().reshape(mats[k].shape) @ uv_t[k][1])) for k in mats}
        gp = orc.gradient_penalty(Pb, real.to(dt), fake.to(dt), torch.from_numpy(eps).to(dt).view(-1, 1, 1, 1), lam=10.0)
        gp.backward()
        res[dt] = (OP, float(gp), sig_a, sig_b, uv_t)
    o64 = res[torch.float64]
    for k in mats:     # one iteration per call: the stacked pass ran the first, the penalty the second
        assert abs(sig_pair[k] - o64[2][k]) <= 1e-4 * o64[2][k] and abs(sig_gp[k] - o64[3][k]) <= 1e-4 * o64[3][k], (k, sig_pair[k], sig_gp[k], o64[2][k], o64[3][k])
    got_uv = read_uv(D)
    for k in mats:
        assert np.abs(got_uv[k][0] - o64[4][k][0].numpy()).max() <= 1e-4 and np.abs(got_uv[k][1] - o64[4][k][1].numpy()).max() <= 1e-4, k
    print("penalty hip", float(pen), "oracle32", res[torch.float32][1], "oracle64", o64[1])
    assert abs(float(pen) - o64[1]) <= (TOL_STACKED_PENALTY if fp16 else 1e-3) * abs(o64[1]) + 1e-6
    bad = []
    for name, p in D.named_parameters():
        key = name.replace("weight_orig", "weight")
        g32, g64 = res[torch.float32][0][key].grad, o64[0][key].grad
        if float(g64.abs().max()) < 1e-9:     # Linear bias (1 - 1, unseen by the penalty); Linear(1,1) weight_orig (W_sn = +-1)
            assert float(p.grad.abs().max()) <= (1e-5 if fp16 else 1e-6), name
            continue
        if fp16:
            err = rel_l2(p.grad.detach().cpu(), g64)
            print(f"sn stacked + gp {cfg} fp16 grad {name}: relL2 {err:.3e} (tol {TOL_STACKED_L2})")
            if not err <= TOL_STACKED_L2:
                bad.append(f"{name}: relL2 {err:.3e} > {TOL_STACKED_L2}")
            continue
        ok, msg = close_to_either(f"sn stacked + gp {cfg} grad {name}", p.grad.detach().cpu(), g32, g64, 2e-3)
        if not ok and rel_l2(p.grad.detach().cpu(), g64) > 2e-3:
            bad.append(msg)
    assert not bad, "\n".join(bad)


def _fixed(HW, N, seed):
    g = np.random.Generator(np.random.PCG64(seed))
    x = [torch.from_numpy(op.synth_batch(seed + i, N, HW, HW)[0]).cuda() for i in (1, 2)]
    dy = [torch.from_numpy(g.standard_normal(size=(N, 1), dtype=np.float32)).cuda() for _ in range(2)]
    return x, dy


def _snapshot(net):
    torch.cuda.synchronize()
    out = {"grads": net.flat_grads().clone(), "buffers": net._flat["buffers"].clone()}
    return out


@pytest.mark.parametrize("dtype", ["fp32", "fp16"])
def test_two_live_forwards_backward_in_reverse_order(dtype):
    """Each backward uses the u, v, sigma of ITS forward (kept per slot) and re-derives the effective weights when a later forward
    has replaced them: two forwards, then their backwards in reverse order, equal the same two run one after the other, bit for bit."""
    HW, N, seed = 64, 4, 311
    P = op.make_patchgan_params(seed, HW, HW)
    mats = sn_ref.critic_matrices(P)
    (x1, x2), (dy1, dy2) = _fixed(HW, N, seed)
    runs = []
    for interleaved in (False, True):
        net = make_sn(P, uv0(seed + 9, mats), HW, dtype)
        net.zero_grad()
        if interleaved:
            ya, sa, ga = net._forward_raw(x1)
            yb, sb, gb = net._forward_raw(x2)
            sig = (net.spectral_sigmas(sa), net.spectral_sigmas(sb))
            dxb = net._backward_raw(sb, gb, dy2, True, True)
            dxa = net._backward_raw(sa, ga, dy1, True, True)
        else:
            ya, sa, ga = net._forward_raw(x1)
            s1 = net.spectral_sigmas(sa)
            dxa = net._backward_raw(sa, ga, dy1, True, True)
            yb, sb, gb = net._forward_raw(x2)
            sig = (s1, net.spectral_sigmas(sb))
            dxb = net._backward_raw(sb, gb, dy2, True, True)
        runs.append(dict(_snapshot(net), ya=ya, yb=yb, dxa=dxa, dxb=dxb, sig=sig))
    a, b = runs
    assert a["sig"] == b["sig"] and a["sig"][0] != a["sig"][1]
    for k in ("ya", "yb", "dxa", "dxb", "buffers", "grads"):
        assert torch.equal(a[k], b[k]), k
    assert float(a["grads"].abs().max()) > 0


@pytest.mark.parametrize("dtype", ["fp32", "fp16"])
def test_phase_split_backward_is_bit_equal_and_completes_the_tail_first(dtype):
    HW, N, seed = 128, 2, 411
    P = op.make_patchgan_params(seed, HW, HW)
    mats = sn_ref.critic_matrices(P)
    (x, _), (dy, _) = _fixed(HW, N, seed)
    lib = B.lib()
    res = []
    for phases in ((0,), (1, 2)):
        net = make_sn(P, uv0(seed + 9, mats), HW, dtype)
        net.zero_grad()
        _, s, g = net._forward_raw(x)
        split = lib.gi_net_phase_split(net._handle)
        for i, ph in enumerate(phases):
            B.check(lib.gi_net_backward_phase(net._handle, s, B.ptr(dy), None, 1, ph))
            torch.cuda.synchronize()
            fg = net.flat_grads()
            if ph == 1:      # what comm.hip relies on: the tail [split, end) is complete after phase 1, the head untouched
                assert float(fg[:split].abs().max()) == 0.0 and float(fg[split:].abs().max()) > 0.0
                tail = fg[split:].clone()
        res.append(net.flat_grads().clone())
    assert torch.equal(res[1][split:], tail), "phase 2 changed the range phase 1 had completed"
    rel = float((res[0].double() - res[1].double()).norm() / res[0].double().norm())
    print(f"sn phases {dtype}: relative difference {rel:.3e}")
    assert torch.equal(res[0], res[1])


@pytest.mark.parametrize("mode", ["clip", "gp"])
def test_wgan_step_moves_weight_orig_and_keeps_sigma_finite(mode):
    from gan_inpainting_amd import trainer
    torch.manual_seed(5)
    G = networks.UnetGenerator(1, 1, 6, ngf=64, use_dropout="False", dtype="fp32").to("cuda")
    D = networks.get_network("discriminator", "patchgan", sigmoid=False, image_size=64, dtype="fp32", spectral_norm=True).to("cuda")
    kw = dict(gp_lambda=10.0) if mode == "gp" else {}
    step = trainer.WGANStep(G, D, optim.RMSprop(G.parameters(), lr=5e-5), optim.RMSprop(D.parameters(), lr=5e-5), **kw)
    g, m = op.synth_batch(1, 4, 64, 64)
    names = [n for n, _ in D.named_parameters() if n.endswith("weight_orig")]
    assert len(names) == 6
    w0 = {n: p.detach().clone() for n, p in D.named_parameters()}
    u0 = read_uv(D)
    L = step(torch.from_numpy(g).cuda(), torch.from_numpy(m).cuda(), True)
    torch.cuda.synchronize()
    assert all(torch.isfinite(v).all() for v in L.values() if torch.is_tensor(v))
    moved = [n for n, p in D.named_parameters() if n.endswith("weight_orig") and not torch.equal(p.detach(), w0[n])]
    assert len(moved) >= 5, moved          # (64 x 64: Linear(1,1)'s weight_orig has an exactly zero gradient; clipping may still move it)
    sig = D.spectral_sigmas()
    assert all(np.isfinite(v) and v > 0 for v in sig.values()), sig
    if mode == "gp":
        assert all(np.isfinite(v) and v > 0 for v in D.spectral_sigmas("gp").values())
    u1 = read_uv(D)
    assert any(not np.array_equal(u0[k][1], u1[k][1]) for k in u0), "the power iteration did not update v"


def _critic_step(D, opt, real, fake, eps):
    n = real.shape[0]
    D.zero_grad()
    y, slot, gen = D._forward_raw(torch.cat([real, fake]), bn_groups=2)
    dy = torch.cat([torch.full((n, 1), -1.0 / n), torch.full((n, 1), 1.0 / n)]).cuda()
    D._backward_raw(slot, gen, dy, False, True)
    D.gradient_penalty(real, fake, eps, lam=10.0)
    grads = D.flat_grads().clone()
    opt.step()
    D.mark_dirty()
    return grads


def test_resumed_critic_equals_the_uninterrupted_one(tmp_path):
    """--save-state semantics through checkpoint.py: u, v travel as buffers of the state dict with no code of their own; after a
    save / load into fresh objects the next step's gradients, weights and u, v are those of the uninterrupted run, bit for bit."""
    HW, n, seed = 64, 4, 511

    def mk():
        torch.manual_seed(seed)
        D = networks.get_network("discriminator", "patchgan", sigmoid=False, image_size=HW, dtype="fp16", spectral_norm=True).to("cuda").train()
        D.set_loss_scale(256.0)            # (these synthetic output gradients are O(1/n), not a mean-reduced loss; travels in training_state)
        return D, optim.RMSprop(D.parameters(), lr=5e-5)
    batches = [(torch.from_numpy(op.synth_batch(seed + 2 * i, n, HW, HW)[0]).cuda(), torch.from_numpy(op.synth_batch(seed + 2 * i + 1, n, HW, HW)[0]).cuda(),
                torch.linspace(0.1, 0.9, n)) for i in range(2)]
    D, opt = mk()
    for b in batches:
        g_ref = _critic_step(D, opt, *b)
    torch.cuda.synchronize()
    D1, opt1 = mk()
    _critic_step(D1, opt1, *batches[0])
    torch.cuda.synchronize()
    path = str(tmp_path / "last_state.pt")
    checkpoint.save_state(path, {"format_version": checkpoint.FORMAT_VERSION,
                                 "nets": {"D": {"state_dict": {k: v.detach().cpu().contiguous() for k, v in D1.state_dict().items()},
                                                "training_state": D1.training_state()}},
                                 "optimizers": {"opt0": opt1.state_dict()}})
    payload = checkpoint.load_state(path)
    assert any(k.endswith("weight_u") for k in payload["nets"]["D"]["state_dict"])
    torch.manual_seed(seed + 1)            # a resumed process draws other initial values before it loads
    D2 = networks.get_network("discriminator", "patchgan", sigmoid=False, image_size=HW, dtype="fp16", spectral_norm=True).to("cuda").train()
    opt2 = optim.RMSprop(D2.parameters(), lr=5e-5)
    D2.load_state_dict(payload["nets"]["D"]["state_dict"])
    D2.load_training_state(payload["nets"]["D"]["training_state"])
    opt2.load_state_dict(payload["optimizers"]["opt0"])
    g2 = _critic_step(D2, opt2, *batches[1])
    torch.cuda.synchronize()
    assert torch.isfinite(g_ref).all() and float(g_ref.abs().max()) > 0
    assert torch.equal(g2, g_ref), "gradients of the resumed step"
    sd, sd2 = D.state_dict(), D2.state_dict()
    for k in sd:
        assert torch.equal(sd[k], sd2[k]), k


PARENT_KEYS = [
    "model.0.weight", "model.2.weight", "model.3.weight", "model.3.bias", "model.3.running_mean", "model.3.running_var",
    "model.3.num_batches_tracked", "model.5.weight", "model.6.weight", "model.6.bias", "model.6.running_mean", "model.6.running_var",
    "model.6.num_batches_tracked", "model.8.weight", "model.9.weight", "model.9.bias", "model.9.running_mean", "model.9.running_var",
    "model.9.num_batches_tracked", "model.11.weight", "model.13.weight", "model.13.bias"]
# recorded from the commit before spectral norm existed, with a build of that commit on an MI355X: gi_net_workspace_bytes of
# gi_patchgan_create(64, 64, sigmoid 0, max_n 8, dtype, 3 slots), and the sha256 of y, dx and the flat gradients of
# tools/net_hashes.py's patchgan(dtype, 8, 64) case
PARENT = {
    "fp32": dict(ws=160257536, y="516e90f6fef91e5229bf12a612004ac00001fdffe58db9fa4904e0f2d6b69fc3",
                 dx="dc86127a47b38630b2b6d71b65208069c7a9333bd73bcda38499dc7f23fde959",
                 grads="1bd06e4b332010a098c4dc179f0091d768dbe1a54948226be4b5e899093fbcb7"),
    "fp16": dict(ws=126440960, y="fea7a7e3e60c43457b848f84e598c14fee23ec2791bcdb1f09a47e817731f65a", dx="5175e9dbcc40d7507ab0cfc047ff8f11059260b83e74f92e9034474cc5bc460d", grads="db6c8d587ab847657f6f08ae03eaa319ec959dd7a2f140fbea447750216a6820"),
}


def _sha(t):
    return hashlib.sha256(t.detach().cpu().contiguous().numpy().tobytes()).hexdigest()


@pytest.mark.parametrize("dtype", ["fp32", "fp16"])
def test_critic_without_the_keyword_is_what_it_was(dtype):
    import ctypes as C
    seed, HW, N = 66, 64, 8
    net = networks.get_network("discriminator", "patchgan", sigmoid=False, image_size=HW, dtype=dtype)
    assert list(net.state_dict()) == PARENT_KEYS
    assert (net._n_params, net._n_buffers) == (2763648, 1792)
    net.load_state_dict({k: torch.from_numpy(np.array(v)) for k, v in op.make_patchgan_params(seed, HW, HW).items()})
    net = net.to("cuda").train()
    net.set_loss_scale(1.0)
    x = torch.from_numpy(op.synth_batch(seed + 2, N, HW, HW)[0]).cuda()
    dy = torch.from_numpy(np.random.Generator(np.random.PCG64(seed)).standard_normal(size=(N, 1), dtype=np.float32)).cuda()
    net.zero_grad()
    y, s, gen = net._forward_raw(x, 2)
    dx = net._backward_raw(s, gen, dy, True, True)
    torch.cuda.synchronize()
    lib = B.lib()
    assert lib.gi_net_workspace_bytes(net._handle) == PARENT[dtype]["ws"]
    assert (_sha(y), _sha(dx), _sha(net.flat_grads())) == (PARENT[dtype]["y"], PARENT[dtype]["dx"], PARENT[dtype]["grads"])
    # gi_patchgan_create_sn(..., spectral_norm = 0, ...) is the same handle
    h = C.c_void_p()
    B.check(lib.gi_patchgan_create_sn(None, HW, HW, 0, 0, 1, N, net._dtype, net.n_slots, C.byref(h)))
    assert lib.gi_net_workspace_bytes(h) == PARENT[dtype]["ws"] and lib.gi_net_tensor_count(h) == 19
    lib.gi_net_destroy(h)
    with pytest.raises(B.BackendError, match="spectral_norm"):
        net.spectral_sigmas()
