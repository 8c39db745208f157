"""GPU tier: DCGANDiscriminator (-d dcgan) on the HIP kernels of csrc/dcgan.hip against the fp64 restatement of
tests/dcgan_ref.py: forward, decision-aware gradients, frozen backward, bit-reproducibility, the stacked [real | fake]
call, the kernels that serve it, a MinimaxStep and the plugins that build it."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import dcgan_ref as R

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _net(dtype, seed=7):
    import gan_inpainting_amd  # noqa: F401
    from gan_inpainting_amd.lib.models import networks
    P = R.make_params(seed)
    d = networks.DCGANDiscriminator(dtype=dtype)
    d.load_state_dict({k: torch.from_numpy(v) for k, v in P.items()})
    return d.to("cuda").train(), P


def _images(n, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.rand(n, 1, 128, 128, generator=g)


@pytest.mark.parametrize("dtype", ["fp32", "fp16"])
@pytest.mark.parametrize("n", [1, 4, 33])
def test_forward_matches_restatement(dtype, n):
    d, P = _net(dtype)
    x = _images(n, 100 + n)
    with torch.no_grad():
        y = d(x.cuda()).cpu().double()
    ref = R.forward(R.to_torch(P), x.double())
    assert y.shape == (2 * n, 1)
    tol = (1e-4 if dtype == "fp32" else 2e-2) * ref.abs().max().item()
    assert (y - ref).abs().max().item() <= tol
    assert torch.allclose(y.view(n, 2).sum(1), torch.ones(n, dtype=torch.float64), atol=1e-5)


def _bias16_floor(dy):
    """The last bias's gradient, sum over images of p0 p1 (dy_0 - dy_1), cancels across images (and is exactly opposite for
    the two logits), so it can be far below its terms. Its error is set by the fp32 probabilities, not by its own size: per
    image <= 2 eps32 p0 p1 |dy_0 - dy_1| <= 6e-8 (|dy_0| + |dy_1|)."""
    return 6e-8 * float(dy.abs().sum())


def _hip_decisions(d, n):
    hps = [63, 30, 14, 6]
    hip = {f"dec{i + 1}": d.saved_activation(1, i + 1, (n, R.CHANS[i + 1], hps[i], hps[i])).cpu() for i in range(4)}
    hip["h12"] = d.saved_activation(2, 1, (n, 4096)).cpu()
    hip["h14"] = d.saved_activation(2, 2, (n, 512)).cpu()
    return hip


def _bands(P, x, dtype):
    wins, h12, h14 = R.pool_preacts(P, x.double())
    if dtype == "fp16":   # oracle/kink.py's fp16 band: 2e-2 of the tensor's largest magnitude
        b = {f"pool{i + 1}": 2e-2 * w.abs().max().item() for i, w in enumerate(wins)}
        b.update(h12=2e-2 * h12.abs().max().item(), h14=2e-2 * h14.abs().max().item())
        return b
    # fp32: 16 x the measured fp32-vs-fp64 error of each tensor
    w32, a32, b32 = R.pool_preacts(P, x.float(), torch.float32)
    b = {f"pool{i + 1}": 16 * max((w - v.double()).abs().max().item(), 1e-12) for i, (w, v) in enumerate(zip(wins, w32))}
    b.update(h12=16 * max((h12 - a32.double()).abs().max().item(), 1e-12), h14=16 * max((h14 - b32.double()).abs().max().item(), 1e-12))
    return b


@pytest.mark.parametrize("dtype", ["fp32", "fp16"])
def test_gradients_decision_aware(dtype):
    n = 3
    d, P = _net(dtype)
    x = _images(n, 5)
    dy = torch.from_numpy(np.random.default_rng(3).choice([-1.0, 1.0], size=(2 * n, 1)).astype(np.float32))
    xg = x.cuda().requires_grad_(True)
    d.zero_grad()
    y = d(xg)
    y.backward(dy.cuda())
    torch.cuda.synchronize()
    hip = _hip_decisions(d, n)
    _, g, st = R.decision_aware(P, x, dy, hip, _bands(P, x, dtype))
    assert st["mismatch"] == 0, st
    assert st["imposed"] <= (1e-4 if dtype == "fp32" else 2e-3) * st["units"], st
    got = {k: p.grad.detach().cpu().double() for k, p in d.named_parameters()}
    got["x"] = xg.grad.detach().cpu().double()
    for k, ref in g.items():
        a = got[k].reshape(ref.shape)
        if dtype == "fp32":
            floor = _bias16_floor(dy) if k == "model.16.bias" else 1e-30
            assert (a - ref).abs().max().item() <= 1e-4 * ref.abs().max().item() + floor, k
        else:
            assert (a - ref).norm().item() <= 3e-2 * ref.norm().item() + 1e-30, k


@pytest.mark.parametrize("dtype", ["fp32", "fp16"])
def test_frozen_backward_and_reproducible(dtype):
    from gan_inpainting_amd.lib.models import util
    n = 4
    d, _ = _net(dtype)
    x = _images(n, 9).cuda()
    dy = torch.linspace(-1, 1, 2 * n, device="cuda").view(-1, 1)
    runs = []
    for _ in range(2):
        d.zero_grad()
        xg = x.clone().requires_grad_(True)
        y = d(xg)
        y.backward(dy)
        runs.append((y.detach().clone(), xg.grad.clone(), d.flat_grads().clone()))
    for a, b in zip(runs[0], runs[1]):
        assert torch.equal(a, b)
    assert torch.isfinite(runs[0][2]).all() and runs[0][2].abs().sum() > 0
    util.set_requires_grad([d], False)
    d.zero_grad()
    before = d.flat_grads().clone()
    xg = x.clone().requires_grad_(True)
    d(xg).backward(dy)
    assert torch.equal(xg.grad, runs[0][1])
    assert torch.equal(d.flat_grads(), before)
    util.set_requires_grad([d], True)


@pytest.mark.parametrize("dtype", ["fp32", "fp16"])
def test_stacked_call_equals_two_calls(dtype):
    n = 3
    d, _ = _net(dtype)
    a, b = _images(n, 11).cuda(), _images(n, 12).cuda()
    dy = torch.linspace(-1, 1, 4 * n, device="cuda").view(-1, 1)
    d.zero_grad()
    y2, slot, gen = d._forward_raw(torch.cat([a, b]), bn_groups=2)
    d._backward_raw(slot, gen, dy, False, True)
    g2 = d.flat_grads().clone()
    d.zero_grad()
    ya, sa, ga = d._forward_raw(a)
    d._backward_raw(sa, ga, dy[:2 * n].contiguous(), False, True)
    yb, sb, gb = d._forward_raw(b)
    d._backward_raw(sb, gb, dy[2 * n:].contiguous(), False, True)
    assert torch.equal(y2, torch.cat([ya, yb]))
    tol = 1e-5 if dtype == "fp32" else 1e-3
    assert (d.flat_grads() - g2).abs().max().item() <= tol * g2.abs().max().item()


def test_kernels_named():
    """Each operation, run last on its own through the backward phases, names the DCGAN kernel that served it."""
    from gan_inpainting_amd import backend as B
    lib = B.lib()
    d, _ = _net("fp16")
    x = _images(2, 1).cuda()
    dy = torch.ones(4, 1, device="cuda")
    y, slot, gen = d._forward_raw(x)
    torch.cuda.synchronize()
    assert B.last_kernel() == "dc_linear_fwd"
    B.check(lib.gi_net_backward_phase(d._handle, slot, B.ptr(dy), None, 0, 1))    # head only, frozen: Linear 12 input gradient last
    assert B.last_kernel() == "dc_linear_dgrad"
    B.check(lib.gi_net_backward_phase(d._handle, slot, B.ptr(dy), None, 1, 1))    # head with parameter gradients
    assert B.last_kernel() == "dc_linear_wgrad"
    B.check(lib.gi_net_backward_phase(d._handle, slot, B.ptr(dy), None, 0, 2))    # convs 3 .. 1 input gradients, no dx
    assert B.last_kernel() == "dc_conv_dgrad"
    B.check(lib.gi_net_backward_phase(d._handle, slot, B.ptr(dy), None, 1, 2))    # conv 0's weight gradient last
    assert B.last_kernel() == "dc_conv_wgrad"
    # the convolution forward: the kernel that wrote the pool decisions and pooled maps the other tests read is the only
    # writer of those buffers; its name is the last one of a forward stopped after it
    B.check(lib.gi_dcgan_debug_forward_convs(d._handle, slot, B.ptr(x), 2))
    assert B.last_kernel() == "dc_conv_fwd"
    torch.cuda.synchronize()


@pytest.mark.parametrize("dtype", ["fp32", "fp16"])
def test_forward_and_gradients_vs_reference_fixture(dtype):
    """dcgan128.npz (tests/golden/make_golden_dcgan.py): the reference module in fp64, N = 4, random-sign objective."""
    from util_golden import load
    fx = load("dcgan128")
    seed, n = int(fx["seed"]), int(fx["N"])
    d, _ = _net(dtype, seed)
    x = torch.from_numpy(np.random.Generator(np.random.PCG64(seed + 1)).random((n, 1, 128, 128), dtype=np.float32))
    dy = torch.from_numpy(np.random.Generator(np.random.PCG64(seed + 2)).choice([-1.0, 1.0], size=(2 * n, 1)).astype(np.float32))
    xg = x.cuda().requires_grad_(True)
    d.zero_grad()
    y = d(xg)
    y.backward(dy.cuda())
    ref = fx["y"]
    assert np.abs(y.detach().cpu().double().numpy() - ref).max() <= (1e-4 if dtype == "fp32" else 2e-2) * np.abs(ref).max()
    tol = 1e-3 if dtype == "fp32" else 3e-2
    got = xg.grad.detach().cpu().double()
    assert abs(got.abs().mean().item() - float(fx["dx_absmean"])) <= tol * float(fx["dx_absmean"])
    names = [str(k) for k in fx["names"]]
    assert names == [k for k, _ in d.named_parameters()]
    for k, p in d.named_parameters():
        g = p.grad.detach().cpu().double()
        ra = float(fx[f"grad_absmean_{k}"])
        floor = _bias16_floor(dy) if k == "model.16.bias" else 0.0
        assert abs(g.abs().mean().item() - ra) <= tol * ra + floor, (k, g.abs().mean().item(), ra)
        if dtype == "fp32":   # fp16: element-level gradients are bounded by the relative-L2 test above, heads are not compared
            head = fx[f"grad_head_{k}"]
            # heads in the reference's NCHW / row-major element order (the logical view of the channels_last weights)
            h = g.contiguous().reshape(-1)[:len(head)].numpy()
            assert np.abs(h - head).max() <= 1e-3 * np.abs(head).max() + floor, k


@pytest.mark.parametrize("dtype", ["fp32", "fp16"])
def test_minimax_step_vs_reference_fixture(dtype):
    """minimax_dcgan_step.npz: two batches of minimaxgan_l1.py:110-173 on the reference UnetGenerator + DCGANDiscriminator with
    torch.optim.Adam, the reference's dropout masks imposed. First batch: fp32 losses within 2e-5 (relative); after an Adam step
    the project's after-Adam tolerances (tests/test_steps_gpu.py)."""
    from util_golden import load, relerr, unpack_masks
    from gan_inpainting_amd import optim, trainer
    from gan_inpainting_amd.lib.models import networks, util
    from oracle import params as op
    from test_steps_gpu import GRADFLOW_TOL_AFTER_ADAM, GRADFLOW_TOL_IT0, LOSS_TOL, LOSS_TOL_AFTER_ADAM, STAT_TOL, abs_sums, check_loss, sd
    fx = load("minimax_dcgan_step")
    seed, N, iters = int(fx["seed"]), int(fx["N"]), int(fx["iters"])
    G = networks.get_network("generator", "unet", dtype=dtype)
    G.load_state_dict(sd(op.make_unet_params(seed)))
    G = G.to("cuda")
    D, _ = _net(dtype, seed + 1)
    oG = optim.Adam(G.parameters(), lr=0.0002, betas=(0.5, 0.999))
    oD = optim.Adam(D.parameters(), lr=0.0002, betas=(0.5, 0.999))
    step = trainer.MinimaxStep(G, D, oG, oD, recon="l1")
    gflow = util.GradFlow(G)
    for it in range(iters):
        g, m = op.synth_batch(seed * 100 + it, N, 128, 128, fractional_edge=(it == 0))
        G.impose_dropout_masks(unpack_masks(fx, f"it{it}_"))
        L = step(torch.from_numpy(g).cuda(), torch.from_numpy(m).cuda())
        torch.cuda.synchronize()
        first = {"fp32": 2e-5, "fp16": LOSS_TOL["fp16"]}[dtype]
        for k in ("d_loss_real", "d_loss_fake", "g_adv", "recon"):
            check_loss(f"minimax-dcgan it{it}", k, L[k].item(), fx[f"it{it}_{k}"], dtype, tol=first if it == 0 else LOSS_TOL_AFTER_ADAM[dtype])
        # the D step's gradients (the G step's frozen backward leaves them as they are) and the G step's gradient flow
        tol = GRADFLOW_TOL_IT0[dtype] if it == 0 else GRADFLOW_TOL_AFTER_ADAM[dtype]
        dref = fx[f"it{it}_d_grad_absmean"]
        dgot = np.array([float(p.grad.abs().mean()) for _, p in D.named_parameters()])
        print(f"minimax-dcgan it{it} D gradient abs-mean worst rel {relerr(dgot, dref, 1e-12):.2e} (bound {tol:.2e})")
        assert relerr(dgot, dref, 1e-12) <= tol
        names = [str(s) for s in fx["g_param_names"]]
        ref = {n: float(v) for n, v in zip(names, fx[f"it{it}_g_grad_absmean"])}
        for n, v in gflow.as_dict().items():
            assert abs(v - ref[n]) <= tol * abs(ref[n]) + 1e-12, f"it{it} G absmean {n}: {v} vs {ref[n]}"
        # Adam's first update moves every element by exactly +-lr: an element whose gradient is at rounding level (a ReLU-dead
        # channel's bias) moves by a sign that rounding picks, in the reference's fp32 as here. Each tensor's abs-sum may
        # therefore also differ by 2 lr per such element; two are allowed (measured: model.3.bias, 4.8e-4 = one flip)
        for net, key in ((D, "d"), (G, "g")):
            got, ref = abs_sums(net), fx[f"it{it}_{key}_param_stats"][:, 1]
            assert np.all(np.abs(got - ref) <= STAT_TOL[dtype] * np.abs(ref) + 2 * 2 * 0.0002), (key, relerr(got, ref))


@pytest.mark.parametrize("exp,check", [("minimaxgan_l1", "dcgan"), ("experiment1_global_local_D", "dcgan"), ("wgan_l1", "patchgan")])
def test_plugin_with_dcgan(tmp_path, exp, check):
    cmd = [sys.executable, os.path.join(ROOT, "gan-inpainting_amd", "train.py"), "-exp", exp, "-d", "dcgan", "--imagedim", "128", "-b", "8",
           "-ep", "1", "--samples", "16", "--saveevery", "1", "--evalevery", "1", "--outdir", str(tmp_path)]
    r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert os.path.exists(os.path.join(str(tmp_path), "model", exp, "epoch1_G.pt"))
    import pickle
    with open(os.path.join(str(tmp_path), "model", exp, "training_epoch_history.obj"), "rb") as h:
        hist = pickle.load(h)
    assert all(np.isfinite(v) for v in hist[-1]["losses"].values())
    log = open(os.path.join(str(tmp_path), "log", f"{exp}.log")).read()
    if check == "patchgan":
        assert "-d dcgan ignored" in log
