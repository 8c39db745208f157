"""GPU tier: whole-network parity against the CPU oracle AT THE BATCH SIZES THE BENCHMARK RUNS (BASELINE.json configs[3], [4]).
The other parity files stop at n <= 4 (generator) / n <= 8 (critic), where d2, u2 ... u4 and the critic's conv2 / conv3 launch 128 - 256
workgroups; here they launch >= 512, the regime of igemm8, of wgrad3's pixel-range splits, of the multi-replica statistics
accumulators and of the BatchNorm-backward sums fused into GEMM epilogues - so this file pins how csrc/net.hip wires those kernels
together (pointers, channel offsets, leading dimensions, replicas, population boundaries), which the single-layer tests of
tests/test_dispatch_gpu.py cannot see. One fixed seed per case, dropout masks imposed, the same checks as
tests/test_nets_gpu.py::test_unet_forward_backward_vs_oracle / test_patchgan_two_populations_vs_oracle: fp32 1e-4 kink-aware
max-norm per tensor; fp16 the absolute bounds and K x the storage-rounded restatement's own error per tensor (oracle/kink.py:
yardstick). Every tensor is compared on its own, never through the flat gradient buffer.

The oracle passes of a case (fp32 and fp64 forward, the restatement, the kink-aware references) are shared between its fp32 and
fp16 runs (oracle.kink's cache: the dtype parameter varies fastest)."""
import time

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import gan_inpainting_amd  # noqa: F401,E402
from oracle import kink  # noqa: E402
from gpu_util import check_grads_vs_kink_reference, record, report  # noqa: E402
from gan_inpainting_amd.lib.models import networks  # noqa: E402

# the bounds of tests/test_nets_gpu.py
TOL_OUT = {"fp32": 1e-4, "fp16": 2e-2}
TOL_GRAD = {"fp32": 1e-4, "fp16": None}
TOL_GRAD_L2 = {"fp32": None, "fp16": 3e-2}


def sd(P):
    return {k: torch.from_numpy(np.array(v)) for k, v in P.items()}


def make_unet(P, nd, dtype):
    net = networks.UnetGenerator(1, 1, nd, ngf=64, use_dropout="False", dtype=dtype)
    net.load_state_dict(sd(P))
    net.set_loss_scale(1.0)   # O(1) synthetic gradients, not a mean-reduced loss
    return net.to("cuda").train()


def make_d(P, HW, sigmoid, dtype):
    net = networks.PatchGANDiscriminator(sigmoid=sigmoid, image_size=HW, dtype=dtype)
    net.load_state_dict(sd(P))
    net.set_loss_scale(1.0)
    return net.to("cuda").train()


def _gemm_tiles(n, hw_out, cout):
    """workgroups of a 4x4 / stride-2 layer's forward GEMM: 256 output pixels x 128 output channels each"""
    return (n * hw_out * hw_out // 256) * ((cout + 127) // 128)


def _forward_checks(what, net, y, case, dtype):
    f32 = kink.forward32(case)
    ok, msg = report(f"{what} out", y.detach().cpu(), f32["y"], TOL_OUT[dtype])
    assert ok, msg
    for k, v in net.state_dict().items():
        if k.endswith("running_mean") or k.endswith("running_var"):
            ok, msg = report(f"{what} {k}", v.cpu(), f32["stats"][k], 1e-4 if dtype == "fp32" else 2e-2)
            assert ok, msg


@pytest.mark.parametrize("dtype", ["fp32", "fp16"])
@pytest.mark.parametrize("cfg", [(7, 32, 256), (7, 8, 512)], ids=["256-n32", "512-n8"])
def test_unet_headline_batch_vs_oracle(dtype, cfg):
    """The generator of configs[3] (256x256, n = 32) and configs[4] (512x512, n = 8: 32-wide patch tiles on 256-wide maps)."""
    nd, N, HW = cfg
    assert _gemm_tiles(N, HW // 4, 128) >= 512, "d2 must launch >= 512 workgroups: the case left the benchmark's regime"
    t0 = time.time()
    seed = 7000 + HW
    case = kink.unet_case(seed, nd, N, HW)
    net = make_unet(case["P"], nd, dtype)
    net.impose_dropout_masks({k: v.clone() for k, v in case["masks"].items()})
    xd = case["x"].cuda().requires_grad_(True)
    y = net(xd)
    (y * case["R"].cuda()).sum().backward()
    torch.cuda.synchronize()
    what = f"headline unet{cfg} {dtype} seed {seed}"
    _forward_checks(what, net, y, case, dtype)
    for k, v in net.state_dict().items():
        if k.endswith("num_batches_tracked"):
            assert int(v) == 1
    check_grads_vs_kink_reference(what, net, case, xd.grad, dtype, TOL_GRAD[dtype], TOL_GRAD_L2[dtype], y=y)
    print(f"{what}: {time.time() - t0:.1f} s")
    record(what + " seconds", time.time() - t0)


@pytest.mark.parametrize("dtype", ["fp32", "fp16"])
def test_patchgan_headline_stacked_batch_vs_oracle(dtype):
    """The stacked critic of configs[3]: 64 images of 256x256 = two BatchNorm populations of 32 in one launch sequence, against
    the oracle's two calls; output, running statistics, input gradient and every parameter gradient."""
    hw, n = 256, 64
    assert _gemm_tiles(n, hw // 4, 128) >= 512, "conv2 must launch >= 512 workgroups: the case left the benchmark's regime"
    t0 = time.time()
    seed = 7900 + hw
    case = kink.patchgan_case(seed, hw, n, False, groups=2)
    net = make_d(case["P"], hw, False, dtype)
    net.zero_grad()
    y, s, g = net._forward_raw(case["x"].cuda(), 2)
    dx = net._backward_raw(s, g, case["R"].cuda(), True, True)
    torch.cuda.synchronize()
    what = f"headline patchgan two populations {hw} n={n} {dtype} seed {seed}"
    _forward_checks(what, net, y, case, dtype)
    names = [k for k, _ in net.named_parameters()]
    assert {"model.3.weight", "model.3.bias", "model.6.weight", "model.6.bias", "model.9.weight", "model.9.bias", "model.13.weight",
            "model.13.bias"} <= set(names)
    for _, p in net.named_parameters():   # _backward_raw accumulated into the flat gradient buffer: exposed as .grad
        assert p.grad is not None
    check_grads_vs_kink_reference(what, net, case, dx, dtype, TOL_GRAD[dtype], TOL_GRAD_L2[dtype], y=y)
    print(f"{what}: {time.time() - t0:.1f} s")
    record(what + " seconds", time.time() - t0)
