"""CPU tier: the fp64 restatements of tests/vgg_ops_ref.py against torch's own operators, autograd and the pinned loss functions of
oracle.torch_ref, and - through gi_debug_igemm_plan, no GPU - which mode-2 kernel serves every convolution case of
tests/test_vgg_ops_gpu.py."""
import importlib.util
import math
import os

import pytest
import torch
import torch.nn.functional as F

import gan_inpainting_amd  # noqa: F401
import vgg_grad_ref as G
import vgg_ops_ref as R
from gan_inpainting_amd import backend as B
from oracle import torch_ref as orc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("dispatch_table", os.path.join(ROOT, "tools", "dispatch_table.py"))
DT = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(DT)
F64 = torch.float64


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _close(a, b, tol=1e-12):
    return float((a - b).abs().max()) <= tol * (float(b.abs().max()) + 1e-300)


def test_conv3x3_and_the_transposed_weight_identity():
    g = _gen(1)
    n, H, W, cin, cout = 2, 5, 7, 8, 16
    x = torch.randn(n, H, W, cin, generator=g, dtype=F64).requires_grad_(True)
    w, b = torch.randn(cout, cin, 3, 3, generator=g, dtype=F64), torch.randn(cout, generator=g, dtype=F64)
    y = F.conv2d(x.permute(0, 3, 1, 2), w, b, padding=1)
    assert _close(R.conv3x3(x.detach(), w, b), y.detach().permute(0, 2, 3, 1))
    assert _close(R.conv3x3(x.detach(), w, b, relu=True), torch.relu(y).detach().permute(0, 2, 3, 1))
    up = torch.randn(n, H, W, cout, generator=g, dtype=F64)
    y.backward(up.permute(0, 3, 1, 2))
    assert _close(R.conv3x3_input_grad(up, w), x.grad)
    # what pack3x3_t_kernel writes, [cin][8 - tap][cout], is transposed_weights in the tap-major layout of pack3x3_kernel
    wt = R.transposed_weights(w)
    packed = w.reshape(cout, cin, 9).flip(2).permute(1, 2, 0)
    assert torch.equal(wt.reshape(cin, cout, 9).permute(0, 2, 1), packed)


def test_mask_add_is_the_relu_backward_of_the_sum():
    g = _gen(2)
    z = torch.randn(3, 4, 5, 8, generator=g, dtype=F64)
    z[::2, ::2] = 0.0
    zz = z.clone().requires_grad_(True)
    y, add = torch.randn(z.shape, generator=g, dtype=F64), torch.randn(z.shape, generator=g, dtype=F64)
    torch.relu(zz).backward(y + add)
    assert torch.equal(R.mask_add(y, torch.relu(z), add), zz.grad)
    assert torch.equal(R.mask_add(y, torch.relu(z)), torch.where(z > 0, y, torch.zeros_like(y)))


def _tied_map(g, n, H, W, C):
    """a post-ReLU-like map with ties inside windows and windows that are zero throughout"""
    a = torch.randint(0, 3, (n, H, W, C), generator=g).to(F64)
    a[:, :2, :2] = 0.0
    a[:, 2:4, 2:4] = 1.0
    return a


def test_pooling_against_max_pool2d_and_its_autograd():
    g = _gen(3)
    n, H, W, C = 2, 6, 10, 8
    for tied in (False, True):
        a = _tied_map(g, n, H, W, C) if tied else torch.randn(n, H, W, C, generator=g, dtype=F64)
        assert torch.equal(R.maxpool2(a), F.max_pool2d(a.permute(0, 3, 1, 2), 2, 2).permute(0, 2, 3, 1))
        up = torch.randn(n, H // 2, W // 2, C, generator=g, dtype=F64)
        # relu = 0: the gradient w.r.t. the pooled map's input itself
        aa = a.clone().requires_grad_(True)
        F.max_pool2d(aa.permute(0, 3, 1, 2), 2, 2).backward(up.permute(0, 3, 1, 2))
        got = R.pool_bwd(up, a, relu=0)
        assert torch.equal(got, aa.grad), tied
        assert int((got != 0).sum()) == up.numel(), "every window routes its value to exactly one position"
        # relu = 1: w.r.t. the pre-activation z, a = relu(z)
        z = torch.where(a > 0, a, -torch.rand(a.shape, generator=g, dtype=F64)).requires_grad_(True)
        F.max_pool2d(torch.relu(z).permute(0, 3, 1, 2), 2, 2).backward(up.permute(0, 3, 1, 2))
        assert torch.equal(R.pool_bwd(up, torch.relu(z.detach()), relu=1), z.grad), tied


def test_act_bwd_against_autograd():
    g = _gen(4)
    shape = (2, 3, 5, 8)
    z = torch.randn(shape, generator=g, dtype=F64)
    z[0, 0] = 0.0
    gg, sd = torch.randn(shape, generator=g).half(), torch.randn(shape, generator=g).half()
    zz = z.clone().requires_grad_(True)
    summed = (gg.float() + sd.float()).half().double()
    torch.relu(zz).backward(summed)
    assert torch.equal(R.act_bwd(gg, torch.relu(z), sd, 1), zz.grad)
    assert torch.equal(R.act_bwd(gg, torch.relu(z), sd, 0), summed)
    assert torch.equal(R.act_bwd(None, torch.relu(z), sd, 0), sd.double()) and torch.equal(R.act_bwd(gg, torch.relu(z), None, 0), gg.double())


def _tap(g, n, H, W, C):
    Fm = (torch.relu(torch.randn(2 * n, H * W, C, generator=g)) * 1.5).half().double()
    as_nchw = lambda t: t.transpose(1, 2).reshape(t.shape[0], C, H, W)   # noqa: E731
    return Fm, as_nchw


def test_gram_and_terms_against_the_oracle():
    n, H, W, C = 2, 3, 5, 64
    Fm, as_nchw = _tap(_gen(5), n, H, W, C)
    assert _close(R.gram(Fm), orc.gram_matrix(as_nchw(Fm)))
    p, s, dG = R.tap_terms(Fm, n)
    pt, st = G.terms([as_nchw(Fm[:n])], [as_nchw(Fm[n:])])
    assert abs(float(p) - float(pt[0])) <= 1e-12 * float(pt[0]) and abs(float(s) - float(st[0])) <= 1e-12 * float(st[0])
    assert _close(dG, orc.gram_matrix(as_nchw(Fm[:n])) - orc.gram_matrix(as_nchw(Fm[n:])))
    assert torch.equal(dG, dG.transpose(1, 2))


@pytest.mark.parametrize("wp,ws", [(1.0, 0.0), (0.0, 1.0), (0.05, 100.0)])
def test_seed_with_unit_scale_is_the_autograd_gradient_of_the_loss(wp, ws):
    """the restated seed differs from the fp64 gradient by what it restates: dG rounded to fp16 after the power-of-two normalisation
    (2^-11 relative per element, fp16's subnormal spacing 2^-24 absolute) and the two coefficients rounded to fp32"""
    n, H, W, C = 2, 4, 4, 64
    Fm, as_nchw = _tap(_gen(6), n, H, W, C)
    fo = Fm[:n].clone().requires_grad_(True)
    pt, st = G.terms([as_nchw(fo)], [as_nchw(Fm[n:])])
    (wp * pt[0] + ws * st[0]).backward()
    dG = R.tap_terms(Fm, n)[2].float()
    dmax = float(dG.abs().max())
    sd, mag, cs1 = R.seed(Fm[:n], Fm[n:], dG, dmax, n, wp, ws)
    assert _close(sd, G.seeds([as_nchw(Fm[:n])], [as_nchw(Fm[n:])], wp, ws)[0].reshape(n, C, H * W).transpose(1, 2), 2e-3)
    bound = 2.0 ** -10 * mag + cs1 * 2.0 ** -24 * Fm[:n].abs().sum(2, keepdim=True) + 2.0 ** -22 * fo.grad.abs() + 1e-300
    assert float(((sd - fo.grad).abs() / bound).max()) <= 1.0
    assert float((sd - fo.grad).abs().max()) > 0 or ws == 0.0


def test_conv1_and_its_adjoint_against_the_replicated_grey_convolution():
    g = _gen(7)
    n, H, W = 2, 6, 16
    w, b = torch.randn(64, 3, 3, 3, generator=g) * 0.2, torch.randn(64, generator=g) * 0.1
    xa, xb = torch.rand(n, H, W, generator=g), torch.rand(n, H, W, generator=g)
    w1 = R.w1_of(w)
    assert w1.dtype == torch.float32 and _close(w1.double(), w.double().sum(1).reshape(64, 9), 1e-6)
    x = torch.cat([xa, xb])[:, None].double().requires_grad_(True)
    y = F.conv2d(x.repeat(1, 3, 1, 1), w.double(), b.double(), padding=1)
    ref, mag = R.conv1(xa, xb, w1, b)
    # (image and summed weights rounded to fp16: 2^-11 each per product)
    assert float(((ref - torch.relu(y).detach().permute(0, 2, 3, 1)).abs() / mag).max()) <= 2.0 ** -10
    D = torch.randn(2 * n, H, W, 64, generator=g).half().double()
    y.backward(D.permute(0, 3, 1, 2))
    adj, amag = R.conv1_adjoint(D, w1, 0.375)
    assert float(((adj - 0.375 * x.grad[:, 0]).abs() / (0.375 * amag)).max()) <= 2.0 ** -22


def test_sampling_rule_and_scale():
    assert R.sampled_blocks(8) == list(range(8)) and R.sampled_blocks(1) == [0]
    assert R.sampled_blocks(9) == [0, 8], "nine blocks: 8 + 3 lies beyond the map, the pass falls back to block 8"
    assert R.sampled_blocks(15) == [0, 11] and R.sampled_blocks(16) == [0, 11] and R.sampled_blocks(17) == [0, 11, 16]
    assert R.sampled_blocks(64) == [8 * j + (3 * j) % 8 for j in range(8)]
    m = R.sampled_mask(2304)
    assert int(m.sum()) == 512 and bool(m[:256].all()) and bool(m[2048:].all())
    for am in (0.3, 1.0, 1e-30, 6e4, 2.0 ** -149):
        s = R.scale(am)
        assert math.frexp(s)[0] == 0.5 and (2.0 ** -3 <= am * s < 2.0 ** -2 or am < 2.0 ** -100)
    assert R.scale(0.0) == 1.0 and R.scale(math.inf) == 1.0 and R.scale(math.nan) == 1.0
    assert R.scale(2.0 ** -140) == 2.0 ** 100 and R.scale(2.0 ** 127) == 2.0 ** -100, "the exponent is clamped to +-100"


# ---- which kernel serves the convolution cases of the GPU tier --------------------------------------------------------------------
def _plan(kernel, opts, shape, d, epi):
    n, Hs, Ws, cin, cout = shape

    def hook(ex):
        if epi.startswith("mask"):
            ex.mask, ex.ldmask, ex.mask_slope = 1 << 20, cout, 0.0
            if epi == "mask+add":
                ex.add, ex.ldadd = 1 << 20, cout
    offered = (DT.OFFER_BIAS if d == "F" else 0) | (DT.OFFER_POOL2 if epi == "pool" else 0)
    return DT.plan_row(B, DT._case(2, n, Hs, Ws, cin, cout, opts=opts), offered=offered, ex_hook=hook)


def test_conv_cases_reach_every_mode2_kernel():
    rows = []
    for kernel, opts, shape, d, epi, pool_applied, mask_applied in R.conv_variants():
        got = _plan(kernel, opts, shape, d, epi)
        assert got["rc"] == 0 and got["kernel"] == kernel, (kernel, shape, d, epi, got["kernel"], got["error"])
        assert got["_info"].pool_applied == pool_applied and got["mask_applied"] == mask_applied, (kernel, shape, d, epi)
        rows.append((kernel, epi, pool_applied, mask_applied))
    assert {r[0] for r in rows} == {"igemm8<2>", "igemm8<2,64>", "igemm5<2,128>", "igemm5<2,64>", "igemm3<2,128>", "igemm3<2,64>"}
    assert any(r[2] == 1 for r in rows), "no case takes the pooled store"
    assert any(r[1] == "pool" and r[2] == 0 for r in rows), "no case is offered the pooled store and declines"
    for fam in ("igemm8", "igemm5"):
        assert any(r[0].startswith(fam) and r[3] == 1 for r in rows), fam
    assert any(r[0].startswith("igemm3") and r[1].startswith("mask") and r[3] == 0 for r in rows)
    # the directions only name channel pairs VGG-19 has
    fwd = {(64, 64), (64, 128), (128, 128), (128, 256), (256, 256), (256, 512), (512, 512)}
    for kernel, opts, shape, dirs, extras in R.CONV_CASES:
        assert ("F" not in dirs or shape[3:] in fwd) and ("T" not in dirs or shape[:2:-1] in fwd), shape
