"""GPU tier of the EMA generator: gi_ema_update against its numpy restatement (tests/ema_ref.py), the overflow guard,
optim.EMA.applied() and the wiring into the step objects."""
import numpy as np
import pytest
import torch

import ema_ref

pytestmark = pytest.mark.gpu

COUNTS = (1, 7, 255, 256, 4099, 2 ** 20 + 5)
DECAYS = (0.0, 0.5, 0.999, 1.0)
PAD = 4      # floats in front of a view: 16 bytes, so the view's float offset 0 / 1 is also its misalignment


def _B():
    import gan_inpainting_amd  # noqa: F401
    from gan_inpainting_amd import backend as B
    return B


def _inputs(count):
    """(ema, p) as float32 numpy, shared by every case of one count: magnitudes from 1e-3 to 1e3, p near ema and far from it."""
    g = torch.Generator().manual_seed(1000 + count % 997)
    scale = 10.0 ** torch.randint(-3, 4, (count,), generator=g).float()
    ema = torch.randn(count, generator=g) * scale
    p = torch.where(torch.rand(count, generator=g) < 0.5, ema + torch.randn(count, generator=g) * scale * 1e-3, torch.randn(count, generator=g) * scale)
    return ema.float().numpy(), p.float().numpy()


def _place(values, off):
    """A device allocation of PAD + off + count + PAD floats holding `values` at float offset PAD + off and a sentinel elsewhere."""
    buf = torch.full((PAD + off + values.size + PAD,), 12345.0, dtype=torch.float32, device="cuda")
    buf[PAD + off: PAD + off + values.size] = torch.from_numpy(values).cuda()
    assert buf.data_ptr() % 16 == 0
    return buf, buf[PAD + off: PAD + off + values.size]


def _update(B, ema_view, p_view, decay, guard=None):
    B.check(B.lib().gi_ema_update(B.get_ctx(ema_view.device), B.ptr(ema_view), B.ptr(p_view), ema_view.numel(), float(decay), B.ptr(guard)))


@pytest.mark.parametrize("count", COUNTS)
def test_kernel_matches_the_restatement(count):
    B = _B()
    ema0, p0 = _inputs(count)
    worst = 0.0
    for eo in (0, 1):
        for po in (0, 1):
            for decay in DECAYS:
                ebuf, ev = _place(ema0, eo)
                pbuf, pv = _place(p0, po)
                before_e, before_p = ebuf.clone(), pbuf.clone()
                _update(B, ev, pv, decay)
                out = ev.cpu().numpy()
                ratio = ema_ref.worst_ratio(out, ema0, p0, decay)
                worst = max(worst, ratio)
                assert ratio <= 1.0, f"count {count} offsets ({eo},{po}) decay {decay}: |out - E| is {ratio:.3f} of the bound"
                ref = ema_ref.ema_update(ema0, p0, decay)
                ulps = np.abs(out.view(np.int32).astype(np.int64) - ref.view(np.int32).astype(np.int64)).max()
                assert ulps <= 1, f"count {count} offsets ({eo},{po}) decay {decay}: {ulps} ulps from the restatement"
                if decay == 1.0:
                    assert np.array_equal(out.view(np.uint32), ema0.view(np.uint32)), "decay = 1 must leave ema bit-identical"
                # nothing outside [0, count) of either buffer, and nothing of p
                lo, hi = PAD + eo, PAD + eo + count
                assert torch.equal(ebuf[:lo], before_e[:lo]) and torch.equal(ebuf[hi:], before_e[hi:]), \
                    f"count {count} offsets ({eo},{po}): elements outside the range were written"
                assert torch.equal(pbuf, before_p)
    print(f"count {count}: worst |out - E| / bound over offsets and decays = {worst:.3f}")


@pytest.mark.parametrize("count", (7, 4099))
def test_equal_inputs_are_a_fixed_point(count):
    B = _B()
    ema0, _ = _inputs(count)
    for off in (0, 1):
        for decay in DECAYS:
            _, ev = _place(ema0, off)
            _, pv = _place(ema0, 1 - off)
            _update(B, ev, pv, decay)
            assert np.array_equal(ev.cpu().numpy().view(np.uint32), ema0.view(np.uint32))


def test_guard_verdict_skips_the_whole_call():
    B = _B()
    ema0, p0 = _inputs(4099)
    _, ev = _place(ema0, 1)
    _, pv = _place(p0, 0)
    skipped = torch.tensor([3, 1, 0, 0], dtype=torch.int32, device="cuda")
    _update(B, ev, pv, 0.5, skipped)
    assert np.array_equal(ev.cpu().numpy().view(np.uint32), ema0.view(np.uint32))
    assert skipped.tolist() == [3, 1, 0, 0]
    taken = torch.tensor([3, 0, 1, 1], dtype=torch.int32, device="cuda")       # only word 1 is the verdict
    _update(B, ev, pv, 0.5, taken)
    out = ev.cpu().numpy()
    assert not np.array_equal(out, ema0) and ema_ref.worst_ratio(out, ema0, p0, 0.5) <= 1.0
    assert taken.tolist() == [3, 0, 1, 1]


def test_ema_follows_the_optimizers_guard():
    """optim.EMA.update(opt) after an update the fp16 guard skipped leaves the average alone; after a taken one it moves."""
    import gan_inpainting_amd  # noqa: F401
    from gan_inpainting_amd import optim
    from gan_inpainting_amd.lib.models import networks
    torch.manual_seed(3)
    net = networks.PatchGANDiscriminator(image_size=64, dtype="fp16").cuda()
    opt = optim.Adam(net.parameters(), lr=2e-4, betas=(0.5, 0.999))
    ema = optim.EMA(net, 0.5)
    ema.flat.add_(1.0)                      # away from the parameters, so that a taken update shows
    before = ema.flat.clone()
    net.flat_grads().normal_()
    net.flat_grads()[5] = float("inf")
    opt.step()
    ema.update(opt)
    assert torch.equal(ema.flat, before)
    net.flat_grads().normal_()
    opt.step()
    ema.update(opt)
    assert not torch.equal(ema.flat, before)
    assert opt.poll_skipped() == 1
    # an fp32 network has no guard: NULL goes to the kernel
    net32 = networks.PatchGANDiscriminator(image_size=64, dtype="fp32").cuda()
    opt32 = optim.Adam(net32.parameters())
    ema32 = optim.EMA(net32, 0.5)
    start = ema32.flat.cpu().numpy()
    net32.flat_grads().normal_()
    opt32.step()
    ema32.update(opt32)
    assert ema_ref.worst_ratio(ema32.flat.cpu().numpy(), start, net32.flat_params().cpu().numpy(), 0.5) <= 1.0
    assert not np.array_equal(ema32.flat.cpu().numpy(), start)


@pytest.mark.parametrize("dtype", ["fp32", "fp16"])
def test_applied_swaps_in_the_average_and_restores(dtype):
    import gan_inpainting_amd  # noqa: F401
    from gan_inpainting_amd import optim
    from gan_inpainting_amd.lib.models import networks
    torch.manual_seed(5)
    G = networks.UnetGenerator(1, 1, 6, ngf=64, dtype=dtype).cuda().eval()
    x = torch.rand(2, 1, 64, 64, device="cuda")
    y_raw = G(x).clone()
    raw = G.flat_params().clone()
    ema = optim.EMA(G, 0.9)
    assert torch.equal(ema.flat, raw) and ema.flat.data_ptr() != raw.data_ptr()
    ema.flat.mul_(0.75)                                           # an average that is not the live weights
    avg = ema.flat.clone()
    with ema.applied():
        assert torch.equal(G.flat_params(), avg)
        y_avg = G(x).clone()
        sd_avg = {k: v.detach().cpu().clone() for k, v in G.state_dict().items()}
    assert torch.equal(G.flat_params(), raw), "the raw parameters must come back bit for bit"
    assert torch.equal(ema.flat, avg)
    assert torch.equal(G(x), y_raw), "the packed weight copies must follow the restored parameters"
    assert not torch.equal(y_avg, y_raw)
    G2 = networks.UnetGenerator(1, 1, 6, ngf=64, dtype=dtype)
    G2.load_state_dict(sd_avg)
    G2 = G2.cuda().eval()
    assert torch.equal(G2(x), y_avg)
    # state round trip
    ema2 = optim.EMA(G, 0.9)
    ema2.load_state_dict(ema.state_dict())
    assert torch.equal(ema2.flat, avg)


def _minimax(seed, **kw):
    import gan_inpainting_amd  # noqa: F401
    from gan_inpainting_amd import optim, trainer
    from gan_inpainting_amd.lib.models import networks
    torch.manual_seed(seed)
    G = networks.UnetGenerator(1, 1, 6, ngf=64, use_dropout="False", dtype="fp32").cuda()
    D = networks.PatchGANDiscriminator(sigmoid=True, image_size=64, dtype="fp32").cuda()
    oG = optim.Adam(G.parameters(), lr=0.0002, betas=(0.5, 0.999))
    oD = optim.Adam(D.parameters(), lr=0.0002, betas=(0.5, 0.999))
    if kw.pop("with_ema", False):
        kw["ema_G"] = optim.EMA(G, 0.9)
    return G, trainer.MinimaxStep(G, D, oG, oD, recon="l1", **kw)


def _batches():
    g = torch.Generator().manual_seed(21)
    out = []
    for _ in range(3):
        ground = torch.rand(4, 1, 64, 64, generator=g)
        mask = torch.zeros(4, 1, 64, 64)
        mask[:, :, 16:40, 20:48] = 1.0
        out.append((ground.cuda(), mask.cuda()))
    return out


def test_step_updates_the_average_after_every_generator_update():
    G, step = _minimax(9, with_ema=True)
    host = G.flat_params().cpu().numpy().astype(np.float64)         # the average, carried in float64 on the host
    om = float(ema_ref.om_of(0.9))
    allowed = np.zeros_like(host)
    for ground, mask in _batches():
        step(ground, mask)
        p = G.flat_params().cpu().numpy()
        allowed += ema_ref.bound(host, p, 0.9)
        host = host + om * (p.astype(np.float64) - host)
    dev = step.ema_G.flat.cpu().numpy().astype(np.float64)
    ratio = float((np.abs(dev - host) / allowed).max())
    print(f"three MinimaxStep calls: worst |device - host| / (three accumulated bounds) = {ratio:.3f}")
    assert ratio <= 1.0
    assert not np.array_equal(dev, G.flat_params().cpu().numpy().astype(np.float64))


def test_average_does_not_touch_training():
    finals = []
    for kw in ({}, {"ema_G": None}, {"with_ema": True}):
        G, step = _minimax(9, **kw)
        for ground, mask in _batches():
            step(ground, mask)
        finals.append(G.flat_params().clone())
    assert torch.equal(finals[0], finals[1]) and torch.equal(finals[0], finals[2])
