"""CPU tier: the restatements of tests/metrics_ref.py are right, against torch and the oracle in float64, and the probe inputs of
tests/test_metric_ops_gpu.py are what they claim. An edge case where a restatement could be wrong about the REFERENCE's behaviour
(argmax of NaN, 0/0 of an empty mask, an all-ignored cross entropy) is settled here, before any kernel is compared with it."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import metrics_ref as R
from oracle import params as op
from oracle import torch_ref as orc


@pytest.mark.parametrize("seed,n,c,h,w,ws", [(62, 2, 3, 33, 47, 11), (64, 2, 1, 24, 24, 7), (65, 1, 2, 9, 70, 11)])     # of make_golden.SSIM_CASES
def test_ssim_map_is_the_oracle_with_the_gaussian(seed, n, c, h, w, ws):
    x, y = (torch.from_numpy(a).double() for a in op.synth_ssim_pair(seed, n, c, h, w))
    m = R.ssim_map(x, y, R.gaussian(ws))
    assert m.dtype == torch.float64 and tuple(m.shape) == (n, c, h, w)
    assert abs(float(m.mean()) - float(orc.ssim(x, y, ws))) <= 1e-12
    assert (m.mean(dim=(1, 2, 3)) - orc.ssim(x, y, ws, size_average=False)).abs().max().item() <= 1e-12
    th, tw = R.tile_of(ws)
    sums, pixels = R.ssim_tiles(m, th, tw)
    assert tuple(sums.shape) == (n * c, -(-h // th), -(-w // tw)) and int(pixels.sum()) == h * w
    assert abs(float(sums.sum()) / (n * c * h * w) - float(m.mean())) <= 1e-12
    assert float(sums[1, 0, 0]) == pytest.approx(float(m.reshape(n * c, h, w)[1, :th, :tw].sum()), rel=1e-13)


def test_ssim_map_orientation_is_cross_correlation():
    """With an asymmetric window the map at one pixel, summed by hand: rows and columns both take g[k] at offset k - r."""
    g = R.asymmetric_window(7, 3)
    x, y = (torch.from_numpy(a).double() for a in op.synth_ssim_pair(5, 1, 1, 12, 15))
    m = R.ssim_map(x, y, g)
    gd, r, (py, px) = g.double(), 3, (5, 9)
    w2 = torch.outer(gd, gd)
    a, b = x[0, 0, py - r: py + r + 1, px - r: px + r + 1], y[0, 0, py - r: py + r + 1, px - r: px + r + 1]
    mu1, mu2 = (w2 * a).sum(), (w2 * b).sum()
    s1, s2, s12 = (w2 * a * a).sum() - mu1 * mu1, (w2 * b * b).sum() - mu2 * mu2, (w2 * a * b).sum() - mu1 * mu2
    ref = ((2 * mu1 * mu2 + R.C1) * (2 * s12 + R.C2)) / ((mu1 * mu1 + mu2 * mu2 + R.C1) * (s1 + s2 + R.C2))
    assert abs(float(m[0, 0, py, px]) - float(ref)) <= 1e-13
    flipped = R.ssim_map(x, y, torch.flip(g, [0]))
    assert (flipped - m).abs().max().item() > 1e-3          # the flip is visible: the GPU comparison can tell the two apart


@pytest.mark.parametrize("shape,ws", R.PROBE_CASES)
@pytest.mark.parametrize("kind", R.PROBE_KINDS)
def test_ssim_probes_reach_only_the_tiles_they_claim(shape, ws, kind):
    """The deficit pixels - sum of a tile is exactly 0 where no window touches the change, and at least 0.1 in each of the four tiles
    that share the first tile corner, for the strips and the two pixels at that corner: the tiles across the border or the corner see
    the change through their halo alone. One pixel in the image's last corner, whose windows are mostly padding, moves its four tiles by
    0.01 to 0.15 only: there the deficit must be positive, and the bound it meets on the device is that of a tile of one to 32 pixels.
    The noise seed of ssim_probe is one at which the single replaced pixels differ visibly from the originals; this test holds it there."""
    th, tw = R.tile_of(ws)
    r, (H, W) = ws // 2, shape[2:]
    x, _ = op.synth_ssim_pair(91, *shape)
    y, region = R.ssim_probe(x, kind, th, tw, r)
    sums, pixels = R.ssim_tiles(R.ssim_map(x, y, R.gaussian(ws)), th, tw)
    deficit = (pixels - sums[0]).numpy()
    reach = R.probe_reach(region, r, H, W, th, tw)
    assert (deficit[~reach] == 0).all(), (kind, deficit)
    assert (deficit[reach] > 0).all()
    rows, cols = R.probe_corner(kind, H, W, th, tw)
    four = deficit[np.ix_(rows, cols)]
    print(f"{shape} ws {ws} {kind}: corner-tile deficits {four.round(3).tolist()}, tiles reached {int(reach.sum())} of {reach.size}")
    assert reach[np.ix_(rows, cols)].all() and (four >= (0.1 if kind != "last" else 0.01)).all(), four
    if kind in ("corner_in", "corner_out") and r < min(th, tw):
        assert int(reach.sum()) == 4


def test_recon_is_the_oracle_on_a_binary_mask():
    g, mk = op.synth_batch(8300, 2, 40, 56, fractional_edge=True)
    gen = np.random.Generator(np.random.PCG64(8301)).random(g.shape, dtype=np.float32)
    m = np.ceil(mk)
    ref = orc.eval_recon_batch(torch.from_numpy(g), torch.from_numpy(gen), torch.from_numpy(mk))
    out, sums, metrics = R.recon(g, gen, m, 1e-16)
    assert out.dtype == np.float32 and np.array_equal(out.view(np.int32), ref[0].numpy().reshape(-1).view(np.int32))
    ref64 = orc.eval_recon_batch(torch.from_numpy(g).double(), torch.from_numpy(gen).double(), torch.from_numpy(mk).double())
    for k in range(4):
        assert abs(float(metrics[k]) - float(ref64[1 + k])) <= 1e-6 * max(1.0, abs(float(ref64[1 + k]))), k
    assert sums[4] == np.count_nonzero(m)


def test_recon_of_an_empty_mask_is_the_oracle_s_zero_over_zero():
    g, _ = op.synth_batch(8302, 1, 16, 16)
    gen = np.random.Generator(np.random.PCG64(8303)).random(g.shape, dtype=np.float32)
    ref = [float(v) for v in orc.eval_recon_batch(torch.from_numpy(g), torch.from_numpy(gen), torch.zeros(g.shape))[1:]]
    out, sums, metrics = R.recon(g, gen, np.zeros_like(g), 1e-16)
    assert np.array_equal(out, g.reshape(-1)) and sums.tolist() == [0, 0, 0, 0, 0]
    assert ref[0] == pytest.approx(1e-8, rel=1e-6) and ref[1] == 0 and np.isnan(ref[2]) and np.isnan(ref[3])
    assert float(metrics[0]) == pytest.approx(1e-8, rel=1e-6) and metrics[1] == 0 and np.isnan(metrics[2]) and np.isnan(metrics[3])


def test_recon_takes_a_fractional_mask_as_given():
    rng = np.random.Generator(np.random.PCG64(8304))
    g, gen = rng.random(777, dtype=np.float32), rng.random(777, dtype=np.float32)
    m = rng.choice(np.array([0, 0.5, 1], np.float32), size=777)
    out, sums, _ = R.recon(g, gen, m, 1e-16)
    tg, tgen, tm = (torch.from_numpy(a) for a in (g, gen, m))
    assert torch.equal(torch.from_numpy(out), tgen * tm + tg * (1 - tm))
    assert sums[4] == int((m != 0).sum())
    assert sums[2] == pytest.approx(float((torch.from_numpy(out) * tm - tg * tm).double().abs().sum()), rel=1e-14)


def test_seg_counts_give_the_oracle_s_ratios():
    labels, logits = op.synth_segmentation(74, 2, 4, 16, 24, with_minus_one=True)
    assert (labels == -1).any()
    uniq = [0, 1, 2, 3]
    counts = R.seg_counts(labels.reshape(2, -1), logits.reshape(2, 4, -1), uniq)
    per, across = R.seg_ratios(counts)
    om, oa = orc.segmentation_eval_metric(torch.from_numpy(labels), torch.from_numpy(logits), uniq)
    for i, u in enumerate(uniq):
        for j, k in enumerate(("precision", "recall", "iou")):
            assert abs(float(per[i, j]) - float(om[u][k])) <= 2e-7, (u, k)
    for j, k in enumerate(("precision", "recall", "iou")):
        assert abs(float(across[j]) - float(oa[k])) <= 2e-7
    pred = torch.argmax(torch.from_numpy(logits), 1).reshape(2, -1).numpy()
    assert counts[1, 2].tolist() == [int(((pred[1] == 2) & ((labels[1].reshape(-1) == 2) | (labels[1].reshape(-1) == -1))).sum()),
                                     int((pred[1] == 2).sum()), int(((labels[1] == 2) | (labels[1] == -1)).sum())]


def test_argmax_rule_is_torch_s():
    nan, inf = float("nan"), float("inf")
    rows = [[1, nan, nan, 5], [nan, 1, 2, 3], [1, 1, 0, 0], [-inf, -inf, -inf, -inf], [inf, nan, inf, 0], [0, inf, inf, -inf], [3, 2, 3, nan]]
    lg = np.array(rows, dtype=np.float32).T[None]                     # (1, K, hw): a row of `rows` is one pixel
    want = torch.argmax(torch.from_numpy(lg), 1)[0].tolist()
    assert want[:3] == [1, 0, 0]
    assert R.argmax_first(lg)[0].tolist() == want
    rng = np.random.Generator(np.random.PCG64(12))
    big = rng.integers(-2, 3, size=(3, 6, 500)).astype(np.float32)      # many ties
    big[rng.random(big.shape) < 0.1] = nan
    assert np.array_equal(R.argmax_first(big), torch.argmax(torch.from_numpy(big), 1).numpy())


def test_tv_and_ce_are_float64_and_full():
    rng = np.random.Generator(np.random.PCG64(13))
    x = rng.random((3, 5, 7), dtype=np.float32)
    loss, grad = R.tv(x, 0.1)
    assert grad.dtype == np.float64 and grad.shape == x.shape
    xd = x.astype(np.float64)
    by_hand = 0.1 * (((xd[:, :-1] - xd[:, 1:]) ** 2).mean() + ((xd[:, :, :-1] - xd[:, :, 1:]) ** 2).mean())
    assert loss == pytest.approx(by_hand, rel=1e-14)
    e = np.zeros_like(xd)
    e[1, 4, 0] = 1e-6                                                  # a pixel of the last row: its gradient has no term from the next plane
    assert (R.tv(xd + e, 0.1)[0] - R.tv(xd - e, 0.1)[0]) / 2e-6 == pytest.approx(grad[1, 4, 0], rel=1e-6)
    z = rng.standard_normal((2, 4, 33)).astype(np.float32)
    y = rng.integers(0, 4, size=(2, 33))
    y[0, :5], y[1, :3], y[1, 3:6] = -100, 7, -3
    w = [0, 1.2, 0.7, 0.7]
    loss, grad, wsum = R.ce(z, y, w, -100)
    valid = (y >= 0) & (y < 4)
    lse = torch.logsumexp(torch.from_numpy(z).double(), 1).numpy()
    wy = np.array(w, dtype=np.float32).astype(np.float64)[np.where(valid, y, 0)] * valid
    zy = np.take_along_axis(z.astype(np.float64), np.where(valid, y, 0)[:, None], 1)[:, 0]
    assert wsum == pytest.approx(wy.sum(), rel=1e-14) and loss == pytest.approx((wy * (lse - zy)).sum() / wy.sum(), rel=1e-13)
    assert (grad[0, :, :5] == 0).all() and (grad[1, :, :6] == 0).all() and grad.dtype == np.float64


def test_ce_all_ignored_is_nan_with_a_zero_gradient():
    z = torch.randn(2, 3, 9, generator=torch.Generator().manual_seed(1))
    for ignore, y in ((-100, torch.full((2, 9), -100)), (255, torch.full((2, 9), 255)), (-100, torch.full((2, 9), 3))):
        loss, grad, wsum = R.ce(z.numpy(), y.numpy(), None, ignore)
        assert np.isnan(loss) and (grad == 0).all() and wsum == 0
    t = z.double().requires_grad_(True)
    ref = F.cross_entropy(t, torch.full((2, 9), -100))
    ref.backward()
    assert torch.isnan(ref) and (t.grad == 0).all()
