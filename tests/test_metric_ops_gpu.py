"""GPU tier: the kernels behind the reported metrics and config 5's auxiliary losses (csrc/ssim.hip, csrc/evalmetrics.hip,
csrc/auxloss.hip) ONE OP AT A TIME through the C-ABI, against the float64 restatements of tests/metrics_ref.py (proved against torch and
the oracle by tests/test_metrics_ref_cpu.py). A mean over thousands of pixels hides a halo column read as zero or a window applied
backwards; here every SSIM tile sum, every integer count, every composite bit and every gradient element is compared.

  SSIM      per tile against ssim_tiles of the float64 map, with the bound MEASURED per case: 8 x max(what the same formula in torch
            float32 deviates from float64 on the case's tiles, pixels x 2^-23); an asymmetric window pins the orientation of both passes,
            window_host = NULL the window built in C, strip and pixel probes next to a tile border the halo loads.
  recon     inpainted_out bit for bit, the count word exactly, the metrics at the project's 1e-6 x max(1, |ref|), NaN for NaN on an empty
            mask; counts below a wave, around a block, off the 2048 multiple and past the 1024-block cap.
  seg       the integer counts exactly (NaN, +-inf, ties, label -1, K = 1, labels >= K, the 64-block cap, every template width).
  TV / CE   loss and the WHOLE gradient at non-square shapes, every K, logits of +-90, labels outside [0, K), gscale != 1.

Every output and scratch buffer is pre-filled (NaN or 0x5A5A5A5A) and followed by 16 guard words that must keep the fill; every input
stands in NaN (or -1) padding. Each test prints its worst error over its bound and records it (GI_PARITY_OUT).

Worst |err| / bound on an MI355X (each test's docstring has its own): SSIM tiles 0.07, asymmetric window 0.04, probes 0.08, built-in
window 0.07 of TOL; reconstruction metrics below 0.001; TV 0.10; cross entropy 0.12, with logits of +-90 0.07. The 140 cases take 4 s.

Found by this file: eval_recon_partial_kernel promised the reference's two roundings through __fadd_rn(__fmul_rn(gen, m), masked) and
compiled to one fused multiply-add all the same (v_fmac_f32 in its loop), an ulp off wherever gen * m is inexact. It now uses
plain operators under `#pragma clang fp contract(off)`; binary masks, and {0, 0.5, 1}, gave and give the same bits."""
import ctypes as C
import functools
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import metrics_ref as R  # noqa: E402
from gpu_util import B, record  # noqa: E402
from oracle import params as op  # noqa: E402

TOL = 2e-6                    # tests/test_ssim_gpu.py: absolute, on a mean in [0, 1]
FILL = 0x5A5A5A5A
GUARD = 16                    # words behind every output that must keep the fill
PAD = 4                       # elements of NaN / -1 in front of and behind every input
INVALID = -1                  # GI_ERR_INVALID
NAN = float("nan")
S11_TH, S11_TW = 16, 64       # ssim11_kernel's tile; ssim_plan gives every window <= 11 the same and the larger ones 8 x 32


# ---- plumbing ---------------------------------------------------------------------------------------------------------------------

def _call(status):
    if status != 0 and b"->" in (B.lib().gi_last_error() or b""):     # a HIP error, not a rejected argument: nothing may follow it
        pytest.exit("HIP error: " + B.lib().gi_last_error().decode(errors="replace"), returncode=3)
    B.check(status)


def _refused(status):
    why = B.lib().gi_last_error() or b""
    if status != 0 and b"->" in why:
        pytest.exit("HIP error: " + why.decode(errors="replace"), returncode=3)
    return status == INVALID and bool(why)


def _sync():
    try:
        torch.cuda.synchronize()
    except RuntimeError as e:     # a fault of the device: the session ends here, no further launch
        pytest.exit(f"device error: {e}", returncode=3)


def _in(a, pad=PAD):
    """A device copy of `a` that stands in NaN (floats) or -1 (integers) padding; the view keeps the allocation alive."""
    v = torch.from_numpy(np.ascontiguousarray(a).reshape(-1))
    buf = torch.full((pad + v.numel() + pad,), NAN if v.dtype.is_floating_point else -1, dtype=v.dtype, device="cuda")
    buf[pad:pad + v.numel()] = v.cuda()
    return buf[pad:pad + v.numel()]


def _fout(n):
    """n fp32 outputs + guard, all NaN"""
    return torch.full((n + GUARD,), NAN, dtype=torch.float32, device="cuda")


def _words(n):
    """n 32-bit words of scratch + guard, all 0x5A5A5A5A (8-byte aligned, as every torch allocation)"""
    t = torch.full((n + GUARD + (n & 1),), FILL, dtype=torch.int32, device="cuda")
    assert t.data_ptr() % 8 == 0
    return t


def _kept_nan(buf, n, what):
    assert bool(torch.isnan(buf[n:]).all()), f"{what}: a guard word behind an output was written"


def _kept_fill(buf, n, what):
    assert bool((buf[n:] == FILL).all()), f"{what}: a guard word behind a scratch buffer was written"


def _floats(seq):
    return C.cast((C.c_float * len(seq))(*[float(v) for v in seq]), C.c_void_p)


def _report(what, ratio, **extra):
    print(f"{what}: worst |err| / bound = {ratio:.3f}" + "".join(f" {k}={v:.3e}" for k, v in extra.items()))
    record("metric_ops " + what, {"ratio": float(ratio), **{k: float(v) for k, v in extra.items()}})


# ---- SSIM -------------------------------------------------------------------------------------------------------------------------

def test_the_constants_these_tests_rely_on_are_the_source_s():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = open(os.path.join(root, "gan-inpainting_amd", "csrc", "ssim.hip")).read()
    assert f"constexpr int S11_TH = {S11_TH}, S11_TW = {S11_TW}," in src
    assert "if (ws <= 11) { p->th = 16; p->tw = 64; } else { p->th = 8; p->tw = 32; }" in src
    assert "if (window_size == 11)" in src and "else if (p.th == 16)" in src
    assert R.tile_of(11) == R.tile_of(1) == (S11_TH, S11_TW) and R.tile_of(13) == R.tile_of(31) == (8, 32)
    assert "p->total_floats = p->partial_floats + 2 * (int64_t)n;" in src          # [partial | pad to even | n doubles]


def _ssim_raw(x, y, ws, window):
    """gi_ssim on (n,c,H,W) numpy pairs; window: a 1-D fp32 tensor, or None for the window built in C. Returns per_sample [n], mean and
    partial [n*c, ty, tx], the per-tile sums the kernel left in the caller's scratch."""
    lib, ctx = B.lib(), B.get_ctx()
    n, c, H, W = x.shape
    th, tw = R.tile_of(ws)
    ty, tx = -(-H // th), -(-W // tw)
    np_ = n * c * ty * tx
    ns = int(lib.gi_ssim_scratch_floats(n, c, H, W, ws))
    assert ns == np_ + (np_ & 1) + 2 * n, "the scratch layout is [partial | pad to even | n doubles]"
    dx, dy = _in(x), _in(y)
    per, mean, scratch = _fout(n), _fout(1), _words(ns)
    _call(lib.gi_ssim(ctx, dx.data_ptr(), dy.data_ptr(), n, c, H, W, ws, _floats(window.tolist()) if window is not None else None,
                      per.data_ptr(), mean.data_ptr(), scratch.data_ptr()))
    _sync()
    what = f"ssim {x.shape} ws {ws}"
    _kept_nan(per, n, what)
    _kept_nan(mean, 1, what)
    _kept_fill(scratch, ns, what)
    s = scratch.cpu().numpy()
    assert (s[np_:np_ + (np_ & 1)] == FILL).all(), f"{what}: the pad word between the tile sums and the sample sums was written"
    sums = s[np_ + (np_ & 1):ns].view(np.float64)
    partial = s[:np_].view(np.float32).reshape(n * c, ty, tx).astype(np.float64)
    assert np.abs(sums - partial.reshape(n, -1).sum(1)).max() <= 1e-9 * max(1.0, np.abs(sums).max()), f"{what}: sample sums are not the tile sums'"
    return per[:n].cpu().numpy().astype(np.float64), float(mean[0]), partial


def _tile_compare(what, x, y, ws, g, window):
    """Every tile sum of gi_ssim(x, y) against the float64 map under the window g; returns (deficit, reference deficit, bound)."""
    th, tw = R.tile_of(ws)
    m64 = R.ssim_map(x, y, g)
    s64, pixels = R.ssim_tiles(m64, th, tw)
    s32, _ = R.ssim_tiles(R.ssim_map(x, y, g, torch.float32), th, tw)
    s64, pixels = s64.numpy(), pixels.numpy()
    dev = float(np.abs(s32.double().numpy() - s64).max())
    bound = 8 * np.maximum(dev, pixels * 2.0 ** -23)[None]                     # [1, ty, tx]
    per, mean, partial = _ssim_raw(x, y, ws, window)
    err = np.abs(partial - s64)
    ratio = float((err / bound).max())
    _report(what, ratio, fp32_dev=dev, bound_max=float(bound.max()), err_max=float(err.max()))
    where = np.unravel_index(int((err / bound).argmax()), err.shape)
    assert ratio <= 1, f"{what}: tile {where} sums to {partial[where]!r}, float64 map {s64[where]!r}, bound {np.broadcast_to(bound, err.shape)[where]:.3e}"
    ref_per = m64.mean(dim=(1, 2, 3)).numpy()
    assert np.abs(per - ref_per).max() <= TOL, f"{what}: per_sample {per} vs {ref_per}"
    assert abs(mean - float(m64.mean())) <= TOL, f"{what}: mean {mean} vs {float(m64.mean())}"
    return pixels[None] - partial, pixels[None] - s64, bound


@functools.lru_cache(maxsize=None)
def _pair(shape):
    return op.synth_ssim_pair(90 + sum(shape), *shape)


SSIM_SHAPES = ([((2, 1, 16, 64), 11), ((1, 1, 15, 63), 11), ((1, 2, 17, 65), 11), ((1, 1, 33, 129), 11), ((3, 1, 1, 1), 11), ((1, 1, 1, 200), 11),
                ((1, 1, 200, 1), 11), ((1, 1, 5, 7), 11)]
               + [(s, ws) for ws in (1, 3, 7, 9) for s in ((1, 2, 17, 65), (1, 1, 33, 129))]
               + [(s, ws) for ws in (13, 21, 31) for s in ((1, 2, 9, 33), (1, 1, 17, 65), (2, 1, 20, 70))])


@pytest.mark.parametrize("shape,ws", SSIM_SHAPES)
def test_ssim_every_tile(shape, ws):
    """The smallest shapes with pixels on both sides of every tile edge, every kernel (ssim11, 16x64 at ws 1..9, 8x32 from ws 13 on).
    Worst |err| / bound on MI355X: 0.071 at (1,2,17,65) ws 11 (error 6.9e-5 on a bound of 9.8e-4: the fp32 resolution of a sum near 1000)."""
    x, y = _pair(shape)
    _tile_compare(f"ssim tiles {shape} ws {ws}", x, y, ws, R.gaussian(ws), R.gaussian(ws))


@pytest.mark.parametrize("shape,ws", [((1, 2, 17, 65), 11), ((1, 1, 33, 129), 7), ((2, 1, 20, 70), 21)])
def test_ssim_asymmetric_window(shape, ws):
    """g[k] != g[ws-1-k]: a kernel that applies the window backwards in either pass, or swaps the passes' windows, differs from the
    restatement (cross-correlation in rows and columns, as F.conv2d) by far more than the bound. Worst |err| / bound on MI355X: 0.044;
    with g[ws-1-k] in the horizontal pass of ssim_tile_kernel: 15522 (ws 7) and 24730 (ws 21)."""
    x, y = _pair(shape)
    g = R.asymmetric_window(ws, 17 + ws)
    _tile_compare(f"ssim asymmetric {shape} ws {ws}", x, y, ws, g, g)


@pytest.mark.parametrize("shape,ws", [((1, 2, 17, 65), 11), ((2, 1, 20, 70), 21)])
def test_ssim_built_in_window(shape, ws):
    """window_host = NULL: the Gaussian built in C. TOL on the means, not bit equality: torch's sum() need not add in the C loop's order.
    Worst |err| / TOL on MI355X: 0.065."""
    x, y = _pair(shape)
    m64 = R.ssim_map(x, y, R.gaussian(ws))
    per, mean, _ = _ssim_raw(x, y, ws, None)
    err = max(float(np.abs(per - m64.mean(dim=(1, 2, 3)).numpy()).max()), abs(mean - float(m64.mean())))
    _report(f"ssim built-in window {shape} ws {ws}", err / TOL)
    assert err <= TOL


@pytest.mark.parametrize("kind", R.PROBE_KINDS)
@pytest.mark.parametrize("shape,ws", R.PROBE_CASES)
def test_ssim_strip_probes(shape, ws, kind):
    """y = x except on a strip or a pixel at a tile border (metrics_ref.ssim_probe): the tiles across the border receive their whole
    deficit pixels - sum through their halo (15 to 20 for a column strip under ws 11 and 7, against a bound near 1e-3), and the tiles
    no window reaches must sum to their pixel count within the bound (the map is exactly 1 there). Worst |err| / bound on MI355X: 0.084
    (cols, (1,1,17,65) ws 21); with the last halo column of ssim11_kernel read as zero: 92 (cols), 39 (rows), 16 and 11 (the two pixels)."""
    th, tw = R.tile_of(ws)
    r, (H, W) = ws // 2, shape[2:]
    x = op.synth_ssim_pair(91, *shape)[0]
    y, region = R.ssim_probe(x, kind, th, tw, r)
    d, d_ref, bound = _tile_compare(f"ssim probe {kind} {shape} ws {ws}", x, y, ws, R.gaussian(ws), R.gaussian(ws))
    assert (np.abs(d - d_ref) <= bound).all()
    reach = R.probe_reach(region, r, H, W, th, tw)
    assert (d_ref[0][~reach] == 0).all()
    assert (np.abs(d[0][~reach]) <= bound[0][~reach]).all(), f"tiles out of reach of the change: deficits {d[0][~reach]}"


def test_ssim_refuses_bad_arguments():
    lib, ctx = B.lib(), B.get_ctx()
    x = _in(np.zeros((1, 1, 8, 8), np.float32))
    per, mean, scratch = _fout(1), _fout(1), _words(64)
    good = dict(x=x.data_ptr(), y=x.data_ptr(), n=1, c=1, H=8, W=8, ws=11, win=None, per=per.data_ptr(), mean=mean.data_ptr(), scr=scratch.data_ptr())
    for change in (dict(x=None), dict(y=None), dict(scr=None), dict(ws=10), dict(ws=33), dict(ws=0), dict(n=0), dict(H=0), dict(scr=scratch.data_ptr() + 4)):
        assert _refused(lib.gi_ssim(ctx, *{**good, **change}.values())), change
    assert lib.gi_ssim_scratch_floats(1, 1, 8, 8, 10) == -1
    _sync()
    _kept_nan(per, 0, "refused ssim")
    _kept_nan(mean, 0, "refused ssim")
    _kept_fill(scratch, 0, "refused ssim")


# ---- reconstruction metrics -------------------------------------------------------------------------------------------------------

RECON_COUNTS = (1, 63, 256, 257, 2047, 2049, 12293, 2_200_003)
RECON_MASKS = ("binary", "ones", "zeros", "fractional", "uniform")     # fractional: {0, 0.5, 1}, whose products are exact; uniform: any float in [0, 1)
EPS = 1e-16


def _recon_blocks(count):
    return max(1, min(1024, -(-count // 2048)))


@functools.lru_cache(maxsize=4)
def _recon_inputs(count, mask, seed=0):
    rng = np.random.Generator(np.random.PCG64(8400 + seed))
    ground, gen = rng.random(count, dtype=np.float32), rng.random(count, dtype=np.float32)
    m = {"binary": lambda: (rng.random(count) < 0.3).astype(np.float32), "ones": lambda: np.ones(count, np.float32),
         "zeros": lambda: np.zeros(count, np.float32),
         "fractional": lambda: rng.choice(np.array([0, 0.5, 1], np.float32), size=count),
         "uniform": lambda: rng.random(count, dtype=np.float32)}[mask]()
    return ground, gen, m


def _recon_raw(ground, gen, m, want_out=True, acc=None, want_batch=True):
    """gi_eval_recon; returns (inpainted_out, batch_out, partial [blocks, 5] float64) as numpy (None where not asked for)."""
    lib, ctx = B.lib(), B.get_ctx()
    count = ground.size
    nb = _recon_blocks(count)
    assert int(lib.gi_eval_recon_scratch_floats(count)) == nb * 10
    out = _fout(count) if want_out else None
    batch = _fout(4) if want_batch else None
    scratch = _words(nb * 10)
    d_ground, d_gen, d_m = _in(ground), _in(gen), _in(m)
    _call(lib.gi_eval_recon(ctx, d_ground.data_ptr(), d_gen.data_ptr(), d_m.data_ptr(), count, EPS, B.ptr(out), B.ptr(acc), B.ptr(batch),
                            scratch.data_ptr()))
    _sync()
    what = f"eval_recon count {count}"
    if want_out:
        _kept_nan(out, count, what)
    if want_batch:
        _kept_nan(batch, 4, what)
    _kept_fill(scratch, nb * 10, what)
    partial = scratch[:nb * 10].cpu().numpy().view(np.float64).reshape(nb, 5)
    return (out[:count].cpu().numpy() if want_out else None), (batch[:4].cpu().numpy() if want_batch else None), partial


def _metrics_close(got, ref):
    nan_g, nan_r = np.isnan(got), np.isnan(ref)
    err = np.where(nan_r, 0.0, np.abs(got.astype(np.float64) - ref.astype(np.float64)) / (1e-6 * np.maximum(1.0, np.abs(ref))))
    return bool((nan_g == nan_r).all()), float(np.nan_to_num(err, nan=np.inf).max())


@pytest.mark.parametrize("mask", RECON_MASKS)
@pytest.mark.parametrize("count", RECON_COUNTS)
def test_recon_counts_and_masks(count, mask):
    """Below a wave, around a block, off the 2048-element step of the grid, past the 1024-block cap (2,200,003); binary, full, empty and
    fractional masks, the ABI taking the mask as given. Under the uniform mask gen * m is inexact, and a composite compiled to one fused
    multiply-add is an ulp off on many elements: eval_recon_partial_kernel was, until it got its fp contract(off); {0, 0.5, 1}
    cannot show that, its products are exact. The composite is the restatement's bit for bit, the count word exact, the five float64 sums within count x 2^-52 of
    the restatement's (the same fp32 terms added in another order), the metrics within 1e-6 x max(1, |ref|) with NaN for NaN.
    Worst metric error over its bound on MI355X: below 0.001."""
    ground, gen, m = _recon_inputs(count, mask)
    ref_out, ref_sums, ref_metrics = R.recon(ground, gen, m, EPS)
    out, batch, partial = _recon_raw(ground, gen, m)
    assert np.array_equal(out.view(np.int32), ref_out.view(np.int32)), f"{int((out.view(np.int32) != ref_out.view(np.int32)).sum())} of {count} composite words differ"
    assert partial[:, 4].sum() == np.count_nonzero(m) and (partial[:, 4] == np.round(partial[:, 4])).all()
    sums = partial.sum(0)
    assert (np.abs(sums - ref_sums) <= count * 2.0 ** -52 * np.abs(ref_sums)).all(), (sums, ref_sums)
    same_nan, ratio = _metrics_close(batch, ref_metrics)
    _report(f"recon count {count} {mask}", ratio)
    assert same_nan and ratio <= 1, (batch, ref_metrics)
    if mask == "zeros":
        assert np.isnan(batch[2]) and np.isnan(batch[3]) and batch[1] == 0 and abs(float(batch[0]) - 1e-8) <= 1e-14


def test_recon_accumulates_three_batches_in_call_order():
    acc = torch.cat([torch.zeros(5), torch.full((GUARD,), NAN)]).cuda()
    batches = []
    for i, (count, mask) in enumerate(((2049, "binary"), (257, "fractional"), (12293, "binary"))):
        ground, gen, m = _recon_inputs(count, mask, seed=i + 1)
        batches.append(_recon_raw(ground, gen, m, want_out=False, acc=acc)[1])
    _sync()
    got = acc.cpu().numpy()
    assert np.isnan(got[5:]).all() and got[4] == 3
    want = (batches[0] + batches[1]) + batches[2]                      # fp32, in call order
    assert want.dtype == np.float32 and np.array_equal(got[:4].view(np.int32), want.view(np.int32)), (got[:4], want)


def test_recon_null_outputs_leave_the_others_unchanged():
    ground, gen, m = _recon_inputs(2049, "binary")

    def run(want_out, want_acc, want_batch):
        acc = torch.cat([torch.zeros(5), torch.full((GUARD,), NAN)]).cuda() if want_acc else None
        out, batch, partial = _recon_raw(ground, gen, m, want_out=want_out, acc=acc, want_batch=want_batch)
        return out, (acc.cpu().numpy() if want_acc else None), batch, partial

    full = run(True, True, True)
    assert np.isnan(full[1][5:]).all() and full[1][4] == 1 and np.array_equal(full[1][:4].view(np.int32), full[2].view(np.int32))
    for flags in ((False, True, True), (True, False, True), (True, True, False), (False, False, False)):
        got = run(*flags)
        for a, b, asked in zip(got, full, flags + (True,)):
            assert (a is None) if not asked else np.array_equal(a.view(np.int32), b.view(np.int32)), flags


def test_recon_refuses_bad_arguments():
    lib, ctx = B.lib(), B.get_ctx()
    x = _in(np.zeros(64, np.float32))
    out, acc, batch, scratch = _fout(64), _fout(5), _fout(4), _words(16)
    good = dict(ground=x.data_ptr(), gen=x.data_ptr(), m=x.data_ptr(), count=64, eps=EPS, out=out.data_ptr(), acc=acc.data_ptr(), batch=batch.data_ptr(),
                scr=scratch.data_ptr())
    for change in (dict(ground=None), dict(gen=None), dict(m=None), dict(scr=None), dict(count=0), dict(count=-5), dict(scr=scratch.data_ptr() + 4)):
        assert _refused(lib.gi_eval_recon(ctx, *{**good, **change}.values())), change
    assert b"eval_recon" in lib.gi_last_error() and lib.gi_eval_recon_scratch_floats(0) == -1
    _sync()
    for buf in (out, acc, batch):
        _kept_nan(buf, 0, "refused eval_recon")
    _kept_fill(scratch, 0, "refused eval_recon")


# ---- segmentation metrics ---------------------------------------------------------------------------------------------------------

SEG_CASES = [(1, 1, 1, (0,)), (2, 2, 255, (1,)), (3, 4, 257, (0, 1, 2, 3)), (2, 19, 1025, (0, 3, 7, 12, 18)),
             (2, 19, 70_001, (0, 1, 2, 3, 17, 18, 5, 9, 11)),            # past the 64-block cap
             (1, 16, 300, tuple(range(16))),
             (2, 8, 513, (0, 1, 2, 3, 4, 5, 9, 7))]                      # 9 >= K; 5 is neither a label nor ever the argmax
SEG_FLAVOURS = ("plain", "minus_one", "nonfinite", "ties")


@functools.lru_cache(maxsize=2)
def _seg_data(n, K, hw, flavour):
    rng = np.random.Generator(np.random.PCG64(7000 + n + 31 * K + hw))
    labels = np.repeat(rng.integers(0, K, size=(n, hw // 8 + 1)), 8, 1)[:, :hw].astype(np.int64)
    logits = rng.standard_normal((n, K, hw)).astype(np.float32)
    logits += 1.5 * (labels[:, None] == np.arange(K)[None, :, None])
    if K == 8:                                                          # class 5: never a label, never the maximum
        labels[labels == 5] = 0
        logits[:, 5] = -10
    if flavour == "minus_one":
        labels[:, ::3] = -1
    if flavour == "nonfinite":
        for value, seed in ((NAN, 1), (np.inf, 2), (-np.inf, 3)):
            logits[np.random.Generator(np.random.PCG64(seed)).random(logits.shape) < 0.08] = value
        if K >= 4:                                                      # the rows of test_argmax_rule_is_torch_s, where the first NaN decides
            logits[0, :4, 0], logits[0, :4, -1] = (1, NAN, NAN, 5), (NAN, 1, 2, 3)
            logits[0, 4:, 0], logits[0, 4:, -1] = -1, -1
    if flavour == "ties":
        logits = np.round(logits).astype(np.float32)                   # integers in about [-3, 5]: the maximum is shared on most pixels
    if K == 8:
        logits[:, 5] = -10
    return labels, logits


def _seg_raw(labels, logits, uniq):
    lib, ctx = B.lib(), B.get_ctx()
    (n, K, hw), nu = logits.shape, len(uniq)
    nuc = 4 if nu <= 4 else (8 if nu <= 8 else 16)
    per, across, counts = _fout(nu * 3), _fout(3), _words(n * nuc * 3)
    hu = (C.c_int * nu)(*uniq)
    d_labels, d_logits = _in(labels), _in(logits)
    _call(lib.gi_seg_metrics(ctx, d_labels.data_ptr(), d_logits.data_ptr(), n, K, hw, C.cast(hu, C.c_void_p), nu, per.data_ptr(), across.data_ptr(),
                             counts.data_ptr()))
    _sync()
    what = f"seg_metrics n {n} K {K} hw {hw} nu {nu}"
    _kept_nan(per, nu * 3, what)
    _kept_nan(across, 3, what)
    _kept_fill(counts, n * nuc * 3, what)
    c = counts[:n * nuc * 3].cpu().numpy().reshape(n, nuc, 3)
    return c[:, :nu].astype(np.int64), per[:nu * 3].cpu().numpy().reshape(nu, 3), across[:3].cpu().numpy()


@pytest.mark.parametrize("flavour", SEG_FLAVOURS)
@pytest.mark.parametrize("n,K,hw,uniq", SEG_CASES)
def test_seg_counts_exactly(n, K, hw, uniq, flavour):
    """The integer counts (|p & g|, |p|, |g|) left in scratch_counts equal the restatement's exactly: nu on both sides of the 4 / 8 / 16
    template widths, hw below a block, off the 256 multiple and past the 64-block cap, K = 1, a class >= K, a class that never occurs;
    labels of -1, NaN and +-inf logits where the first NaN decides, and integer logits with a shared maximum on most pixels."""
    labels, logits = _seg_data(n, K, hw, flavour)
    ref = R.seg_counts(labels, logits, uniq)
    ref_per, ref_across = R.seg_ratios(ref)
    counts, per, across = _seg_raw(labels, logits, uniq)
    assert np.array_equal(counts, ref), f"{int((counts != ref).sum())} of {ref.size} counts differ: first {counts.reshape(-1, 3)[:4].tolist()} vs {ref.reshape(-1, 3)[:4].tolist()}"
    err = max(float(np.abs(per.astype(np.float64) - ref_per).max()), float(np.abs(across.astype(np.float64) - ref_across).max()))
    _report(f"seg n {n} K {K} hw {hw} nu {len(uniq)} {flavour}", err / 2e-7)
    assert err <= 2e-7
    if flavour == "nonfinite" and K >= 4:
        assert torch.argmax(torch.from_numpy(logits[0, :, 0])) == 1 and torch.argmax(torch.from_numpy(logits[0, :, -1])) == 0
    if K == 8:          # uniq[5] = 5 never occurs, uniq[6] = 9 >= K is never predicted: only a label of -1 counts for them
        assert ref[:, 5:7, :2].sum() == 0 and (per[5:7] == 0).all() and (flavour == "minus_one" or ref[:, 5:7].sum() == 0)


def test_seg_refuses_bad_arguments():
    lib, ctx = B.lib(), B.get_ctx()
    labels, logits = _in(np.zeros(64, np.int64)), _in(np.zeros(4 * 64, np.float32))
    per, across, counts = _fout(48), _fout(3), _words(48)
    hu = (C.c_int * 17)(*range(17))
    good = dict(labels=labels.data_ptr(), logits=logits.data_ptr(), n=1, K=4, hw=64, uniq=C.cast(hu, C.c_void_p), nu=4, per=per.data_ptr(),
                across=across.data_ptr(), counts=counts.data_ptr())
    for change in (dict(nu=0), dict(nu=17), dict(n=0), dict(K=0), dict(hw=0), dict(labels=None), dict(counts=None), dict(uniq=None)):
        assert _refused(lib.gi_seg_metrics(ctx, *{**good, **change}.values())), change
    assert b"seg_metrics" in lib.gi_last_error()
    _sync()
    _kept_nan(per, 0, "refused seg_metrics")
    _kept_nan(across, 0, "refused seg_metrics")
    _kept_fill(counts, 0, "refused seg_metrics")


# ---- total variation --------------------------------------------------------------------------------------------------------------

TV_SHAPES = [(1, 2, 2), (3, 2, 9), (3, 9, 2), (2, 5, 7), (4, 33, 65), (1, 1100, 2001)]     # the last: past the 1024-block cap


def _loss_blocks(count):
    return max(1, min(1024, -(-count // 2048)))


def _tv_raw(x, weight, gscale, want_grad=True):
    lib, ctx = B.lib(), B.get_ctx()
    planes, H, W = x.shape
    nb = _loss_blocks(x.size)
    loss, grad, scratch = _fout(1), (_fout(x.size) if want_grad else None), _words(nb * 4)
    dx = _in(x, PAD + W + W % 2)          # a row of NaN on either side: a neighbour taken across the image's end reads NaN, not foreign memory
    _call(lib.gi_loss_tv(ctx, dx.data_ptr(), planes, H, W, weight, loss.data_ptr(), B.ptr(grad), gscale, scratch.data_ptr()))
    _sync()
    what = f"loss_tv {x.shape}"
    _kept_nan(loss, 1, what)
    _kept_fill(scratch, nb * 4, what)
    if want_grad:
        _kept_nan(grad, x.size, what)
    return loss[:1].cpu().numpy(), (grad[:x.size].cpu().numpy().reshape(x.shape) if want_grad else None)


@pytest.mark.parametrize("planes,H,W", TV_SHAPES)
def test_tv_loss_and_whole_gradient(planes, H, W):
    """Non-square shapes (H and W exchanged in an index line shows on every row), several planes (the reference gradient has no term across
    a plane boundary), tv_weight and gscale != 1: the loss within 1e-6 ref + 1e-7 and EVERY gradient element within 1e-6 max|ref grad|.
    Worst |err| / bound on MI355X: 0.100 (1x1100x2001)."""
    x = np.random.Generator(np.random.PCG64(planes + H + W)).random((planes, H, W), dtype=np.float32)
    worst = 0.0
    for weight in (1.0, 0.1):
        ref_loss, ref_grad = R.tv(x, weight)
        for gscale in (1.0, 1024.0):
            loss, grad = _tv_raw(x, weight, gscale)
            e_loss = abs(float(loss[0]) - ref_loss) / (1e-6 * ref_loss + 1e-7)
            e_grad = float(np.abs(grad - gscale * ref_grad).max()) / (1e-6 * gscale * float(np.abs(ref_grad).max()))
            worst = max(worst, e_loss, e_grad)
            assert e_loss <= 1, f"weight {weight}: loss {float(loss[0])!r} vs {ref_loss!r}"
            where = np.unravel_index(int(np.abs(grad - gscale * ref_grad).argmax()), grad.shape)
            assert e_grad <= 1, f"weight {weight} gscale {gscale}: gradient at {where} is {grad[where]!r}, float64 {gscale * ref_grad[where]!r}"
        alone, _ = _tv_raw(x, weight, 1.0, want_grad=False)
        assert alone.view(np.int32)[0] == loss.view(np.int32)[0], "grad = NULL changed the loss"
    _report(f"tv {planes}x{H}x{W}", worst)


def test_tv_refuses_a_single_row_or_column():
    lib, ctx = B.lib(), B.get_ctx()
    x = _in(np.zeros(64, np.float32))
    loss, grad, scratch = _fout(1), _fout(64), _words(8)
    for planes, H, W in ((1, 1, 64), (1, 64, 1), (0, 8, 8), (2, 1, 1)):
        assert _refused(lib.gi_loss_tv(ctx, x.data_ptr(), planes, H, W, 1.0, loss.data_ptr(), grad.data_ptr(), 1.0, scratch.data_ptr())), (planes, H, W)
    assert b"loss_tv" in lib.gi_last_error()
    assert _refused(lib.gi_loss_tv(ctx, x.data_ptr(), 1, 8, 8, 1.0, loss.data_ptr(), grad.data_ptr(), 1.0, scratch.data_ptr() + 4))
    _sync()
    _kept_nan(loss, 0, "refused loss_tv")
    _kept_nan(grad, 0, "refused loss_tv")
    _kept_fill(scratch, 0, "refused loss_tv")


# ---- cross entropy ----------------------------------------------------------------------------------------------------------------

CE_SHAPES = [(2, 3, 257), (3, 3, 257), (4, 3, 257), (8, 3, 257), (16, 3, 257), (2, 1, 1), (2, 2, 1_100_003)]     # (K, n, hw)
FACE_WEIGHT = (0, 1.2, 0.7, 0.7)


def _ce_raw(z, y, weight, ignore, gscale, want_grad=True):
    lib, ctx = B.lib(), B.get_ctx()
    n, K, hw = z.shape
    nb = _loss_blocks(n * hw)
    loss, grad, scratch = _fout(2), (_fout(z.size) if want_grad else None), _words(nb * 4)
    dz, dy = _in(z), _in(y)
    _call(lib.gi_loss_cross_entropy(ctx, dz.data_ptr(), dy.data_ptr(), n, K, hw, _floats(weight) if weight is not None else None, ignore,
                                    loss.data_ptr(), B.ptr(grad), gscale, scratch.data_ptr()))
    _sync()
    what = f"cross_entropy K {K} n {n} hw {hw}"
    _kept_nan(loss, 2, what)
    _kept_fill(scratch, nb * 4, what)
    if want_grad:
        _kept_nan(grad, z.size, what)
    return loss[:2].cpu().numpy(), (grad[:z.size].cpu().numpy().reshape(z.shape) if want_grad else None)


def _ce_weights(K):
    w = 0.25 + np.random.Generator(np.random.PCG64(50 + K)).random(K)
    w[K // 2] = 0
    return tuple(float(np.float32(v)) for v in w)


def _ce_labels(rng, n, K, hw, ignore):
    y = rng.integers(0, K, size=(n, hw)).astype(np.int64)
    if hw > 16:
        y[:, 3::11], y[:, 5::13], y[0, 7::17], y[-1, 2::19], y[0, 1::23] = ignore, K, K + 3, -1, -7          # ignored, >= K, < 0
    return y


def _ce_compare(what, z, y, weight, ignore, gscale):
    """Loss, weight sum and the whole gradient against float64; the bounds are the file's floors (2e-6 ref; 2e-6 max|ref grad| + 1e-10) or,
    where larger, 8 x what torch's own fp32 F.cross_entropy deviates from float64 on the same input. Returns the worst ratio."""
    ref_loss, ref_grad, ref_wsum = R.ce(z, y, weight, ignore)
    f32_loss, f32_grad, _ = R.ce(z, y, weight, ignore, torch.float32)
    loss, grad = _ce_raw(z, y, weight, ignore, gscale)
    assert abs(float(loss[1]) - ref_wsum) <= 1e-6 * ref_wsum, f"{what}: weight sum {float(loss[1])!r} vs {ref_wsum!r}"
    nan_l, nan_g = np.isnan(ref_loss), np.isnan(ref_grad)
    assert np.isnan(loss[0]) == nan_l and np.array_equal(np.isnan(grad), nan_g), f"{what}: NaN where float64 torch has none, or the reverse"
    if nan_l:
        assert (grad[~nan_g] == 0).all()
        return 0.0
    dev_loss, dev_grad = abs(f32_loss - ref_loss), float(np.abs(f32_grad - ref_grad).max())
    b_loss = max(2e-6 * abs(ref_loss), 8 * dev_loss)
    b_grad = gscale * max(2e-6 * float(np.abs(ref_grad).max()) + 1e-10, 8 * dev_grad)
    e_loss, e_grad = abs(float(loss[0]) - ref_loss), float(np.abs(grad - gscale * ref_grad).max())
    ratio = max(e_loss / b_loss, e_grad / b_grad)
    _report(what, ratio, loss_floor=2e-6 * abs(ref_loss), loss_fp32_dev=dev_loss, grad_floor=2e-6 * float(np.abs(ref_grad).max()) + 1e-10,
            grad_fp32_dev=dev_grad, loss_err=e_loss, grad_err=e_grad / gscale)
    assert e_loss <= b_loss, f"{what}: loss {float(loss[0])!r} vs {ref_loss!r} (bound {b_loss:.3e})"
    where = np.unravel_index(int(np.abs(grad - gscale * ref_grad).argmax()), grad.shape)
    assert e_grad <= b_grad, f"{what}: gradient at {where} is {grad[where]!r}, float64 {gscale * ref_grad[where]!r} (bound {b_grad:.3e})"
    return ratio


@pytest.mark.parametrize("K,n,hw", CE_SHAPES)
def test_cross_entropy_loss_and_whole_gradient(K, n, hw):
    """Every instantiated K, a single pixel, and 2,200,006 pixels (past the 1024-block cap); no weights, random positive weights with one
    zero and, at K = 4, the face-parsing weights; ignore_index -100 and 255; gscale 1 and 1024 (the trainer passes the fp16 loss scale);
    labels equal to ignore_index, >= K and < 0 among them. On MI355X the worst |err| / bound is 0.122 (K 16); torch's own fp32 deviates
    from float64 by at most 7.2e-7 on the loss (floors 2.6e-6 to 8.9e-6, so the floor decides) and by 3e-10 to 1.1e-9 on the gradient, where
    8 x that passes the floor of 6.3e-9 to 6.8e-9 for K = 2 only."""
    rng = np.random.Generator(np.random.PCG64(60 + K + hw))
    z = (2 * rng.standard_normal((n, K, hw))).astype(np.float32)
    rnd = _ce_weights(K)
    combos = [(None, -100, 1.0), (rnd, 255, 1024.0)] if hw > 100_000 else [(None, -100, 1.0), (None, 255, 1024.0), (rnd, -100, 1024.0), (rnd, 255, 1.0)]
    if K == 4:
        combos += [(FACE_WEIGHT, -100, 1.0), (FACE_WEIGHT, 255, 1024.0)]
    for weight, ignore, gscale in combos:
        y = _ce_labels(rng, n, K, hw, ignore)
        if hw == 1:      # the one pixel carries its less likely class: the loss is of the logits' size, not a small difference of two of them
            z[0, :, 0], y[:] = (-1.5, 0.75), 0
        _ce_compare(f"ce K {K} n {n} hw {hw} w {'none' if weight is None else 'face' if weight == FACE_WEIGHT else 'random'} ignore {ignore} gscale {gscale:g}",
                    z, y, weight, ignore, gscale)


@pytest.mark.parametrize("K", [2, 3, 4, 8, 16])
def test_cross_entropy_large_logits(K):
    """Logits uniform in +-90: exp(90) overflows fp32, so loss and gradient are finite only because the maximum is subtracted first.
    On MI355X the worst |err| / bound is 0.068; torch's fp32 loss deviates by 2.5e-6 to 1.2e-5 from float64 on losses of 30 to 80 (floors
    6.1e-5 to 1.6e-4 decide). Without the subtraction in ce_grad_kernel every case has NaN gradients."""
    rng = np.random.Generator(np.random.PCG64(70 + K))
    z = rng.uniform(-90, 90, size=(3, K, 257)).astype(np.float32)
    y = _ce_labels(rng, 3, K, 257, -100)
    assert float(z.max()) > 89 and np.exp(89.0) > np.finfo(np.float32).max
    _ce_compare(f"ce large logits K {K}", z, y, _ce_weights(K), -100, 1024.0)


@pytest.mark.parametrize("K", [2, 4, 16])
def test_cross_entropy_nothing_counts(K):
    """An all-ignored batch (ignore_index, labels >= K and < 0): loss NaN, weight sum 0, gradient all zero. And a batch whose only valid
    labels carry weight 0: whatever float64 torch yields, NaN for NaN."""
    rng = np.random.Generator(np.random.PCG64(80 + K))
    z = rng.standard_normal((2, K, 300)).astype(np.float32)
    y = rng.choice(np.array([-100, K, K + 5, -1]), size=(2, 300)).astype(np.int64)
    loss, grad = _ce_raw(z, y, None, -100, 1024.0)
    assert np.isnan(loss[0]) and loss[1] == 0 and (grad == 0).all() and not np.signbit(grad).any()
    w = _ce_weights(K)
    y2 = np.where(rng.random((2, 300)) < 0.5, K // 2, -100).astype(np.int64)          # the class of weight 0, or ignored
    _ce_compare(f"ce only weight-0 labels K {K}", z, y2, w, -100, 1.0)


def test_cross_entropy_refuses_an_unbuilt_class_count():
    lib, ctx = B.lib(), B.get_ctx()
    z, y = _in(np.zeros(5 * 64, np.float32)), _in(np.zeros(64, np.int64))
    loss, grad, scratch = _fout(2), _fout(5 * 64), _words(8)
    for K in (5, 1, 17, 0):
        assert _refused(lib.gi_loss_cross_entropy(ctx, z.data_ptr(), y.data_ptr(), 1, K, 64, None, -100, loss.data_ptr(), grad.data_ptr(), 1.0, scratch.data_ptr())), K
        assert b"num_classes" in lib.gi_last_error()
    assert _refused(lib.gi_loss_cross_entropy(ctx, z.data_ptr(), y.data_ptr(), 1, 4, 64, None, -100, loss.data_ptr(), grad.data_ptr(), 1.0, scratch.data_ptr() + 4))
    assert _refused(lib.gi_loss_cross_entropy(ctx, z.data_ptr(), y.data_ptr(), 0, 4, 64, None, -100, loss.data_ptr(), grad.data_ptr(), 1.0, scratch.data_ptr()))
    _sync()
    _kept_nan(loss, 0, "refused cross_entropy")
    _kept_nan(grad, 0, "refused cross_entropy")
    _kept_fill(scratch, 0, "refused cross_entropy")
