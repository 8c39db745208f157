"""GPU tier: every kernel of the FID path (csrc/inception.hip) against a high-precision reference of that same step on the very input
the device gave it, read back through the debug seam (gi_inception_debug_forward_steps / gi_inception_debug_read), with the
tolerances derived in tests/inception_ref.py (step_reference, input_reference, gap_reference): no yardstick, no accumulation over
layers. Then the concatenations, the input geometries the C-ABI promises, the production batch of 50 (grid-stride loops past their
first iteration, the workspace used to its end) and the streaming statistics away from d = 2048. The CPU tier
(tests/test_fid_layers_cpu.py) shows that the tolerances are satisfiable and that they bite. Reads fixtures only.
Measured ratios: DESIGN.md section 4.4 and profiles/fid_layers_parity.json."""
import numpy as np
import pytest
import torch

import inception_ref as R
from test_fid_gpu import _record
from util_golden import load

pytestmark = pytest.mark.gpu

SEED, IMAGES = 4242, (77, 2, 1, 128)
GEOMETRIES = [(64, 64), (128, 128), (299, 299), (512, 512), (200, 360), (360, 200), (1, 1), (2, 3), (300, 298)]
DTYPES = ["fp32", "fp16"]


def _inception():
    import gan_inpainting_amd  # noqa: F401
    from gan_inpainting_amd.lib.fid import inception
    return inception


def _model(P, dt, max_batch):
    m = _inception().InceptionV3([3], dtype=dt, max_batch=max_batch)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in P.items()})
    return m.cuda()


@pytest.fixture(scope="module")
def exact():
    P = R.make_params_exact_fold(SEED)
    return dict(T64=R.to_torch(P, torch.float64), models={dt: _model(P, dt, 4) for dt in DTYPES})


@pytest.fixture(scope="module")
def generic_params():
    return R.make_params(int(load("fid_inception")["param_seed"]))


def _kind(step):
    s = R.STEPS[step]
    return s["kind"] if s["kind"] != "conv" else "pointwise" if R.CONV_BY_NAME[s["name"]][3] == (1, 1) else "taps"


def _run_step(m, x, step):
    m.debug_forward_steps(x, step + 1)
    return m.debug_read(step, 0).cpu(), m.debug_read(step, 1).cpu()


def _check_steps(m, T64, x, steps, dt):
    """[(step, record)] and the failure lines of the given steps on input x."""
    recs, bad = [], []
    for step in steps:
        a, out = _run_step(m, x, step)
        s = R.STEPS[step]
        assert tuple(a.shape[1:]) == s["in_chw"] and tuple(out.shape[1:]) == s["out_chw"]
        with torch.no_grad():
            ref, tol = R.step_reference(step, a, T64, dt)
        ratio, (img, ch, y, xx) = R.worst_ratio(out, ref, tol)
        exact_kind = s["kind"].startswith("max")
        ok = bool(torch.isfinite(out).all()) and (torch.equal(out.double(), ref) if exact_kind else ratio <= 1.0)
        recs.append(dict(step=step, layer=R.step_label(step), kind=_kind(step), error_over_tol=ratio, max_ref=float(ref.abs().max())))
        if not ok:
            bad.append(f"step {step} ({R.step_label(step)}, {_kind(step)}): worst at image {img} channel {ch} y {y} x {xx}: got "
                       f"{float(out[img, ch, y, xx])!r}, reference {float(ref[img, ch, y, xx])!r}, error / tol {ratio:.4g}")
    return recs, bad


def _worst_by_kind(recs):
    w = {}
    for r in recs:
        w[r["kind"]] = max(w.get(r["kind"], 0.0), r["error_over_tol"])
    return w


@pytest.mark.parametrize("dt", DTYPES)
def test_every_step_matches_its_own_reference(exact, dt):
    m, T64 = exact["models"][dt], exact["T64"]
    x = torch.from_numpy(R.make_images(*IMAGES)).cuda()
    recs, bad = _check_steps(m, T64, x, range(len(R.STEPS)), dt)
    # the global average: the last step's whole destination rows against the features of the production call
    last = len(R.STEPS) - 1
    m.debug_forward_steps(x, last + 1)
    rows = m.debug_read(last, 2).cpu()
    feats = m.features(x).cpu()
    ref, tol = R.gap_reference(rows)
    g, (img, ch) = R.worst_ratio(feats, ref, tol)
    if not (g <= 1.0 and bool(torch.isfinite(feats).all())):
        bad.append(f"global average: worst at image {img} feature {ch}: got {float(feats[img, ch])!r}, reference {float(ref[img, ch])!r}, error / tol {g:.4g}")
    assert float((feats > 0).double().mean()) > 0.5
    worst = _worst_by_kind(recs)
    worst["global_average"] = g
    print(f"steps {dt}: worst error / tol per kind {worst}")
    _record(f"layers_steps_{dt}", dict(worst_by_kind=worst, steps=recs, global_average=g))
    assert not bad, f"{len(bad)} of 108 checks fail ({dt}):\n" + "\n".join(bad)


@pytest.mark.parametrize("dt", DTYPES)
def test_concatenations_keep_every_branch(exact, dt):
    m = exact["models"][dt]
    x = torch.from_numpy(R.make_images(*IMAGES)).cuda()
    bw = R.block_writers()
    assert len(bw) == 11
    for block, writers in bw.items():
        views = {}
        for step in writers:
            m.debug_forward_steps(x, step + 1)
            views[step] = m.debug_read(step, 1)
        rows = m.debug_read(writers[-1], 2)
        s = R.STEPS[writers[-1]]
        assert tuple(rows.shape[1:]) == (s["ldout"],) + s["out_chw"][1:]
        covered = 0
        for step in writers:
            t = R.STEPS[step]
            got = rows[:, t["coffout"]:t["coffout"] + t["out_chw"][0]]
            assert torch.equal(got, views[step]), f"{block}: the channels of step {step} ({R.step_label(step)}) changed after it was written"
            assert float(views[step].abs().max()) > 0
            covered += t["out_chw"][0]
        assert covered == s["ldout"]
    _record(f"layers_concatenations_{dt}", dict(blocks=len(bw), bit_equal=True))


@pytest.mark.parametrize("dt", DTYPES)
def test_stem_with_three_channels_and_three_images(exact, dt):
    """c = 3: the first convolution sees three distinct channels; n = 3: the 64-row M tiles straddle the image boundaries elsewhere."""
    m, T64 = exact["models"][dt], exact["T64"]
    x = torch.from_numpy(R.make_images(78, 3, 3, 128)).cuda()
    recs, bad = _check_steps(m, T64, x, range(7), dt)
    a, _ = _run_step(m, x, 0)
    assert not torch.equal(a[:, 0], a[:, 1]) and not torch.equal(a[:, 1], a[:, 2])
    print(f"stem c=3 n=3 {dt}: worst error / tol per kind {_worst_by_kind(recs)}")
    _record(f"layers_stem_c3_n3_{dt}", dict(worst_by_kind=_worst_by_kind(recs), steps=recs))
    assert not bad, "\n".join(bad)


def _geometry_images(h, w, c, seed):
    """Image 0: uniform noise (the largest neighbour differences), image 1: a smooth picture (the smallest tolerance)."""
    rng = np.random.Generator(np.random.PCG64(seed))
    noise = rng.random((1, c, h, w), dtype=np.float32)
    smooth = R.make_images(seed + 1, 1, c, max(h, w, 2))[:, :, :h, :w]
    return torch.from_numpy(np.ascontiguousarray(np.concatenate([noise, smooth])))


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("c", [1, 3])
@pytest.mark.parametrize("hw", GEOMETRIES, ids=[f"{h}x{w}" for h, w in GEOMETRIES])
def test_input_kernel_geometry(exact, hw, c, dt):
    m = exact["models"][dt]
    x = _geometry_images(hw[0], hw[1], c, 500 + 3 * hw[0] + hw[1] + c)
    m.debug_forward_steps(x.cuda(), 1)
    got = m.debug_read(0, 0).cpu()
    assert tuple(got.shape) == (2, 8, 299, 299)
    assert bool((got[:, 3:] == 0).all()), "the padding channels 3..7 of the resized input are not exactly 0"
    if c == 1:
        assert torch.equal(got[:, 0], got[:, 1]) and torch.equal(got[:, 0], got[:, 2])
    ref, tol = R.input_reference(x, dt)
    ratio, (img, ch, y, xx) = R.worst_ratio(got[:, :3], ref, tol)
    print(f"input {hw} c={c} {dt}: error / tol {ratio:.3f}")
    _record(f"layers_input_{hw[0]}x{hw[1]}_c{c}_{dt}", dict(error_over_tol=ratio))
    assert bool(torch.isfinite(got).all())
    assert ratio <= 1.0, (f"input kernel {hw} c={c} {dt}: worst at image {img} channel {ch} y {y} x {xx}: got {float(got[img, ch, y, xx])!r}, "
                          f"reference {float(ref[img, ch, y, xx])!r}, error / tol {ratio:.4g}")
    if hw == (299, 299) and dt == "fp32":
        x3 = x.expand(-1, 3, -1, -1) if c == 1 else x
        assert torch.equal(got[:, :3], 2 * x3 - 1), "at 299x299 the resize is the identity: 2 x - 1 in fp32, bit for bit"


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("hw", [(512, 512), (200, 360)], ids=["512x512", "200x360"])
def test_features_at_the_untested_geometries(generic_params, hw, dt):
    """Downsampling (config 5 trains at 512x512) and a non-square input through the whole network with the fixture's generic
    parameters, against the fp64 restatement; yardsticks as the fixture's: (a) the restatement in fp32, (b) with round_fp16."""
    h, w = hw
    x = torch.from_numpy(np.ascontiguousarray(R.make_images(91 + h, 2, 1, max(h, w))[:, :, :h, :w]))
    with torch.no_grad():
        f64 = R.forward(R.to_torch(generic_params, torch.float64), x.double())
        T32 = R.to_torch(generic_params, torch.float32)
        yard = float((R.forward(T32, x).double() - f64).abs().max()) if dt == "fp32" else \
            float((R.forward(T32, x, round_fn=R.round_fp16).double() - f64).abs().max())
    bound = (8.0 if dt == "fp32" else 4.0) * yard
    got = _model(generic_params, dt, 2).features(x.cuda()).double().cpu()
    err = float((got - f64).abs().max())
    print(f"features {h}x{w} {dt}: max|err| {err:.3e}, bound {bound:.3e}, ratio to yardstick {err / yard:.3f}, max|ref| {float(f64.abs().max()):.3f}")
    _record(f"layers_features_{h}x{w}_{dt}", dict(max_err=err, bound=bound, ratio_to_yardstick=err / yard))
    assert bool(torch.isfinite(got).all())
    assert err <= bound


def _sliced(m, x, k):
    return torch.cat([m.features(x[i:i + k]) for i in range(0, x.shape[0], k)])


@pytest.mark.parametrize("dt,case", [("fp32", "g128"), ("fp16", "g128"), ("fp16", "g256")])
def test_production_batch(generic_params, dt, case):
    """max_batch = 50, the default and the FID batch: the pools', the input kernel's and the average's grid-stride loops run past
    their first iteration and the activations fill the workspace up to the packed weights behind them."""
    fx = load("fid_inception")
    n, c, hw, _ = (int(v) for v in fx[f"{case}_shape"])
    g = R.make_images(int(fx[f"{case}_seed"]), n, c, hw)
    x = torch.from_numpy(np.concatenate([g, R.make_images(33, 50 - 2 * n, c, hw), g])).cuda()
    assert x.shape[0] == 50
    big, small = _model(generic_params, dt, 50), _model(generic_params, dt, 4)
    assert big.max_batch == 50 == _inception().InceptionV3().max_batch
    first4 = big.features(x[:4]).clone()                      # before any full batch
    f50 = big.features(x)
    by4, by1 = _sliced(small, x, 4), _sliced(small, x, 1)
    assert torch.equal(f50, by4), f"batch 50 differs from slices of 4 in rows {sorted(set((f50 != by4).nonzero()[:, 0].tolist()))}"
    assert torch.equal(f50, by1), f"batch 50 differs from slices of 1 in rows {sorted(set((f50 != by1).nonzero()[:, 0].tolist()))}"
    # the fixture rows, first and last, against the reference (the bound of tests/test_fid_gpu.py)
    ref = fx[f"{case}_features"]
    bound = 8.0 * float(fx[f"{case}_yardstick_a"]) if dt == "fp32" else 4.0 * float(fx[f"{case}_yardstick_b"])
    for rows in (f50[:n], f50[-n:]):
        assert float(np.abs(rows.double().cpu().numpy() - ref).max()) <= bound
    x53 = torch.cat([x, x[:3]])                               # the wrapper's 50 + 3 split
    f53 = big.features(x53)
    assert torch.equal(f53[:50], f50) and torch.equal(f53[50:], f50[:3])
    again = big.features(x[:4])                               # a write past the last image's rows would have hit the packed weights
    assert torch.equal(again, first4) and torch.equal(first4, f50[:4])
    _record(f"layers_batch50_{case}_{dt}", dict(bit_equal_to_slices_of_4=True, bit_equal_to_slices_of_1=True, split_50_3=True,
                                                first4_unchanged=True))


@pytest.mark.parametrize("n", [2, 37])
@pytest.mark.parametrize("d", [1, 5, 255, 257, 1030])
def test_streaming_statistics_at_other_widths(d, n):
    """The 4-row groups and 256-column blocks of fid_xtx_kernel with ragged ends."""
    import gan_inpainting_amd  # noqa: F401
    from gan_inpainting_amd.lib.fid import fid_score
    rng = np.random.Generator(np.random.PCG64(40 + d + n))
    x = (rng.standard_normal((n, d)) * rng.uniform(0.5, 2.0, d) + rng.uniform(-1, 1, d)).astype(np.float32)
    mu_ref = np.mean(x.astype(np.float64), axis=0)
    sig_ref = np.cov(x.astype(np.float64), rowvar=False).reshape(d, d)
    scale = float(np.abs(sig_ref).max())
    xd = torch.from_numpy(x).cuda()

    def run(chunks):
        st = fid_score.FidStats("cuda", d)
        i = 0
        for k in chunks:
            st.update(xd[i:i + k])
            i += k
        assert i == n
        return st.finish()
    results = [run(ch) for ch in ([[2], [1, 1]] if n == 2 else [[37], [5, 1, 17, 14], [1] * 36 + [1], [36, 1]])]
    for mu, s in results:
        assert mu.shape == (d,) and s.shape == (d, d)
        e_mu, e_s = float(np.abs(mu - mu_ref).max()), float(np.abs(s - sig_ref).max())
        assert e_mu <= 1e-10 * scale and e_s <= 1e-10 * scale, (d, n, e_mu, e_s, scale)
        assert np.array_equal(mu, results[0][0]) and np.array_equal(s, results[0][1])          # any chunking: the same bits
    _record(f"layers_statistics_d{d}_n{n}", dict(max_dmu=float(np.abs(results[0][0] - mu_ref).max()),
                                                 max_dsigma=float(np.abs(results[0][1] - sig_ref).max()), max_sigma=scale))
