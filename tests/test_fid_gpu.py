"""GPU tier: the FID path on the device against the fixtures recorded from the reference (tests/golden/make_golden_fid.py) and
tests/inception_ref.py. Reads fixtures only.

Feature bounds are not chosen here: fp32 may err at most 8x yardstick (a) (the reference module in fp32 on the CPU against its
fp64 self: same arithmetic, other summation order), fp16 at most 4x yardstick (b) (the restatement with weights and every
layer's output rounded to fp16: same rounding points; MFMA accumulation order and the BatchNorm fold differ), each yardstick
taken per fixture case. Measured ratios: DESIGN.md section 4.4 and profiles/r06_fid_parity.json.
"""
import json
import os
import pickle

import numpy as np
import pytest
import torch

import inception_ref as R
from util_golden import load

pytestmark = pytest.mark.gpu

CASES = ("g128", "c128", "g256", "c256")
PARITY_OUT = os.environ.get("GI_FID_PARITY_OUT", "")


def _fid():
    import gan_inpainting_amd  # noqa: F401
    from gan_inpainting_amd.lib.fid import fid_score, inception
    return inception, fid_score


@pytest.fixture(scope="module")
def params():
    fx = load("fid_inception")
    return R.make_params(int(fx["param_seed"]))


@pytest.fixture(scope="module")
def models(params):
    inception, _ = _fid()
    out = {}
    for dt in ("fp16", "fp32"):
        m = inception.InceptionV3([3], dtype=dt, max_batch=4)
        m.load_state_dict({k: torch.from_numpy(v) for k, v in params.items()})
        out[dt] = m.cuda()
    return out


def _record(key, value):
    if PARITY_OUT:
        d = json.load(open(PARITY_OUT)) if os.path.exists(PARITY_OUT) else {}
        d[key] = value
        json.dump(d, open(PARITY_OUT, "w"), indent=1, sort_keys=True)


def _bound(fx, case, dt):
    return 8.0 * float(fx[f"{case}_yardstick_a"]) if dt == "fp32" else 4.0 * float(fx[f"{case}_yardstick_b"])


@pytest.mark.parametrize("dt", ["fp32", "fp16"])
@pytest.mark.parametrize("case", CASES)
def test_features_match_the_reference(models, dt, case):
    fx = load("fid_inception")
    n, c, hw, _ = (int(v) for v in fx[f"{case}_shape"])
    x = torch.from_numpy(R.make_images(int(fx[f"{case}_seed"]), n, c, hw)).cuda()
    got = models[dt](x)[0]
    assert tuple(got.shape) == (n, 2048, 1, 1)
    got = got.reshape(n, 2048).double().cpu().numpy()
    ref = fx[f"{case}_features"]
    err, bound = float(np.abs(got - ref).max()), _bound(fx, case, dt)
    print(f"features {case} {dt}: max|err| {err:.3e}, yardstick bound {bound:.3e}, ratio to yardstick {err / (bound / (8 if dt == 'fp32' else 4)):.3f}, max|ref| {np.abs(ref).max():.3f}")
    _record(f"features_{case}_{dt}", dict(max_err=err, bound=bound, ratio_to_yardstick=err / (bound / (8 if dt == "fp32" else 4))))
    assert np.isfinite(got).all()
    assert err <= bound


@pytest.mark.parametrize("dt", ["fp32", "fp16"])
def test_features_do_not_depend_on_the_batch(models, dt):
    x = torch.from_numpy(R.make_images(21, 4, 1, 128)).cuda()
    m = models[dt]
    all4 = m.features(x)
    single = torch.cat([m.features(x[i:i + 1]) for i in range(4)])
    rev = m.features(x.flip(0)).flip(0)
    assert torch.equal(all4, single) and torch.equal(all4, rev)
    big = torch.cat([x, x.flip(0)])                      # 8 > max_batch: sliced by the wrapper
    assert torch.equal(m.features(big)[:4], all4)


def test_device_statistics_match_numpy_and_are_reproducible():
    _, fid_score = _fid()
    fx = load("fid_frechet")
    x = fx["stat_x"]
    mu_ref = np.mean(x.astype(np.float64), axis=0)
    sig_ref = np.cov(x.astype(np.float64), rowvar=False)
    assert np.array_equal(mu_ref, fx["stat_mu"]) or np.abs(mu_ref - fx["stat_mu"]).max() < 1e-14
    assert np.abs(sig_ref[:8] - fx["stat_sigma_rows"]).max() < 1e-13
    scale = float(fx["stat_sigma_max"])
    xd = torch.from_numpy(x).cuda()

    def run(chunks):
        st = fid_score.FidStats("cuda", 2048)
        i = 0
        for k in chunks:
            st.update(xd[i:i + k])
            i += k
        assert i == x.shape[0]
        return st.finish()
    mu1, s1 = run([37])
    mu2, s2 = run([5, 1, 17, 14])
    mu3, s3 = run([5, 1, 17, 14])
    for mu, s in ((mu1, s1), (mu2, s2)):
        e_mu, e_s = np.abs(mu - mu_ref).max(), np.abs(s - sig_ref).max()
        print(f"device statistics: max|d mu| {e_mu:.3e}, max|d sigma| {e_s:.3e} (max|sigma| {scale:.3e})")
        assert e_mu <= 1e-10 * scale and e_s <= 1e-10 * scale
        assert np.abs(np.diag(s) - fx["stat_sigma_diag"]).max() <= 1e-10 * scale
    assert np.array_equal(mu2, mu3) and np.array_equal(s2, s3)              # same chunking: the same bits
    # and, by construction (every element's fma chain continues from the stored accumulator), any chunking: the same bits
    assert np.array_equal(mu1, mu2) and np.array_equal(s1, s2)
    _record("device_statistics", dict(max_dmu=float(np.abs(mu1 - mu_ref).max()), max_dsigma=float(np.abs(s1 - sig_ref).max()), max_sigma=scale))


class _FixedNet:
    def __init__(self, gens):
        self.gens, self.i = gens, 0

    def __call__(self, masked):
        g = self.gens[self.i]
        self.i += 1
        return g


def _eval_batches():
    from oracle import params as op
    batches, gens = [], []
    for b, n in enumerate((3, 3)):
        rng = np.random.Generator(np.random.PCG64(9100 + b))
        g = R.make_images(9000 + b, n, 1, 128)
        _, mk = op.synth_batch(9200 + b, n, 128, 128)
        batches.append((torch.from_numpy(g), torch.from_numpy(mk), 0))
        gens.append(torch.from_numpy(rng.random((n, 1, 128, 128), dtype=np.float32)).cuda())
    return batches, gens


@pytest.mark.parametrize("dt", ["fp32", "fp16"])
def test_calculate_metric_with_fid(models, params, dt):
    """The pass's (mu, sigma) against the fp64 restatement on the very composites it fed to Inception, within the feature bound
    propagated to first order: |d mu| <= e, |d sigma| <= 2 e max|x - mu|, e the per-feature bound of the 128x128 cases;
    the reported fid equals calculate_frechet_distance of the pass's own statistics exactly. The distance is not compared
    across precisions (fewer images than dimensions: its square-root term amplifies small eigenvalue errors); the observed
    difference is recorded only."""
    import gan_inpainting_amd  # noqa: F401
    from gan_inpainting_amd.lib.models import evaluate
    _, fid_score = _fid()
    fx = load("fid_inception")
    batches, gens = _eval_batches()
    rng = np.random.Generator(np.random.PCG64(5))
    truth = rng.random((12, 2048))
    fid_stats = (truth.mean(axis=0), np.cov(truth, rowvar=False))
    cap = {}
    met = evaluate.calculate_metric(torch.device("cuda"), batches, _FixedNet(gens), fid_stats=fid_stats, inception_model=models[dt],
                                    epoch=2, fid_capture=cap)
    comps = torch.cat(cap["composites"])
    assert tuple(comps.shape) == (6, 1, 128, 128)
    # what the reference saves per image: out * m + masked, truncated to 8 bits
    for (g, mk, _), gen, comp in zip(batches, gens, cap["composites"]):
        m = torch.ceil(mk)
        want = torch.floor((gen.cpu() * m + g * (1 - m)) * 255.0).clamp(0, 255) / 255.0
        assert torch.equal(comp, want)
    T64 = R.to_torch(params, torch.float64)
    with torch.no_grad():
        f64 = R.forward(T64, comps.double()).numpy()
    mu_ref, sig_ref = f64.mean(axis=0), np.cov(f64, rowvar=False)
    e = max(_bound(fx, c, dt) for c in ("g128", "c128"))                    # per-feature bound at 128x128
    n = f64.shape[0]
    dev = float(np.abs(f64 - mu_ref).max())
    e_mu, e_s = float(np.abs(cap["mu"] - mu_ref).max()), float(np.abs(cap["sigma"] - sig_ref).max())
    b_s = 2.0 * e * dev
    print(f"calculate_metric {dt}: max|d mu| {e_mu:.3e} (bound {e:.3e}), max|d sigma| {e_s:.3e} (bound {b_s:.3e}), max|x - mu| {dev:.3f}")
    assert e_mu <= e and e_s <= b_s
    assert met["fid"] == fid_score.calculate_frechet_distance(fid_stats[0], fid_stats[1], cap["mu"], cap["sigma"])
    assert np.isfinite(met["fid"]) and met["fid"] >= 0 and met["epoch"] == 2
    fid64 = fid_score.calculate_frechet_distance(fid_stats[0], fid_stats[1], mu_ref, sig_ref)
    _record(f"calculate_metric_{dt}", dict(max_dmu=e_mu, mu_bound=e, max_dsigma=e_s, sigma_bound=b_s, fid=met["fid"], fid_fp64_features=fid64))
    print(f"calculate_metric {dt}: fid {met['fid']:.6f}, from fp64 features {fid64:.6f}")


def test_calculate_metric_without_statistics_or_model_reports_minus_one(models):
    import gan_inpainting_amd  # noqa: F401
    from gan_inpainting_amd.lib.models import evaluate
    batches, gens = _eval_batches()
    stats = (np.zeros(2048), np.eye(2048))
    assert evaluate.calculate_metric(torch.device("cuda"), batches, _FixedNet(gens), inception_model=models["fp16"])["fid"] == -1
    assert evaluate.calculate_metric(torch.device("cuda"), batches, _FixedNet(gens), fid_stats=stats)["fid"] == -1
    assert evaluate.calculate_metric(torch.device("cuda"), batches, _FixedNet(gens))["fid"] == -1


def test_plugin_writes_fid_with_fid_weights(tmp_path, params):
    import gan_inpainting_amd  # noqa: F401
    from gan_inpainting_amd import train
    wpath = str(tmp_path / "pt_inception_standin.pth")
    sd = {k: torch.from_numpy(v) for k, v in params.items()}
    sd["fc.weight"], sd["fc.bias"] = torch.zeros(8, 2048), torch.zeros(8)
    torch.save(sd, wpath)
    train.main(["-exp", "minimaxgan_l1", "-ep", "1", "-b", "4", "--imagedim", "64", "--saveevery", "1", "--evalevery", "1",
                "--samples", "16", "--outdir", str(tmp_path), "--dtype", "fp16", "--fid-weights", wpath])
    with open(os.path.join(str(tmp_path), "model", "minimaxgan_l1", "eval_history.obj"), "rb") as h:
        ev = pickle.load(h)
    assert set(ev[-1]) == {"train", "test"}
    for part in ev[-1].values():
        assert isinstance(part["fid"], float) and np.isfinite(part["fid"]) and part["fid"] >= 0.0
        assert set(part) == {"recon_rmse_global", "recon_l1_global", "recon_rmse_local", "recon_l1_local", "fid", "epoch"}


@pytest.mark.parametrize("dt", ["fp32", "fp16"])
def test_which_kernel_serves_which_convolution(models, dt):
    import gan_inpainting_amd  # noqa: F401
    from gan_inpainting_amd import backend as B
    x = torch.rand(1, 1, 64, 64, device="cuda")
    tag = "f16" if dt == "fp16" else "f32"
    names = [c[0] for c in R.CONVS]
    for name in ("Conv2d_1a_3x3", "Conv2d_3b_1x1", "Mixed_5b.branch5x5_2", "Mixed_6a.branch3x3", "Mixed_6b.branch7x7_2",
                 "Mixed_6b.branch7x7_3", "Mixed_7b.branch3x3_2a", "Mixed_7c.branch_pool"):
        _, _, _, (kh, kw), stride, _ = R.CONV_BY_NAME[name]
        models[dt].debug_forward_convs(x, names.index(name) + 1)
        torch.cuda.synchronize()
        form = "pointwise" if (kh, kw, stride) == (1, 1, 1) else "taps"
        assert B.last_kernel() == f"inc_gemm_kernel<{tag},{form}>", (name, B.last_kernel())
