#!/usr/bin/env python
"""Generate the FID fixtures from the UNMODIFIED reference (runs only where the reference is present; the GPU tests read the
.npz files, never the reference).

    python tests/golden/make_golden_fid.py [--ref /root/reference]

The reference's lib/fid/inception.py imports torchvision and, when a model is built, fetches the published weights. Neither
exists here, so an in-memory stub `torchvision` is installed in sys.modules BEFORE the reference module is imported:
  * torchvision.models.inception: plain constructors for BasicConv2d and InceptionA..E / inception_v3 (written from the
    public architecture; InceptionB / D carry the forwards the reference does not override);
  * torchvision.models.utils.load_state_dict_from_url: a local function that returns tests/inception_ref.py's stand-in
    state dict and opens no connection. Because the import of it succeeds, the reference's torch.utils.model_zoo fallback is
    never taken; this script also replaces torch.hub / model_zoo loaders with functions that raise, so nothing can reach out.
The reference's InceptionV3.forward and its FIDInceptionA / C / E_1 / E_2.forward then run as written.

fid_inception.npz   seeds, pool3 features (fp64) of the reference module for 128x128 and 256x256 images with one and three
                    channels, per-block statistics after Mixed_5d / 6e / 7c, and two error yardsticks against the fp64 features:
                    (a) the reference module in fp32 on the CPU, (b) tests/inception_ref.py in fp32 (fp32 accumulation) with
                    weights and every layer's output rounded to fp16. The per-block statistics are for a bisect on the host
                    (tests/inception_ref.forward(blocks=...) at another precision); the device offers no block read-back.
fid_frechet.npz     the value of the reference's calculate_frechet_distance (scipy) for the (mu, sigma) pairs of
                    tests/inception_ref.py FRECHET_CASES: well-conditioned (d = 64, 256) and rank-deficient (d = 256 with 100
                    samples, d = 2048 with 300). The pairs are regenerated from their seeds (only d = 64 fits a committed file and
                    is stored as well); and a feature matrix with its np.mean / np.cov (diagonal and first rows).
"""
import argparse
import os
import sys
import types

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import inception_ref as R  # noqa: E402

PARAM_SEED = 20260
CASES = (("g128", 1, 128, 11, 3), ("c128", 3, 128, 12, 3), ("g256", 1, 256, 13, 2), ("c256", 3, 256, 14, 2))   # name, channels, size, seed, images


# ---- the stub ---------------------------------------------------------------------------------------------------------------
class BasicConv2d(nn.Module):
    def __init__(self, in_channels, out_channels, **kwargs):
        super().__init__()
        self.conv = nn.Conv2d(in_channels, out_channels, bias=False, **kwargs)
        self.bn = nn.BatchNorm2d(out_channels, eps=0.001)

    def forward(self, x):
        return F.relu(self.bn(self.conv(x)), inplace=True)


class InceptionA(nn.Module):
    def __init__(self, in_channels, pool_features):
        super().__init__()
        self.branch1x1 = BasicConv2d(in_channels, 64, kernel_size=1)
        self.branch5x5_1 = BasicConv2d(in_channels, 48, kernel_size=1)
        self.branch5x5_2 = BasicConv2d(48, 64, kernel_size=5, padding=2)
        self.branch3x3dbl_1 = BasicConv2d(in_channels, 64, kernel_size=1)
        self.branch3x3dbl_2 = BasicConv2d(64, 96, kernel_size=3, padding=1)
        self.branch3x3dbl_3 = BasicConv2d(96, 96, kernel_size=3, padding=1)
        self.branch_pool = BasicConv2d(in_channels, pool_features, kernel_size=1)


class InceptionB(nn.Module):
    def __init__(self, in_channels):
        super().__init__()
        self.branch3x3 = BasicConv2d(in_channels, 384, kernel_size=3, stride=2)
        self.branch3x3dbl_1 = BasicConv2d(in_channels, 64, kernel_size=1)
        self.branch3x3dbl_2 = BasicConv2d(64, 96, kernel_size=3, padding=1)
        self.branch3x3dbl_3 = BasicConv2d(96, 96, kernel_size=3, stride=2)

    def forward(self, x):
        d = self.branch3x3dbl_3(self.branch3x3dbl_2(self.branch3x3dbl_1(x)))
        return torch.cat([self.branch3x3(x), d, F.max_pool2d(x, kernel_size=3, stride=2)], 1)


class InceptionC(nn.Module):
    def __init__(self, in_channels, channels_7x7):
        super().__init__()
        c7 = channels_7x7
        self.branch1x1 = BasicConv2d(in_channels, 192, kernel_size=1)
        self.branch7x7_1 = BasicConv2d(in_channels, c7, kernel_size=1)
        self.branch7x7_2 = BasicConv2d(c7, c7, kernel_size=(1, 7), padding=(0, 3))
        self.branch7x7_3 = BasicConv2d(c7, 192, kernel_size=(7, 1), padding=(3, 0))
        self.branch7x7dbl_1 = BasicConv2d(in_channels, c7, kernel_size=1)
        self.branch7x7dbl_2 = BasicConv2d(c7, c7, kernel_size=(7, 1), padding=(3, 0))
        self.branch7x7dbl_3 = BasicConv2d(c7, c7, kernel_size=(1, 7), padding=(0, 3))
        self.branch7x7dbl_4 = BasicConv2d(c7, c7, kernel_size=(7, 1), padding=(3, 0))
        self.branch7x7dbl_5 = BasicConv2d(c7, 192, kernel_size=(1, 7), padding=(0, 3))
        self.branch_pool = BasicConv2d(in_channels, 192, kernel_size=1)


class InceptionD(nn.Module):
    def __init__(self, in_channels):
        super().__init__()
        self.branch3x3_1 = BasicConv2d(in_channels, 192, kernel_size=1)
        self.branch3x3_2 = BasicConv2d(192, 320, kernel_size=3, stride=2)
        self.branch7x7x3_1 = BasicConv2d(in_channels, 192, kernel_size=1)
        self.branch7x7x3_2 = BasicConv2d(192, 192, kernel_size=(1, 7), padding=(0, 3))
        self.branch7x7x3_3 = BasicConv2d(192, 192, kernel_size=(7, 1), padding=(3, 0))
        self.branch7x7x3_4 = BasicConv2d(192, 192, kernel_size=3, stride=2)

    def forward(self, x):
        a = self.branch3x3_2(self.branch3x3_1(x))
        b = self.branch7x7x3_4(self.branch7x7x3_3(self.branch7x7x3_2(self.branch7x7x3_1(x))))
        return torch.cat([a, b, F.max_pool2d(x, kernel_size=3, stride=2)], 1)


class InceptionE(nn.Module):
    def __init__(self, in_channels):
        super().__init__()
        self.branch1x1 = BasicConv2d(in_channels, 320, kernel_size=1)
        self.branch3x3_1 = BasicConv2d(in_channels, 384, kernel_size=1)
        self.branch3x3_2a = BasicConv2d(384, 384, kernel_size=(1, 3), padding=(0, 1))
        self.branch3x3_2b = BasicConv2d(384, 384, kernel_size=(3, 1), padding=(1, 0))
        self.branch3x3dbl_1 = BasicConv2d(in_channels, 448, kernel_size=1)
        self.branch3x3dbl_2 = BasicConv2d(448, 384, kernel_size=3, padding=1)
        self.branch3x3dbl_3a = BasicConv2d(384, 384, kernel_size=(1, 3), padding=(0, 1))
        self.branch3x3dbl_3b = BasicConv2d(384, 384, kernel_size=(3, 1), padding=(1, 0))
        self.branch_pool = BasicConv2d(in_channels, 192, kernel_size=1)


class Inception3(nn.Module):
    """The attribute holder the reference picks its layers from (its own InceptionV3.forward drives them); no fc head:
    the stand-in state dict has none."""

    def __init__(self):
        super().__init__()
        self.Conv2d_1a_3x3 = BasicConv2d(3, 32, kernel_size=3, stride=2)
        self.Conv2d_2a_3x3 = BasicConv2d(32, 32, kernel_size=3)
        self.Conv2d_2b_3x3 = BasicConv2d(32, 64, kernel_size=3, padding=1)
        self.Conv2d_3b_1x1 = BasicConv2d(64, 80, kernel_size=1)
        self.Conv2d_4a_3x3 = BasicConv2d(80, 192, kernel_size=3)
        self.Mixed_5b = InceptionA(192, pool_features=32)
        self.Mixed_5c = InceptionA(256, pool_features=64)
        self.Mixed_5d = InceptionA(288, pool_features=64)
        self.Mixed_6a = InceptionB(288)
        self.Mixed_6b = InceptionC(768, channels_7x7=128)
        self.Mixed_6c = InceptionC(768, channels_7x7=160)
        self.Mixed_6d = InceptionC(768, channels_7x7=160)
        self.Mixed_6e = InceptionC(768, channels_7x7=192)
        self.Mixed_7a = InceptionD(768)
        self.Mixed_7b = InceptionE(1280)
        self.Mixed_7c = InceptionE(2048)


def install_stub(state_dict):
    def refuse(*a, **k):
        raise RuntimeError("the fixture generator must not fetch anything")
    import torch.hub
    import torch.utils.model_zoo
    torch.hub.load_state_dict_from_url = refuse
    torch.hub.download_url_to_file = refuse
    torch.utils.model_zoo.load_url = refuse

    tv = types.ModuleType("torchvision")
    tv.__version__ = "0.6.0"
    models = types.ModuleType("torchvision.models")
    inc = types.ModuleType("torchvision.models.inception")
    utils = types.ModuleType("torchvision.models.utils")
    for cls in (BasicConv2d, InceptionA, InceptionB, InceptionC, InceptionD, InceptionE, Inception3):
        setattr(inc, cls.__name__, cls)
    models.inception_v3 = lambda *a, **k: Inception3()
    inc.inception_v3 = models.inception_v3
    utils.load_state_dict_from_url = lambda url, progress=True, **k: {k2: v.clone() for k2, v in state_dict.items()}   # local: no connection
    models.inception, models.utils, tv.models = inc, utils, models
    sys.modules.update({"torchvision": tv, "torchvision.models": models, "torchvision.models.inception": inc,
                        "torchvision.models.utils": utils})


def block_stats(t):
    """(n, 3): mean, mean |.|, max per image."""
    t = t.double()
    return torch.stack([t.mean(dim=(1, 2, 3)), t.abs().mean(dim=(1, 2, 3)), t.amax(dim=(1, 2, 3))], 1).numpy()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref", default="/root/reference")
    args = ap.parse_args()
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    P = R.make_params(PARAM_SEED)
    for k, v in P.items():
        if k.endswith("running_var"):
            assert v.min() > 100 * R.BN_EPS
    sd32 = {k: torch.from_numpy(v) for k, v in P.items()}
    install_stub(sd32)
    assert "torchvision.models.utils" in sys.modules
    sys.path.insert(0, args.ref)
    import lib.fid.inception as ref_inc       # the unmodified reference
    import lib.fid.fid_score as ref_fid
    assert ref_inc.load_state_dict_from_url is sys.modules["torchvision.models.utils"].load_state_dict_from_url

    model32 = ref_inc.InceptionV3([ref_inc.InceptionV3.BLOCK_INDEX_BY_DIM[2048]]).eval()
    model64 = ref_inc.InceptionV3([3]).double().eval()
    T64, T32 = R.to_torch(P, torch.float64), R.to_torch(P, torch.float32)

    out = {"param_seed": np.int64(PARAM_SEED), "cases": np.array([c[0] for c in CASES])}
    feats_all = []
    ya = yb = 0.0
    with torch.no_grad():
        for name, ch, hw, seed, n in CASES:
            x = torch.from_numpy(R.make_images(seed, n, ch, hw))
            x3 = x.expand(-1, 3, -1, -1) if ch == 1 else x       # the reference feeds grey2rgb images
            f64 = model64(x3.double())[0].reshape(n, -1)
            blocks = {}
            r64 = R.forward(T64, x.double(), blocks=blocks)
            err = float((r64 - f64).abs().max())
            assert err < 1e-10, (name, err)
            f32 = model32(x3)[0].reshape(n, -1).double()
            r32 = R.forward(T32, x).double()
            rel32 = float((r32 - f32).abs().max() / f32.abs().max())
            assert rel32 < 1e-4, (name, rel32)
            r16 = R.forward(T32, x, round_fn=R.round_fp16).double()      # fp16 rounding points, fp32 accumulation
            a = float((f32 - f64).abs().max())
            b = float((r16 - f64).abs().max())
            ya, yb = max(ya, a), max(yb, b)
            print(f"{name}: restatement vs module fp64 {err:.2e}, fp32 rel {rel32:.2e}; yardstick a {a:.3e} b {b:.3e}; max|f| {float(f64.abs().max()):.3f}")
            out[f"{name}_seed"] = np.int64(seed)
            out[f"{name}_shape"] = np.array([n, ch, hw, hw], np.int64)
            out[f"{name}_features"] = f64.numpy()
            out[f"{name}_yardstick_a"] = np.float64(a)
            out[f"{name}_yardstick_b"] = np.float64(b)
            for bn, t in blocks.items():
                out[f"{name}_{bn}_stats"] = block_stats(t)
            feats_all.append(f64.numpy())
    allf = np.concatenate(feats_all)
    assert (allf.max(axis=0) - allf.min(axis=0)).min() > 0, "a feature dimension is constant across the fixture's images: dead network"
    out["yardstick_a"] = np.float64(ya)
    out["yardstick_b"] = np.float64(yb)
    np.savez_compressed(os.path.join(HERE, "fid_inception.npz"), **out)

    # ---- Frechet distance and statistics ------------------------------------------------------------------------------------
    rng = np.random.Generator(np.random.PCG64(77))
    fr = {"cases": np.array(list(R.FRECHET_CASES))}
    for name in R.FRECHET_CASES:
        m1, s1, m2, s2 = R.frechet_case(name)
        val = float(ref_fid.calculate_frechet_distance(m1, s1, m2, s2))
        print(f"frechet {name}: {val:.12g}")
        fr[f"{name}_value"] = np.float64(val)
        # a checksum of the regenerated pair: a test that regenerates something else fails on it, not on the distance
        fr[f"{name}_check"] = np.array([m1.sum(), np.trace(s1), m2.sum(), np.trace(s2)])
        if name == "d64":
            fr["d64_mu1"], fr["d64_sigma1"], fr["d64_mu2"], fr["d64_sigma2"] = m1, s1, m2, s2
    x = (rng.standard_normal((37, 2048)) * rng.uniform(0.1, 1.0, 2048) + rng.uniform(0.0, 1.0, 2048)).astype(np.float32)
    fr["stat_x"] = x
    fr["stat_mu"] = np.mean(x.astype(np.float64), axis=0)
    sig = np.cov(x.astype(np.float64), rowvar=False)
    fr["stat_sigma_diag"] = np.diag(sig).copy()
    fr["stat_sigma_rows"] = sig[:8].copy()
    fr["stat_sigma_max"] = np.float64(np.abs(sig).max())
    fr["stat_sigma_fro"] = np.float64(np.sqrt((sig ** 2).sum()))
    np.savez_compressed(os.path.join(HERE, "fid_frechet.npz"), **fr)
    for f in ("fid_inception.npz", "fid_frechet.npz"):
        print(f, os.path.getsize(os.path.join(HERE, f)), "bytes")


if __name__ == "__main__":
    main()
