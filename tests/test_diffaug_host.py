"""CPU tier: host logic of --diffaug (train.py's parser, the policy strings and keys of lib/models/augment.py against the numpy
restatement, the resume compatibility record)."""
import importlib.util
import os

import pytest

import gan_inpainting_amd  # noqa: F401
from gan_inpainting_amd import checkpoint
from gan_inpainting_amd.lib.models import augment
import diffaug_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def parser():
    spec = importlib.util.spec_from_file_location("gi_train_cli", os.path.join(ROOT, "gan-inpainting_amd", "train.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod.build_parser()


def test_cli_accepts_every_subset_and_refuses_the_rest():
    p = parser()
    a = p.parse_args(["-exp", "wgan_l1"])
    assert a.diffaug is None and a.diffaug_seed == 0
    for policy in ("color", "translation", "cutout", "color,cutout", "cutout,translation,color"):
        a = p.parse_args(["-exp", "wgan_l1", "minimaxgan_rmse", "--diffaug", policy, "--diffaug-seed", "7"])
        assert a.diffaug == policy and a.diffaug_seed == 7
    for bad in (["-exp", "wgan_l1", "--diffaug", "colour"], ["-exp", "wgan_l1", "--diffaug", ""], ["-exp", "wgan_l1", "--diffaug", "color,,cutout"],
                ["-exp", "experiment1_global_local_D", "--diffaug", "color"], ["-exp", "wgan_l1", "experiment1_global_local_D", "--diffaug", "cutout"],
                ["-exp", "wgan_l1", "--diffaug-seed", "3"]):
        with pytest.raises(SystemExit):
            p.parse_args(bad)


def test_policy_bits_and_keys_match_the_restatement():
    for policy in ("color", "translation", "cutout", "color,translation", "cutout, color", "color,translation,cutout"):
        assert augment.parse_policy(policy) == R.policy_bits(policy)
    for bad in ("", "colour", "color;cutout", "color,"):
        with pytest.raises(ValueError):
            augment.parse_policy(bad)
    n = 32
    for step, call, rank, i in ((0, 0, 0, 0), (5, 2, 3, 31), (1 << 20, 1, 7, 0)):
        assert augment.key0(step, call, rank * n) + i == R.key_of(step, call, rank, n, i)
    with pytest.raises(ValueError):
        augment.key0(0, 4)


def test_resume_record_carries_the_policy_only_when_it_is_on():
    base = {"imagedim": 128, "batchsize": 8}
    off = checkpoint.compat_args(dict(base, diffaug=None, diffaug_seed=0), 1, {})
    assert "diffaug" not in off and off == checkpoint.compat_args(base, 1, {})
    on = checkpoint.compat_args(dict(base, diffaug="cutout,color", diffaug_seed=3), 1, {})
    assert on["diffaug"] == 5 and on["diffaug_seed"] == 3
    checkpoint.check_compatible(on, checkpoint.compat_args(dict(base, diffaug="color,cutout", diffaug_seed=3), 1, {}))
    for other in (off, checkpoint.compat_args(dict(base, diffaug="color", diffaug_seed=3), 1, {}),
                  checkpoint.compat_args(dict(base, diffaug="cutout,color", diffaug_seed=4), 1, {})):
        with pytest.raises(checkpoint.CheckpointError):
            checkpoint.check_compatible(on, other)
