"""CPU tier of resumable training and the EMA generator: the parser rules of the new flags, the checkpoint module
(gan_inpainting_amd/checkpoint.py) and the numpy restatement of the EMA kernel (tests/ema_ref.py)."""
import os

import numpy as np
import pytest
import torch

import ema_ref


def _parser():
    import gan_inpainting_amd  # noqa: F401
    from gan_inpainting_amd import train
    return train.build_parser()


@pytest.mark.parametrize("argv, word", [
    (["-exp", "wgan_l1", "wgan_rmse", "--resume", "/some/last_state.pt"], "--resume"),
    (["-exp", "wgan_l1", "--ema-decay", "1.0"], "--ema-decay"),
    (["-exp", "wgan_l1", "--ema-decay", "-0.1"], "--ema-decay"),
    (["-exp", "wgan_l1", "--state-every", "0"], "--state-every"),
])
def test_parser_refuses(argv, word, capsys):
    with pytest.raises(SystemExit) as e:
        _parser().parse_args(argv)
    assert e.value.code == 2
    assert word in capsys.readouterr().err


def test_parser_accepts_and_defaults():
    a = _parser().parse_args(["-exp", "wgan_l1"])
    assert (a.save_state, a.state_every, a.resume, a.ema_decay) == (False, None, "", 0.0)      # nothing new without a new flag
    a = _parser().parse_args(["-exp", "wgan_l1", "wgan_rmse", "--resume", "auto", "--save-state", "--state-every", "3", "--ema-decay", "0.999"])
    assert (a.save_state, a.state_every, a.resume, a.ema_decay) == (True, 3, "auto", 0.999)
    a = _parser().parse_args(["-exp", "wgan_l1", "--resume", "/some/last_state.pt"])
    assert a.resume == "/some/last_state.pt"


def _args(**kw):
    from gan_inpainting_amd import checkpoint
    state = {"imagedim": 64, "batchsize": 4, "dtype": "fp32", "generator": "unet", "discriminator": "patchgan", "gp_lambda": 0.0,
             "g_every": 2, "masks": "files", "mask_seed": 0, "flip": False, "ema_decay": 0.0, "perceptual_grad": False,
             "face_parsing": "off", "numepoch": 3, "saveevery": 1, "evalevery": 1, "outdir": "/a", "workers": 0, "cache": "off",
             "cache_budget_gb": None}
    state.update(kw)
    nets = {"G": torch.nn.Linear(3, 2), "D0": torch.nn.Linear(5, 1)}
    return checkpoint.compat_args(state, 1, nets)


def test_check_compatible_names_the_key():
    from gan_inpainting_amd import checkpoint
    saved = _args()
    checkpoint.check_compatible(saved, _args())
    # what may differ between the run that saved and the run that resumes
    checkpoint.check_compatible(saved, _args(numepoch=9, saveevery=5, evalevery=7, outdir="/b", workers=4, cache="device", cache_budget_gb=2.0))
    for key, other in [("imagedim", 128), ("batchsize", 8), ("dtype", "fp16"), ("discriminator", "dcgan"), ("gp_lambda", 10.0),
                       ("g_every", 0), ("masks", "rect"), ("mask_seed", 3), ("flip", True), ("ema_decay", 0.9), ("perceptual_grad", True),
                       ("face_parsing", "random")]:
        with pytest.raises(checkpoint.CheckpointError) as e:
            checkpoint.check_compatible(saved, _args(**{key: other}))
        msg = str(e.value)
        assert key in msg and repr(saved[key]) in msg and repr(other) in msg, msg
    cur = dict(saved, world_size=8)
    with pytest.raises(checkpoint.CheckpointError, match="world_size"):
        checkpoint.check_compatible(saved, cur)
    cur = dict(saved)
    cur["params/G"] += 1
    with pytest.raises(checkpoint.CheckpointError, match="params/G"):
        checkpoint.check_compatible(saved, cur)


def test_parameter_counts_are_in_the_arguments():
    a = _args()
    assert a["params/G"] == 3 * 2 + 2 and a["params/D0"] == 5 + 1 and a["world_size"] == 1


def test_rng_file_names():
    from gan_inpainting_amd import checkpoint
    assert checkpoint.rng_path("/x/last_state.pt", 0) == "/x/last_state.rng0.pt"
    assert checkpoint.rng_path("/x/last_state.pt", 5) == "/x/last_state.rng5.pt"
    assert checkpoint.rng_path("/x/mine", 2) == "/x/mine.rng2.pt"


def test_resolve_auto_and_path(tmp_path):
    from gan_inpainting_amd import checkpoint
    assert checkpoint.resolve("", str(tmp_path)) is None
    assert checkpoint.resolve("auto", str(tmp_path)) is None                 # no file yet: a fresh start
    f = tmp_path / checkpoint.STATE_FILE
    checkpoint.save_state(str(f), {"format_version": checkpoint.FORMAT_VERSION})
    assert checkpoint.resolve("auto", str(tmp_path)) == str(f)
    assert checkpoint.resolve(str(f), "/nowhere") == str(f)
    with pytest.raises(checkpoint.CheckpointError):
        checkpoint.resolve(str(tmp_path / "missing.pt"), str(tmp_path))


class _Explodes:
    def __reduce__(self):
        raise RuntimeError("serialisation failed half-way")


def test_failed_save_keeps_the_previous_file(tmp_path):
    from gan_inpainting_amd import checkpoint
    f = str(tmp_path / "last_state.pt")
    good = {"format_version": checkpoint.FORMAT_VERSION, "epoch": 4, "t": torch.arange(5)}
    checkpoint.save_state(f, good)
    before = open(f, "rb").read()
    with pytest.raises(RuntimeError, match="half-way"):
        checkpoint.save_state(f, {"format_version": checkpoint.FORMAT_VERSION, "big": torch.zeros(1000), "bad": _Explodes()})
    assert open(f, "rb").read() == before
    assert not os.path.exists(f + ".tmp")
    assert checkpoint.load_state(f)["epoch"] == 4


def test_state_round_trips(tmp_path):
    from gan_inpainting_amd import checkpoint
    f = str(tmp_path / "s.pt")
    g = torch.Generator().manual_seed(3)
    payload = {"format_version": checkpoint.FORMAT_VERSION, "title": "wgan_l1", "epoch": 2, "args": _args(),
               "history": [{"losses": {"recon": 0.25}, "g_updates": 2}], "eval_hist": [{"train": {"fid": -1}}],
               "counters": {"G_iter_count": 7}, "nets": {"G": {"state_dict": {"w": torch.randn(4, 3, generator=g)}}},
               "rng": {"torch": torch.get_rng_state()}}
    checkpoint.save_state(f, payload)
    back = checkpoint.load_state(f)
    assert back["counters"] == {"G_iter_count": 7} and back["history"] == payload["history"] and back["args"] == payload["args"]
    assert torch.equal(back["nets"]["G"]["state_dict"]["w"], payload["nets"]["G"]["state_dict"]["w"])
    assert torch.equal(back["rng"]["torch"], payload["rng"]["torch"])
    torch.save({"something": "else"}, f)
    with pytest.raises(checkpoint.CheckpointError):
        checkpoint.load_state(f)
    torch.save({"format_version": checkpoint.FORMAT_VERSION + 1}, f)
    with pytest.raises(checkpoint.CheckpointError, match="version"):
        checkpoint.load_state(f)


DECAYS = (0.0, 0.5, 0.9, 0.999, 0.9999, 1.0)


@pytest.mark.parametrize("magnitude", [1e-6, 1.0, 1e4])
def test_ema_ref_within_its_bound_of_fp64(magnitude):
    """The restatement against torch's float64 lerp-style evaluation ema + om * (p - ema) of the same float32 inputs."""
    g = torch.Generator().manual_seed(11)
    ema = (torch.randn(20001, generator=g) * magnitude).float()
    p = (ema + torch.randn(20001, generator=g) * magnitude * 0.01).float()
    for decay in DECAYS:
        out = ema_ref.ema_update(ema.numpy(), p.numpy(), decay)
        om = float(ema_ref.om_of(decay))
        e64 = (ema.double() + om * (p.double() - ema.double())).numpy()
        assert np.array_equal(e64, ema_ref.exact(ema.numpy(), p.numpy(), decay))
        ratio = ema_ref.worst_ratio(out, ema.numpy(), p.numpy(), decay)
        print(f"magnitude {magnitude:g} decay {decay:g}: worst |out - E| / bound = {ratio:.3f}")
        assert ratio <= 1.0


def test_ema_ref_exact_cases():
    g = torch.Generator().manual_seed(12)
    ema = torch.randn(4099, generator=g).numpy()
    p = torch.randn(4099, generator=g).numpy()
    assert np.array_equal(ema_ref.ema_update(ema, p, 1.0).view(np.uint32), ema.view(np.uint32))       # decay = 1: untouched
    for decay in DECAYS:
        assert np.array_equal(ema_ref.ema_update(ema, ema.copy(), decay).view(np.uint32), ema.view(np.uint32))   # p == ema
    assert np.array_equal(ema_ref.ema_update(ema, p, 0.0), (ema + (p - ema)).astype(np.float32))       # decay = 0: ema + diff
