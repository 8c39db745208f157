"""CPU tier: the command-line surface of the LPIPS generator term (train.py --lpips-loss): what it requires, where it is refused, and
what a resumable state records about it."""
import pytest


def _train():
    import gan_inpainting_amd  # noqa: F401
    from gan_inpainting_amd import train
    return train


def test_lpips_loss_needs_the_weights(capsys):
    with pytest.raises(SystemExit):
        _train().main(["-exp", "wgan_l1", "--lpips-loss", "0.5"])
    assert "--lpips-weights" in capsys.readouterr().err


@pytest.mark.parametrize("exp", ["minimaxgan_l1", "minimaxgan_rmse", "experiment1_global_local_D"])
def test_lpips_loss_is_refused_where_no_oracle_pins_it(exp, capsys):
    with pytest.raises(SystemExit):
        _train().main(["-exp", exp, "--lpips-loss", "0.5", "--lpips-weights", "nowhere.pth"])
    assert "only the WGAN plugins" in capsys.readouterr().err


def test_plugins_refuse_and_default_is_off():
    import gan_inpainting_amd  # noqa: F401
    from gan_inpainting_amd.experiment_list import _common as C
    assert C.lpips_loss_kw({}) == {} and C.lpips_loss_kw({"lpips_loss": 0.0, "lpips_model": None}) == {}
    C.refuse_lpips_loss({}, "minimaxgan_l1")
    with pytest.raises(ValueError):
        C.refuse_lpips_loss({"lpips_loss": 1.0}, "minimaxgan_l1")
    with pytest.raises(ValueError):
        C.lpips_loss_kw({"lpips_loss": 1.0, "lpips_model": None})

    class Plain:
        grad = False
    with pytest.raises(ValueError):
        C.lpips_loss_kw({"lpips_loss": 1.0, "lpips_model": Plain()})

    class Grad:
        grad = True
    m = Grad()
    assert C.lpips_loss_kw({"lpips_loss": 0.25, "lpips_model": m}) == {"lpips": m, "lpips_weight": 0.25}


def test_compat_args_carry_the_weight_only_when_set():
    import gan_inpainting_amd  # noqa: F401
    from gan_inpainting_amd import checkpoint
    off = checkpoint.compat_args({"lpips_loss": 0.0}, 1, {})
    assert "lpips_loss" not in off and off == checkpoint.compat_args({}, 1, {})
    on = checkpoint.compat_args({"lpips_loss": 0.5}, 1, {})
    assert on["lpips_loss"] == 0.5
    with pytest.raises(checkpoint.CheckpointError):
        checkpoint.check_compatible(off, on)


def test_steps_without_the_term_keep_their_state_keys():
    """A WGAN step built without lpips reports the extra state it always did (no GPU needed: the method reads host fields only)."""
    import gan_inpainting_amd  # noqa: F401
    from gan_inpainting_amd import trainer
    s = object.__new__(trainer.WGANStep)
    s.aug, s.lpips = None, None
    assert s._extra_state() == {}
