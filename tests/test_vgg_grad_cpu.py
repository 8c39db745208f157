"""CPU tier of the differentiable VGG-19 perceptual / style terms: the test helper (tests/vgg_grad_ref.py) against the oracle's
pinned functions, its analytic seeds against autograd, and the host-side surface (exported symbols, command line, unchanged
defaults)."""
import numpy as np
import pytest
import torch

import vgg_grad_ref as R
from oracle import params as op
from oracle import torch_ref as orc


def _case(seed=21, n=2, hw=32):
    P = {k: torch.from_numpy(v).double() for k, v in op.make_vgg19_params(seed).items()}
    g, mk = op.synth_batch(seed + 1, n, hw, hw)
    gen = np.random.Generator(np.random.PCG64(seed + 2)).random((n, 1, hw, hw), dtype=np.float32)
    out = gen * np.ceil(mk) + g * (1 - np.ceil(mk))
    return P, torch.from_numpy(g).double(), torch.from_numpy(out.astype(np.float32)).double()


def test_helper_values_equal_the_oracle():
    P, tgt, out = _case()
    fo, fr = R.features(P, out), orc.vgg19_tap_features(P, out)
    assert len(fo) == 5 and all(torch.equal(a, b) for a, b in zip(fo, fr))
    p, s = R.loss(P, out.clone().requires_grad_(True), tgt, 0.01, 0.02)
    pr, sr, _, _ = orc.perceptual_and_style_loss(P, out, tgt, 0.01, 0.02)
    assert p.grad_fn is not None and s.grad_fn is not None
    assert abs(float(p) - float(pr)) <= 1e-12 * float(pr) and abs(float(s) - float(sr)) <= 1e-12 * float(sr)


@pytest.mark.parametrize("wp,ws", [(1.0, 0.0), (0.0, 1.0), (0.01, 0.01)])
def test_analytic_seeds_equal_autograd(wp, ws):
    P, tgt, out = _case()
    fo = [f.detach().requires_grad_(True) for f in R.features(P, out)]
    ft = R.features(P, tgt)
    p_terms, s_terms = R.terms(fo, ft)
    (wp * sum(p_terms) + ws * sum(s_terms)).backward()
    for tap, (f, sd) in enumerate(zip(fo, R.seeds([f.detach() for f in fo], ft, wp, ws))):
        assert R.rel_l2(sd, f.grad) <= 1e-10, tap


def test_scaled_store_helper_is_consistent():
    """scale only moves the fp16 rounding: without a store a power of two changes nothing; the layer capture returns 13 maps whose
    shapes follow the pooling."""
    P, tgt, out = _case()
    Pf = {k: v.float() for k, v in P.items()}
    g1 = R.grad(Pf, out, tgt, 1.0, 1.0)
    g2, layers = R.grad(Pf, out, tgt, 1.0, 1.0, scale=2.0 ** 20, layers=True)
    assert torch.equal(g1, g2)
    assert [tuple(x.shape[1:]) for x in layers] == [(c, 32 >> d, 32 >> d) for c, d in zip(
        (64, 64, 128, 128, 256, 256, 256, 256, 512, 512, 512, 512, 512), (0, 0, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4))]
    s = R.pow2_scale_for(g1)
    assert 2.0 ** -4 <= float(g1.abs().max()) * s < 2.0 ** -3
    ge = R.grad(Pf, out, tgt, 1.0, 0.0, store=orc.store_fp16, scale=R.pow2_scale_for(R.grad(Pf, out, tgt, 1.0, 0.0)))
    assert 0 < R.rel_l2(ge, R.grad(Pf, out, tgt, 1.0, 0.0)) < 0.1


def test_library_exports_the_grad_entries():
    import gan_inpainting_amd  # noqa: F401
    from gan_inpainting_amd import backend
    lib = backend.lib()
    for name in ("gi_vgg19_grad_workspace_bytes", "gi_vgg19_bind_grad", "gi_vgg19_perceptual_style_grad", "gi_vgg19_grad_layer"):
        assert hasattr(lib, name), name
    assert lib.gi_vgg19_grad_workspace_bytes(None) == -1


def test_train_parser_has_the_flag_off_by_default():
    import gan_inpainting_amd  # noqa: F401
    from gan_inpainting_amd import train
    parser = train.build_parser()
    assert parser.parse_args(["-exp", "x"]).perceptual_grad is False
    assert parser.parse_args(["-exp", "x", "--perceptual-grad"]).perceptual_grad is True
    assert "reference" in [a for a in parser._actions if a.dest == "perceptual_grad"][0].help


def test_defaults_on_cpu_tensors_raise_what_they_raised():
    import warnings
    import gan_inpainting_amd  # noqa: F401
    from gan_inpainting_amd import backend
    from gan_inpainting_amd.lib.models import loss, networks
    x, t = torch.rand(1, 1, 16, 16), torch.rand(1, 1, 16, 16)
    loss.set_vgg(networks.VGG19Wrapper(max_pairs=1))
    try:
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            for call in (lambda: loss.perceptual_and_style_loss(x, t, 0.01, 0.01, differentiable=False),
                         lambda: loss.perceptual_and_style_loss(x, t), lambda: loss.perceptual_loss(x, t), lambda: loss.style_loss(x, t)):
                with pytest.raises(backend.BackendError, match="float32 tensors on the gfx950 device"):
                    call()
            # the switch needs a wrapper that owns the backward's workspace
            with pytest.raises(backend.BackendError, match="grad=True"):
                loss.perceptual_and_style_loss(x.requires_grad_(), t, differentiable=True)
    finally:
        loss.set_vgg(None)
