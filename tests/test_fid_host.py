"""CPU tier: the host surface of the FID path (the library loads without a GPU): lib.fid imports without torchvision or scipy,
InceptionV3's inventory / state dict, the Frechet distance against the reference's scipy-based function, the eps fallback,
the .npz shortcut, the C-ABI entries and the refusals.

Frechet distance, eigenvalue form against the recorded values of the reference's function (relative difference; bound 1e-6):
    d64 3.1e-15, d256 1.4e-13, d256_n100 1.2e-08, d2048_n300 2.3e-08   (measured where the fixture was generated)
"""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

import inception_ref as R
from util_golden import load

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _fid():
    import gan_inpainting_amd  # noqa: F401
    from gan_inpainting_amd.lib.fid import fid_score, inception
    return inception, fid_score


def test_imports_without_torchvision_or_scipy():
    code = ("import sys; sys.modules['torchvision'] = None; sys.modules['scipy'] = None; sys.path.insert(0, %r)\n"
            "import numpy as np, gan_inpainting_amd\n"
            "from gan_inpainting_amd.lib.fid import inception, fid_score\n"
            "m = inception.InceptionV3([inception.InceptionV3.BLOCK_INDEX_BY_DIM[2048]])\n"
            "v = fid_score.calculate_frechet_distance(np.zeros(3), np.eye(3), np.ones(3), 4 * np.eye(3))\n"
            "assert abs(v - 6.0) < 1e-12, v\n"
            "assert 'scipy.linalg' not in sys.modules and 'torchvision.models' not in sys.modules\n") % ROOT
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_inventory_and_state_dict_round_trip():
    inception, _ = _fid()
    m = inception.InceptionV3()
    assert inception.InceptionV3.BLOCK_INDEX_BY_DIM == {64: 0, 192: 1, 768: 2, 2048: 3} and inception.InceptionV3.DEFAULT_BLOCK_INDEX == 3
    sd = m.state_dict()
    assert [(k, tuple(v.shape)) for k, v in sd.items()] == R.keys_and_shapes()
    assert len(sd) == 94 * 5 and m.flat.numel() == R.param_count() == 21820000
    assert all(float(v.abs().max()) == 0.0 for v in sd.values())          # nothing is fetched: parameters start at zero
    g = torch.Generator().manual_seed(3)
    new = {k: torch.randn(v.shape, generator=g) for k, v in sd.items()}
    extra = dict(new)
    extra["fc.weight"] = torch.zeros(1008, 2048)                            # the published file's classifier head: ignored
    extra["fc.bias"] = torch.zeros(1008)
    extra["Conv2d_1a_3x3.bn.num_batches_tracked"] = torch.tensor(0)
    assert m.load_state_dict(extra) == []
    back = m.state_dict()
    assert all(torch.equal(back[k], new[k]) for k in new)
    short = {k: v for k, v in new.items() if not k.startswith("Mixed_7c.branch_pool")}
    with pytest.raises(RuntimeError, match="missing keys"):
        m.load_state_dict(short)
    assert sorted(m.load_state_dict(short, strict=False)) == sorted(k for k in new if k.startswith("Mixed_7c.branch_pool"))
    with pytest.raises(RuntimeError, match="shape"):
        m.load_state_dict({"Conv2d_1a_3x3.conv.weight": torch.zeros(32, 3, 5, 5)}, strict=False)


def test_refusals():
    inception, fid_score = _fid()
    for kw in (dict(output_blocks=[0]), dict(output_blocks=[2, 3]), dict(resize_input=False), dict(normalize_input=False),
               dict(requires_grad=True), dict(use_fid_inception=False)):
        with pytest.raises(NotImplementedError):
            inception.InceptionV3(**kw)
    with pytest.raises(NotImplementedError):
        fid_score.calculate_activation_statistics(torch.zeros(2, 1, 8, 8), inception.InceptionV3(), dims=768)


def test_compute_on_a_context_free_handle_fails():
    import gan_inpainting_amd  # noqa: F401
    from gan_inpainting_amd import backend as B
    lib = B.lib()
    h = C.c_void_p()
    B.check(lib.gi_inception_create(None, B.GI_F16, 4, C.byref(h)))
    try:
        assert lib.gi_inception_param_floats(h) == R.param_count()
        assert lib.gi_inception_workspace_bytes(h) > 0
        buf = (C.c_float * 16)()
        with pytest.raises(B.BackendError):
            B.check(lib.gi_inception_bind(h, C.cast(buf, C.c_void_p), C.cast(buf, C.c_void_p), 64))
        with pytest.raises(B.BackendError):
            B.check(lib.gi_inception_features(h, C.cast(buf, C.c_void_p), 1, 1, 2, 2, C.cast(buf, C.c_void_p)))
    finally:
        lib.gi_inception_destroy(h)
    if not torch.cuda.is_available():
        inception, _ = _fid()
        with pytest.raises(B.BackendError):
            inception.InceptionV3()(torch.zeros(1, 1, 16, 16))


@pytest.mark.parametrize("name", list(R.FRECHET_CASES))
def test_frechet_distance_matches_the_reference_value(name):
    _, fid_score = _fid()
    fx = load("fid_frechet")
    m1, s1, m2, s2 = R.frechet_case(name)
    check = np.array([m1.sum(), np.trace(s1), m2.sum(), np.trace(s2)])
    assert np.allclose(check, fx[f"{name}_check"], rtol=1e-9, atol=1e-9), "the regenerated pair is not the recorded one"
    if name == "d64":
        m1, s1, m2, s2 = (fx[f"d64_{k}"] for k in ("mu1", "sigma1", "mu2", "sigma2"))
    got, ref = fid_score.calculate_frechet_distance(m1, s1, m2, s2), float(fx[f"{name}_value"])
    rel = abs(got - ref) / abs(ref)
    print(f"frechet {name}: got {got:.12g} reference {ref:.12g} relative difference {rel:.2e}")
    assert rel <= 1e-6


def test_eps_fallback_equals_the_main_formula_on_shifted_covariances(monkeypatch):
    """No input of the fixture's kind makes the reference take its fallback, so the first attempt is forced non-finite here."""
    _, fid_score = _fid()
    fx = load("fid_frechet")
    m1, s1, m2, s2 = (fx[f"d64_{k}"] for k in ("mu1", "sigma1", "mu2", "sigma2"))
    eps = 1e-3
    off = np.eye(64) * eps
    tr_shifted = fid_score._trace_sqrt_product(s1 + off, s2 + off)
    want = float((m1 - m2).dot(m1 - m2) + np.trace(s1) + np.trace(s2) - 2 * tr_shifted)      # fid_score.py:163-179: traces of the UNshifted
    real, calls = fid_score._trace_sqrt_product, []

    def first_fails(a, b):
        calls.append(1)
        return float("nan") if len(calls) == 1 else real(a, b)
    monkeypatch.setattr(fid_score, "_trace_sqrt_product", first_fails)
    got = fid_score.calculate_frechet_distance(m1, s1, m2, s2, eps=eps)
    assert len(calls) == 2 and got == want
    assert abs(got - float(fx["d64_value"])) > 1e-6          # the shift is visible: the fallback was really taken


def test_npz_shortcut(tmp_path):
    inception, fid_score = _fid()
    mu, sigma = np.arange(5.0), np.eye(5) * 2
    p = tmp_path / "stats.npz"
    np.savez(p, mu=mu, sigma=sigma)
    m, s = fid_score._compute_statistics_of_path(str(p), None, 50, 2048, True)
    assert np.array_equal(m, mu) and np.array_equal(s, sigma)


def test_new_symbols_are_declared_and_prototyped():
    import gan_inpainting_amd  # noqa: F401
    from gan_inpainting_amd import backend as B
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "ganinpaint.h")).read(), flags=re.S)
    names = ["gi_inception_create", "gi_inception_destroy", "gi_inception_param_floats", "gi_inception_workspace_bytes",
             "gi_inception_num_tensors", "gi_inception_tensor_desc", "gi_inception_bind", "gi_inception_sync_weights",
             "gi_inception_features", "gi_inception_debug_forward_convs", "gi_fid_stats_acc_doubles", "gi_fid_stats_update",
             "gi_fid_stats_finish", "gi_inception_num_steps", "gi_inception_step_desc", "gi_inception_debug_forward_steps",
             "gi_inception_debug_read"]
    for n in names:
        assert re.search(r"\b%s\s*\(" % n, txt), n
        assert n in B.PROTOTYPES and hasattr(B.lib(), n), n
    assert B.lib().gi_fid_stats_acc_doubles(2048) == 1 + 2048 + 2048 * 2048
    assert "inception.hip" in open(os.path.join(ROOT, "gan-inpainting_amd", "csrc", "build.sh")).read()


def test_step_inventory_equals_the_restated_program():
    """The library's 107-step program (context-free handle) against tests/inception_ref.steps(), entry by entry."""
    inception, _ = _fid()
    import gan_inpainting_amd  # noqa: F401
    from gan_inpainting_amd import backend as B
    lib = B.lib()
    prog = inception.InceptionV3.program()
    assert len(prog) == len(R.STEPS) == 107
    for i, (got, want) in enumerate(zip(prog, R.STEPS)):
        assert got == {k: want[k] for k in got}, (i, got, want)
        assert set(got) == {"kind", "conv", "in_chw", "out_chw", "src", "dst", "ldout", "coffout"}
    assert [R.CONVS[p["conv"]][0] for p in prog if p["kind"] == "conv"] == [c[0] for c in R.CONVS]
    h = C.c_void_p()
    B.check(lib.gi_inception_create(None, B.GI_F16, 2, C.byref(h)))
    try:
        assert lib.gi_inception_num_steps(h) == 107 and lib.gi_inception_num_steps(None) == -1
        five = (C.c_int * 5)()
        p = C.cast(five, C.c_void_p)
        for bad in (-1, 107):
            with pytest.raises(B.BackendError):
                B.check(lib.gi_inception_step_desc(h, bad, p, p, p, p, p))
        with pytest.raises(B.BackendError):
            B.check(lib.gi_inception_step_desc(h, 0, p, p, None, p, p))
        # the debug entries compute: refused on a context-free handle, on the host
        buf = (C.c_float * 16)()
        with pytest.raises(B.BackendError):
            B.check(lib.gi_inception_debug_forward_steps(h, C.cast(buf, C.c_void_p), 1, 1, 2, 2, 0))
        with pytest.raises(B.BackendError):
            B.check(lib.gi_inception_debug_read(h, 0, 0, 1, C.cast(buf, C.c_void_p)))
    finally:
        lib.gi_inception_destroy(h)


def test_train_flag_defaults_off():
    src = open(os.path.join(ROOT, "gan-inpainting_amd", "train.py")).read()
    assert '"--fid-weights"' in src and 'default=""' in src
    import gan_inpainting_amd  # noqa: F401
    from gan_inpainting_amd.lib.models import evaluate
    assert evaluate._no_fid_stats((-1, -1)) and evaluate._no_fid_stats(None) and evaluate._no_fid_stats(-1)
    assert not evaluate._no_fid_stats((np.zeros(3), np.eye(3)))
