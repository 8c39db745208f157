"""GPU tier of Inpainter(windows="per-hole"): one window per group of holes. Every comparison is bit-exact: a
window's result equals a single-window run on the mask that holds that group alone (the folded-BatchNorm forward is per sample, and
tests/test_inpaint_gpu.py pins batched against separate calls), and the default windows="single" is the path of DESIGN.md 4.10."""
import numpy as np
import pytest
import torch

import imageout_ref as R
from components_ref import CHAIN

pytestmark = pytest.mark.gpu

S, CONTEXT, FEATHER = 64, 2.0, 5


@pytest.fixture(scope="module")
def net():
    import gan_inpainting_amd  # noqa: F401
    from gan_inpainting_amd.lib.models import networks
    torch.manual_seed(1234)
    g = networks.UnetGenerator(1, 1, 6, ngf=64, use_dropout="False", dtype="fp32")     # the smallest U-Net: 64 x 64
    return g.to("cuda:0").eval()


def _inpainter(net, **kw):
    from gan_inpainting_amd.lib.inpaint import Inpainter
    args = dict(imagedim=S, context=CONTEXT, feather=FEATHER, batch=4)
    args.update(kw)
    return Inpainter(net, **args)


def _image(seed, H, W):
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:H, 0:W]
    a = 120 + 80 * np.sin(y / 9.0 + seed) * np.cos(x / 13.0) + rng.integers(-30, 31, (H, W))
    return np.clip(a, 0, 255).astype(np.uint8)


def _boxes_mask(H, W, boxes, value=255):
    m = np.zeros((H, W), np.uint8)
    for y0, x0, y1, x1 in boxes:
        m[y0:y1 + 1, x0:x1 + 1] = value
    return m


def _run(inp, imgs, masks, capture=False):
    inp.capture = {} if capture else None
    out = inp([torch.from_numpy(i).cuda() for i in imgs], [torch.from_numpy(m).cuda() for m in masks])
    cap, inp.capture = inp.capture, None
    out = [o.cpu().numpy() for o in out]
    return (out, cap) if capture else out


def _window_view(a, win):
    return a[win[0]:win[0] + win[2], win[1]:win[1] + win[3]]


def test_one_hole_equals_single(net):
    img, mask = _image(1, 150, 200), _boxes_mask(150, 200, [(60, 90, 89, 133)], value=3)
    (single,), cap_s = _run(_inpainter(net), [img], [mask], capture=True)
    per = _inpainter(net, windows="per-hole")
    (got,), cap_p = _run(per, [img], [mask], capture=True)
    assert np.array_equal(got, single) and cap_p["windows"] == cap_s["windows"] and per.holes == [(1, 1)] and per.forward_calls == 1
    assert (got != img).any()


def test_two_holes_in_opposite_corners(net):
    H, W = 300, 520
    A, B = (10, 12, 29, 35), (262, 470, 283, 499)
    img = _image(2, H, W)
    per = _inpainter(net, windows="per-hole")
    (got,), cap = _run(per, [img], [_boxes_mask(H, W, [A, B])], capture=True)
    wins = cap["windows"]
    assert len(wins) == 2 and all(w[2:] == (64, 64) for w in wins) and per.holes == [(2, 2)] and per.forward_calls == 1
    assert wins == [R.plan_window(H, W, b, S, CONTEXT, FEATHER) for b in (A, B)]
    (single_all,), cap_s = _run(_inpainter(net), [img], [_boxes_mask(H, W, [A, B])], capture=True)
    assert cap_s["windows"][0][2:] == (H, W)                      # what the single window costs: the whole picture, 520 -> 64
    outside = np.ones((H, W), bool)
    for box, win in zip((A, B), wins):
        (alone,) = _run(_inpainter(net), [img], [_boxes_mask(H, W, [box])])
        assert np.array_equal(_window_view(got, win), _window_view(alone, win)), box
        assert (_window_view(got, win) != _window_view(img, win)).any()
        _window_view(outside, win)[:] = False
    assert np.array_equal(got[outside], img[outside])             # everything else is the original


def test_two_nearby_holes_share_a_window(net):
    H, W = 150, 200
    boxes = [(40, 50, 59, 69), (44, 80, 63, 99)]
    img, mask = _image(3, H, W), _boxes_mask(H, W, boxes, value=128)
    per = _inpainter(net, windows="per-hole")
    (got,), cap = _run(per, [img], [mask], capture=True)
    (single,), cap_s = _run(_inpainter(net), [img], [mask], capture=True)
    assert len(cap["windows"]) == 1 and cap["windows"] == cap_s["windows"] and per.holes == [(2, 1)]
    assert np.array_equal(got, single)


def test_chain_case(net):
    c = CHAIN
    assert (c["S"], c["context"], c["feather"]) == (S, CONTEXT, FEATHER)
    img, mask = _image(4, c["H"], c["W"]), _boxes_mask(c["H"], c["W"], c["boxes"])
    per = _inpainter(net, windows="per-hole")
    (got,), cap = _run(per, [img], [mask], capture=True)
    (single,), cap_s = _run(_inpainter(net), [img], [mask], capture=True)
    assert per.holes == [(3, 1)] and cap["windows"] == cap_s["windows"] == [R.plan_window(c["H"], c["W"], (100, 100, 200, 160), S, CONTEXT, FEATHER)]
    assert np.array_equal(got, single)


def test_more_holes_than_max_holes_takes_the_single_window(net):
    H, W = 300, 520
    boxes = [(10, 12, 29, 35), (262, 470, 283, 499), (150, 250, 160, 262), (20, 400, 30, 410), (250, 30, 270, 50)]
    img, mask = _image(5, H, W), _boxes_mask(H, W, boxes)
    per = _inpainter(net, windows="per-hole", max_holes=4)
    (got,), cap = _run(per, [img], [mask], capture=True)
    (single,), cap_s = _run(_inpainter(net), [img], [mask], capture=True)
    assert per.holes == [(5, 1)] and cap["windows"] == cap_s["windows"] and np.array_equal(got, single)
    at_limit = _inpainter(net, windows="per-hole", max_holes=5)
    _run(at_limit, [img], [mask])
    assert at_limit.holes == [(5, 5)] and at_limit.forward_calls == 2       # five windows, batch 4


def test_mixed_images_and_forward_calls(net):
    imgs = [_image(6, 300, 520), _image(7, 96, 70), _image(8, 150, 200), _image(9, 400, 400)]
    masks = [_boxes_mask(300, 520, [(10, 12, 29, 35), (262, 470, 283, 499), (150, 250, 160, 262)]), np.zeros((96, 70), np.uint8),
             _boxes_mask(150, 200, [(60, 90, 89, 133)]), _boxes_mask(400, 400, CHAIN["boxes"] + [(350, 20, 360, 40)])]
    results = {}
    for batch in (1, 2, 4, 16):
        inp = _inpainter(net, windows="per-hole", batch=batch)
        results[batch], cap = _run(inp, imgs, masks, capture=True)
        assert inp.holes == [(3, 3), (0, 0), (1, 1), (4, 2)]
        assert len(cap["windows"]) == 6 and inp.forward_calls == -(-6 // batch) == len(cap["output"])      # ceil(windows / batch)
    for batch in (1, 2, 4):
        assert all(np.array_equal(a, b) for a, b in zip(results[batch], results[16])), batch
    for i in range(4):
        (alone,) = _run(_inpainter(net, windows="per-hole"), [imgs[i]], [masks[i]])
        assert np.array_equal(results[16][i], alone), i
    assert np.array_equal(results[16][1], imgs[1])


def test_single_is_the_default_and_labels_nothing(net, monkeypatch):
    from gan_inpainting_amd.lib import imageout
    H, W = 300, 520
    boxes = [(10, 12, 29, 35), (262, 470, 283, 499)]
    img, mask = _image(10, H, W), _boxes_mask(H, W, boxes)

    def refuse(*a, **k):
        raise AssertionError("windows='single' labels no components")

    monkeypatch.setattr(imageout, "mask_components", refuse)
    inp = _inpainter(net)
    assert inp.windows == "single"
    (got,), cap = _run(inp, [img], [mask], capture=True)
    assert cap["windows"] == [R.plan_window(H, W, R.bbox(mask), S, CONTEXT, FEATHER)] and inp.holes == [] and inp.forward_calls == 1
    ref, _ = R.inpaint_given_generator_output(img, mask, S, CONTEXT, FEATHER, cap["output"][0][0, 0].cpu().numpy())
    assert np.array_equal(got, ref)                                 # the restatement of DESIGN.md 4.10, unchanged
    with pytest.raises(ValueError):
        _inpainter(net, windows="tiles")
    with pytest.raises(ValueError):
        _inpainter(net, windows="per-hole", max_holes=0)


def test_feather_paste_out(net):
    """out=: the window's bytes go into the given tensor, everything else of it stays; the default still returns a fresh copy."""
    from gan_inpainting_amd.lib import imageout
    rng = np.random.default_rng(3)
    orig = rng.integers(0, 256, (40, 56), dtype=np.uint8)
    mask = _boxes_mask(40, 56, [(12, 20, 18, 30)])
    win = (8, 11, 24, 33)
    patch = rng.integers(0, 256, (24, 33), dtype=np.uint8)
    d_orig, d_mask, d_patch = (torch.from_numpy(a).cuda() for a in (orig, mask, patch))
    ref = R.feather_paste(orig, mask, win, patch, 3)
    base = rng.integers(0, 256, (40, 56), dtype=np.uint8)
    out = torch.from_numpy(base).cuda()
    res = imageout.feather_paste(d_orig, d_mask, win, d_patch, 3, out=out)
    assert res is out
    want = base.copy()
    _window_view(want, win)[:] = _window_view(ref, win)
    assert np.array_equal(out.cpu().numpy(), want)
    fresh = imageout.feather_paste(d_orig, d_mask, win, d_patch, 3)
    assert fresh.data_ptr() != d_orig.data_ptr() and np.array_equal(fresh.cpu().numpy(), ref) and np.array_equal(d_orig.cpu().numpy(), orig)
    with pytest.raises(ValueError):
        imageout.feather_paste(d_orig, d_mask, win, d_patch, 3, out=out[:, :50])


def _write(path, a):
    from PIL import Image
    Image.fromarray(a, mode="L").save(path)


def _read(path):
    from PIL import Image
    with Image.open(path) as im:
        return np.asarray(im).copy()


def test_command_line(net, tmp_path, capsys):
    from gan_inpainting_amd import inpaint as cli
    H, W = 300, 520
    img, mask = _image(11, H, W), _boxes_mask(H, W, [(10, 12, 29, 35), (262, 470, 283, 499)])
    _write(tmp_path / "a.png", img)
    _write(tmp_path / "m.png", mask)
    torch.save({k: v.cpu() for k, v in net.state_dict().items()}, tmp_path / "epoch1_G.pt")
    base = ["-m", str(tmp_path / "epoch1_G.pt"), "-i", str(tmp_path / "a.png"), "--mask", str(tmp_path / "m.png"), "--imagedim", str(S),
            "--dtype", "fp32", "--context", str(CONTEXT), "--feather", str(FEATHER), "--batchsize", "4"]
    written = cli.main(base + ["-o", str(tmp_path / "per"), "--windows", "per-hole"])
    assert "a.png: 2 holes, 2 windows" in capsys.readouterr().out
    (want,) = _run(_inpainter(net, windows="per-hole"), [img], [mask])
    assert np.array_equal(_read(written[0]), want)
    written = cli.main(base + ["-o", str(tmp_path / "capped"), "--windows", "per-hole", "--max-holes", "1"])
    assert "2 holes, 1 windows" in capsys.readouterr().out
    (single,) = _run(_inpainter(net), [img], [mask])
    assert np.array_equal(_read(written[0]), single) and not np.array_equal(single, want)
    written = cli.main(base + ["-o", str(tmp_path / "single")])
    assert capsys.readouterr().out == "" and np.array_equal(_read(written[0]), single)
    for bad in (["--windows", "tiles"], ["--windows", "per-hole", "--max-holes", "0"], ["--max-holes", "65537"], ["--max-holes", "many"]):
        with pytest.raises(SystemExit):
            cli.main(base + ["-o", str(tmp_path / "bad")] + bad)
