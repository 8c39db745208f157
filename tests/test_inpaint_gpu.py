"""GPU tier of lib.inpaint.Inpainter and the inpaint.py command: everything around the generator equals the numpy restatement
(tests/imageout_ref.py) bit for bit when that is fed the device generator's own output (the generator against the oracle is pinned
in tests/test_nets_gpu.py, so no floating-point tolerance appears here), plus the edge cases and the command line."""
import numpy as np
import pytest
import torch

import imageout_ref as R

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
    """Smooth content plus noise: resampling and blending have something to get wrong."""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:H, 0:W]
    a = 120 + 80 * np.sin(y / 9.0 + seed) * np.cos(x / 13.0) + rng.integers(-30, 31, (H, W))
    return np.clip(a, 0, 255).astype(np.uint8)


def _rect_mask(H, W, y0, x0, h, w, value=255):
    m = np.zeros((H, W), np.uint8)
    m[y0:y0 + h, x0:x0 + w] = value
    return m


def _run(inp, imgs, masks):
    out = inp([torch.from_numpy(i).cuda() for i in imgs], [torch.from_numpy(m).cuda() for m in masks])
    return [o.cpu().numpy() for o in out]


def _check_against_restatement(inp, img, mask, feather=FEATHER):
    """One image through the device chain with the capture on; returns (device result, window, masked, m, generator output)."""
    inp.capture = {}
    got = _run(inp, [img], [mask])[0]
    cap, inp.capture = inp.capture, None
    win = cap["windows"][0]
    assert win == R.plan_window(img.shape[0], img.shape[1], R.bbox(mask), S, CONTEXT, feather)
    masked, m = R.model_input(img, mask, win, S)
    d_masked, d_m, d_out = (cap[k][0][0, 0].cpu().numpy() for k in ("masked", "mask", "output"))
    assert np.array_equal(d_masked.view(np.uint32), masked.view(np.uint32)), "the model input differs from the restatement"
    assert np.array_equal(d_m.view(np.uint32), m.view(np.uint32)), "the model-size mask differs from the restatement"
    ref, ref_win = R.inpaint_given_generator_output(img, mask, S, CONTEXT, feather, d_out)
    assert ref_win == win
    diff = int((got != ref).sum())
    assert diff == 0, f"{diff} of {ref.size} result bytes differ from the restatement"
    return got, win, masked, m, d_out


def test_chained_parity_and_window_regions(net):
    img, mask = _image(1, 150, 200), _rect_mask(150, 200, 60, 90, 30, 44, value=3)
    got, win, masked, m, out = _check_against_restatement(_inpainter(net), img, mask)
    wy, wx, wh, ww = win
    assert (wh, ww) == (88, 88)                                   # 2 x the 44-pixel hole: the window is resampled both ways
    outside = np.ones(img.shape, bool)
    outside[wy:wy + wh, wx:wx + ww] = False
    assert np.array_equal(got[outside], img[outside])             # outside the window: the original
    patch = R.enlarged_patch(masked, m, out, win)
    hole = mask[wy:wy + wh, wx:wx + ww] != 0
    assert np.array_equal(got[wy:wy + wh, wx:wx + ww][hole], patch[hole])     # inside the hole: the enlarged patch
    assert (got[wy:wy + wh, wx:wx + ww][hole] != img[wy:wy + wh, wx:wx + ww][hole]).mean() > 0.5       # and it did change


def test_scale_one(net):
    """A 64 x 64 image is its own window: no resampling in either direction, hole pixels are q(composite)."""
    img, mask = _image(2, 64, 64), _rect_mask(64, 64, 20, 24, 16, 20)
    got, win, masked, m, out = _check_against_restatement(_inpainter(net), img, mask)
    assert win == (0, 0, 64, 64)
    assert np.array_equal(masked, (img.astype(np.float32) / np.float32(255.0)) * (1 - m))
    comp = R.quantize(masked + out * m)
    assert np.array_equal(got[mask != 0], comp[mask != 0])


def test_empty_mask_costs_no_forward(net):
    inp = _inpainter(net)
    img = _image(3, 70, 90)
    got = _run(inp, [img], [np.zeros_like(img)])[0]
    assert np.array_equal(got, img) and inp.forward_calls == 0
    _run(inp, [img], [_rect_mask(70, 90, 10, 10, 9, 9)])
    assert inp.forward_calls == 1


def test_hole_at_the_corner_and_narrow_image(net):
    inp = _inpainter(net)
    img = _image(4, 150, 200)
    _check_against_restatement(inp, img, _rect_mask(150, 200, 0, 0, 25, 31))
    _check_against_restatement(inp, img, _rect_mask(150, 200, 130, 170, 20, 30))
    narrow = _image(5, 40, 300)                                    # shorter than S: the window is 40 rows, enlarged to 64
    got, win, *_ = _check_against_restatement(inp, narrow, _rect_mask(40, 300, 5, 100, 26, 60))
    assert win[2] == 40 and win[3] == 120
    _check_against_restatement(_inpainter(net, feather=0), img, _rect_mask(150, 200, 40, 50, 20, 20), feather=0)


def test_mixed_sizes_in_one_call(net):
    imgs = [_image(6, 150, 200), _image(7, 96, 70), _image(8, 64, 64)]
    masks = [_rect_mask(150, 200, 30, 40, 33, 21), np.zeros((96, 70), np.uint8), _rect_mask(64, 64, 8, 8, 12, 30)]
    inp = _inpainter(net)
    together = _run(inp, imgs, masks)
    assert inp.forward_calls == 1                                  # two windows, one forward
    for i in range(3):
        alone = _run(_inpainter(net), [imgs[i]], [masks[i]])[0]
        assert np.array_equal(together[i], alone), i
    one_by_one = _run(_inpainter(net, batch=1), imgs, masks)
    assert all(np.array_equal(a, b) for a, b in zip(together, one_by_one))


def _write(path, a):
    from PIL import Image
    Image.fromarray(a, mode="L").save(path)


def _read(path):
    from PIL import Image
    with Image.open(path) as im:
        assert im.mode == "L"
        return np.asarray(im).copy()


def test_command_line(net, tmp_path):
    from gan_inpainting_amd import inpaint as cli
    imgs = {"a": _image(9, 90, 130), "b": _image(10, 64, 80)}
    masks = {"a": _rect_mask(90, 130, 20, 30, 25, 35), "b": _rect_mask(64, 80, 30, 5, 14, 40)}
    (tmp_path / "img").mkdir()
    (tmp_path / "mask").mkdir()
    for k in imgs:
        _write(tmp_path / "img" / f"{k}.png", imgs[k])
        _write(tmp_path / "mask" / f"{k}.png", masks[k])
    torch.save({k: v.cpu() for k, v in net.state_dict().items()}, tmp_path / "epoch1_G.pt")
    out = tmp_path / "out"
    written = cli.main(["-m", str(tmp_path / "epoch1_G.pt"), "-i", str(tmp_path / "img"), "--mask", str(tmp_path / "mask"), "-o", str(out),
                        "--imagedim", str(S), "--dtype", "fp32", "--context", str(CONTEXT), "--feather", str(FEATHER), "--batchsize", "4",
                        "--panel"])
    assert [w.split("/")[-1] for w in written] == ["a.png", "b.png"]
    want = _run(_inpainter(net), [imgs["a"], imgs["b"]], [masks["a"], masks["b"]])
    for k, w in zip(("a", "b"), want):
        assert np.array_equal(_read(out / f"{k}.png"), w), k
        H, W = imgs[k].shape
        panel = _read(out / f"{k}_panel.png")
        assert panel.shape == (H + 4, 3 * (W + 2) + 2)
        assert np.array_equal(panel[2:2 + H, 2:2 + W], imgs[k])                           # first tile: the original
        assert np.array_equal(panel[2:2 + H, 4 + W:4 + 2 * W], imgs[k] * (masks[k] == 0))
        assert np.array_equal(panel[2:2 + H, 6 + 2 * W:6 + 3 * W], w)
        assert (panel[:2] == 255).all() and (panel[:, :2] == 255).all()
    # generated holes: one file, --masks
    one = cli.main(["-m", str(tmp_path / "epoch1_G.pt"), "-i", str(tmp_path / "img" / "a.png"), "--masks", "rect", "--mask-seed", "4",
                    "-o", str(tmp_path / "out2"), "--imagedim", str(S), "--dtype", "fp32"])
    res = _read(one[0])
    assert res.shape == imgs["a"].shape and (res != imgs["a"]).any()


def test_refusals(tmp_path):
    from gan_inpainting_amd import inpaint as cli
    base = ["-m", "x.pt", "-i", str(tmp_path), "-o", str(tmp_path / "o")]
    with pytest.raises(SystemExit):
        cli.main(base + ["--mask", "m.png", "--masks", "rect"])
    with pytest.raises(SystemExit):
        cli.main(base)
    with pytest.raises(NotImplementedError):
        cli.main(base + ["--mask", "m.png", "-g", "vgg19"])
    big = np.zeros((8, 20), np.uint8)
    _write(tmp_path / "tiny.png", big)
    with pytest.raises(SystemExit, match="16 .. 4096"):
        cli.main(["-m", "x.pt", "-i", str(tmp_path / "tiny.png"), "-o", str(tmp_path / "o"), "--masks", "freeform"])
