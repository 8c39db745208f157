"""CPU tier of the image-output path: the numpy restatement (tests/imageout_ref.py) against literal definitions, the properties of
lib.inpaint.plan_window, the restated enlargement against Pillow itself, and the PNG writer."""
import numpy as np

import imageout_ref as R


def test_box_count_equals_nested_loops():
    rng = np.random.default_rng(1)
    hole = (rng.random((9, 11)) < 0.3).astype(np.uint8) * 255
    for r in (0, 1, 2, 5):
        ref = np.zeros((9, 11), np.int64)
        for y in range(9):
            for x in range(11):
                for yy in range(y - r, y + r + 1):
                    for xx in range(x - r, x + r + 1):
                        if 0 <= yy < 9 and 0 <= xx < 11 and hole[yy, xx]:
                            ref[y, x] += 1
        assert np.array_equal(R.box_count(hole, r), ref), r


def test_feather_ramp_at_a_straight_edge():
    """Hole = the left half of a tall, wide window; on a middle row the weight at distance d = 1 .. r from the edge is
    2 (2r+1) (r+1-d) / A = 2a / A, and 0 from distance r + 1 on. r = 4: 0.889, 0.667, 0.444, 0.222, 0."""
    for r in (1, 4, 9):
        hole = np.zeros((4 * r + 9, 4 * r + 10), np.uint8)
        edge = 2 * r + 5                     # hole columns [0, edge)
        hole[:, :edge] = 1
        alpha, A = R.feather_alpha(hole, r)
        row = alpha[2 * r + 4]
        assert np.all(row[:edge] == A)
        for d in range(1, r + 4):
            a = (2 * r + 1) * max(r + 1 - d, 0)
            assert row[edge - 1 + d] == min(A, 2 * a), (r, d)
        assert row[edge + r] == 0 and row[edge + r - 1] > 0
    alpha, A = R.feather_alpha(np.pad(np.ones((30, 12), np.uint8), ((0, 0), (0, 18))), 4)
    assert [round(v / A, 3) for v in alpha[15, 12:17]] == [0.889, 0.667, 0.444, 0.222, 0.0]


def test_feather_r0_is_a_hard_paste():
    rng = np.random.default_rng(2)
    orig = rng.integers(0, 256, (12, 15), dtype=np.uint8)
    mask = (rng.random((12, 15)) < 0.4).astype(np.uint8)
    patch = rng.integers(0, 256, (7, 9), dtype=np.uint8)
    win = (3, 4, 7, 9)
    out = R.feather_paste(orig, mask, win, patch, 0)
    exp = orig.copy()
    sub = exp[3:10, 4:13]
    sub[mask[3:10, 4:13] != 0] = patch[mask[3:10, 4:13] != 0]
    assert np.array_equal(out, exp)


def test_quantize_round_trips_every_byte():
    v = np.arange(256, dtype=np.uint8)
    assert np.array_equal(R.quantize(v.astype(np.float32) / np.float32(255.0)), v)
    x = np.array([-0.0, -1.0, 2.0, np.inf, -np.inf, np.nan, 0.5 / 255, 1.5 / 255, 2.5 / 255], np.float32)
    assert R.quantize(x).tolist()[:6] == [0, 0, 255, 255, 0, 0]


def _check_window(H, W, box, S, context, feather, win):
    y0, x0, y1, x1 = box
    wy, wx, wh, ww = win
    assert 0 <= wy and 0 <= wx and wy + wh <= H and wx + ww <= W and wh > 0 and ww > 0          # inside the image
    assert wy <= y0 and y1 < wy + wh and wx <= x0 and x1 < wx + ww                                # contains the box
    for lo_gap, at_edge in ((y0 - wy, wy == 0), (wy + wh - 1 - y1, wy + wh == H), (x0 - wx, wx == 0), (wx + ww - 1 - x1, wx + ww == W)):
        assert at_edge or lo_gap >= feather + 1, (H, W, box, S, context, feather, win)           # margin on interior borders


def test_plan_window_properties():
    import gan_inpainting_amd  # noqa: F401
    from gan_inpainting_amd.lib.inpaint import plan_window
    rng = np.random.default_rng(3)
    for _ in range(20000):
        H, W = int(rng.integers(1, 400)), int(rng.integers(1, 400))
        y0, x0 = int(rng.integers(0, H)), int(rng.integers(0, W))
        y1, x1 = int(rng.integers(y0, H)), int(rng.integers(x0, W))
        S, feather = int(rng.choice([64, 128])), int(rng.integers(0, 64))
        context = float(rng.choice([1.0, 1.5, 2.0, 3.0]))
        win = plan_window(H, W, (y0, x0, y1, x1), S, context, feather)
        _check_window(H, W, (y0, x0, y1, x1), S, context, feather, win)
        assert win == plan_window(H, W, (y0, x0, y1, x1), S, context, feather) == R.plan_window(H, W, (y0, x0, y1, x1), S, context, feather)
    assert plan_window(1, 1, (0, 0, 0, 0), 64, 2.0, 8) == (0, 0, 1, 1)                   # a 1 x 1 image
    assert plan_window(90, 70, (0, 0, 89, 69), 64, 2.0, 8) == (0, 0, 90, 70)             # the hole is the image
    win = plan_window(40, 300, (5, 100, 30, 220), 64, 2.0, 8)                            # wider than the short edge
    assert win[0] == 0 and win[2] == 40 and win[3] == 242
    _check_window(40, 300, (5, 100, 30, 220), 64, 2.0, 8, win)
    import pytest
    with pytest.raises(ValueError):
        plan_window(10, 10, (10, 10, -1, -1), 64, 2.0, 8)


def test_restated_enlargement_equals_pillow():
    from PIL import Image
    from oracle import resize_ref as rr
    rng = np.random.default_rng(4)
    a = rng.integers(0, 256, (64, 64), dtype=np.uint8)
    ref = np.asarray(Image.fromarray(a).resize((80, 96), Image.BILINEAR))
    assert ref.shape == (96, 80) and np.array_equal(rr.resize_bilinear_u8(a, 96, 80), ref)


def test_png_round_trip(tmp_path):
    import gan_inpainting_amd  # noqa: F401
    from gan_inpainting_amd.lib import imageout
    from gan_inpainting_amd.lib.data.dataset import pil_loader
    rng = np.random.default_rng(5)
    a = rng.integers(0, 256, (37, 53), dtype=np.uint8)
    path = tmp_path / "sub" / "a.png"
    imageout.write_png(str(path), a)
    back = pil_loader(str(path))
    assert back.mode == "L" and np.array_equal(np.asarray(back), a)


def test_chain_with_empty_mask_and_identity_patch():
    rng = np.random.default_rng(6)
    img = rng.integers(0, 256, (50, 70), dtype=np.uint8)
    out, win = R.inpaint_given_generator_output(img, np.zeros_like(img), 64, 2.0, 8, np.zeros((64, 64), np.float32))
    assert win is None and np.array_equal(out, img)
    mask = np.zeros_like(img)
    mask[10:20, 30:45] = 7
    out, win = R.inpaint_given_generator_output(img, mask, 64, 2.0, 3, np.full((64, 64), 0.5, np.float32))
    assert win == R.plan_window(50, 70, (10, 30, 19, 44), 64, 2.0, 3)
    outside = np.ones_like(img, bool)
    outside[win[0]:win[0] + win[2], win[1]:win[1] + win[3]] = False
    assert np.array_equal(out[outside], img[outside])
    far = R.box_count(mask, 3) == 0
    assert np.array_equal(out[far], img[far])                    # weight 0 beyond the feather
