"""GPU tier of the image-output kernels (csrc/imageout.hip): exact equality with the numpy restatement (tests/imageout_ref.py) at
every path the kernels distinguish - vector and byte paths, ragged rows, partial tiles, halos that cross workgroup tiles - and
the argument checks."""
import ctypes as C

import numpy as np
import pytest
import torch

import imageout_ref as R

pytestmark = pytest.mark.gpu


def _mods():
    import gan_inpainting_amd  # noqa: F401
    from gan_inpainting_amd import backend as B
    from gan_inpainting_amd.lib import imageout
    return B, imageout


def _same_bytes(got, ref, what):
    got = got.cpu().numpy().view(np.uint8)
    ref = np.ascontiguousarray(ref).view(np.uint8)
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    diff = int((got != ref).sum())
    assert diff == 0, f"{what}: {diff} of {ref.size} bytes differ from the restatement"


# ---- quantize -------------------------------------------------------------------------------------------------------------------
def _quantize_inputs():
    k = np.arange(256, dtype=np.float32)
    quot = k / np.float32(255.0)
    half = ((np.arange(255, dtype=np.float64) + 0.5) / 255.0).astype(np.float32)       # the rounding boundaries
    near = np.concatenate([np.nextafter(half, np.float32(-1)), half, np.nextafter(half, np.float32(2))])
    special = np.array([-0.0, -1.0, 2.0, np.inf, -np.inf, np.nan, 0.0, 1.0], np.float32)
    return np.concatenate([quot, near, special]).astype(np.float32)


def test_quantize_values():
    B, io = _mods()
    x = _quantize_inputs()
    _same_bytes(io.quantize(torch.from_numpy(x).cuda()), R.quantize(x), "quantize values")
    k = np.arange(256, dtype=np.uint8)
    _same_bytes(io.quantize(torch.from_numpy(k.astype(np.float32) / np.float32(255.0)).cuda()), k, "quantize round trip")


@pytest.mark.parametrize("count", [1, 3, 4, 1023, 4099])
@pytest.mark.parametrize("src_off,dst_off", [(0, 0), (0, 1), (1, 0), (1, 5)])
def test_quantize_counts_and_alignments(count, src_off, dst_off):
    """src_off floats (4 bytes each) and dst_off bytes past a 256-byte aligned allocation: the 16-byte path, the 4-byte loads
    under a 16-byte store, and the ragged head and tail."""
    B, io = _mods()
    rng = np.random.default_rng(count * 7 + src_off + dst_off)
    x = np.resize(np.concatenate([_quantize_inputs(), rng.random(4200, dtype=np.float32) * 1.2 - 0.1]), count + src_off).astype(np.float32)
    src = torch.from_numpy(x).cuda()
    dst = torch.full((count + dst_off + 16,), 0x5A, dtype=torch.uint8, device="cuda")
    B.check(B.lib().gi_image_quantize(B.get_ctx(), src.data_ptr() + 4 * src_off, count, dst.data_ptr() + dst_off))
    ref = np.full(count + dst_off + 16, 0x5A, np.uint8)
    ref[dst_off:dst_off + count] = R.quantize(x[src_off:])
    _same_bytes(dst, ref, f"quantize count {count} offsets {src_off}/{dst_off}")


# ---- panel ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ncol", [1, 4, 8])
@pytest.mark.parametrize("H,W", [(16, 16), (5, 7)])
@pytest.mark.parametrize("g", [0, 2])
def test_panel(ncol, H, W, g):
    B, io = _mods()
    n = 3
    rng = np.random.default_rng(ncol * 100 + H + g)
    cols = [(rng.random((n, 1, H, W), dtype=np.float32) * 1.4 - 0.2).astype(np.float32) for _ in range(ncol)]
    dev = [torch.from_numpy(c).cuda() for c in cols]
    Hc, Wc = io.panel_shape(ncol, n, H, W, g)
    assert (Hc, Wc) == (n * (H + g) + g, ncol * (W + g) + g)
    canvas = torch.full((Hc * Wc + 8,), 0x5A, dtype=torch.uint8, device="cuda")       # every byte must be written; none beyond
    ptrs = (C.c_void_p * ncol)(*[d.data_ptr() for d in dev])
    for off in (0, 3):                                                                   # rows that start on and off a word boundary
        canvas.fill_(0x5A)
        B.check(B.lib().gi_panel_assemble(B.get_ctx(), C.cast(ptrs, C.c_void_p), ncol, n, H, W, g, canvas.data_ptr() + off))
        ref = np.full(Hc * Wc + 8, 0x5A, np.uint8)
        ref[off:off + Hc * Wc] = R.panel(cols, g).reshape(-1)
        _same_bytes(canvas, ref, f"panel ncol {ncol} {H}x{W} g {g} offset {off}")
    _same_bytes(io.assemble_panel(dev, gutter=g), R.panel(cols, g), "assemble_panel")


# ---- bbox -----------------------------------------------------------------------------------------------------------------------
def _bbox_masks(H, W, value):
    """empty, full, one pixel at each corner, two separated blobs (as far as the size allows)."""
    z = np.zeros((H, W), np.uint8)
    out = [z.copy(), np.full((H, W), value, np.uint8)]
    for y, x in ((0, 0), (0, W - 1), (H - 1, 0), (H - 1, W - 1)):
        m = z.copy()
        m[y, x] = value
        out.append(m)
    m = z.copy()
    m[H // 5:H // 5 + max(1, H // 8), W // 6:W // 6 + max(1, W // 9)] = value
    m[(3 * H) // 4:(3 * H) // 4 + max(1, H // 10), (2 * W) // 3:(2 * W) // 3 + max(1, W // 7)] = value
    out.append(m)
    return out


@pytest.mark.parametrize("H,W", [(1, 1), (5, 7), (64, 64), (130, 257)])
@pytest.mark.parametrize("value", [1, 255])
def test_bbox(H, W, value):
    B, io = _mods()
    masks = _bbox_masks(H, W, value)
    ref = np.array([R.bbox(m) for m in masks], np.int32)
    for lo in (0, 3):                       # n = 4 masks per launch; odd H * W puts the later images off every alignment
        batch = np.stack(masks[lo:lo + 4])
        got = io.mask_bbox(torch.from_numpy(batch).cuda())
        assert got.dtype == torch.int32 and np.array_equal(got.cpu().numpy(), ref[lo:lo + 4]), (H, W, lo, got.cpu().tolist(), ref[lo:lo + 4].tolist())
    assert R.bbox(masks[0]) == (H, W, -1, -1)


# ---- crop -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("binarize", [False, True])
def test_crop(binarize):
    B, io = _mods()
    H, W = 40, 57
    rng = np.random.default_rng(11)
    src = rng.integers(0, 4, (H, W), dtype=np.uint8) * rng.integers(0, 86, (H, W), dtype=np.uint8)
    dev = torch.from_numpy(src).cuda()
    for win in ((0, 0, 13, 21), (0, W - 21, 13, 21), (H - 13, 0, 13, 21), (H - 13, W - 21, 13, 21), (7, 5, 20, 33), (0, 0, H, W), (39, 56, 1, 1)):
        _same_bytes(io.window_crop(dev, win, binarize=binarize), R.crop(src, win, binarize), f"crop {win} binarize {binarize}")


# ---- feather paste --------------------------------------------------------------------------------------------------------------
def _freeform(H, W, seed):
    from gan_inpainting_amd.lib.data.masks import DeviceMaskGenerator
    m = DeviceMaskGenerator("freeform", H, W, seed)(torch.tensor([3], dtype=torch.int64))
    return (m[0, 0] * 255).to(torch.uint8).cpu().numpy()


def _holes(H, W, win):
    """Whole-image masks (holes outside the window must not count): one pixel, a rectangle on the window border, the whole
    window and more, free-form strokes."""
    wy, wx, wh, ww = win
    one = np.zeros((H, W), np.uint8)
    one[wy + wh // 2, wx + ww // 3] = 1
    rect = np.zeros((H, W), np.uint8)
    rect[wy:wy + max(1, wh // 3), max(0, wx - 2):wx + max(1, ww // 2)] = 200
    return {"pixel": one, "rect": rect, "all": np.full((H, W), 255, np.uint8), "freeform": _freeform(max(H, 16), max(W, 16), 5)[:H, :W]}


def _paste_case(H, W, win, r, mask, seed):
    B, io = _mods()
    rng = np.random.default_rng(seed)
    orig = rng.integers(0, 256, (H, W), dtype=np.uint8)
    patch = rng.integers(0, 256, (win[2], win[3]), dtype=np.uint8)
    got = io.feather_paste(torch.from_numpy(orig).cuda(), torch.from_numpy(mask).cuda(), win, torch.from_numpy(patch).cuda(), r)
    ref = R.feather_paste(orig, mask, win, patch, r)
    _same_bytes(got, ref, f"feather_paste {H}x{W} window {win} r {r}")
    outside = np.ones((H, W), bool)
    outside[win[0]:win[0] + win[2], win[1]:win[1] + win[3]] = False
    assert np.array_equal(got.cpu().numpy()[outside], orig[outside])         # only the window is written


WINDOWS = [(8, 11, 24, 33), (0, 11, 24, 33), (16, 11, 24, 33), (8, 0, 24, 33), (8, 23, 24, 33), (0, 0, 40, 56)]


@pytest.mark.parametrize("r", [0, 1, 3, 63])
@pytest.mark.parametrize("hole", ["pixel", "rect", "all", "freeform"])
def test_feather_paste_small(r, hole):
    for i, win in enumerate(WINDOWS):
        _paste_case(40, 56, win, r, _holes(40, 56, win)[hole], 100 * r + i)


def test_feather_paste_halo_across_tiles():
    """(300, 520) image, (260, 400) window, r = 63: 5 x 7 workgroup tiles, partial last tiles, every halo reaches the neighbours."""
    win = (20, 60, 260, 400)
    _paste_case(300, 520, win, 63, _freeform(300, 520, 9), 7)
    _paste_case(300, 520, win, 8, _holes(300, 520, win)["rect"], 8)


# ---- argument checks ------------------------------------------------------------------------------------------------------------
def test_invalid_arguments():
    B, io = _mods()
    lib, ctx = B.lib(), B.get_ctx()
    INVALID = -1                            # GI_ERR_INVALID
    u8 = torch.zeros((16, 16), dtype=torch.uint8, device="cuda")
    f32 = torch.zeros((1, 1, 16, 16), dtype=torch.float32, device="cuda")
    box = torch.zeros(4, dtype=torch.int32, device="cuda")
    p, q, fp = u8.data_ptr(), u8.clone().data_ptr(), f32.data_ptr()
    assert lib.gi_feather_paste(ctx, p, p, 16, 16, 0, 0, 16, 16, p, 64, q) == INVALID          # r = 64
    assert lib.gi_feather_paste(ctx, p, p, 16, 16, 0, 0, 16, 16, p, -1, q) == INVALID
    assert lib.gi_feather_paste(ctx, p, p, 16, 16, 4, 4, 13, 8, p, 2, q) == INVALID            # the window leaves the image
    assert lib.gi_feather_paste(ctx, p, None, 16, 16, 0, 0, 16, 16, p, 2, q) == INVALID
    assert lib.gi_window_crop(ctx, p, 16, 16, 0, 9, 16, 8, 0, q) == INVALID
    assert lib.gi_window_crop(ctx, p, 16, 16, -1, 0, 4, 4, 0, q) == INVALID
    assert lib.gi_window_crop(ctx, None, 16, 16, 0, 0, 4, 4, 0, q) == INVALID
    ptrs9 = (C.c_void_p * 9)(*([fp] * 9))
    assert lib.gi_panel_assemble(ctx, C.cast(ptrs9, C.c_void_p), 9, 1, 16, 16, 2, q) == INVALID  # ncol = 9
    assert lib.gi_panel_assemble(ctx, C.cast(ptrs9, C.c_void_p), 0, 1, 16, 16, 2, q) == INVALID
    assert lib.gi_panel_assemble(ctx, None, 1, 1, 16, 16, 2, q) == INVALID
    null1 = (C.c_void_p * 1)(None)
    assert lib.gi_panel_assemble(ctx, C.cast(null1, C.c_void_p), 1, 1, 16, 16, 2, q) == INVALID
    assert lib.gi_mask_bbox(ctx, None, 1, 16, 16, box.data_ptr()) == INVALID
    assert lib.gi_mask_bbox(ctx, p, 1, 65536, 65536, box.data_ptr()) == INVALID                 # H * W >= 2^31
    assert lib.gi_image_quantize(ctx, None, 4, q) == INVALID
    assert lib.gi_image_quantize(ctx, fp, 0, q) == INVALID
    assert b"image_quantize" in lib.gi_last_error()
    torch.cuda.synchronize()
    assert int(u8.sum()) == 0
