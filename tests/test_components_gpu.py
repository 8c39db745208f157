"""GPU tier of gi_mask_components (csrc/components.hip): labels, count and table equal the Python restatement
(tests/components_ref.py) exactly, at both connectivities, at sizes around the tile and patterns aimed at the places a tiled
union-find goes wrong: diagonal contact across the corner where four tiles meet, components that cross many tile borders back and
forth, and sizes that are no multiple of the tile or of 4."""
import functools
import os

import numpy as np
import pytest
import torch

import components_ref as CR

pytestmark = pytest.mark.gpu

TILE = 64                     # CT of csrc/components.hip: the side of the LDS tile
FILL = 0x5A5A5A5A
GUARD = 16                    # int32 words behind every output that must keep the fill
SIZES = [(1, 1), (1, 257), (257, 1), (2, 2), (63, 65), (64, 64), (65, 63), (130, 257), (200, 333), (512, 512)]
PATTERNS = ["empty", "full", "corners", "checkerboard", "diagonal", "anti_diagonal", "diag_contact", "anti_diag_contact", "serpentine", "rings",
            "random0.1", "random0.4", "random0.6"]


def _mods():
    import gan_inpainting_amd  # noqa: F401
    from gan_inpainting_amd import backend as B
    from gan_inpainting_amd.lib import imageout
    return B, imageout


def test_the_largest_size_has_three_tiles_each_way():
    H, W = SIZES[-1]
    assert H // TILE >= 3 and W // TILE >= 3
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = open(os.path.join(root, "gan-inpainting_amd", "csrc", "components.hip")).read()
    assert f"constexpr int CT = {TILE};" in src, "TILE of this test is the kernel's tile side"


@functools.lru_cache(maxsize=None)
def _reference(name, H, W, conn):
    labels, count, table = CR.components(CR.pattern(name, H, W, TILE), conn, cap=1 << 30)
    for a in (labels, table):
        a.setflags(write=False)
    return labels, count, table


def _values(mask, seed):
    """The hole bytes drawn from {1, 128, 255}: any nonzero byte is a hole."""
    rng = np.random.default_rng(seed)
    return (mask * rng.choice(np.array([1, 128, 255], np.uint8), size=mask.shape)).astype(np.uint8)


def _call(mask, conn, cap, offset=0):
    """The raw entry on a mask `offset` bytes past an aligned allocation, every output pre-filled and followed by a guard; returns
    the status and the three buffers (int32 numpy, guards included)."""
    B, _ = _mods()
    lib = B.lib()
    H, W = mask.shape
    buf = torch.zeros(H * W + offset + 8, dtype=torch.uint8, device="cuda")
    buf[offset:offset + H * W] = torch.from_numpy(np.ascontiguousarray(mask).reshape(-1)).cuda()
    labels = torch.full((H * W + GUARD,), FILL, dtype=torch.int32, device="cuda")
    count = torch.full((1 + GUARD,), FILL, dtype=torch.int32, device="cuda")
    table = torch.full((cap * 6 + GUARD,), FILL, dtype=torch.int32, device="cuda")
    nbytes = int(lib.gi_mask_components_workspace_bytes(H, W, cap))
    assert nbytes > 0
    ws = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    st = lib.gi_mask_components(B.get_ctx(), buf.data_ptr() + offset, H, W, conn, cap, labels.data_ptr(), count.data_ptr(), table.data_ptr(), ws.data_ptr())
    return st, labels.cpu().numpy(), count.cpu().numpy(), table.cpu().numpy()


def _check(mask, ref, conn, cap, offset=0, what=""):
    ref_labels, ref_count, ref_table = ref
    H, W = mask.shape
    st, labels, count, table = _call(mask, conn, cap, offset)
    assert st == 0, what
    assert int(count[0]) == ref_count, f"{what}: count {int(count[0])}, restatement {ref_count}"
    bad = int((labels[:H * W].reshape(H, W) != ref_labels).sum())
    assert bad == 0, f"{what}: {bad} of {H * W} labels differ from the restatement"
    rows = min(ref_count, cap)
    assert np.array_equal(table[:rows * 6].reshape(rows, 6), ref_table[:rows]), f"{what}: table rows differ"
    assert (table[rows * 6:] == FILL).all(), f"{what}: table rows beyond min(count, cap) or the guard were written"
    assert (labels[H * W:] == FILL).all() and (count[1:] == FILL).all(), f"{what}: a guard word was written"
    return labels, count, table


@pytest.mark.parametrize("conn", [4, 8])
@pytest.mark.parametrize("name", PATTERNS)
@pytest.mark.parametrize("H,W", SIZES)
def test_patterns(H, W, name, conn):
    mask = _values(CR.pattern(name, H, W, TILE), H * 1000 + W)
    _check(mask, _reference(name, H, W, conn), conn, 256, what=f"{name} {H}x{W} conn {conn}")


def test_pattern_expectations():
    """The patterns are what they claim (the restatement's counts): a wrong pattern would test nothing."""
    assert _reference("serpentine", 512, 512, 4)[1] == 1 and _reference("serpentine", 512, 512, 8)[1] == 1
    assert _reference("checkerboard", 65, 63, 8)[1] == 1 and _reference("checkerboard", 65, 63, 4)[1] == (65 * 63 + 1) // 2
    corners = (512 // TILE - 1) ** 2
    assert _reference("diag_contact", 512, 512, 8)[1] == corners and _reference("diag_contact", 512, 512, 4)[1] == 2 * corners
    assert _reference("anti_diag_contact", 512, 512, 8)[1] == corners and _reference("anti_diag_contact", 512, 512, 4)[1] == 2 * corners
    assert _reference("diagonal", 512, 512, 8)[1] == 1 and _reference("diagonal", 512, 512, 4)[1] == 512
    assert _reference("rings", 512, 512, 8)[1] == 128
    assert _reference("full", 200, 333, 4)[2].tolist() == [[0, 0, 0, 199, 332, 200 * 333]]


@pytest.mark.parametrize("conn", [4, 8])
@pytest.mark.parametrize("H,W", SIZES)
def test_isolated_pixels_and_cap(H, W, conn):
    """Isolated pixels on every other row and column: the most components a mask can have, with cap below, at and above the count."""
    ref = _reference("isolated", H, W, conn)
    n = ((H + 1) // 2) * ((W + 1) // 2)
    assert ref[1] == n
    mask = _values(CR.pattern("isolated", H, W), 5)
    for cap in sorted({max(n - 1, 1), n, min(n + 1, 65536)}):
        _check(mask, ref, conn, cap, what=f"isolated {H}x{W} conn {conn} cap {cap}")


@pytest.mark.parametrize("offset", [1, 3])
@pytest.mark.parametrize("H,W", [(65, 63), (130, 257)])
def test_mask_alignment(H, W, offset):
    mask = _values(CR.pattern("random0.4", H, W), 9)
    for conn in (4, 8):
        _check(mask, _reference("random0.4", H, W, conn), conn, 256, offset=offset, what=f"offset {offset} {H}x{W} conn {conn}")


def test_two_calls_give_identical_bytes():
    mask = _values(CR.pattern("random0.4", 512, 512), 11)
    a = _check(mask, _reference("random0.4", 512, 512, 8), 8, 4096, what="first call")
    b = _check(mask, _reference("random0.4", 512, 512, 8), 8, 4096, what="second call")
    assert all(np.array_equal(x, y) for x, y in zip(a, b))


def test_wrapper_trims_the_table():
    _, io = _mods()
    mask = CR.pattern("random0.1", 130, 257)
    ref_labels, ref_count, ref_table = _reference("random0.1", 130, 257, 8)
    for cap in (7, 65536):
        labels, count, table = io.mask_components(torch.from_numpy(mask * 255).cuda(), 8, cap)
        assert count == ref_count and table.dtype == torch.int32 and labels.dtype == torch.int32
        assert np.array_equal(labels.cpu().numpy(), ref_labels)
        assert np.array_equal(table.cpu().numpy(), ref_table[:min(cap, ref_count)])
    labels, count, table = io.mask_components(torch.zeros((5, 7), dtype=torch.uint8, device="cuda"))
    assert count == 0 and tuple(table.shape) == (0, 6) and int((labels != -1).sum()) == 0


def test_invalid_arguments():
    B, _ = _mods()
    lib, ctx = B.lib(), B.get_ctx()
    INVALID = -1                            # GI_ERR_INVALID
    m = torch.zeros((16, 16), dtype=torch.uint8, device="cuda")
    out = torch.zeros(16 * 16 + 8 * 6 + 64, dtype=torch.int32, device="cuda")
    ws = torch.zeros(int(lib.gi_mask_components_workspace_bytes(16, 16, 8)), dtype=torch.uint8, device="cuda")
    lab, cnt, tab = out.data_ptr(), out.data_ptr() + 4 * 256, out.data_ptr() + 4 * 272
    good = (m.data_ptr(), 16, 16, 8, 8, lab, cnt, tab, ws.data_ptr())

    def call(**kw):
        a = dict(zip(("mask", "H", "W", "conn", "cap", "labels", "count", "table", "ws"), good))
        a.update(kw)
        return lib.gi_mask_components(ctx, *a.values())

    assert call() == 0
    for name in ("mask", "labels", "count", "table", "ws"):
        assert call(**{name: None}) == INVALID, name
    assert lib.gi_mask_components(None, *good) == INVALID
    for conn in (0, 6, 9, -8):
        assert call(conn=conn) == INVALID
    for cap in (0, -1, 65537):
        assert call(cap=cap) == INVALID
    assert call(H=0) == INVALID and call(W=-3) == INVALID
    assert call(H=65536, W=65536) == INVALID and call(H=46341, W=46341) == INVALID          # H * W >= 2^31 - 32
    assert b"mask_components" in lib.gi_last_error()
    assert lib.gi_mask_components_workspace_bytes(65536, 65536, 8) == 0 and lib.gi_mask_components_workspace_bytes(16, 16, 0) == 0
    torch.cuda.synchronize()
    assert int(out[256:].sum()) == 0        # the refused calls wrote nothing (the valid one: an empty mask, count 0, no table row)
