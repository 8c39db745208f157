"""Restatement of csrc/components.hip and of lib.inpaint.plan_windows for the tests: connected components of a
mask by a two-pass raster union-find over row runs, a literal flood fill to check that against, the test patterns of the GPU tier,
and window planning written as plain loops. Nothing here imports the package."""
import numpy as np

import imageout_ref as R


# ---- labelling ----------------------------------------------------------------------------------------------------------------------
def components(mask, connectivity=8, cap=256):
    """(labels, count, table): labels (H,W) int32, -1 on background, else the smallest linear index y * W + x of the pixel's
    component (bytes != 0, 4- or 8-connected); count: the number of components; table (min(count, cap), 6) int32, a row
    (label, y0, x0, y1, x1, area) per component in label order, the box inclusive.
    First pass: the runs of every row in raster order, and a union (to the smaller run) of every pair of runs of consecutive rows
    that touch. Second pass: every run takes its root's first pixel."""
    assert connectivity in (4, 8)
    hole = np.asarray(mask) != 0
    H, W = hole.shape
    labels = np.full((H, W), -1, np.int32)
    pad = np.zeros((H, W + 2), bool)
    pad[:, 1:-1] = hole
    ys, xs = np.nonzero(pad[:, 1:] != pad[:, :-1])          # per row: start, end (exclusive), start, end, ...
    ry, rs, re = ys[0::2].astype(np.int64), xs[0::2].astype(np.int64), xs[1::2].astype(np.int64)
    n = ry.size
    if n == 0:
        return labels, 0, np.zeros((0, 6), np.int32)
    c = 1 if connectivity == 8 else 0
    K = W + 4
    # run b of row y touches run a of row y - 1 when a.start < b.end + c and b.start < a.end + c; the runs of a row are sorted
    lo = np.searchsorted((ry + 1) * K + re, ry * K + rs - c, side="right")
    hi = np.searchsorted((ry + 1) * K + rs, ry * K + re + c, side="left")
    cnt = np.maximum(hi - lo, 0)
    b_idx = np.repeat(np.arange(n), cnt)
    a_idx = np.repeat(lo, cnt) + (np.arange(cnt.sum()) - np.repeat(np.cumsum(cnt) - cnt, cnt))
    parent = list(range(n))

    def find(i):
        while parent[i] != i:
            parent[i] = parent[parent[i]]
            i = parent[i]
        return i

    for a, b in zip(a_idx.tolist(), b_idx.tolist()):
        a, b = find(a), find(b)
        if a != b:
            parent[max(a, b)] = min(a, b)
    root = np.array([find(i) for i in range(n)], np.int64)
    run_label = (ry * W + rs)[root]                          # the first run of a component starts at its smallest pixel
    labels.ravel()[np.flatnonzero(hole.ravel())] = np.repeat(run_label, re - rs).astype(np.int32)
    uniq, comp = np.unique(run_label, return_inverse=True)
    count = int(uniq.size)
    tab = np.zeros((count, 6), np.int64)
    tab[:, 0] = uniq
    tab[:, 1], tab[:, 2] = H, W
    tab[:, 3:5] = -1
    np.minimum.at(tab[:, 1], comp, ry)
    np.minimum.at(tab[:, 2], comp, rs)
    np.maximum.at(tab[:, 3], comp, ry)
    np.maximum.at(tab[:, 4], comp, re - 1)
    np.add.at(tab[:, 5], comp, re - rs)
    return labels, count, tab[:min(count, cap)].astype(np.int32)


def flood_fill(mask, connectivity=8):
    """The definition, literally: pixels in raster order, each unlabelled hole pixel floods its component with its own index."""
    hole = np.asarray(mask) != 0
    H, W = hole.shape
    labels = np.full((H, W), -1, np.int32)
    nb = [(-1, 0), (1, 0), (0, -1), (0, 1)] + ([(-1, -1), (-1, 1), (1, -1), (1, 1)] if connectivity == 8 else [])
    rows = []
    for y in range(H):
        for x in range(W):
            if not hole[y, x] or labels[y, x] >= 0:
                continue
            lab = y * W + x
            labels[y, x] = lab
            stack, box, area = [(y, x)], [y, x, y, x], 0
            while stack:
                cy, cx = stack.pop()
                area += 1
                box = [min(box[0], cy), min(box[1], cx), max(box[2], cy), max(box[3], cx)]
                for dy, dx in nb:
                    ny, nx = cy + dy, cx + dx
                    if 0 <= ny < H and 0 <= nx < W and hole[ny, nx] and labels[ny, nx] < 0:
                        labels[ny, nx] = lab
                        stack.append((ny, nx))
            rows.append([lab] + box + [area])
    return labels, len(rows), np.array(rows, np.int32).reshape(-1, 6)


# ---- the masks of the GPU tier --------------------------------------------------------------------------------------------------------
def serpentine(H, W):
    """One component whose path crosses every tile border many times: every other row is full, and consecutive full rows are
    joined by one pixel, at the right and the left end in turn."""
    m = np.zeros((H, W), np.uint8)
    m[0::2] = 1
    for k, y in enumerate(range(1, H, 2)):
        if y + 1 < H:
            m[y, W - 1 if k % 2 == 0 else 0] = 1
    return m


def rings(H, W):
    """Concentric one-pixel rectangles, two pixels apart: min(H, W) / 4 nested components, each crossing every tile it encloses."""
    m = np.zeros((H, W), np.uint8)
    for d in range(0, (min(H, W) + 1) // 2, 2):
        m[d, d:W - d] = m[H - 1 - d, d:W - d] = 1
        m[d:H - d, d] = m[d:H - d, W - 1 - d] = 1
    return m


def diagonal_contacts(H, W, tile):
    """At every interior tile corner (ty, tx): a 3 x 3 blob ending at (ty - 1, tx - 1) and one starting at (ty, tx): they touch only
    diagonally, through the corner where four tiles meet (one component with 8 neighbours, two with 4)."""
    m = np.zeros((H, W), np.uint8)
    for ty in range(tile, H, tile):
        for tx in range(tile, W, tile):
            m[max(ty - 3, 0):ty, max(tx - 3, 0):tx] = 1
            m[ty:ty + 3, tx:tx + 3] = 1
    return m


def anti_diagonal_contacts(H, W, tile):
    """The mirror image: a blob ending at (ty - 1, tx) up-right of one ending at (ty, tx - 1): contact across the corner the other way."""
    m = np.zeros((H, W), np.uint8)
    for ty in range(tile, H, tile):
        for tx in range(tile, W, tile):
            m[max(ty - 3, 0):ty, tx:tx + 3] = 1
            m[ty:ty + 3, max(tx - 3, 0):tx] = 1
    return m


def scratches(H, W, seed, n=5):
    """n short thick strokes (6 .. 24 pixels wide, up to min(H, W) / 16 long) at seeded places: small damage scattered over a scan,
    the case per-hole windows are for (the planning evidence of DESIGN.md 4.12, next to the free-form masks)."""
    rng = np.random.default_rng(seed)
    m = np.zeros((H, W), np.uint8)
    for _ in range(n):
        r = int(rng.integers(3, 13))
        length = int(rng.integers(1, max(2, min(H, W) // 16)))
        y, x = int(rng.integers(0, H)), int(rng.integers(0, W))
        dy, dx = ((0, 1), (1, 0), (1, 1), (1, -1))[int(rng.integers(0, 4))]
        for t in range(0, length, max(1, r)):
            cy, cx = y + dy * t, x + dx * t
            m[max(cy - r, 0):cy + r + 1, max(cx - r, 0):cx + r + 1] = 1
    return m


def pattern(name, H, W, tile=64):
    z = np.zeros((H, W), np.uint8)
    if name == "empty":
        return z
    if name == "full":
        return z + 1
    if name == "corners":
        z[0, 0] = z[0, W - 1] = z[H - 1, 0] = z[H - 1, W - 1] = 1
        return z
    if name == "isolated":
        z[0::2, 0::2] = 1
        return z
    if name == "checkerboard":
        y, x = np.mgrid[0:H, 0:W]
        return ((y + x) % 2 == 0).astype(np.uint8)
    if name == "diagonal":
        k = np.arange(min(H, W))
        z[k, k] = 1                                   # passes exactly through the corners where four tiles meet
        return z
    if name == "anti_diagonal":
        k = np.arange(min(H, W))
        z[k, W - 1 - k] = 1
        return z
    if name == "diag_contact":
        return diagonal_contacts(H, W, tile)
    if name == "anti_diag_contact":
        return anti_diagonal_contacts(H, W, tile)
    if name == "serpentine":
        return serpentine(H, W)
    if name == "rings":
        return rings(H, W)
    if name.startswith("random"):
        density = float(name[len("random"):])
        rng = np.random.default_rng(int(density * 100) * 7919 + H * 31 + W)
        return (rng.random((H, W)) < density).astype(np.uint8)
    raise ValueError(name)


# the chain case of window planning, on the host and on the device: A's and B's windows intersect, C's window meets neither, and
# only the window of A + B reaches C's: one group in the end
CHAIN = dict(H=400, W=400, S=64, context=2.0, feather=5, boxes=[(100, 100, 110, 110), (100, 150, 110, 160), (190, 125, 200, 135)])


# ---- window planning ------------------------------------------------------------------------------------------------------------------
def windows_intersect(a, b):
    return a[0] < b[0] + b[2] and b[0] < a[0] + a[2] and a[1] < b[1] + b[3] and b[1] < a[1] + a[3]


def plan_windows(H, W, boxes, S, context, feather):
    """Groups start as one per box; the lexicographically first pair of groups whose windows share a pixel merges (union of the
    boxes into the first, the second deleted, the window planned again) until no pair does."""
    boxes = [tuple(int(v) for v in b) for b in boxes]
    wins = [R.plan_window(H, W, b, S, context, feather) for b in boxes]
    merged = True
    while merged:
        merged = False
        for i in range(len(wins)):
            for j in range(i + 1, len(wins)):
                if windows_intersect(wins[i], wins[j]):
                    a, b = boxes[i], boxes[j]
                    boxes[i] = (min(a[0], b[0]), min(a[1], b[1]), max(a[2], b[2]), max(a[3], b[3]))
                    boxes.pop(j)
                    wins.pop(j)
                    wins[i] = R.plan_window(H, W, boxes[i], S, context, feather)
                    merged = True
                    break
            if merged:
                break
    return wins, boxes
