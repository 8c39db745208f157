"""GPU tier: the differentiable-augmentation kernels (csrc/diffaug.hip) one operation at a time through the C-ABI entries and
the DiffAugment module, against the numpy restatement tests/diffaug_ref.py: the parameter table and the data
movement bit for bit, the colour arithmetic exactly where every intermediate is exact and within the derived bounds elsewhere."""
import itertools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import gan_inpainting_amd  # noqa: F401,E402
from gan_inpainting_amd import backend as B  # noqa: E402
from gan_inpainting_amd.lib.models import augment  # noqa: E402
import diffaug_ref as R  # noqa: E402

SIZES = [(1, 1), (5, 7), (17, 33), (64, 64), (64, 96)]
SENTINEL = 0x7FC0BEEF      # a NaN with a payload: an untouched word is recognisable, a converted one would not survive


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def as_i32(a):
    return np.ascontiguousarray(a).view(np.int32)


def run(entry, x_t, table_t, n, H, W, colour, out_t):
    """One C-ABI call on device tensors (int32 views of the words); x_t / out_t may be row slices of larger buffers."""
    B.check(getattr(B.lib(), entry)(B.get_ctx(x_t.device), B.ptr(x_t), B.ptr(table_t), n, H, W, colour, B.ptr(out_t)))


def call(entry, x, table, colour):
    """x: (n, H, W) float32 (or uint32 words); table (n, 8) uint32 -> same dtype as x."""
    n, H, W = x.shape
    xt, tt = dev(as_i32(x)), dev(as_i32(table))
    out = torch.full_like(xt, SENTINEL)
    run(entry, xt, tt, n, H, W, colour, out)
    torch.cuda.synchronize()
    return out.cpu().numpy().view(x.dtype)


def hand_rows(H, W):
    """t = 0, +-H/8, |t| >= H (all zero); windows empty, whole-image and clipped at each of the four borders."""
    ch, cw = H // 2, W // 2
    shifts = [(0, 0), (H // 8, W // 8), (-(H // 8), -(W // 8)), (H // 8, -(W // 8)), (H, 0), (0, -W), (-H - 3, W + 5)]
    windows = [(0, 0, 0, 0), (0, 0, H, W), (-(ch // 2) - 1, 1, ch + 1, cw), (H - ch // 2, 0, ch + 1, cw), (1, -(cw // 2) - 1, ch, cw + 1),
               (0, W - cw // 2, ch, cw + 1), (H // 4, W // 4, ch, cw)]
    return [(0.0, 1.0, ty, tx) + w for (ty, tx), w in itertools.product(shifts, windows)]


def special_words(rng, shape):
    """Random fp32 words with +-0, denormals, +-inf and NaNs (payloads included) sprinkled everywhere."""
    x = rng.standard_normal(shape).astype(np.float32).view(np.uint32)
    specials = np.array([0x00000000, 0x80000000, 0x00000001, 0x807FFFFF, 0x7F800000, 0xFF800000, 0x7FC00000, 0xFFC12345, 0x7F800001],
                        np.uint32)
    pick = rng.random(shape) < 0.3
    x[pick] = specials[rng.integers(0, len(specials), size=int(pick.sum()))]
    return x


# ---- parameter table ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H,W", [(64, 64), (64, 96), (17, 33)])
def test_parameter_table_is_bit_exact(H, W):
    lib, ctx = B.lib(), B.get_ctx()
    for bits, n, (seed, key0) in itertools.product(range(1, 8), (1, 3, 64), ((0, 0), (0x1234567890ABCDEF, ((5 * 4 + 2) << 32) | 7),
                                                                               (3, (1 << 63) + 11))):
        t = torch.full((n, 8), -1, dtype=torch.int32, device="cuda")
        B.check(lib.gi_diffaug_params(ctx, bits, seed, key0, n, H, W, B.ptr(t)))
        got = t.cpu().numpy().view(np.uint32)
        assert np.array_equal(got, R.table(bits, seed, key0, n, H, W)), (bits, n, seed, key0)


def test_module_params_follow_the_key_formula():
    aug = augment.DiffAugment("translation,cutout,color", seed=9)
    assert aug.bits == 7 and aug.policy == "color,translation,cutout"
    t = aug.params(step=3, call=1, n=4, H=64, W=96, row0=8).cpu().numpy().view(np.uint32)
    assert np.array_equal(t, R.table(7, 9, R.key_of(3, 1, 2, 4, 0), 4, 64, 96))      # rank 2 of per-rank batches of 4
    with pytest.raises(ValueError):
        augment.DiffAugment("colour")
    with pytest.raises(ValueError):
        augment.DiffAugment("")


# ---- translation and cutout alone: bit for bit --------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 3])
@pytest.mark.parametrize("H,W", SIZES)
def test_translation_and_cutout_move_the_bits(H, W, n):
    rng = np.random.default_rng(H * 1000 + W + n)
    rows = hand_rows(H, W)
    while len(rows) % n:
        rows.append(rows[len(rows) % 7])
    x = special_words(rng, (len(rows), H, W))
    table = np.stack([R.table_row(*r) for r in rows])
    xt, tt = dev(as_i32(x)), dev(as_i32(table))
    for entry, ref in (("gi_diffaug_fwd", R.move), ("gi_diffaug_bwd", R.move_adjoint)):
        out = torch.full_like(xt, SENTINEL)
        for g in range(0, len(rows), n):       # every call reads and writes an n-row slice of the larger buffers
            run(entry, xt[g:g + n], tt[g:g + n], n, H, W, 0, out[g:g + n])
        torch.cuda.synchronize()
        got = out.cpu().numpy().view(np.uint32)
        for i, r in enumerate(rows):
            assert np.array_equal(got[i], ref(x[i], r)), f"{entry} {H}x{W} row {i}: {r}"
    all_zero = [i for i, r in enumerate(rows) if abs(r[2]) >= H or abs(r[3]) >= W]
    assert all_zero and not got[all_zero].any()


@pytest.mark.parametrize("H,W", [(17, 33), (64, 64)])
@pytest.mark.parametrize("colour", [0, 1])
def test_rows_outside_the_slice_stay_untouched(H, W, colour):
    rng = np.random.default_rng(5)
    x = rng.standard_normal((5, H, W)).astype(np.float32)
    table = R.table(7, 1, 40, 5, H, W)
    xt, tt = dev(as_i32(x)), dev(as_i32(table))
    for entry in ("gi_diffaug_fwd", "gi_diffaug_bwd"):
        out = torch.full_like(xt, SENTINEL)
        run(entry, xt[1:4], tt[1:4], 3, H, W, colour, out[1:4])
        torch.cuda.synchronize()
        got = out.cpu().numpy()
        assert (got[0] == SENTINEL).all() and (got[4] == SENTINEL).all()
        assert not (got[1:4] == SENTINEL).any()


# ---- colour ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H,W", [(8, 8), (16, 32), (64, 64)])
def test_colour_is_exact_where_the_arithmetic_is(H, W):
    """Small-integer images, dyadic b and c, power-of-two pixel counts: the mean and every intermediate are exact in fp32."""
    rng = np.random.default_rng(H + W)
    rows = [(0.25, 0.5, 1, -1, -1, 2, H // 2, W // 2), (-0.5, 1.25, 0, 0, 0, 0, 0, 0), (0.125, 0.75, -(H // 8), W // 8, H - 2, W - 3, H // 2, W // 2)]
    x = rng.integers(-8, 9, size=(3, H, W)).astype(np.float32)
    table = np.stack([R.table_row(*r) for r in rows])
    y = call("gi_diffaug_fwd", x, table, 1)
    dx = call("gi_diffaug_bwd", x, table, 1)
    for i, r in enumerate(rows):
        assert np.array_equal(y[i].astype(np.float64), R.fwd(x[i], r, True)), f"forward row {i}"
        assert np.array_equal(dx[i].astype(np.float64), R.bwd(x[i], r, True)), f"adjoint row {i}"


def drawn(H, W, n=3, seed=11, key0=(2 << 32) | 5, scale=1.0):
    rng = np.random.default_rng(H * 7 + W)
    x = (scale * rng.standard_normal((n, H, W)) + 0.5).astype(np.float32)
    dy = (scale * rng.standard_normal((n, H, W))).astype(np.float32)
    table = R.table(7, seed, key0, n, H, W)
    return x, dy, table


@pytest.mark.parametrize("H,W", SIZES)
def test_colour_is_within_the_derived_bounds(H, W):
    x, dy, table = drawn(H, W)
    y, dx = call("gi_diffaug_fwd", x, table, 1), call("gi_diffaug_bwd", dy, table, 1)
    worst_f = worst_b = 0.0
    for i in range(x.shape[0]):
        p = R.unpack_row(table[i])
        ef, bf = np.abs(y[i] - R.fwd(x[i], p, True)), R.fwd_bound(x[i], p)
        eb, bb = np.abs(dx[i] - R.bwd(dy[i], p, True)), R.bwd_bound(dy[i], p)
        assert not y[i].view(np.uint32)[~R.keep_mask(p, H, W)].any()       # the zero fill is +0, exactly
        worst_f = max(worst_f, float((ef[bf > 0] / bf[bf > 0]).max()) if (bf > 0).any() else 0.0)
        worst_b = max(worst_b, float((eb[bb > 0] / bb[bb > 0]).max()) if (bb > 0).any() else 0.0)
        assert (ef <= bf).all(), f"forward {H}x{W} sample {i}: worst ratio {np.nanmax(ef / bf)}"
        assert (eb <= bb).all(), f"adjoint {H}x{W} sample {i}: worst ratio {np.nanmax(eb / bb)}"
    print(f"{H}x{W}: worst error / bound forward {worst_f:.3f}, adjoint {worst_b:.3f}")


@pytest.mark.parametrize("H,W", SIZES)
@pytest.mark.parametrize("colour", [0, 1])
def test_adjoint_identity_on_device_outputs(H, W, colour):
    """<T x - T 0, dy> = <x, T* dy> (T is affine with colour on: T 0 is the brightness b on the kept positions), in fp64 on the
    device's outputs."""
    x, dy, table = drawn(H, W)
    y, dx = call("gi_diffaug_fwd", x, table, colour), call("gi_diffaug_bwd", dy, table, colour)
    for i in range(x.shape[0]):
        p = R.unpack_row(table[i])
        t0 = p[0] * R.keep_mask(p, H, W) if colour else 0.0
        lhs = ((y[i].astype(np.float64) - t0) * dy[i]).sum()
        rhs = (x[i].astype(np.float64) * dx[i]).sum()
        bound = R.adjoint_bound(x[i], dy[i], p, bool(colour))
        print(f"{H}x{W} colour={colour} sample {i}: |lhs - rhs| = {abs(lhs - rhs):.3e}, bound {bound:.3e}")
        assert abs(lhs - rhs) <= bound


def test_production_entries_equal_table_entries():
    """gi_diffaug_apply / _apply_bwd (draws in the kernels) == gi_diffaug_params + gi_diffaug_fwd / _bwd, for every policy."""
    H, W, n, seed, k0 = 64, 96, 3, 21, (7 << 32) | 2
    x, dy, _ = drawn(H, W)
    lib, ctx = B.lib(), B.get_ctx()
    for bits in range(1, 8):
        table = R.table(bits, seed, k0, n, H, W)
        for entry, prod, src in (("gi_diffaug_fwd", lib.gi_diffaug_apply, x), ("gi_diffaug_bwd", lib.gi_diffaug_apply_bwd, dy)):
            want = call(entry, src, table, bits & 1)
            st = dev(src)
            out = torch.empty_like(st)
            B.check(prod(ctx, bits, seed, k0, B.ptr(st), n, H, W, B.ptr(out)))
            assert np.array_equal(out.cpu().numpy().view(np.uint32), want.view(np.uint32)), (bits, entry)


# ---- determinism ----------------------------------------------------------------------------------------------------------------
def test_two_runs_are_bit_identical():
    rng = np.random.default_rng(1)
    x = dev(rng.standard_normal((64, 1, 64, 64)).astype(np.float32))
    aug = augment.DiffAugment("color,translation,cutout", seed=4)
    outs = []
    for _ in range(2):
        y, dx = torch.empty_like(x), torch.empty_like(x)
        aug.into(x, y, 3, 0)
        aug.adjoint_into(x, dx, 3, 0)
        outs.append((y.cpu().numpy().view(np.uint32), dx.cpu().numpy().view(np.uint32)))
    assert np.array_equal(outs[0][0], outs[1][0]) and np.array_equal(outs[0][1], outs[1][1])


@pytest.mark.parametrize("H,W", [(64, 64), (17, 33)])
def test_a_sample_does_not_depend_on_n_or_its_row(H, W):
    rng = np.random.default_rng(2)
    one = rng.standard_normal((1, 1, H, W)).astype(np.float32)
    batch = rng.standard_normal((8, 1, H, W)).astype(np.float32)
    batch[5] = one[0]
    aug = augment.DiffAugment("color,translation,cutout", seed=4)
    a, b = dev(one), dev(batch)
    for fn in (aug.into, aug.adjoint_into):
        ya, yb = torch.empty_like(a), torch.empty_like(b)
        fn(a, ya, 6, 1, 13)          # the key of row 13 ...
        fn(b, yb, 6, 1, 8)           # ... is row 5 of a batch that starts at row 8
        assert np.array_equal(ya.cpu().numpy().view(np.uint32)[0], yb.cpu().numpy().view(np.uint32)[5])


# ---- autograd -------------------------------------------------------------------------------------------------------------------
def test_module_backward_is_the_adjoint_kernel():
    H, W, n = 64, 96, 3
    x, dy, _ = drawn(H, W)
    aug = augment.DiffAugment("color,translation,cutout", seed=11)
    step, call_, row0 = 2, 1, 4
    table = R.table(7, 11, R.key_of(step, call_, 0, n, row0), n, H, W)
    xt = dev(x[:, None]).requires_grad_(True)
    y = aug(xt, step, call_, row0)
    y.backward(dev(dy[:, None]))
    torch.cuda.synchronize()
    assert np.array_equal(y.detach().cpu().numpy()[:, 0].view(np.uint32), call("gi_diffaug_fwd", x, table, 1).view(np.uint32))
    got = xt.grad.cpu().numpy()[:, 0]
    assert np.array_equal(got.view(np.uint32), call("gi_diffaug_bwd", dy, table, 1).view(np.uint32))
    for i in range(n):      # gradcheck is not applicable in fp32: the reference's adjoint instead
        p = R.unpack_row(table[i])
        assert (np.abs(got[i] - R.bwd(dy[i], p, True)) <= R.bwd_bound(dy[i], p)).all()


def test_invalid_arguments_are_refused():
    lib, ctx = B.lib(), B.get_ctx()
    x = torch.zeros(2, 1, 8, 8, device="cuda")
    assert lib.gi_diffaug_apply(ctx, 0, 0, 0, B.ptr(x), 2, 8, 8, B.ptr(torch.empty_like(x))) != 0
    assert lib.gi_diffaug_apply(ctx, 8, 0, 0, B.ptr(x), 2, 8, 8, B.ptr(torch.empty_like(x))) != 0
    assert lib.gi_diffaug_apply(ctx, 7, 0, 0, B.ptr(x), 2, 8, 8, B.ptr(x)) != 0          # in place
    with pytest.raises(B.BackendError):
        augment.DiffAugment("cutout")(torch.zeros(2, 3, 8, 8, device="cuda"), 0, 0)
