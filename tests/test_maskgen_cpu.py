"""CPU tier of the device mask generator: the definition's numpy restatement (tests/maskgen_ref.py) against
hand-computed values and its distribution, and the host surface around the kernel - key packing, the datasets' masks="generated"
switch, global row ids under sharding, the --masks option."""
import os

import numpy as np
import pytest
import torch

import maskgen_ref as R

SEED = 0x5EED


def test_draws_match_published_splitmix64_outputs():
    """splitmix64 seeded with 0 yields mix(G), mix(2G), mix(3G) = the generator's published first outputs; draw(k) on stream 0 is the
    upper half of output k, and stream_of(0, 0) = mix(G) is the first output itself."""
    out = [0xE220A8397B1DCDAF, 0x6E789E6AA1B965F4, 0x06C45D188009454F]
    assert [R.mix(R.G * (k + 1)) for k in range(3)] == out
    assert R.stream_of(0, 0) == out[0]
    assert [R.draw(0, k) for k in range(3)] == [0xE220A839, 0x6E789E6A, 0x06C45D18]
    # uni = lo + floor(draw / 2^32 * (hi - lo + 1)):  0.88331 * 10 -> 8 ;  0.43153 * 9 -> 3, - 4 ;  0.02643 * 4 -> 0, + 2
    assert R.uni(0, 0, 0, 9) == 8
    assert R.uni(0, 1, -4, 4) == -1
    assert R.uni(0, 2, 2, 5) == 2
    # the key enters modulo 2^64: -1 is key 2^64 - 1, and stream = mix(seed + G * 0)
    assert R.stream_of(5, -1) == R.mix(5)


@pytest.mark.parametrize("H,W", [(64, 64), (37, 53)])
def test_rect_is_one_rectangle_within_bounds(H, W):
    hs = set()
    for key in range(1000):
        h, w, y0, x0 = R.rect_params(SEED, key, H, W)
        assert H // 8 <= h <= H // 2 and W // 8 <= w <= W // 2
        assert 0 <= y0 and y0 + h <= H and 0 <= x0 and x0 + w <= W
        hs.add(h)
        m = R.mask("rect", SEED, key, H, W)
        assert m.sum() == h * w and m[y0:y0 + h, x0:x0 + w].all()
    assert min(hs) == H // 8 and max(hs) == H // 2      # both inclusive bounds are reached in 1000 draws


def test_freeform_coverage_at_64():
    cov = []
    for key in range(300):
        segs = R.freeform_segments(SEED, key, 64, 64)
        assert 2 * 3 <= len(segs) <= 55
        for ax, ay, bx, by, r in segs:
            assert 0 <= ax < 64 and 0 <= ay < 64 and 0 <= bx < 64 and 0 <= by < 64 and 1 <= r <= 4
            assert abs(bx - ax) <= 8 and abs(by - ay) <= 8
        cov.append(float(R.mask("freeform", SEED, key, 64, 64).mean()))
    print(f"freeform 64x64, keys 0..299: mean {np.mean(cov):.3f} min {min(cov):.3f} max {max(cov):.3f}")
    assert all(0.0 < c < 0.6 for c in cov)
    assert 0.12 <= np.mean(cov) <= 0.25


def test_capsule_test_handles_points_and_long_segments():
    """The three branches of the point-in-capsule test on a mask made by hand: a zero-length segment is a disc, a long one a stadium."""
    segs = [(10, 10, 10, 10, 3), (20, 30, 40, 30, 2)]
    py, px = np.mgrid[0:48, 0:48]
    want = ((px - 10) ** 2 + (py - 10) ** 2 <= 9) | ((np.abs(py - 30) <= 2) & (px >= 20) & (px <= 40)) \
        | ((px - 20) ** 2 + (py - 30) ** 2 <= 4) | ((px - 40) ** 2 + (py - 30) ** 2 <= 4)
    orig = R.freeform_segments
    try:
        R.freeform_segments = lambda *a: segs
        got = R.mask("freeform", 0, 0, 48, 48)
    finally:
        R.freeform_segments = orig
    assert np.array_equal(got.astype(bool), want)


def test_mask_key_packing():
    import gan_inpainting_amd  # noqa: F401
    from gan_inpainting_amd.lib.data.masks import mask_key
    assert mask_key("train", 0, 0) == 0
    assert mask_key("train", 7, 5) == (7 << 32) | 5
    assert mask_key("test", 0, 5) == (1 << 56) | 5
    assert mask_key("extra", 0, 5) == (2 << 56) | 5
    # evaluation splits ignore the epoch, the training split does not
    assert mask_key("test", 3, 9) == mask_key("test", 0, 9) and mask_key("extra", 3, 9) == mask_key("extra", 0, 9)
    assert mask_key("train", 3, 9) != mask_key("train", 4, 9)
    rows = torch.tensor([0, 1, 4000000000], dtype=torch.int64)
    assert mask_key("train", 2, rows).tolist() == [mask_key("train", 2, int(r)) for r in rows]
    assert mask_key("test", 2, rows).dtype == torch.int64
    with pytest.raises(ValueError):
        mask_key("train", 0, 1 << 32)
    with pytest.raises(KeyError):
        mask_key("validation", 0, 0)


def test_generated_masks_dataset_rows_and_cli(tmp_path):
    """A CSV without a mask_source column: masks="generated" yields row ids, the ids stay global under sharding, and the launcher
    knows the option."""
    pytest.importorskip("PIL")
    from PIL import Image
    import pandas as pd
    import gan_inpainting_amd  # noqa: F401
    from gan_inpainting_amd import train
    from gan_inpainting_amd.lib.data import dataset
    (tmp_path / "img").mkdir()
    rows = []
    for i in range(8):
        Image.fromarray(np.full((20, 24), 10 * i, np.uint8), mode="L").save(tmp_path / "img" / f"g{i}.png")
        rows.append({"groundtruth_source": f"img/g{i}.png"})
    csv = tmp_path / "train_all_masks.csv"
    pd.DataFrame(rows).to_csv(csv, index=False)

    ds = dataset.InpaintingDataset(str(tmp_path), dataframe=train.load_rows(str(csv), 0, 1, 2), masks="generated")
    ground, row, segment = ds[3]
    assert ground.dtype == torch.uint8 and tuple(ground.shape) == (20, 24) and int(ground[0, 0]) == 30
    assert row.dtype == torch.int64 and row.dim() == 0 and int(row) == 3
    batch = next(iter(torch.utils.data.DataLoader(ds, batch_size=4)))
    assert batch[1].dtype == torch.int64 and batch[1].tolist() == [0, 1, 2, 3]
    # without a `_row` column the index is the id
    assert int(dataset.InpaintingDataset(str(tmp_path), csv_file=str(csv), masks="generated")[5][1]) == 5
    # the default still reads the files: this CSV has none
    with pytest.raises(KeyError):
        dataset.InpaintingDataset(str(tmp_path), csv_file=str(csv))[0]

    seen = []
    for rank in range(2):
        shard = dataset.InpaintingDataset(str(tmp_path), dataframe=train.load_rows(str(csv), rank, 2, 2), masks="generated")
        ids = [int(shard[i][1]) for i in range(len(shard))]
        assert ids == list(range(rank, 8, 2))
        assert all(int(shard[i][0][0, 0]) == 10 * r for i, r in enumerate(ids))     # the id names the image it came with
        seen += ids
    assert sorted(seen) == list(range(8))

    args = train.build_parser().parse_args(["-exp", "wgan_l1", "--masks", "freeform", "--mask-seed", "11"])
    assert args.masks == "freeform" and args.mask_seed == 11
    assert train.build_parser().parse_args(["-exp", "wgan_l1"]).masks == "files"
    with pytest.raises(SystemExit):
        train.build_parser().parse_args(["-exp", "wgan_l1", "--masks", "circles"])


def test_synthetic_dataset_switch_keeps_the_default():
    import gan_inpainting_amd  # noqa: F401
    from gan_inpainting_amd.train import SyntheticInpainting
    host = SyntheticInpainting(4, 32, 1)[2]
    gen = SyntheticInpainting(4, 32, 1, masks="generated", row0=100)[2]
    assert host[1].dtype == torch.float32 and tuple(host[1].shape) == (1, 32, 32) and 16 <= int(host[1].sum()) <= 256
    assert gen[1].dtype == torch.int64 and int(gen[1]) == 102
    assert torch.equal(host[0], gen[0])     # the same image either way
    # the host path is today's: ground, four rectangle draws, labels, in that order from one seeded generator
    g = torch.Generator().manual_seed(1 + 2)
    assert torch.equal(host[0], torch.rand((1, 32, 32), generator=g))
    h, w = (int(torch.randint(4, 17, (1,), generator=g)) for _ in range(2))
    assert int(host[1].sum()) == h * w


def test_row_ids_without_a_generator_are_refused():
    """The loop never guesses: row ids with --masks files (no kind to generate) are an error, mask pixels pass through untouched."""
    import gan_inpainting_amd  # noqa: F401
    from gan_inpainting_amd.experiment_list import _common as C
    with pytest.raises(ValueError):
        C.to_device_mask(torch.arange(4), torch.zeros(4, 1, 16, 16), torch.device("cpu"), {"masks": "files"}, "train", 0)
    m = torch.rand(2, 1, 16, 16)
    assert torch.equal(C.to_device_mask(m, m, torch.device("cpu"), {}, "train", 0), m)


def test_mask_kernels_have_no_scratch():
    """The three instances of maskgen_kernel (rect, freeform with 32-bit and with 64-bit cross products) are in the build record
    (csrc/build/resources.txt) and do not spill."""
    res = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "gan-inpainting_amd", "csrc", "build", "resources.txt")
    assert os.path.exists(res), "no build record: build() always writes csrc/build/resources.txt, so the build did not run or failed"
    rows = [line.rstrip("\n").split("\t") for line in open(res)]
    mine = [(name, dict(x.split("=", 1) for x in kv)) for src, name, *kv in rows if src == "maskgen" and "maskgen_kernel" in name]
    assert len(mine) == 3, [name for name, _ in mine]
    assert all(d.get("scratch") == "0" for _, d in mine), mine
