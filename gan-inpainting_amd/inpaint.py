#!/usr/bin/env python3
"""Inpaint pictures of any size with a saved generator (lib/inpaint.py; not in the reference):

    python gan-inpainting_amd/inpaint.py -m runs/model/wgan_l1/epoch100_G.pt -i photo.png --mask hole.png -o out/
    python gan-inpainting_amd/inpaint.py -m epoch100_G.pt -i photos/ --masks freeform --mask-seed 3 -o out/ --panel
    python gan-inpainting_amd/inpaint.py -m epoch100_G.pt -i scan.png --mask scratches.png -o out/ --windows per-hole

-i names an image or a directory of images; --mask a mask file, or a directory holding a mask under each image's file name (a
nonzero mask pixel is a hole); --masks rect|freeform draws the holes with the device mask generator instead (lib/data/masks.py,
images of 16 .. 4096 pixels a side). Every picture is decoded to 8-bit grey like the training data, repaired at its own size and
written as <outdir>/<name>.png; --windows per-hole repairs every group of holes in a window of its own and prints
the holes and windows of each image; --panel adds <name>_panel.png: original | original with the hole blanked | result."""
import argparse
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

IMAGE_SUFFIXES = (".png", ".jpg", ".jpeg", ".bmp", ".tif", ".tiff", ".pgm", ".webp")


def build_parser():
    p = argparse.ArgumentParser(description="Inpaint images at their own size with a generator checkpoint")
    p.add_argument("-m", "--model", required=True, help="generator state dict (epoch<N>_G.pt)")
    p.add_argument("-i", "--input", required=True, help="image file or directory")
    p.add_argument("--mask", default=None, help="mask file, or directory of masks named like the images")
    p.add_argument("--masks", choices=["rect", "freeform"], default=None, help="generate the holes on the device instead of reading them")
    p.add_argument("--mask-seed", dest="mask_seed", type=int, default=0, help="seed of the generated masks")
    p.add_argument("-o", "--outdir", required=True)
    p.add_argument("-g", "--generator", choices=["unet", "vgg19"], default="unet")
    p.add_argument("--imagedim", type=int, default=128, help="the size the generator was trained at")
    p.add_argument("--dtype", default="fp16", choices=["fp16", "fp32"])
    p.add_argument("--context", type=float, default=2.0, help="window side / hole side")
    p.add_argument("--feather", type=int, default=8, help="blend radius in pixels (0 .. 63; 0 = hard paste)")
    p.add_argument("--batchsize", type=int, default=16, help="windows per generator forward")
    p.add_argument("--windows", choices=["single", "per-hole"], default="single",
                   help="single: one window around all holes of an image; per-hole: one window per group of holes (connected components)")
    p.add_argument("--max-holes", dest="max_holes", type=int, default=256,
                   help="per-hole: an image with more components than this takes the single window (1 .. 65536)")
    p.add_argument("--panel", action="store_true", help="also write <name>_panel.png: original | hole blanked | result")
    return p


def _list_images(path):
    if os.path.isdir(path):
        names = sorted(f for f in os.listdir(path) if f.lower().endswith(IMAGE_SUFFIXES))
        if not names:
            raise SystemExit(f"{path}: no image files")
        return [os.path.join(path, f) for f in names]
    return [path]


def _load_u8(path, device):
    import numpy as np
    from gan_inpainting_amd.lib.data.dataset import pil_loader
    return torch.from_numpy(np.asarray(pil_loader(path), dtype=np.uint8).copy()).to(device)


def load_generator(path, imagedim, dtype, device):
    """The U-Net the training plugins build for --imagedim (experiment_list/_common.py: 7 levels from 128 pixels, else 6)."""
    from gan_inpainting_amd.lib.models import networks
    if imagedim >= 128:
        net = networks.get_network("generator", "unet", dtype=dtype)
    else:
        net = networks.UnetGenerator(1, 1, 6, ngf=64, use_dropout="False", dtype=dtype)
    net.load_state_dict(torch.load(path, map_location="cpu"))
    return net.to(device).eval()


def main(argv=None):
    parser = build_parser()
    args = parser.parse_args(argv)
    if (args.mask is None) == (args.masks is None):
        parser.error("give exactly one of --mask <file | directory> and --masks rect|freeform")
    if not 1 <= args.max_holes <= 65536:
        parser.error("--max-holes takes 1 .. 65536")
    if args.generator != "unet":
        raise NotImplementedError("HIP backend accelerates -g unet (the reference default, eval.py:29)")
    from gan_inpainting_amd import backend as B
    from gan_inpainting_amd.lib import imageout
    from gan_inpainting_amd.lib.inpaint import Inpainter
    B.lib()   # fails loudly when the HIP library is missing
    device = torch.device("cuda:0")
    paths = _list_images(args.input)
    images = [_load_u8(p, device) for p in paths]
    if args.mask is not None:
        if os.path.isdir(args.mask):
            mask_paths = [os.path.join(args.mask, os.path.basename(p)) for p in paths]
        elif len(paths) == 1:
            mask_paths = [args.mask]
        else:
            parser.error("--mask names one file but -i holds several images: give a directory of masks named like the images")
        masks = [_load_u8(p, device) for p in mask_paths]
        for p, im, mk in zip(paths, images, masks):
            if im.shape != mk.shape:
                raise SystemExit(f"{p}: the image is {tuple(im.shape)}, its mask {tuple(mk.shape)}")
    else:
        from gan_inpainting_amd.lib.data.masks import DeviceMaskGenerator
        masks = []
        for i, (p, im) in enumerate(zip(paths, images)):
            H, W = im.shape
            if not (16 <= H <= 4096 and 16 <= W <= 4096):
                raise SystemExit(f"{p}: --masks draws holes for images of 16 .. 4096 pixels a side, this one is {H} x {W}; give --mask")
            m = DeviceMaskGenerator(args.masks, H, W, args.mask_seed)(torch.tensor([i], dtype=torch.int64))
            masks.append((m[0, 0] * 255).to(torch.uint8))
    net = load_generator(args.model, args.imagedim, args.dtype, device)
    inpainter = Inpainter(net, imagedim=args.imagedim, context=args.context, feather=args.feather, batch=args.batchsize,
                          windows=args.windows, max_holes=args.max_holes)
    results = inpainter(images, masks)
    if args.windows == "per-hole":
        for p, (holes, wins) in zip(paths, inpainter.holes):
            print(f"{os.path.basename(p)}: {holes} holes, {wins} windows" + (" (more than --max-holes: single window)" if holes > args.max_holes else ""))
    os.makedirs(args.outdir, exist_ok=True)
    written = []
    for p, im, mk, res in zip(paths, images, masks, results):
        name = os.path.splitext(os.path.basename(p))[0]
        out = os.path.join(args.outdir, name + ".png")
        imageout.write_png(out, res)
        written.append(out)
        if args.panel:
            cols = [t.to(torch.float32).div(255)[None, None] for t in (im, im * (mk == 0), res)]     # v / 255 quantises back to v
            imageout.write_png(os.path.join(args.outdir, name + "_panel.png"), imageout.assemble_panel(cols, gutter=2))
    return written


if __name__ == "__main__":
    main()
