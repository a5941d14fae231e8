#!/usr/bin/env python3
"""gs360_MaskFinish -- everything gs360_SegmentationMaskTool.py does to a mask after the network, on the GPU (MSK-SPEC v1).

The reference tool runs Mask R-CNN and then, on every image, a fixed chain: close, expand, fuse to the frame edges, OR in the manual
add layer, invert, compose (SEG:680-781).  This tool is that chain.  It keeps the reference's interface for it -- the flag names and
defaults, the parser's complaints about negative amounts, the `Mask expand:` / `Edge fuse:` / `Manual mask dir:` lines and the output
file names -- and nothing else of it; the network is not part of this build.  The raw masks come from any segmenter as `<stem>.png`
files in --raw-mask-dir (target where > 127; a missing file means no detection; another size is resized with Pillow NEAREST, as the
manual layer is), or there are none and the manual layers of --manual-mask-dir (`<view or file key>__add.png`) are the only content.

Outputs: `<stem>.png` (mask, alpha), `<stem>_cutout.png`, `<stem>_<mode>.png` (SEG:740-781), written by the device PNG encoder with
GS360_PNG_ENCODER=device, else by gs360/imageio.py.  Every image is looked at before the first one is finished, so a run that ends
with an [ERR] line has written nothing.  --include_shadow adds the reference's shadow estimate (SEG:499-558, MSK-SHADOW v1) between
the close and the expansion when the environment says GS360_MASK_SHADOW=device; the estimate is not pinned against cv2 yet, so
without that variable the flag is refused as before.  It reads the images in every mode.  --mode inpaint (SEG:809-815) fills the
finished mask's region of the image and writes `<stem>_inpaint.png` when the environment says GS360_MASK_INPAINT=device
(MSK-INPAINT v1: Telea's weights in a level-ordered march; not pinned against cv2.inpaint, so without that variable the mode is
refused as before).  Not built, and refused with one [ERR] line each: --mode inpaint without GS360_MASK_INPAINT=device,
--include_shadow without GS360_MASK_SHADOW=device, 16-bit images in the compose modes, in the inpaint mode
and with the shadow estimate, --edge-fuse-pixels above an image's shorter side or above 1024, an expansion above 512 pixels, an image
side above 32768.
"""
import argparse
import sys
from pathlib import Path

_PKG = Path(__file__).resolve().parent.parent
if str(_PKG) not in sys.path:
    sys.path.insert(0, str(_PKG))

IMAGE_SUFFIXES = (".jpg", ".jpeg", ".png", ".tif", ".tiff")
# mode -> (output kind, invert, what follows the stem in the file name); inpaint fills the image under the mask of kind "mask"
OUTPUTS = {"mask": ("mask", True, ""), "alpha": ("rgba", True, ""), "cutout": ("rgba", False, "_cutout"),
           "keep_person": ("keep", False, "_keep_person"), "remove_person": ("remove", False, "_remove_person"),
           "inpaint": ("mask", False, "_inpaint")}
LAYER_THRESH = 127          # a raw mask or manual layer counts where it is brighter than this
BATCH = 16                  # images per device call


def create_arg_parser():
    ap = argparse.ArgumentParser(description="Finish segmentation masks on the GPU: close, expand, edge fuse, manual layer, compose.")
    ap.add_argument("-i", "--in", dest="input_dir", type=str, required=True,
                    help="folder of images; its jpg / jpeg / png / tif / tiff files are taken in name order, subfolders are not")
    ap.add_argument("--raw-mask-dir", type=str, default=None,
                    help="folder of raw masks <stem>.png from any segmenter: target where brighter than 127, no file = nothing detected")
    ap.add_argument("-o", "--out", type=str, default=None, help="folder for the results (default: _mask beside the input folder)")
    ap.add_argument("--mode", type=str, default="mask", choices=list(OUTPUTS),
                    help="what to write: the mask (target black), the image with the mask as alpha, the cutout, or the image with the "
                         "target kept / blacked out; inpaint fills the target from its surroundings and runs with "
                         "GS360_MASK_INPAINT=device in the environment, else ends the run with an [ERR] line")
    ap.add_argument("--close", type=int, default=5, help="side of the ellipse that closes small holes first (1 or less: no closing)")
    ap.add_argument("--include_shadow", action="store_true",
                    help="add the estimated cast shadow to the mask; runs with GS360_MASK_SHADOW=device in the environment, else ends "
                         "the run with an [ERR] line")
    ap.add_argument("--mask-expand-mode", type=str, choices=["pixels", "percent"], default="pixels",
                    help="grow the mask by --mask-expand-pixels, or by --mask-expand-percent of the image's longer side")
    ap.add_argument("--mask-expand-pixels", type=int, default=15, help="growth in pixels (mode pixels)")
    ap.add_argument("--mask-expand-percent", type=float, default=1.0, help="growth in percent of the longer side (mode percent)")
    ap.add_argument("--edge-fuse-pixels", type=int, default=25,
                    help="mask parts this close to a frame edge are extended to the edge, after the growth and before the manual layer")
    ap.add_argument("--manual-mask-dir", type=str, default=None,
                    help="folder of painted layers <view or file key>__add.png that are added to the masks")
    return ap


def default_out_dir(input_dir):
    """`_mask` beside the input folder, or inside it when it has no parent of its own (the rule of SEG:1026-1030)"""
    beside = input_dir.parent
    return (input_dir if beside == input_dir else beside) / "_mask"


def existing_dir(text, label):
    """-> (Path or None, None) or (None, the message for a folder that was named and is not there)"""
    if not text:
        return None, None
    path = Path(text)
    return (path, None) if path.is_dir() else (None, f"{label} directory not found: {path}")


def read_layer(path, size):
    """a mask file -> H x W uint8 of 0 / 255, set where its gray is above LAYER_THRESH, brought to size = (W, H) by nearest
    neighbour; None without a file"""
    import numpy as np
    from PIL import Image
    if not path.is_file():
        return None
    with Image.open(path) as im:
        gray = im.convert("L")
        gray = gray if gray.size == size else gray.resize(size, Image.NEAREST)
        return ((np.asarray(gray) > LAYER_THRESH) * np.uint8(255)).astype(np.uint8)


def survey(images, params, kind, mode, shadow=False):
    """every image's (W, H) and, for the compose modes, the inpaint mode and the shadow estimate, whether it is an 8-bit image ->
    (sizes, None) or (None, the reason this build does not take the run)"""
    from PIL import Image
    from gs360 import capi, maskfinish
    sizes = []
    for path in images:
        with Image.open(path) as im:
            sizes.append(im.size)                         # the header alone: the mask mode never reads pixels
            if (kind != "mask" or mode == "inpaint") and im.mode.startswith("I"):
                return None, f"{path.name}: 16-bit images are not built for --mode {mode}"
            if shadow and im.mode.startswith("I"):
                return None, f"{path.name}: 16-bit images are not built for --include_shadow"
    try:
        jobs, _rows = maskfinish.build_jobs([(h, w) for w, h in sizes], params, kind)
    except ValueError as exc:
        return None, str(exc)
    for path, j in zip(images, jobs):
        if max(j.H, j.W) > capi.MASK_MAX_SIDE:
            return None, f"{path.name}: sides above {capi.MASK_MAX_SIDE} are not built"
        if j.expand_kh > capi.MASK_MAX_ELEMENT:
            return None, f"{path.name}: a mask expansion above {maskfinish.MAX_EXPAND} pixels is not built (got {j.expand_kh // 2})"
        if j.fuse > capi.MASK_MAX_FUSE:
            return None, f"--edge-fuse-pixels above {capi.MASK_MAX_FUSE} is not built"
    return sizes, None


def fail(text):
    print(f"[ERR] {text}")
    return 1


def main(argv=None):
    ap = create_arg_parser()
    args = ap.parse_args(argv)
    for flag, value in (("--mask-expand-pixels", args.mask_expand_pixels), ("--mask-expand-percent", args.mask_expand_percent),
                        ("--edge-fuse-pixels", args.edge_fuse_pixels)):
        if value < 0:
            ap.error(f"{flag} must be 0 or greater")
    if args.mode == "inpaint":
        from gs360 import maskfinish
        try:
            on_device = maskfinish.inpaint_mode_from_env()
        except ValueError as exc:
            return fail(str(exc))
        if not on_device:
            return fail("--mode inpaint is not built: Telea inpainting is not part of this tool")
    if args.include_shadow:
        from gs360 import maskfinish
        try:
            on_device = maskfinish.shadow_mode_from_env()
        except ValueError as exc:
            return fail(str(exc))
        if not on_device:
            return fail("--include_shadow is not built: the contour-filtered shadow estimate is not part of this tool")

    input_dir = Path(args.input_dir)
    if not input_dir.is_dir():
        print(f"Input directory not found: {input_dir}", file=sys.stderr)
        return 1
    raw_dir, missing = existing_dir(args.raw_mask_dir, "Raw mask")
    manual_dir, missing_manual = existing_dir(args.manual_mask_dir, "Manual mask")
    if missing or missing_manual:
        print(missing or missing_manual, file=sys.stderr)
        return 1
    if raw_dir is None and manual_dir is None:
        return fail("the segmentation network is not part of this build: give --raw-mask-dir (masks from any segmenter) "
                    "and/or --manual-mask-dir")
    out_dir = Path(args.out) if args.out is not None else default_out_dir(input_dir)

    amount = f"{args.mask_expand_pixels} px" if args.mask_expand_mode == "pixels" else f"{args.mask_expand_percent}%"
    print(f"Mask expand: {amount}")
    print(f"Edge fuse: {args.edge_fuse_pixels} px")
    if manual_dir is not None:
        print(f"Manual mask dir: {manual_dir}")

    images = sorted(p for p in input_dir.iterdir() if p.is_file() and p.suffix.lower() in IMAGE_SUFFIXES)
    if not images:
        print("No images found.", file=sys.stderr)
        return 1

    import numpy as np
    from PIL import Image
    from gs360 import capi, imageio, maskfinish, pngenc
    kind, invert, suffix = OUTPUTS[args.mode]
    params = maskfinish.Params(close=args.close, expand_mode=args.mask_expand_mode, expand_pixels=args.mask_expand_pixels,
                               expand_percent=args.mask_expand_percent, edge_fuse_pixels=args.edge_fuse_pixels, thresh=LAYER_THRESH)
    sizes, reason = survey(images, params, kind, args.mode, args.include_shadow)
    if reason:
        return fail(reason)
    device_png = pngenc.mode_from_env()
    try:
        with capi.Context(device=0, n_slots=1) as ctx:
            out_dir.mkdir(parents=True, exist_ok=True)
            for at in range(0, len(images), BATCH):
                batch = list(zip(images[at:at + BATCH], sizes[at:at + BATCH]))
                masks = [(read_layer(raw_dir / f"{p.stem}.png", size) if raw_dir is not None else None) for p, size in batch]
                masks = [m if m is not None else (size[1], size[0]) for m, (_p, size) in zip(masks, batch)]
                adds = [read_layer(manual_dir / f"{maskfinish.manual_key(p)}__add.png", size) if manual_dir is not None else None
                        for p, size in batch]
                pixels = None
                if kind != "mask" or args.include_shadow or args.mode == "inpaint":
                    pixels = []
                    for p, _size in batch:
                        with Image.open(p) as im:
                            pixels.append(np.asarray(im.convert("RGB")))
                with ctx.slot_locks[0]:
                    if args.mode == "inpaint":
                        items, _counts = maskfinish.finish_with_inpaint_device(ctx, masks, params, adds, pixels, args.include_shadow)
                    elif args.include_shadow:
                        items, _counts = maskfinish.finish_with_shadow_device(ctx, masks, params, None, adds, pixels, kind, invert)
                    else:
                        items, _counts = maskfinish.finish_device(ctx, masks, params, adds, pixels, kind, invert)
                    try:
                        if device_png:
                            files = pngenc.encode_buffers(ctx, items)
                        else:
                            files = [ctx.download(o, (H, W) if C == 1 else (H, W, C), np.uint8) for o, H, W, C, _b, _s in items]
                    finally:
                        for it in items:
                            ctx.free(it[0])
                for (p, _size), data in zip(batch, files):
                    target = out_dir / f"{p.stem}{suffix}.png"
                    if device_png:
                        target.write_bytes(data)
                    else:
                        imageio.write_image(target, data)
    except capi.Gs360Error as exc:
        return fail(str(exc))
    return 0


if __name__ == "__main__":
    sys.exit(main())
