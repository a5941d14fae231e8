#!/usr/bin/env python3
"""Test double for the external `ffmpeg` binary as cli_tools/gs360_Video2Frames.py drives it (tests/fake_ffmpeg.py, the PPM decoder
of gs360/video.py, stays as it is).  Two roles:

  probe    <prog> -hide_banner -i clip.npz            -> a `Duration:` and a `Stream #0:0: Video:` line on stderr, exit 1 (no output
                                                         file, as the real program ends such a call)
  decoder  <prog> -hide_banner [-ss S] -i clip.npz [-to T] [-map M] -vf fps=F -f yuv4mpegpipe -strict -1 pipe:1
                                                      -> the clip as YUV4MPEG2 on stdout

`clip.npz` holds y [N, H, W], u and v [N, h, w] (uint8 or uint16) and `tag`, the stream's C tag; optional `full` (XCOLORRANGE=FULL),
`interlace` (the I field) and `cut` (bytes missing from the last frame).  Frame n has timestamp n seconds; -ss / -to bound the
timestamps, fps=F keeps every round(1/F)-th frame (F <= 1 in the tests).  Any argv that contains `colorspace=` or an RGB pixel format
is refused with exit code 3, so a test notices when the host is asked to do the colour work; `broken.npz` cannot be opened (exit 1).
"""
import re
import sys

import numpy as np


def main(argv):
    args = argv[1:]
    text = " ".join(args)
    if "colorspace=" in text or re.search(r"\b(rgb24|rgb48le|rgb48be|gbrp\w*|bgr24)\b", text):
        sys.stderr.write("fake_ffmpeg_y4m: the host was asked to convert colours\n")
        return 3
    opts, src, i = {}, None, 0
    while i < len(args):
        tok = args[i]
        if tok in ("-hide_banner", "-nostdin", "-y", "-n", "pipe:1"):
            i += 1
            continue
        if i + 1 >= len(args):
            sys.stderr.write("fake_ffmpeg_y4m: dangling option {}\n".format(tok))
            return 3
        if tok == "-i":
            src = args[i + 1]
        else:
            opts[tok] = args[i + 1]
        i += 2
    if src is None or src.endswith("broken.npz"):
        sys.stderr.write("fake_ffmpeg_y4m: cannot open input\n")
        return 1
    clip = np.load(src)
    y, u, v, tag = clip["y"], clip["u"], clip["v"], str(clip["tag"])
    n, H, W = y.shape
    if args[-1] != "pipe:1":                                   # probe role
        bits = "yuv420p10le" if y.dtype == np.uint16 else "yuv420p"
        sys.stderr.write("  Duration: 00:00:{:05.2f}, start: 0.000000, bitrate: 1 kb/s\n".format(float(n)))
        sys.stderr.write("  Stream #0:0: Video: h264, {}(tv, bt709), {}x{}, 1 fps\n".format(bits, W, H))
        sys.stderr.write("At least one output file must be specified\n")
        return 1
    if opts.get("-f") != "yuv4mpegpipe" or opts.get("-strict") != "-1" or not re.fullmatch(r"fps=[0-9.]+", opts.get("-vf", "")):
        sys.stderr.write("fake_ffmpeg_y4m: unexpected decoder command line\n")
        return 3
    lo = float(opts["-ss"]) if "-ss" in opts else None
    hi = float(opts["-to"]) if "-to" in opts else None
    keep = [k for k in range(n) if (lo is None or k >= lo) and (hi is None or k < hi)]
    step = max(1, int(round(1.0 / float(opts["-vf"][4:]))))
    keep = keep[::step]
    out = sys.stdout.buffer
    extra = " XCOLORRANGE=FULL" if "full" in clip and bool(clip["full"]) else ""
    interlace = str(clip["interlace"]) if "interlace" in clip else "p"
    out.write("YUV4MPEG2 W{} H{} F1:1 I{} A1:1 C{}{}\n".format(W, H, interlace, tag, extra).encode())
    cut = int(clip["cut"]) if "cut" in clip else 0
    sys.stderr.write("  Duration: 00:00:{:05.2f}, start: 0.000000, bitrate: 1 kb/s\n".format(float(n)))
    for j, k in enumerate(keep):
        body = b"".join(np.ascontiguousarray(p[k]).astype(p.dtype.newbyteorder("<")).tobytes() for p in (y, u, v))
        if cut and j == len(keep) - 1:
            body = body[:-cut]
        out.write(b"FRAME\n" + body)
    out.flush()
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv))
