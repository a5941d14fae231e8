#!/usr/bin/env python3
"""Test double for the external `ffmpeg` binary as gs360/video.py drives it for a 360PerspCut video job (tests/fake_ffmpeg.py and
tests/fake_ffmpeg_y4m.py stay as they are; the latter refuses this argv: -loglevel, -nostdin, -an, select=).  Two decoder roles:

  Y4M   <prog> -hide_banner -loglevel error -nostdin [-copyts] [-ss S] -i clip.npz [-to T] [-vsync vfr]
               -vf <fps=F | select='eq(n\\,i)+...' | null> -an -f yuv4mpegpipe -strict -1 pipe:1     -> the clip as YUV4MPEG2
  PPM   the same head, -vf <chain>,format=rgb24|rgb48be -an -f image2pipe -c:v ppm pipe:1            -> the clip's `rgb` frames

`clip.npz` holds y [N, H, W], u and v [N, h, w] (uint8 or uint16) and `tag`, the stream's C tag; optional `full` (XCOLORRANGE=FULL)
and `rgb` [N, H, W, 3] (uint8 or uint16), what the PPM role delivers (without it that role cannot open its input: exit 1).  Frame n
has timestamp n seconds; -ss / -to bound the timestamps, select= keeps the listed indices, fps=F keeps every round(1/F)-th frame.
Exit 3: `colorspace=` or an RGB pixel format in the Y4M role (the host was asked to convert colours), `v360=` in either role (a view
job was routed to the per-view subprocess), any other command line.
"""
import re
import sys

import numpy as np

RGB_FORMAT = re.compile(r"\b(rgb24|rgb48le|rgb48be|gbrp\w*|bgr24)\b")


def main(argv):
    args = argv[1:]
    if not args or args[-1] != "pipe:1":
        sys.stderr.write("fake_ffmpeg_planes: only the pipe decoder roles are emulated\n")
        return 3
    opts, src, i = {}, None, 0
    while i < len(args) - 1:
        tok = args[i]
        if tok in ("-hide_banner", "-nostdin", "-copyts", "-an", "-y"):
            i += 1
            continue
        if i + 1 >= len(args) - 1:
            sys.stderr.write("fake_ffmpeg_planes: dangling option {}\n".format(tok))
            return 3
        if tok == "-i":
            src = args[i + 1]
        else:
            opts[tok] = args[i + 1]
        i += 2
    chain = opts.get("-vf", "")
    if "v360=" in chain:
        sys.stderr.write("fake_ffmpeg_planes: a view job reached the decoder double\n")
        return 3
    y4m_role = opts.get("-f") == "yuv4mpegpipe"
    if y4m_role:
        if "colorspace=" in " ".join(args) or RGB_FORMAT.search(" ".join(args)):
            sys.stderr.write("fake_ffmpeg_planes: the host was asked to convert colours\n")
            return 3
        if opts.get("-strict") != "-1" or "-c:v" in opts:
            sys.stderr.write("fake_ffmpeg_planes: unexpected Y4M decoder command line\n")
            return 3
    else:
        deep = chain.endswith("format=rgb48be")
        if opts.get("-f") != "image2pipe" or opts.get("-c:v") != "ppm" or not (chain.endswith("format=rgb24") or deep):
            sys.stderr.write("fake_ffmpeg_planes: unexpected decoder command line\n")
            return 3
    if src is None or src.endswith("broken.npz"):
        sys.stderr.write("fake_ffmpeg_planes: cannot open input\n")
        return 1
    clip = np.load(src)
    n = clip["y"].shape[0]
    lo = float(opts["-ss"]) if "-ss" in opts else None
    hi = float(opts["-to"]) if "-to" in opts else None
    keep = [k for k in range(n) if (lo is None or k >= lo) and (hi is None or k < hi)]
    m = re.search(r"select='([^']*)'", chain)
    if m:
        want = {int(t) for t in re.findall(r"eq\(n\\,(\d+)\)", m.group(1))}
        keep = [k for k in keep if k in want]
    m = re.search(r"fps=([0-9.]+)", chain)
    if m:
        keep = keep[::max(1, int(round(1.0 / float(m.group(1)))))]
    out = sys.stdout.buffer
    if y4m_role:
        y, u, v = clip["y"], clip["u"], clip["v"]
        extra = " XCOLORRANGE=FULL" if "full" in clip and bool(clip["full"]) else ""
        out.write("YUV4MPEG2 W{} H{} F1:1 Ip A1:1 C{}{}\n".format(y.shape[2], y.shape[1], str(clip["tag"]), extra).encode())
        for k in keep:
            out.write(b"FRAME\n" + b"".join(np.ascontiguousarray(p[k]).astype(p.dtype.newbyteorder("<")).tobytes() for p in (y, u, v)))
        out.flush()
        return 0
    if "rgb" not in clip:
        sys.stderr.write("fake_ffmpeg_planes: cannot open input (the clip has no rgb frames for the PPM role)\n")
        return 1
    for k in keep:
        fr = np.ascontiguousarray(clip["rgb"][k])
        if deep:          # 16-bit PPM: maxval 65535, big-endian samples (an 8-bit clip is widened like ffmpeg's format filter)
            fr16 = fr.astype(np.uint16) * (257 if fr.dtype == np.uint8 else 1)
            out.write(b"P6\n%d %d\n65535\n" % (fr.shape[1], fr.shape[0]))
            out.write(fr16.astype(">u2").tobytes())
            continue
        out.write(b"P6\n%d %d\n255\n" % (fr.shape[1], fr.shape[0]))
        out.write(fr.astype(np.uint8).tobytes())
    out.flush()
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv))
