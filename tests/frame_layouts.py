"""Device layouts of test frames for the FrameSelector entry points: packed rows, rows with `pad` filler bytes, and windows into
a larger parent image.  Every buffer comes from ctx.to_device (64 readable bytes of slack behind it), every filler byte is 0xA5,
and a window lies wholly inside its parent at a byte offset that is a multiple of 4, so that no kernel reads outside an allocation
whatever the layout."""
import numpy as np

from gs360 import framescore

FILL = 0xA5
TILE_W = 256          # kFsTileW of csrc/gs360_framescore.hip: columns per staged tile
RAW_DWORDS = 260      # kFsRawDw: dwords of one staged row


class Window:
    """A frame inside a parent allocation: the entry points' bindings read only .ptr of a frame."""

    def __init__(self, ptr):
        self.ptr = ptr


def channels(frame):
    return 1 if frame.ndim == 2 else frame.shape[2]


def window_column(first, stride, row, C):
    """The first column >= first at which a window at `row` of a parent of row stride `stride` starts on a multiple of 4 bytes."""
    col = first
    while (row * stride + col * C) % 4:
        col += 1
    return col


def upload(ctx, frames, pad=0, window=None):
    """-> (objs, stride, bufs): objs carry .ptr of each frame, stride is what the entry point takes (0 = packed), bufs are the
    allocations to free.  pad: filler bytes behind every row.  window = (parent_h, parent_w, row, col): each frame sits at
    (row, col) of a parent of its own."""
    H, W = frames[0].shape[:2]
    C = channels(frames[0])
    if window:
        PH, PW, row, col = window
        stride = PW * C
        off = row * stride + col * C
        assert off % 4 == 0 and row + H <= PH and col + W <= PW
        bufs = []
        for f in frames:
            host = np.full((PH, stride), FILL, np.uint8)
            host[row:row + H, col * C:(col + W) * C] = f.reshape(H, W * C)
            bufs.append(ctx.to_device(host))
        return [Window(b.ptr + off) for b in bufs], stride, bufs
    if pad:
        stride = W * C + pad
        bufs = []
        for f in frames:
            host = np.full((H, stride), FILL, np.uint8)
            host[:, :W * C] = f.reshape(H, W * C)
            bufs.append(ctx.to_device(host))
        return bufs, stride, bufs
    bufs = [ctx.to_device(f) for f in frames]
    return bufs, 0, bufs


def device_frames(objs, frames, stride):
    """framescore.DeviceFrames over upload()'s objs."""
    H, W = frames[0].shape[:2]
    return [framescore.DeviceFrame(o, H, W, channels(frames[0]), stride) for o in objs]


def mixed_strides(ctx, frames):
    """-> (DeviceFrames, bufs): frame k of one shape H x W x C is stored with row stride (0, W*C, W*C + 8)[k % 3].  Every buffer
    has H * (W*C + 8) bytes, so that reading a packed frame with the widest stride gives wrong numbers, not a read outside it."""
    H, W = frames[0].shape[:2]
    C = channels(frames[0])
    out, bufs = [], []
    for k, f in enumerate(frames):
        stride = (0, W * C, W * C + 8)[k % 3]
        host = np.full((H, W * C + 8), FILL, np.uint8)
        if stride > W * C:
            host[:, :W * C] = f.reshape(H, W * C)
        else:
            host.reshape(-1)[:H * W * C] = f.reshape(-1)
        bufs.append(ctx.to_device(host))
        out.append(framescore.DeviceFrame(bufs[-1], H, W, C, stride))
    return out, bufs


MAXIMAL = (20, 514, 4)            # H, W, C: a first tile with a right halo, a middle tile with both halos, a last tile of 2 columns
MAXIMAL_BAND = (3, 19)


def check_maximal_staging(pad):
    """The point of the MAXIMAL shape with `pad` filler bytes a row, computed from the stride and the tile geometry over the band's
    rows (their stencils read the halo columns): the middle tile stages 258 pixels (1032 bytes), which with a row start off a dword
    boundary makes 259 of the kFsRawDw = 260 dwords -- the one case in which the second load and the guarded second LDS write of a
    row carry pixel data.  An odd stride walks address & 3 through all four values over the rows, so some staged row starts at
    address & 3 == 3 (the last dword then holds the halo pixel's G, B and A); pad 2 reaches 0 and 2 only (B and A)."""
    H, W, C = MAXIMAL
    staged = [staged_row(W, C, W * C + pad, y, tile=1) for y in range(*MAXIMAL_BAND)]
    assert W > 2 * TILE_W and MAXIMAL_BAND[1] <= H
    assert {a for a, _ in staged} == ({0, 1, 2, 3} if pad % 2 else {0, 2})
    assert all(n == RAW_DWORDS - 1 - (a == 0) for a, n in staged)


def staged_row(W, C, stride, y, tile):
    """(address & 3, dwords) of row y of tile `tile` as fs_strip_kernel stages it from a 4-byte aligned frame pointer: pixel
    columns max(x0 - 1, 0) .. min(x0 + nx, W - 1), rounded out to whole dwords."""
    x0 = tile * TILE_W
    nx = min(TILE_W, W - x0)
    xa, xb = max(x0 - 1, 0), min(x0 + nx, W - 1)
    a = (y * stride + xa * C) & 3
    return a, (a + (xb - xa + 1) * C + 3) >> 2
