"""The host path the device encoders share (gs360/jpegenc.py, JPG-SPEC v1; gs360/pngenc.py, PNG-SPEC v1; DESIGN.md sections 11 and 13).

Either encoder codes a list of device images in one call into buffers of a first capacity, codes the few that overflowed again, alone,
into buffers of the bound, and gives back every buffer it took but the ones that hold the results.  What differs between the codecs
(capacities, the job tuple, the call and what it brings back, the overflow sentinel) is passed in.
"""
import collections

import numpy as np

from . import capi

# an encoder mode, tagged by its type: which codec writes a view, and how
JpegMode = collections.namedtuple("JpegMode", "quality huffman")
PngMode = collections.namedtuple("PngMode", "")


def code_items(items, take, give, capacity, bound, job, start, overflow, what):
    """(the caller holds the slot) items -> [(DeviceBuffer holding the item's coded bytes, their length, the codec's extra)].
    capacity(item) / bound(item): the bytes of an item's first buffer and of one that holds any result; job(item, out, cap): the job
    tuple of the codec's call; start(room) takes the call's length (and table or checksum) buffers, sized for all items, and returns
    run(jobs) -> (lengths, extras), which is called once for all jobs and once more for every item whose length came back as
    `overflow`.  `what` names the stream in the error an item raises that does not fit its bound either.
    Device memory comes from take(nbytes) and goes back through give(buffer): everything taken but the result buffers returned is given
    back before this returns or raises; those are the caller's to give back."""
    if not items:
        return []
    taken, kept = [], []

    def room(nbytes):
        taken.append(take(nbytes))
        return taken[-1]
    try:
        caps = [capacity(item) for item in items]
        outs = [room(cap) for cap in caps]
        run = start(room)
        lengths, extras = run([job(item, out, cap) for item, out, cap in zip(items, outs, caps)])
        for i, length in enumerate(lengths):
            if length != overflow:
                continue
            full = bound(items[i])
            if full <= caps[i]:
                raise capi.Gs360Error(-2, f"the {what} did not fit its bound")
            outs[i] = room(full)
            (lengths[i],), (extras[i],) = run([job(items[i], outs[i], full)])
            if lengths[i] == overflow:
                raise capi.Gs360Error(-2, f"the {what} did not fit its bound")
        kept = outs
        return list(zip(outs, lengths, extras))
    finally:
        for b in taken:
            if not any(b is k for k in kept):
                give(b)


def files_of(ctx, items, coded, frame, slot):
    """coded: code_items' result for `items`, in the context's own memory -> [bytes]: each item's coded bytes come back and
    frame(item, bytes, extra) makes the file of them; the buffers are freed"""
    try:
        return [frame(item, ctx.download(d, (length,), np.uint8, slot).tobytes(), extra) for item, (d, length, extra) in zip(items, coded)]
    finally:
        for d, _length, _extra in coded:
            ctx.free(d)


def encode_images(ctx, images, as_item, encode, slot):
    """images: ndarrays or ready item tuples (device images) -> encode(items) under the slot's lock.  as_item(array) -> (the contiguous
    array to upload, the item's fields behind its buffer); the buffers uploaded here are freed"""
    items, owned = [], []
    try:
        for im in images:
            if isinstance(im, tuple):
                items.append(im)
                continue
            a, fields = as_item(im)
            owned.append(ctx.to_device(a, slot))
            items.append((owned[-1],) + fields)
        with ctx.slot_locks[slot]:
            return encode(items)
    finally:
        for b in owned:
            ctx.free(b)
