"""VID-COLOR v1 on the GPU, through the C ABI (Context.video_rgb_dev), byte for byte against tests/vidcolor_np.py: a sweep over the
sample levels, shapes around the 8 x 2 pixel group and the 512-group tile, tight / padded / non-dword strides with a sentinel-filled
destination, sixteen different jobs in one call, and every refused argument.

Which path a layout takes (csrc/gs360_vidsteps.h): a job whose four pointers and four strides are all multiples of 4 converts whole
groups of eight pixels with dword loads and stores and the last partial group of a row pixel by pixel; any other job goes pixel by
pixel.  Tight rows are dword multiples only for some widths, so the padded layouts are what reaches the group path at odd widths."""
import numpy as np
import pytest

import vidcolor_np as ref
from gs360 import capi, vidcolor

pytestmark = pytest.mark.gpu

GUARD = 64
FILL = 0xA5
SUB_CODE = vidcolor.SUBSAMPLING


@pytest.fixture(scope="module")
def stages(ctx):
    made = {}

    def get(depth, full=False, keep=False):
        if (depth, full, keep) not in made:
            made[depth, full, keep] = vidcolor.VideoColor(depth, full, keep)
        return made[depth, full, keep]
    yield get
    for s in made.values():
        s.close()


def stride_of(layout, row_bytes, sample_bytes):
    if layout == "tight":
        return row_bytes
    padded = (row_bytes + 3) // 4 * 4 + 8
    if layout == "padded":
        return padded
    odd = ((row_bytes + 1) | 1) if sample_bytes == 1 else padded + 2      # no multiple of 4; even for 16-bit samples
    assert odd % 4 != 0 and odd % sample_bytes == 0 and odd > row_bytes
    return odd


def laid_out(plane, stride, fill):
    """the plane's rows `stride` bytes apart in a byte buffer filled with `fill`"""
    H = plane.shape[0]
    row = plane.shape[1] * plane.itemsize
    buf = np.full(H * stride, fill, np.uint8)
    buf.reshape(H, stride)[:, :row] = np.ascontiguousarray(plane).view(np.uint8).reshape(H, row)
    return buf


def planes_of(rng, H, W, sub, depth, top=None):
    dt = np.uint8 if depth == 8 else np.uint16
    top = top or (1 << depth)
    ch, cw = ref.chroma_shape(H, W, sub)
    return tuple(rng.integers(0, top, size=s).astype(dt) for s in ((H, W), (ch, cw), (ch, cw)))


class Job:
    """one frame on the device under a layout per plane and for the destination"""

    def __init__(self, ctx, planes, sub, layouts=("tight",) * 4):
        self.ctx, self.sub = ctx, sub
        self.H, self.W = planes[0].shape
        self.item = planes[0].itemsize
        self.strides = [stride_of(l, p.shape[1] * self.item, self.item) for l, p in zip(layouts[:3], planes)]
        self.bufs = [ctx.to_device(laid_out(p, s, 0x5A)) for p, s in zip(planes, self.strides)]
        self.row = self.W * 3 * self.item
        self.dstride = stride_of(layouts[3], self.row, self.item)
        self.total = self.H * self.dstride + GUARD
        self.dst = ctx.to_device(np.full(self.total, FILL, np.uint8))
        self.explicit = any(l != "tight" for l in layouts)

    def args(self):
        tail = tuple(self.strides) + (self.dstride,) if self.explicit else ()     # none = 0 = tight, the library's default
        return (self.bufs[0], self.bufs[1], self.bufs[2], self.W, self.H, self.sub, self.dst) + tail

    def check(self, want, what):
        got = self.ctx.download(self.dst, (self.total,))
        rows = got[:self.H * self.dstride].reshape(self.H, self.dstride)
        assert np.array_equal(rows[:, :self.row], np.ascontiguousarray(want).view(np.uint8).reshape(self.H, self.row)), what
        assert np.all(rows[:, self.row:] == FILL) and np.all(got[self.H * self.dstride:] == FILL), what + ": bytes outside the rows were written"

    def untouched(self):
        return bool(np.all(self.ctx.download(self.dst, (self.total,)) == FILL))

    def free(self):
        for b in self.bufs + [self.dst]:
            self.ctx.free(b)


def run(ctx, stage, jobs):
    stage.convert_dev(ctx, [j.args() for j in jobs])
    ctx.sync(0)


@pytest.mark.parametrize("depth", [8, 10])
def test_level_sweep(ctx, stages, depth):
    """16 frames of 256 x 256 per call: Y = x, Cb = y, Cr = 16 k + a seeded offset (8 bits); a seeded ramp over 0 .. 1023 with both
    ends and samples above 1023 (10 bits).  Both encodes, both ranges."""
    rng = np.random.default_rng(170 + depth)
    frames = []
    for k in range(16):
        if depth == 8:
            y = np.tile(np.arange(256, dtype=np.uint8)[None, :], (256, 1))
            cb = np.tile(np.arange(256, dtype=np.uint8)[:, None], (1, 256))
            cr = np.full((256, 256), 16 * k + int(rng.integers(0, 16)), np.uint8)
        else:
            ramp = np.sort(rng.integers(0, 1024, size=256)).astype(np.uint16)
            ramp[0], ramp[-2], ramp[-1] = 0, 1023, 1024 + int(rng.integers(0, 64000))
            y = np.tile(ramp[None, :], (256, 1))
            cb = np.tile(rng.permutation(ramp)[:, None], (1, 256))
            cr = np.full((256, 256), min(64 * k + int(rng.integers(0, 64)), 1023) if k < 15 else 2000, np.uint16)
        frames.append((y, cb, cr))
    jobs = [Job(ctx, f, "444") for f in frames]
    try:
        for full in (False, True):
            for keep in (False, True):
                run(ctx, stages(depth, full, keep), jobs)
                for k, (j, f) in enumerate(zip(jobs, frames)):
                    j.check(ref.convert(*f, depth, "444", full, keep), f"frame {k} full={full} keep={keep}")
    finally:
        for j in jobs:
            j.free()


SHAPES = [(33, 5), (70, 6), (1, 1), (8, 2), (9, 3), (530, 18)]


@pytest.mark.parametrize("depth", [8, 10])
@pytest.mark.parametrize("sub", ["420", "422", "444"])
def test_shapes(ctx, stages, depth, sub):
    """around the group (8 x 2) and, at 530 x 18 (67 groups a row, 9 group rows = 603 groups), past one tile of 512 groups; every
    shape tight and padded"""
    rng = np.random.default_rng(depth * 10 + len(sub))
    made = []
    try:
        for W, H in SHAPES:
            for layout in ("tight", "padded"):
                planes = planes_of(rng, H, W, sub, depth, top=1100 if depth == 10 else None)
                made.append((Job(ctx, planes, sub, (layout,) * 4), planes, f"{W}x{H} {layout}"))
        for at in range(0, len(made), capi.MAX_FRAMES):
            run(ctx, stages(depth), [m[0] for m in made[at:at + capi.MAX_FRAMES]])
        for job, planes, what in made:
            job.check(ref.convert(*planes, depth, sub), what)
    finally:
        for m in made:
            m[0].free()


@pytest.mark.parametrize("depth", [8, 10])
def test_strides_per_plane_and_destination(ctx, stages, depth):
    """tight, padded and non-dword strides for each plane and for the destination in turn (one odd stride sends the whole job pixel
    by pixel), 4:2:0 at 21 x 7"""
    rng = np.random.default_rng(1720 + depth)
    planes = planes_of(rng, 7, 21, "420", depth)
    want = ref.convert(*planes, depth, "420")
    cases = [("padded",) * 4, ("odd",) * 4]
    for which in range(4):
        for layout in ("padded", "odd"):
            cases.append(tuple(layout if k == which else "tight" for k in range(4)))
            cases.append(tuple("padded" if k != which else layout for k in range(4)))
    cases = sorted(set(cases))
    jobs = [Job(ctx, planes, "420", c) for c in cases]
    try:
        for at in range(0, len(jobs), capi.MAX_FRAMES):
            run(ctx, stages(depth), jobs[at:at + capi.MAX_FRAMES])
        for j, c in zip(jobs, cases):
            j.check(want, str(c))
    finally:
        for j in jobs:
            j.free()


@pytest.mark.parametrize("depth", [8, 10])
def test_sixteen_different_jobs_in_one_call(ctx, stages, depth):
    rng = np.random.default_rng(1730 + depth)
    made = []
    try:
        for k in range(16):
            W, H = int(rng.integers(1, 200)), int(rng.integers(1, 40))
            if k == 3:
                W, H = 4100, 3            # two tiles of its own
            sub = ("420", "422", "444")[k % 3]
            planes = planes_of(rng, H, W, sub, depth)
            made.append((Job(ctx, planes, sub, (("tight", "padded", "odd")[k % 3 if k % 5 else 0],) * 4), planes, sub))
        run(ctx, stages(depth, keep=True), [m[0] for m in made])
        for k, (job, planes, sub) in enumerate(made):
            job.check(ref.convert(*planes, depth, sub, keep_rec709=True), f"job {k}")
    finally:
        for m in made:
            m[0].free()


def test_the_host_convenience(ctx, stages):
    rng = np.random.default_rng(1740)
    for depth in (8, 10):
        for sub in ("420", "422", "444"):
            planes = planes_of(rng, 11, 37, sub, depth)
            assert np.array_equal(stages(depth).convert(ctx, *planes), ref.convert(*planes, depth, sub))


def test_refused_arguments_write_nothing(ctx, stages):
    rng = np.random.default_rng(1750)
    L = ctx.L

    def code_of(call):
        with pytest.raises(capi.Gs360Error) as e:
            call()
        return e.value.code

    s8, s10 = stages(8), stages(10)
    for depth in (0, 9, 12, 16):
        assert code_of(lambda: ctx.video_plan(depth, False, False, s8.matrix, s8.linear, s8.encode)) == capi.ERR_UNSUPPORTED
    bad = s8.linear.copy()
    bad[100] = 1.5
    assert code_of(lambda: ctx.video_plan(8, False, False, s8.matrix, bad, s8.encode)) == capi.ERR_ARG
    bad = s8.encode.copy()
    bad[5, 1] = np.nan
    assert code_of(lambda: ctx.video_plan(8, False, False, s8.matrix, s8.linear, bad)) == capi.ERR_ARG
    bad = s8.matrix.copy()
    bad[1, 1] = np.inf
    assert code_of(lambda: ctx.video_plan(8, False, False, bad, s8.linear, s8.encode)) == capi.ERR_ARG
    assert code_of(lambda: ctx.video_plan(8, 2, False, s8.matrix, s8.linear, s8.encode)) == capi.ERR_ARG

    for depth, stage in ((8, s8), (10, s10)):
        good = Job(ctx, planes_of(rng, 6, 10, "420", depth), "420", ("padded",) * 4)
        victim = Job(ctx, planes_of(rng, 6, 10, "420", depth), "420", ("padded",) * 4)
        try:
            y, cb, cr, W, H, sub, dst, ys, cbs, crs, ds = victim.args()
            item = victim.item
            refused = {
                "width 0": ((y, cb, cr, 0, H, sub, dst, ys, cbs, crs, ds), capi.ERR_ARG),
                "height 0": ((y, cb, cr, W, 0, sub, dst, ys, cbs, crs, ds), capi.ERR_ARG),
                "negative width": ((y, cb, cr, -3, H, sub, dst, ys, cbs, crs, ds), capi.ERR_ARG),
                "width 65536": ((y, cb, cr, 65536, H, sub, dst, 1 << 20, 1 << 20, 1 << 20, 1 << 20), capi.ERR_ARG),
                "height 65536": ((y, cb, cr, W, 65536, sub, dst, ys, cbs, crs, ds), capi.ERR_ARG),
                "short luma stride": ((y, cb, cr, W, H, sub, dst, W * item - item, cbs, crs, ds), capi.ERR_ARG),
                "short cb stride": ((y, cb, cr, W, H, sub, dst, ys, (W // 2) * item - item, crs, ds), capi.ERR_ARG),
                "short cr stride": ((y, cb, cr, W, H, sub, dst, ys, cbs, (W // 2) * item - item, ds), capi.ERR_ARG),
                "short destination stride": ((y, cb, cr, W, H, sub, dst, ys, cbs, crs, 3 * W * item - item), capi.ERR_ARG),
                "null plane": ((y, 0, cr, W, H, sub, dst, ys, cbs, crs, ds), capi.ERR_ARG),
                "null destination": ((y, cb, cr, W, H, sub, 0, ys, cbs, crs, ds), capi.ERR_ARG),
            }
            if depth == 10:
                refused["odd luma stride"] = ((y, cb, cr, W, H, sub, dst, ys + 1, cbs, crs, ds), capi.ERR_ARG)
                refused["odd destination stride"] = ((y, cb, cr, W, H, sub, dst, ys, cbs, crs, ds + 1), capi.ERR_ARG)
                refused["odd plane address"] = ((y, cb.ptr + 1, cr, W, H, sub, dst, ys, cbs, crs, ds), capi.ERR_ARG)
            for what, (args, code) in refused.items():
                # the bad job comes second: the good one before it must not be converted either
                assert code_of(lambda: ctx.video_rgb_dev(stage.plan(ctx), [good.args()[:5] + (SUB_CODE["420"],) + good.args()[6:],
                                                                            args[:5] + (SUB_CODE["420"],) + args[6:]])) == code, what
                ctx.sync(0)
                assert good.untouched() and victim.untouched(), what
            plan = stage.plan(ctx)
            one = good.args()[:5] + (7,) + good.args()[6:]
            assert code_of(lambda: ctx.video_rgb_dev(plan, [one])) == capi.ERR_UNSUPPORTED
            ok = good.args()[:5] + (SUB_CODE["420"],) + good.args()[6:]
            assert code_of(lambda: ctx.video_rgb_dev(plan, [ok] * 17)) == capi.ERR_ARG
            assert code_of(lambda: ctx.video_rgb_dev(plan, [ok], slot=99)) == capi.ERR_ARG
            ctx.sync(0)
            assert good.untouched()
            ctx.video_rgb_dev(plan, [])            # no job: nothing to do
            assert L.gs360_video_rgb(ctx.handle, None, None, 1, 0) == capi.ERR_ARG
        finally:
            good.free()
            victim.free()
