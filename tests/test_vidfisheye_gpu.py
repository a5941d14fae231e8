"""VID-FISHEYE v1 on the GPU, through the C ABI (Context.video_fisheye_rgb_dev), byte for byte against tests/vidfisheye_np.py, with
sentinel-filled destinations and guard bytes behind them.

The workgroup tile is 32 x 16 output pixels (kVfTileW x kVfTileH of csrc/gs360_vidfishsteps.h), a wavefront takes 16 x 4 of them.
Which path a lane takes: a job whose three plane pointers and strides are all multiples of 4 fetches the four taps of a row as 2
(uint8) or 3 (uint16) aligned dwords wherever the 4 x 4 window lies inside the plane and the dwords inside the row; every other lane,
and every lane of any other job, reads sample by sample with clamped indices.  At 48 x 32 -> 64 under a 120 degree lens and a 150
degree view about half of the view looks past the lens (black) and the visible part reaches all four edges of the source."""
import numpy as np
import pytest

import vidcolor_np as vc
import vidfisheye_np as ref
from gs360 import capi, vidcolor, vidfisheye

pytestmark = pytest.mark.gpu

GUARD = 64
FILL = 0xA5
WIDE = (120.0, 150.0, 150.0)          # input fov, view fov: half of the view is invisible
SUB_CODE = vidcolor.SUBSAMPLING
PROJ_CODE = vidfisheye.PROJECTIONS


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


def laid_out(plane, stride, fill, lead=0):
    """the plane's rows `stride` bytes apart, `lead` bytes into a byte buffer filled with `fill`"""
    H = plane.shape[0]
    row = plane.shape[1] * plane.itemsize
    buf = np.full(lead + H * stride, fill, np.uint8)
    buf[lead:].reshape(H, stride)[:, :row] = np.ascontiguousarray(plane).view(np.uint8).reshape(H, row)
    return buf


def planes_of(rng, H, W, sub, depth, top=None):
    dt = np.uint8 if depth == 8 else np.uint16
    top = top or (1 << depth)
    ch, cw = vc.chroma_shape(H, W, sub)
    return tuple(rng.integers(0, top, size=s).astype(dt) for s in ((H, W), (ch, cw), (ch, cw)))


class Job:
    """one source frame on the device under a layout per plane, and an S x S destination under its own"""

    def __init__(self, ctx, planes, sub, S, layouts=("tight",) * 4, lead=(0, 0, 0)):
        self.ctx, self.sub, self.S = ctx, sub, S
        self.H, self.W = planes[0].shape
        self.item = planes[0].itemsize
        self.strides = [stride_of(l, p.shape[1] * self.item, self.item) for l, p in zip(layouts[:3], planes)]
        self.bufs = [ctx.to_device(laid_out(p, s, 0x5A, n)) for p, s, n in zip(planes, self.strides, lead)]
        self.lead = lead
        self.row = S * 3 * self.item
        self.dstride = stride_of(layouts[3], self.row, self.item)
        self.total = S * self.dstride + GUARD
        self.dst = ctx.to_device(np.full(self.total, FILL, np.uint8))
        self.explicit = any(l != "tight" for l in layouts)

    def args(self):
        tail = tuple(self.strides) + (self.dstride,) if self.explicit else ()     # none = 0 = tight, the library's default
        return tuple(b.ptr + n for b, n in zip(self.bufs, self.lead)) + (self.W, self.H, self.sub, self.dst) + tail

    def check(self, want, what):
        got = self.ctx.download(self.dst, (self.total,))
        rows = got[:self.S * self.dstride].reshape(self.S, self.dstride)
        assert np.array_equal(rows[:, :self.row], np.ascontiguousarray(want).view(np.uint8).reshape(self.S, self.row)), what
        assert np.all(rows[:, self.row:] == FILL) and np.all(got[self.S * self.dstride:] == FILL), what + ": bytes outside the rows were written"

    def untouched(self):
        return bool(np.all(self.ctx.download(self.dst, (self.total,)) == FILL))

    def free(self):
        for b in self.bufs + [self.dst]:
            self.ctx.free(b)


def view_of(projection, S, geo=WIDE):
    return vidfisheye.FisheyeView(projection, S, *geo)


def run(ctx, color, view, jobs):
    vidfisheye.FisheyeStage(view, color.depth, color=color).convert_dev(ctx, [j.args() for j in jobs])
    ctx.sync(0)


def render(planes, depth, sub, view, full=False, keep=False):
    return ref.render(*planes, depth, sub, view.projection, view.size, view.input_fov_deg, view.h_fov_deg, view.v_fov_deg, full, keep)


@pytest.mark.parametrize("projection", ["equidistant", "equisolid"])
@pytest.mark.parametrize("depth", [8, 10])
@pytest.mark.parametrize("sub", ["420", "422", "444"])
def test_depths_and_subsamplings(ctx, stages, sub, depth, projection):
    """48 x 32 -> 64 (half invisible, every edge clamped) and 33 x 5 -> 7, tight and padded"""
    rng = np.random.default_rng(1800 + depth + len(projection) * 7 + int(sub))
    for W, H, S in ((48, 32, 64), (33, 5, 7)):
        view = view_of(projection, S)
        planes = planes_of(rng, H, W, sub, depth)
        jobs = [Job(ctx, planes, sub, S, (layout,) * 4) for layout in ("tight", "padded")]
        try:
            run(ctx, stages(depth), view, jobs)
            want = render(planes, depth, sub, view)
            assert want.any() and (want == 0).all(axis=2).any()        # visible and invisible pixels
            for j, layout in zip(jobs, ("tight", "padded")):
                j.check(want, f"{W}x{H} -> {S} {layout}")
        finally:
            for j in jobs:
                j.free()


@pytest.mark.parametrize("depth", [8, 10])
def test_tile_edges(ctx, stages, depth):
    """the tile is 32 x 16: S one less than, equal to and one more than each side, and 70 (3 x 5 tiles per job, two jobs)"""
    rng = np.random.default_rng(1810 + depth)
    planes = [planes_of(rng, 32, 48, "420", depth) for _ in range(2)]
    for S in (15, 16, 17, 31, 32, 33, 70):
        view = view_of("equisolid", S)
        jobs = [Job(ctx, p, "420", S, ("padded",) * 4) for p in planes]
        try:
            run(ctx, stages(depth), view, jobs)
            for k, (j, p) in enumerate(zip(jobs, planes)):
                j.check(render(p, depth, "420", view), f"S {S} job {k}")
        finally:
            for j in jobs:
                j.free()


def test_a_source_of_one_sample(ctx, stages):
    rng = np.random.default_rng(1820)
    for depth in (8, 10):
        for sub in ("420", "444"):
            for projection, S in (("equidistant", 9), ("equisolid", 1)):
                planes = planes_of(rng, 1, 1, sub, depth)
                view = view_of(projection, S, (180.0, 90.0, 90.0))
                job = Job(ctx, planes, sub, S)
                try:
                    run(ctx, stages(depth), view, [job])
                    want = render(planes, depth, sub, view)
                    assert want[S // 2, S // 2].tolist() == vc.convert_triples(*(p[0, 0] for p in planes), depth).tolist()
                    job.check(want, f"1x1 -> {S} {sub} {depth}")
                finally:
                    job.free()


def test_samples_above_1023(ctx, stages):
    """a 10-bit source whose samples run up to 65535: each is clamped to 1023 before it is weighted"""
    rng = np.random.default_rng(1830)
    planes = planes_of(rng, 32, 48, "422", 10, top=65536)
    planes[0][::3, ::2] = 65535
    view = view_of("equidistant", 64)
    job = Job(ctx, planes, "422", 64, ("padded",) * 4)
    try:
        run(ctx, stages(10), view, [job])
        job.check(render(planes, 10, "422", view), "large samples")
        job.check(render(tuple(np.minimum(p, 1023) for p in planes), 10, "422", view), "the clamped source gives the same view")
    finally:
        job.free()


def test_ranges_and_curves(ctx, stages):
    rng = np.random.default_rng(1840)
    for depth, full, keep in ((8, True, False), (10, False, True), (8, True, True)):
        planes = planes_of(rng, 32, 48, "420", depth)
        view = view_of("equisolid", 33)
        job = Job(ctx, planes, "420", 33, ("padded",) * 4)
        try:
            run(ctx, stages(depth, full, keep), view, [job])
            want = render(planes, depth, "420", view, full, keep)
            assert not np.array_equal(want, render(planes, depth, "420", view))
            job.check(want, f"full {full} keep {keep}")
        finally:
            job.free()


@pytest.mark.parametrize("depth", [8, 10])
def test_layouts_per_plane_and_destination(ctx, stages, depth):
    """tight, padded and non-dword strides for each plane and for the destination in turn, and each plane's pointer off a dword
    boundary (by one sample) under padded strides: one such plane sends the whole job sample by sample"""
    rng = np.random.default_rng(1850 + depth)
    planes = planes_of(rng, 32, 48, "420", depth)
    view = view_of("equidistant", 33)
    want = render(planes, depth, "420", view)
    cases = [(("padded",) * 4, (0, 0, 0)), (("odd",) * 4, (0, 0, 0))]
    for which in range(4):
        for layout in ("padded", "odd"):
            cases.append((tuple(layout if k == which else "tight" for k in range(4)), (0, 0, 0)))
            cases.append((tuple("padded" if k != which else layout for k in range(4)), (0, 0, 0)))
    item = 1 if depth == 8 else 2
    for which in range(3):
        cases.append((("padded",) * 4, tuple(item if k == which else 0 for k in range(3))))
    cases = sorted(set(cases))
    jobs = [Job(ctx, planes, "420", 33, c, lead) for c, lead in cases]
    try:
        for at in range(0, len(jobs), capi.MAX_FRAMES):
            run(ctx, stages(depth), view, jobs[at:at + capi.MAX_FRAMES])
        for j, c in zip(jobs, cases):
            j.check(want, str(c))
    finally:
        for j in jobs:
            j.free()


@pytest.mark.parametrize("depth", [8, 10])
def test_sixteen_different_sources_in_one_call(ctx, stages, depth):
    rng = np.random.default_rng(1860 + depth)
    view = view_of("equisolid", 40, (150.0, 140.0, 140.0))
    made = []
    try:
        for k in range(16):
            sub = ("420", "422", "444")[k % 3]
            planes = planes_of(rng, 27, 53, sub, depth)
            made.append((Job(ctx, planes, sub, 40, (("tight", "padded", "odd")[k % 3 if k % 5 else 0],) * 4), planes, sub))
        run(ctx, stages(depth, keep=True), view, [m[0] for m in made])
        for k, (job, planes, sub) in enumerate(made):
            job.check(render(planes, depth, sub, view, keep=True), f"job {k}")
    finally:
        for m in made:
            m[0].free()


def test_the_host_convenience(ctx):
    rng = np.random.default_rng(1870)
    for depth in (8, 10):
        for sub in ("420", "422", "444"):
            planes = planes_of(rng, 11, 37, sub, depth)
            view = vidfisheye.view_from_args(8.0, 21, "equisolid", 180.0)
            stage = vidfisheye.FisheyeStage(view, depth)
            try:
                got = stage.convert(ctx, *planes)
            finally:
                stage.close()
            assert got.shape == (21, 21, 3) and np.array_equal(got, render(planes, depth, sub, view))


def test_refused_arguments_write_nothing(ctx, stages):
    rng = np.random.default_rng(1880)
    L = ctx.L

    def code_of(call):
        with pytest.raises(capi.Gs360Error) as e:
            call()
        return e.value.code

    for depth in (8, 10):
        plan = stages(depth).plan(ctx)
        S, W, H = 20, 10, 6
        good = Job(ctx, planes_of(rng, H, W, "420", depth), "420", S, ("padded",) * 4)
        victim = Job(ctx, planes_of(rng, H, W, "420", depth), "420", S, ("padded",) * 4)
        try:
            y, cb, cr, _, _, _, dst, ys, cbs, crs, ds = victim.args()
            item = victim.item
            code = SUB_CODE["420"]
            view = (PROJ_CODE["equisolid"], S, W, H, 120.0, 150.0, 150.0)
            ok = good.args()[:5] + (code,) + good.args()[6:]

            def job(y=y, cb=cb, cr=cr, W=W, H=H, sub=code, dst=dst, ys=ys, cbs=cbs, crs=crs, ds=ds):
                return (y, cb, cr, W, H, sub, dst, ys, cbs, crs, ds)

            def with_view(**kw):
                d = dict(zip(("projection", "size", "W", "H", "ifov", "hfov", "vfov"), view))
                d.update(kw)
                return tuple(d.values())
            refused = {
                "S 0": (with_view(size=0), job(), capi.ERR_ARG),
                "S 16385": (with_view(size=16385), job(ds=1 << 20), capi.ERR_ARG),
                "source side 16385": (with_view(W=16385), job(W=16385, ys=1 << 20, cbs=1 << 20, crs=1 << 20), capi.ERR_ARG),
                "another width than the view's": (view, job(W=W - 2), capi.ERR_ARG),
                "another height than the view's": (view, job(H=H - 2), capi.ERR_ARG),
                "short luma stride": (view, job(ys=W * item - item), capi.ERR_ARG),
                "short cb stride": (view, job(cbs=(W // 2) * item - item), capi.ERR_ARG),
                "short cr stride": (view, job(crs=(W // 2) * item - item), capi.ERR_ARG),
                "short destination stride": (view, job(ds=3 * S * item - item), capi.ERR_ARG),
                "a destination stride of the source's row": (view, job(ds=3 * W * item), capi.ERR_ARG),
                "null plane": (view, job(cb=0), capi.ERR_ARG),
                "null destination": (view, job(dst=0), capi.ERR_ARG),
                "subsampling 7": (view, job(sub=7), capi.ERR_UNSUPPORTED),
                "projection 7": (with_view(projection=7), job(), capi.ERR_ARG),
                "input fov 0": (with_view(ifov=0.0), job(), capi.ERR_ARG),
                "input fov 361": (with_view(ifov=361.0), job(), capi.ERR_ARG),
                "view fov 0": (with_view(hfov=0.0), job(), capi.ERR_ARG),
                "view fov 179.5": (with_view(vfov=179.5), job(), capi.ERR_ARG),
                "a fov that is no number": (with_view(hfov=float("nan")), job(), capi.ERR_ARG),
                "a null view": (None, job(), capi.ERR_ARG),
            }
            if depth == 10:
                refused["odd luma stride"] = (view, job(ys=ys + 1), capi.ERR_ARG)
                refused["odd destination stride"] = (view, job(ds=ds + 1), capi.ERR_ARG)
                refused["odd plane address"] = (view, job(cb=cb + 1), capi.ERR_ARG)
                refused["odd destination address"] = (view, job(dst=dst.ptr + 1), capi.ERR_ARG)
            for what, (v, bad, want) in refused.items():
                # the bad job comes second: the good one before it must not be rendered either
                assert code_of(lambda: ctx.video_fisheye_rgb_dev(plan, v, [ok, bad])) == want, what
                ctx.sync(0)
                assert good.untouched() and victim.untouched(), what
            assert code_of(lambda: ctx.video_fisheye_rgb_dev(plan, view, [ok] * 17)) == capi.ERR_ARG
            assert code_of(lambda: ctx.video_fisheye_rgb_dev(plan, view, [ok], slot=99)) == capi.ERR_ARG
            ctx.sync(0)
            assert good.untouched()
            ctx.video_fisheye_rgb_dev(plan, view, [])          # no job: nothing to do
            assert L.gs360_video_fisheye_rgb(ctx.handle, None, None, None, 1, 0) == capi.ERR_ARG
            # and the good job, sent alone, is rendered
            ctx.video_fisheye_rgb_dev(plan, view, [ok])
            ctx.sync(0)
            assert not good.untouched()
        finally:
            good.free()
            victim.free()
