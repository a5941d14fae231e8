"""VID-FEED v1 on the GPU.  The (10, 8) format through the C ABI, byte for byte against tests/vidfeed_np.py, with
its refusals; and gs360_360PerspCut.py's video jobs under GS360_VIDEO_FEED=planes with a double standing in for the ffmpeg binary
(tests/fake_ffmpeg_planes.py, which refuses to convert colours): clip -> Y4M pipe -> device planes -> resident RGB frames -> views ->
numbered files, every resident frame against the restatement and every written view against the oracle's view of that frame."""
import stat
import sys
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

import vidcolor_np as ref
import vidfeed_np as feed_ref
from conftest import ROOT
from gs360 import capi, imageio, vidcolor, video
from test_vidcolor_cpu import extremes10
from test_vidcolor_gpu import FILL, GUARD, Job, planes_of, stride_of
from test_vidfeed_cpu import plan_jobs
from util import HFOV_12MM

pytestmark = pytest.mark.gpu

FAKE = ROOT / "tests" / "fake_ffmpeg_planes.py"


# ---- the (10, 8) format through gs360_video_rgb ------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def stages(ctx):
    made = {}

    def get(full=False, keep=False):
        if (full, keep) not in made:
            made[full, keep] = vidcolor.VideoColor(10, full, keep, out_bits=8)
        return made[full, keep]
    yield get
    for s in made.values():
        s.close()


class FeedJob(Job):
    """uint16 planes, a uint8 destination: the destination's row, stride and sentinel follow the 8-bit samples"""

    def __init__(self, ctx, planes, sub, layouts=("tight",) * 4):
        super().__init__(ctx, planes, sub, layouts)
        ctx.free(self.dst)
        self.row = self.W * 3
        self.dstride = stride_of(layouts[3], self.row, 1)
        self.total = self.H * self.dstride + GUARD
        self.dst = ctx.to_device(np.full(self.total, FILL, np.uint8))


def run(ctx, stage, jobs):
    stage.convert_dev(ctx, [j.args() for j in jobs])
    ctx.sync(0)


SHAPES = [(17, 5, "420"), (24, 6, "422"), (9, 3, "444"), (7, 1, "420")]
LAYOUTS = [("tight",) * 4, ("padded",) * 4, ("padded", "odd", "padded", "odd")]      # the last one: a plane and the destination off the dword


@pytest.mark.parametrize("full", [False, True])
@pytest.mark.parametrize("keep", [False, True])
def test_shapes_layouts_ranges_and_curves(ctx, stages, full, keep):
    rng = np.random.default_rng(1930 + 2 * full + keep)
    made = []
    try:
        for W, H, sub in SHAPES:
            for layout in LAYOUTS:
                planes = planes_of(rng, H, W, sub, 10, top=1100)
                made.append((FeedJob(ctx, planes, sub, layout), planes, sub, f"{W}x{H} {sub} {layout}"))
        assert len(made) <= capi.MAX_FRAMES
        run(ctx, stages(full, keep), [m[0] for m in made])
        for job, planes, sub, what in made:
            job.check(feed_ref.convert(*planes, sub, full, keep), what)
    finally:
        for m in made:
            m[0].free()


def test_sixteen_mixed_jobs_one_past_a_tile_and_the_extremes(ctx, stages):
    """one call of 16 jobs: mixed sizes, subsamplings and layouts; 264 x 32 (33 groups a row, 16 group rows = 528 groups, past a tile
    of 512 lanes); every 10-bit triple with two components at an end, as a one-row 4:4:4 image"""
    rng = np.random.default_rng(1934)
    made = []
    try:
        t = extremes10().astype(np.uint16)
        ext = tuple(np.ascontiguousarray(t[:, c][None, :]) for c in range(3))
        made.append((FeedJob(ctx, ext, "444", ("padded",) * 4), ext, "444"))
        big = planes_of(rng, 32, 264, "420", 10, top=1100)
        assert -(-264 // 8) * (32 // 2) == 528
        made.append((FeedJob(ctx, big, "420"), big, "420"))
        for k in range(14):
            W, H = int(rng.integers(1, 120)), int(rng.integers(1, 24))
            sub = ("420", "422", "444")[k % 3]
            planes = planes_of(rng, H, W, sub, 10, top=1100)
            made.append((FeedJob(ctx, planes, sub, (("tight", "padded", "odd")[k % 3 if k % 5 else 0],) * 4), planes, sub))
        assert len(made) == capi.MAX_FRAMES == 16
        run(ctx, stages(), [m[0] for m in made])
        for k, (job, planes, sub) in enumerate(made):
            job.check(feed_ref.convert(*planes, sub), f"job {k}")
    finally:
        for m in made:
            m[0].free()


def test_the_host_convenience_and_the_default_pairing(ctx, stages):
    rng = np.random.default_rng(1935)
    planes = planes_of(rng, 11, 37, "420", 10)
    got = stages().convert(ctx, *planes)
    assert got.dtype == np.uint8 and np.array_equal(got, feed_ref.convert(*planes, "420"))
    s = vidcolor.VideoColor(10)
    try:
        assert np.array_equal(s.convert(ctx, *planes), ref.convert(*planes, 10, "420"))
    finally:
        s.close()


def test_refusals(ctx, stages):
    rng = np.random.default_rng(1936)

    def code_of(call):
        with pytest.raises(capi.Gs360Error) as e:
            call()
        return e.value.code

    s = stages()
    assert code_of(lambda: ctx.video_plan(8, False, False, s.matrix, s.linear, s.encode, out_bits=16)) == capi.ERR_UNSUPPORTED
    for depth in (8, 10):
        for out_bits in (12, 0, 10, 32):
            assert code_of(lambda: ctx.video_plan(depth, False, False, s.matrix, s.linear, s.encode, out_bits=out_bits)) == capi.ERR_UNSUPPORTED
    # the encode cells are checked against the plan's own largest level: a 16-bit table is no (10, 8) table
    assert code_of(lambda: ctx.video_plan(10, False, False, s.matrix, s.linear, vidcolor.encode_table(False, 65535), out_bits=8)) == capi.ERR_ARG
    # the fisheye entry point takes no (10, 8) plan, and says so before anything is written
    victim = FeedJob(ctx, planes_of(rng, 6, 10, "420", 10), "420", ("padded",) * 4)
    try:
        view = (capi.FISHEYE_EQUIDISTANT, 4, 10, 6, 180.0, 90.0, 90.0)
        assert code_of(lambda: ctx.video_fisheye_rgb_dev(s.plan(ctx), view, [victim.args()])) == capi.ERR_UNSUPPORTED
        ctx.sync(0)
        assert victim.untouched()
        # an odd destination stride is fine for uint8 RGB, an odd plane address is not
        y, cb, cr, W, H, sub, dst, ys, cbs, crs, ds = victim.args()
        assert code_of(lambda: s.convert_dev(ctx, [(y.ptr + 1, cb, cr, W, H, sub, dst, ys, cbs, crs, ds)])) == capi.ERR_ARG
        ctx.sync(0)
        assert victim.untouched()
    finally:
        victim.free()


# ---- gs360_360PerspCut.py under GS360_VIDEO_FEED=planes ---------------------------------------------------------------------------------
VIEWS = ((0.0, "A"), (120.0, "B"), (-120.0, "C"))


def make_clip(path, n, H, W, depth, tag, full=False, seed=1940):
    rng = np.random.default_rng(seed)
    dt = np.uint8 if depth == 8 else np.uint16
    y = rng.integers(0, 1 << depth, size=(n, H, W)).astype(dt)
    u, v = (rng.integers(0, 1 << depth, size=(n, H // 2, W // 2)).astype(dt) for _ in range(2))
    np.savez(path, y=y, u=u, v=v, tag=tag, full=full)
    return y, u, v


def double_program(tmp_path):
    p = tmp_path / "ffmpeg_double"
    p.write_text("#!/bin/sh\nexec {} {} \"$@\"\n".format(sys.executable, FAKE))
    p.chmod(p.stat().st_mode | stat.S_IXUSR)
    return str(p)


@pytest.fixture
def planes_engine(monkeypatch):
    """a fresh engine that reads GS360_VIDEO_FEED=planes, and a fresh one again for whatever runs next; the resident frames as the
    reader publishes them"""
    from gs360 import engine
    import gs360_360PerspCut as cut
    monkeypatch.setenv("GS360_VIDEO_FEED", "planes")
    monkeypatch.setenv("GS360_INTERP", "linear")
    engine.shutdown()
    cut.stop_event.clear()
    published = []
    real = video.VideoSession._publish

    def spy(self, st, buf, h, w, fdtype, nbytes):
        with st.upload_lock:
            published.append(st.ctx.download(buf, (h, w, 3), dtype=fdtype, slot=st.upload_slot))
        return real(self, st, buf, h, w, fdtype, nbytes)
    monkeypatch.setattr(video.VideoSession, "_publish", spy)
    yield engine, cut, published
    engine.shutdown()


def run_jobs(cut, cmds, workers=3):
    with ThreadPoolExecutor(max_workers=workers) as pool:
        results = list(pool.map(cut.run_one, cmds))
    assert results == [(0, "")] * len(cmds), results


def check_views(orc, out_dir, frames, ext, jpeg_q=None, size=40):
    """every written view equals the oracle's view of that RGB frame (a .jpg: the host encoder's bytes of the oracle's view)"""
    for yaw, tag in VIEWS:
        for n, fr in enumerate(frames):
            path = out_dir / f"clip_{n:07d}_{tag}.{ext}"
            views = [orc.make_view(yaw, 0.0, HFOV_12MM, HFOV_12MM, size, size)]
            want = (orc.equirect_views_u16 if fr.dtype == np.uint16 else orc.equirect_views_u8)(fr, views)[0]
            if ext == "jpg":
                imageio.write_image(out_dir / "want.jpg", want, jpeg_q=jpeg_q)
                assert path.read_bytes() == (out_dir / "want.jpg").read_bytes(), (tag, n)
            else:
                got = imageio.read_image(path)
                assert got.dtype == want.dtype and np.array_equal(got, want), (tag, n)
        assert not (out_dir / f"clip_{len(frames):07d}_{tag}.{ext}").exists()


def test_8_bit_clip_png_views(tmp_path, orc, planes_engine):
    engine, cut, published = planes_engine
    y, u, v = make_clip(tmp_path / "clip.npz", 5, 32, 64, 8, "420jpeg")
    res = plan_jobs(tmp_path, ["-f", "1", "--ext", "png", "--count", "3", "--size", "40"], ffmpeg=double_program(tmp_path), name="clip.npz")
    (tmp_path / "out").mkdir()
    run_jobs(cut, [cmd for cmd, _s, _d in res.jobs])
    eng = engine.get_engine()
    assert eng.video_feed == "planes" and eng.video_feed_stats() == {"plane_fed_frames": 5, "feed_fallbacks": 0}
    assert not eng.videos
    want = [ref.convert(y[k], u[k], v[k], 8, "420") for k in range(5)]
    assert len(published) == 5 and all(g.dtype == np.uint8 and np.array_equal(g, w) for g, w in zip(published, want))
    check_views(orc, tmp_path / "out", want, "png")


def test_10_bit_clip_feeds_8_bit_frames_to_jpg_views(tmp_path, orc, planes_engine):
    engine, cut, published = planes_engine
    y, u, v = make_clip(tmp_path / "clip.npz", 5, 32, 64, 10, "420p10", seed=1941)
    res = plan_jobs(tmp_path, ["-f", "1", "--count", "3", "--size", "40"], bit_depth=10, ffmpeg=double_program(tmp_path), name="clip.npz")
    assert res.jobs[0][0][-1].endswith(".jpg")
    (tmp_path / "out").mkdir()
    run_jobs(cut, [cmd for cmd, _s, _d in res.jobs])
    assert engine.get_engine().video_feed_stats() == {"plane_fed_frames": 5, "feed_fallbacks": 0}
    want = [feed_ref.convert(y[k], u[k], v[k], "420") for k in range(5)]
    assert len(published) == 5 and all(g.dtype == np.uint8 and np.array_equal(g, w) for g, w in zip(published, want))
    from gs360.jobspec import parse_job_argv
    check_views(orc, tmp_path / "out", want, "jpg", jpeg_q=parse_job_argv(res.jobs[0][0]).jpeg_q)


def test_10_bit_clip_and_a_job_that_asks_for_rgb24(tmp_path, orc, planes_engine):
    engine, cut, published = planes_engine
    y, u, v = make_clip(tmp_path / "clip.npz", 5, 32, 64, 10, "420p10", seed=1942)
    res = plan_jobs(tmp_path, ["-f", "1", "--ext", "png", "--count", "3", "--size", "40"], ffmpeg=double_program(tmp_path), name="clip.npz")
    cmds = [cmd for cmd, _s, _d in res.jobs]
    assert all(c[c.index("-pix_fmt") + 1] == "rgb24" for c in cmds)
    (tmp_path / "out").mkdir()
    run_jobs(cut, cmds)
    assert engine.get_engine().video_feed_stats() == {"plane_fed_frames": 5, "feed_fallbacks": 0}
    want = [feed_ref.convert(y[k], u[k], v[k], "420") for k in range(5)]
    assert len(published) == 5 and all(g.dtype == np.uint8 and np.array_equal(g, w) for g, w in zip(published, want))
    check_views(orc, tmp_path / "out", want, "png")


def test_10_bit_clip_and_rgb48le_keep_16_bit_frames(tmp_path, orc, planes_engine):
    engine, cut, published = planes_engine
    y, u, v = make_clip(tmp_path / "clip.npz", 5, 32, 64, 10, "420p10", seed=1943)
    res = plan_jobs(tmp_path, ["-f", "1", "--ext", "png", "--count", "3", "--size", "40"], bit_depth=10, ffmpeg=double_program(tmp_path),
                    name="clip.npz")
    cmds = [cmd for cmd, _s, _d in res.jobs]
    assert all(c[c.index("-pix_fmt") + 1] == "rgb48le" for c in cmds)
    (tmp_path / "out").mkdir()
    run_jobs(cut, cmds)
    assert engine.get_engine().video_feed_stats() == {"plane_fed_frames": 5, "feed_fallbacks": 0}
    want = [ref.convert(y[k], u[k], v[k], 10, "420") for k in range(5)]
    assert len(published) == 5 and all(g.dtype == np.uint16 and np.array_equal(g, w) for g, w in zip(published, want))
    check_views(orc, tmp_path / "out", want, "png")


def test_full_range_clip_and_keep_rec709(tmp_path, orc, planes_engine):
    engine, cut, published = planes_engine
    y, u, v = make_clip(tmp_path / "clip.npz", 5, 32, 64, 8, "420jpeg", full=True, seed=1944)
    res = plan_jobs(tmp_path, ["-f", "1", "--ext", "png", "--count", "3", "--size", "40", "--keep-rec709"], ffmpeg=double_program(tmp_path),
                    name="clip.npz")
    (tmp_path / "out").mkdir()
    run_jobs(cut, [cmd for cmd, _s, _d in res.jobs])
    assert engine.get_engine().video_feed_stats() == {"plane_fed_frames": 5, "feed_fallbacks": 0}
    want = [ref.convert(y[k], u[k], v[k], 8, "420", full_range=True, keep_rec709=True) for k in range(5)]
    assert len(published) == 5 and all(np.array_equal(g, w) for g, w in zip(published, want))
    assert not np.array_equal(want[0], ref.convert(y[0], u[0], v[0], 8, "420"))
    check_views(orc, tmp_path / "out", want, "png")


def test_streaming_past_the_budget(tmp_path, orc, planes_engine, monkeypatch):
    """tests/test_video_session.py's budget test under the planes feed: a budget of two RGB frames, 10 frames x 3 views with two
    workers (the third view job arrives after the first frames were retired and is served by a second decode); the frames written are
    complete and in order"""
    engine, cut, published = planes_engine
    y, u, v = make_clip(tmp_path / "clip.npz", 10, 64, 128, 8, "420jpeg", seed=1945)
    monkeypatch.setattr(video, "_BUDGET_BYTES", 2 * 64 * 128 * 3 + 100)
    res = plan_jobs(tmp_path, ["-f", "1", "--ext", "png", "--count", "3", "--size", "40"], ffmpeg=double_program(tmp_path), name="clip.npz")
    (tmp_path / "out").mkdir()
    run_jobs(cut, [cmd for cmd, _s, _d in res.jobs], workers=2)
    eng = engine.get_engine()
    stats = eng.video_feed_stats()
    assert not eng.videos and stats["feed_fallbacks"] == 0 and stats["plane_fed_frames"] >= 10
    want = [ref.convert(y[k], u[k], v[k], 8, "420") for k in range(10)]
    check_views(orc, tmp_path / "out", want, "png")
