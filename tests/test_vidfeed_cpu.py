"""VID-FEED v1 without a GPU: the `planes` decode plans derived from the planner's and the GUI's job argv,
the GS360_VIDEO_FEED switch, the (10, 8) restatement (tests/vidfeed_np.py) against test_vidcolor_cpu's float64 mathematics, and the
session's way back to the PPM feed at a stream header it cannot convert (decoder double as a real child process, device memory faked)."""
import sys

import numpy as np
import pytest

import vidfeed_np as feed_ref
from conftest import ROOT
from gs360 import video
from gs360.jobspec import parse_job_argv
from test_vidcolor_cpu import extremes10, ideal_encode, ideal_linear
from test_video_session import _FakeState, gui_select_rewrite

FAKE = ROOT / "tests" / "fake_ffmpeg_planes.py"
CS = "colorspace=iall=bt709:all=smpte170m"


def plan_jobs(tmp_path, extra, bit_depth=8, ffmpeg="ffmpeg", name="clip.mp4"):
    import gs360_360PerspCut as cut
    args = cut.create_arg_parser().parse_args(["-i", str(tmp_path / name), "--ffmpeg", ffmpeg] + extra)
    for attr in ("size", "hfov", "focal_mm"):
        setattr(args, f"{attr}_explicit", getattr(args, f"{attr}_explicit", False))
    args.input_is_video, args.video_bit_depth = True, bit_depth
    return cut.build_view_jobs(args, [tmp_path / name], tmp_path / "out")


def y4m_tail(chain):
    return ["-vf", chain, "-an", "-f", "yuv4mpegpipe", "-strict", "-1", "pipe:1"]


# ---- decode plans ---------------------------------------------------------------------------------------------------------------------
def test_planes_plan_of_the_planners_png_job(tmp_path):
    res = plan_jobs(tmp_path, ["-f", "2", "--ext", "png", "--start", "3", "--end", "12.5", "--count", "4"])
    jobs = [parse_job_argv(cmd) for cmd, _s, _d in res.jobs]
    plans = [video.build_decode_plan(j, "planes") for j in jobs]
    assert len({p.key for p in plans}) == 1                     # every view shares one decode
    p, src = plans[0], str(tmp_path / "clip.mp4")
    head = ["ffmpeg", "-hide_banner", "-loglevel", "error", "-nostdin", "-ss", "3.0", "-i", src, "-to", "12.5", "-vsync", "vfr"]
    assert list(p.argv) == head + y4m_tail("fps=2.0")
    assert (p.feed, p.keep_rec709, p.out_bits, p.numbers, p.start_number) == ("planes", False, 8, None, 0)
    ppm = video.build_decode_plan(jobs[0])
    assert list(ppm.argv) == head + ["-vf", "fps=2.0," + CS + ":trc=iec61966-2-1:format=yuv444p,format=rgb24", "-an", "-f", "image2pipe",
                                     "-c:v", "ppm", "pipe:1"]
    assert p.fallback_argv == ppm.argv and p.key != ppm.key
    assert video.output_path(jobs[1], p, 41).endswith("clip_0000041_B.png")


def test_planes_plans_of_jpg_deep_and_keep_rec709_jobs(tmp_path):
    jpg = parse_job_argv(plan_jobs(tmp_path, ["-f", "1", "--count", "2"]).jobs[0][0])
    assert "range=jpeg" in ",".join(jpg.filters)
    p = video.build_decode_plan(jpg, "planes")
    assert list(p.argv[-8:]) == y4m_tail("fps=1.0") and (p.feed, p.keep_rec709, p.out_bits) == ("planes", False, 8)
    assert "range=jpeg:format=yuv444p,format=rgb24" in p.fallback_argv[p.fallback_argv.index("-vf") + 1]

    deep = parse_job_argv(plan_jobs(tmp_path, ["-f", "1", "--ext", "png", "--count", "2"], bit_depth=10).jobs[0][0])
    assert deep.options["-pix_fmt"] == "rgb48le"
    p = video.build_decode_plan(deep, "planes")
    assert list(p.argv[-8:]) == y4m_tail("fps=1.0") and (p.feed, p.keep_rec709, p.out_bits) == ("planes", False, 16)
    assert p.fallback_argv[p.fallback_argv.index("-vf") + 1].endswith(",format=rgb48be")

    keep = parse_job_argv(plan_jobs(tmp_path, ["-f", "1", "--ext", "png", "--count", "2", "--keep-rec709"]).jobs[0][0])
    assert CS + ":format=yuv444p" in keep.filters
    p = video.build_decode_plan(keep, "planes")
    assert list(p.argv[-8:]) == y4m_tail("fps=1.0") and (p.feed, p.keep_rec709, p.out_bits) == ("planes", True, 8)
    srgb = video.build_decode_plan(parse_job_argv(plan_jobs(tmp_path, ["-f", "1", "--ext", "png", "--count", "2"]).jobs[0][0]), "planes")
    assert srgb.argv == p.argv and srgb.key != p.key            # the curve left the command line: it is part of the key


def test_planes_plan_of_the_gui_selection(tmp_path):
    cmd = plan_jobs(tmp_path, ["-f", "1", "--count", "2"]).jobs[0][0]
    job = parse_job_argv(gui_select_rewrite(cmd, [40, 7, 19]))
    q = video.build_decode_plan(job, "planes")
    src = str(tmp_path / "clip.mp4")
    assert list(q.argv) == ["ffmpeg", "-hide_banner", "-loglevel", "error", "-nostdin", "-copyts", "-i", src, "-vsync", "vfr"] + \
        y4m_tail("select='eq(n\\,40)+eq(n\\,7)+eq(n\\,19)'")
    assert (q.feed, q.keep_rec709, q.out_bits, q.numbers) == ("planes", False, 8, (7, 19, 40))
    assert q.fallback_argv == video.build_decode_plan(job).argv


def test_other_colorspace_filters_keep_the_ppm_plan(tmp_path):
    cmd = plan_jobs(tmp_path, ["-f", "1", "--ext", "png", "--count", "2"]).jobs[0][0]
    v = cmd.index("-vf") + 1
    ours = CS + ":trc=iec61966-2-1:format=yuv444p"
    assert ours in cmd[v]

    def with_filter(text):
        c = list(cmd)
        c[v] = c[v].replace(ours, text)
        job = parse_job_argv(c)
        return video.build_decode_plan(job, "planes"), video.build_decode_plan(job)
    for text in (ours + ":dither=fsb",                                           # a foreign option
                 "colorspace=iall=bt601-6-625:all=smpte170m:format=yuv444p",     # another input
                 "colorspace=iall=bt709:all=smpte170m",                          # no format
                 ours + ":range=tv",
                 ours + ":format=yuv444p",                                       # an option twice
                 "null",                                                         # no colorspace filter at all
                 ours + "," + ours):                                             # two of them
        got, ppm = with_filter(text)
        assert got is not None and got == ppm and got.feed == "ppm" and got.fallback_argv == (), text
    got, ppm = with_filter("colorspace=format=yuv444p:range=jpeg:all=smpte170m:iall=bt709")      # the options in any order
    assert got.feed == "planes" and got.keep_rec709 and got.fallback_argv == ppm.argv


def test_feed_ppm_is_todays_plan_and_refusals_stay(tmp_path):
    cmd = plan_jobs(tmp_path, ["-f", "1", "--ext", "png", "--count", "2", "--start", "3", "--end", "9"]).jobs[0][0]
    job = parse_job_argv(cmd)
    a, b = video.build_decode_plan(job), video.build_decode_plan(job, feed="ppm")
    assert a == b and (a.feed, a.keep_rec709, a.out_bits, a.fallback_argv) == ("ppm", False, 8, ())
    assert video.DecodePlan(a.argv, a.key, a.numbers, a.start_number) == a      # the new fields trail, with defaults
    with pytest.raises(ValueError):
        video.build_decode_plan(job, "y4m")

    def mutate(fn):
        c = list(cmd)
        fn(c)
        return video.build_decode_plan(parse_job_argv(c), "planes")
    assert mutate(lambda c: c.__setitem__(c.index("-pix_fmt") + 1, "gbrp12le")) is None
    assert mutate(lambda c: c.__setitem__(c.index("-vf") + 1, c[c.index("-vf") + 1] + ",hflip")) is None
    assert mutate(lambda c: c.__setitem__(slice(-1, -1), ["-metadata", "x=y"])) is None
    assert mutate(lambda c: c.__setitem__(slice(-1, -1), ["-frame_pts", "1"])) is None
    assert video.build_decode_plan(parse_job_argv(gui_select_rewrite(cmd, [1, 4, 7])), "planes") is None     # a selection with a seek window


def test_feed_from_env():
    assert video.feed_from_env({}) == "ppm"
    assert video.feed_from_env({"GS360_VIDEO_FEED": ""}) == "ppm"
    assert video.feed_from_env({"GS360_VIDEO_FEED": "ppm"}) == "ppm"
    assert video.feed_from_env({"GS360_VIDEO_FEED": "planes"}) == "planes"
    with pytest.raises(ValueError, match="GS360_VIDEO_FEED"):
        video.feed_from_env({"GS360_VIDEO_FEED": "device"})


# ---- accuracy of the (10, 8) format ----------------------------------------------------------------------------------------------------
def test_10_bit_triples_to_8_bit_levels_are_within_one_level_of_the_ideal():
    """at most one 8-bit level, the condition DESIGN.md 17.6 sets for 8-bit output: half a level of the final rounding and half a
    level for everything before it.  Worst of the four cases with this restatement and seed: 0.64 (full range, sRGB)."""
    rng = np.random.default_rng(1910)
    t = np.concatenate([rng.integers(0, 1024, size=(4_000_000, 3)), extremes10()])
    Y, U, V = t[:, 0], t[:, 1], t[:, 2]
    for full in (False, True):
        lin = ideal_linear(Y, U, V, 10, full)
        q = feed_ref.ref.rgb14(Y, U, V, 10, full)
        for keep in (False, True):
            err = float(np.abs(feed_ref.levels8(q, keep).astype(np.float64) - ideal_encode(lin, keep, 255)).max())
            print("(10, 8) full_range={} keep_rec709={}: worst error {:.4f} levels".format(full, keep, err))
            assert err <= 1.0
    assert feed_ref.convert_triples([940, 64], [512, 512], [512, 512]).tolist() == [[255] * 3, [0] * 3]
    assert feed_ref.convert_triples([1023, 0], [512, 512], [512, 512], True).tolist() == [[255] * 3, [0] * 3]


def test_video_color_pairs():
    from gs360 import vidcolor
    for depth, out_bits, want in ((8, None, (8, 255, np.uint8)), (10, None, (16, 65535, np.uint16)), (10, 8, (8, 255, np.uint8)),
                                  (8, 8, (8, 255, np.uint8)), (10, 16, (16, 65535, np.uint16))):
        s = vidcolor.VideoColor(depth, out_bits=out_bits)
        assert (s.out_bits, s.outmax, s.out_dtype) == want
        assert np.array_equal(s.encode, vidcolor.encode_table(False, want[1]))
    for depth, out_bits in ((8, 16), (10, 12), (10, 10)):
        with pytest.raises(ValueError):
            vidcolor.VideoColor(depth, out_bits=out_bits)


# ---- the session's fallback ---------------------------------------------------------------------------------------------------------------
def test_a_12_bit_stream_restarts_on_the_ppm_command(tmp_path):
    rng = np.random.default_rng(1911)
    n, H, W = 4, 6, 10
    rgb = rng.integers(0, 256, size=(n, H, W, 3), dtype=np.uint8)
    np.savez(tmp_path / "clip.npz", y=rng.integers(0, 4096, size=(n, H, W)).astype(np.uint16),
             u=rng.integers(0, 4096, size=(n, 3, 5)).astype(np.uint16), v=rng.integers(0, 4096, size=(n, 3, 5)).astype(np.uint16),
             tag="420p12", rgb=rgb)
    head = (sys.executable, str(FAKE), "-hide_banner", "-loglevel", "error", "-nostdin", "-i", str(tmp_path / "clip.npz"))
    y4m_argv = head + tuple(y4m_tail("fps=1.0"))
    ppm_argv = head + ("-vf", "fps=1.0," + CS + ":format=yuv444p,format=rgb24", "-an", "-f", "image2pipe", "-c:v", "ppm", "pipe:1")
    plan = video.DecodePlan(y4m_argv, ("clip", y4m_argv[1:]), None, 0, "planes", True, 8, ppm_argv)
    st = _FakeState()
    stats = video.FeedStats()
    sess = video.VideoSession([st], plan, budget=1 << 20, feed_stats=stats)
    tok = sess.join()
    got = []
    k = 0
    while True:
        fr = sess.frame(tok, k)
        if fr is None:
            break
        _st, buf, h, w, dt = fr
        assert dt == np.uint8
        got.append(st.ctx.live[buf].reshape(h, w, 3).copy())
        k += 1
    sess.leave(tok)
    assert sess.error is None and sess.finished
    assert len(got) == n and all(np.array_equal(a, b) for a, b in zip(got, rgb))
    assert (sess.feed_fallbacks, sess.plane_fed_frames) == (1, 0) and (stats.feed_fallbacks, stats.plane_fed_frames) == (1, 0)
    assert sess.proc.args[:len(ppm_argv)] == list(ppm_argv)
    sess.close()
    assert not st.ctx.live
