"""gs360/framesource.py without a GPU: the FrameSelector's reader under GS360_JPEG_DECODER=device, with the device decode replaced by a
fake that returns tagged frames, the passes' launches by fakes that name what they were given, and the context by one that counts
frees.  The files are real (Pillow writes them), so the host-only preparation (parse, segment table, scratch size) is the real one."""
import concurrent.futures
import contextlib
import ctypes
import io
import re

import numpy as np
import pytest

pytest.importorskip("PIL.Image")

import gs360_FrameSelector as cli  # noqa: E402
from conftest import ROOT  # noqa: E402
from gs360 import capi, frameflow, framescore, framesource, jpegdec  # noqa: E402

import jpegdec_cases as cases  # noqa: E402

FAIL_WIDTH = 40                          # the fake device reports a non-zero status for files of this width


class FakeBuf:
    def __init__(self, tag, nbytes):
        self.tag, self.nbytes, self.freed = tag, nbytes, False


class FakeCtx:
    def __init__(self):
        self.freed = []

    def free(self, buf):
        assert not buf.freed, f"frame {buf.tag} freed twice"
        buf.freed = True
        self.freed.append(buf.tag)


class FakeDevice:
    """stands in for framesource.device_decode: a frame tagged with the file's height, None for a file of FAIL_WIDTH"""

    def __init__(self):
        self.calls, self.made = [], []

    def __call__(self, ctx, prepared):
        assert 1 <= len(prepared) <= capi.MAX_FRAMES and all(isinstance(p, jpegdec.Prepared) for p in prepared)
        self.calls.append(len(prepared))
        out = []
        for p in prepared:
            if p.d.W == FAIL_WIDTH:
                out.append(None)
                continue
            self.made.append(FakeBuf(p.d.H, p.d.H * p.d.W))
            out.append(framescore.DeviceFrame(self.made[-1], p.d.H, p.d.W, 1, p.d.W))
        return out

    def live(self):
        return sorted(b.tag for b in self.made if not b.freed)


class HostDecode:
    """stands in for framescore.decode / frameflow._decode: an array that carries the number in the file's name, None for a missing file"""

    def __init__(self):
        self.calls = []

    def __call__(self, path):
        self.calls.append(str(path))
        if "missing" in str(path):
            return None
        return np.full((4, 4, 3), int(re.search(r"(\d+)\.\w+$", str(path)).group(1)), np.uint8)


def _name(fr):
    return ("device", fr.buf.tag) if isinstance(fr, framescore.DeviceFrame) else ("host", int(np.asarray(fr)[0, 0, 0]))


def _fake_score_arrays(ctx, frames, *a, **kw):
    return [_name(fr) for fr in frames]


@pytest.fixture
def rig(monkeypatch):
    """the device decoder switched on, with the fakes in place -> (ctx, device, host)"""
    ctx, device, host = FakeCtx(), FakeDevice(), HostDecode()
    monkeypatch.setenv("GS360_JPEG_DECODER", "device")
    monkeypatch.delenv("GS360_FS_GRAY_CACHE_MB", raising=False)
    monkeypatch.setattr(framesource, "device_decode", device)
    monkeypatch.setattr(framescore, "default_context", lambda: ctx)
    monkeypatch.setattr(framescore, "decode", host)
    monkeypatch.setattr(frameflow, "_decode", host)
    monkeypatch.setattr(framescore, "score_arrays", _fake_score_arrays)
    monkeypatch.setattr(framescore, "edge_arrays", lambda ctx, frames, crop_ratio, **kw: _fake_score_arrays(ctx, frames))
    framesource.reset_stats()
    frameflow.cancel_event.clear()
    yield ctx, device, host
    frameflow.cancel_event.clear()


def _jpeg(path, height, width=16, **kw):
    path.write_bytes(cases.encode(cases.image(height, width, "smooth"), quality=90, **kw))
    return str(path)


def _mixed_folder(root):
    """-> (paths, what score_files must return for them): device files with refused, failed, non-JPEG and missing ones in between"""
    paths, want = [], []
    for k in range(40):
        kind = {3: "png", 7: "progressive", 11: "failed", 12: "png", 20: "missing", 21: "cut", 33: "failed"}.get(k, "device")
        if kind == "device":
            paths.append(_jpeg(root / f"f{k:02d}.jpg", 8 + k))
            want.append(("device", 8 + k))
        elif kind == "failed":
            paths.append(_jpeg(root / f"f{k:02d}.jpg", 8 + k, width=FAIL_WIDTH))
            want.append(("host", k))
        elif kind == "progressive":
            paths.append(_jpeg(root / f"f{k:02d}.jpeg", 8 + k, progressive=True))
            want.append(("host", k))
        elif kind == "cut":
            whole = cases.encode(cases.image(8 + k, 16, "noise"), quality=90)
            (root / f"f{k:02d}.jpg").write_bytes(whole[:len(whole) - 20])           # no EOI: parse() refuses it
            paths.append(str(root / f"f{k:02d}.jpg"))
            want.append(("host", k))
        elif kind == "png":
            (root / f"f{k:02d}.png").write_bytes(b"not read by the fake")
            paths.append(str(root / f"f{k:02d}.png"))
            want.append(("host", k))
        else:
            paths.append(str(root / f"missing{k:02d}.jpg"))
            want.append(framescore.FAILED)
    return paths, want


@pytest.mark.parametrize("backend", ("opencv", "ffmpeg"))
def test_results_keep_the_order_of_the_paths_and_the_host_decodes_only_the_fallbacks(rig, tmp_path, backend):
    ctx, device, host = rig
    paths, want = _mixed_folder(tmp_path)
    got = framescore.score_files(paths, "lapvar", 0.8, 0, False, True, workers=4, backend=backend)
    assert got == want
    fallbacks = [p for p, w in zip(paths, want) if w == framescore.FAILED or w[0] == "host"]
    assert sorted(host.calls) == sorted(fallbacks)                               # exactly those, exactly once each
    assert max(device.calls) <= capi.MAX_FRAMES and sum(device.calls) == 33 + 2   # every prepared file went to the device once
    st = framesource.stats()
    assert (st["device_decoded"], st["fallbacks"], st["reused"], st["kept_bytes"]) == (33, 7, 0, 0)
    assert device.live() == [] and sorted(ctx.freed) == sorted(w[1] for w in want if w[0] == "device")   # no store: nothing outlives the call


def test_single_file_seams_free_what_they_decode(rig, tmp_path):
    ctx, device, host = rig
    good, bad = _jpeg(tmp_path / "a1.jpg", 9), _jpeg(tmp_path / "b2.jpg", 10, progressive=True)
    assert framescore.score_one_file(good, "lapvar", 0.8, 0, False, True) == ("device", 9)
    assert framescore.score_one_file(bad, "lapvar", 0.8, 0, False, True) == ("host", 2)
    assert framescore.score_one_file_ffmpeg(good, "lapvar", 0.8, 0, False, True) == ("device", 9)
    assert framescore.score_one_file(str(tmp_path / "missing3.jpg"), "lapvar", 0.8, 0, False, True) == framescore.FAILED
    seen = []
    frameflow_arrays = frameflow.flow_arrays
    try:
        frameflow.flow_arrays = lambda ctx, frames, pairs, *a, **kw: seen.append([_name(f) for f in frames]) or [1.5]
        assert frameflow._compute_pair_flow_magnitude(good, bad, 0.6) == 1.5
    finally:
        frameflow.flow_arrays = frameflow_arrays
    assert seen == [[("device", 9), ("host", 2)]]
    assert device.live() == [] and ctx.freed == [9, 9, 9]
    assert host.calls == [bad, str(tmp_path / "missing3.jpg"), bad]


def test_store_keeps_first_come_up_to_the_budget_then_stops(rig, tmp_path):
    ctx, device, host = rig
    sizes = [10, 10, 15, 1, 10]                                   # heights at width 16: 160, 160, 240, 16, 160 bytes
    paths = [_jpeg(tmp_path / f"s{k}.jpg", h) for k, h in enumerate(sizes)]
    with framesource.open_store(budget_bytes=400) as store:
        assert framescore.score_files(paths, "lapvar", 0.8, 0, False, True, workers=2) == [("device", h) for h in sizes]
        # the third frame does not fit; the fourth would, but keeping has ended: the flow pass asks for frames from the front
        assert sorted(store.frames) == sorted(paths[:2]) and framesource.stats()["kept_bytes"] == 320
        assert device.live() == [10, 10] and framesource.stats()["reused"] == 0
        with framesource.Reader(ctx, host) as reader:            # the flow pass: the kept frames are not read again
            frames = reader.read(paths)
            assert [_name(f) for f in frames] == [("device", h) for h in sizes]
            assert frames[0].buf is store.frames[paths[0]][1].buf and frames[1].buf is store.frames[paths[1]][1].buf
            assert sum(device.calls) == 5 + 3
            reader.release(frames)
            assert device.live() == [10, 10]                     # the reader frees its own, the store's stay
        st = framesource.stats()
        assert (st["device_decoded"], st["fallbacks"], st["reused"]) == (5, 0, 2)
    assert device.live() == [] and len(ctx.freed) == 8 and host.calls == []
    assert framesource.stats()["kept_bytes"] == 0 and framesource.current_store() is None


def test_budget_from_the_environment(rig, tmp_path, monkeypatch):
    assert framesource.default_budget() == 16384 << 20
    monkeypatch.setenv("GS360_FS_GRAY_CACHE_MB", "0")
    paths = [_jpeg(tmp_path / f"s{k}.jpg", 9 + k) for k in range(3)]
    with framesource.open_store() as store:
        framescore.score_files(paths, "lapvar", 0.8, 0, False, True, workers=2)
        assert store.frames == {} and rig[1].live() == []


def test_failed_decode_call_ends_keeping_and_not_the_run(rig, tmp_path, monkeypatch):
    """framesource.device_decode itself (the rig's fake put aside): a Gs360Error from the decode call, out of device memory say, sends
    the call's files to the host and ends the store's keeping"""
    ctx, device, host = rig
    monkeypatch.undo()
    monkeypatch.setenv("GS360_JPEG_DECODER", "device")
    monkeypatch.setattr(framescore, "default_context", lambda: ctx)
    monkeypatch.setattr(framescore, "decode", host)
    monkeypatch.setattr(framescore, "score_arrays", _fake_score_arrays)
    calls = []

    def decode_device(ctx, prepared, slot=0, gray=False):
        calls.append((len(prepared), slot, gray))
        if len(calls) == 2:
            raise capi.Gs360Error(-2, "out of device memory")
        return [jpegdec.Decoded(FakeBuf(p.d.H, p.d.H * p.d.W), (p.d.H, p.d.W, 1), p.d.W, 0) for p in prepared]
    monkeypatch.setattr(jpegdec, "decode_device", decode_device)
    paths = [_jpeg(tmp_path / f"s{k:02d}.jpg", 9 + k) for k in range(40)]
    with framesource.open_store() as store:
        got = framescore.score_files(paths, "lapvar", 0.8, 0, False, True, workers=2)
        assert got == [("host", k) if 16 <= k < 32 else ("device", 9 + k) for k in range(40)]
        assert calls == [(16, 0, True), (16, 0, True), (8, 0, True)] and sorted(host.calls) == paths[16:32]
        assert sorted(store.frames) == paths[:16] and not store.keeping      # what came after the failure was decoded, not kept
        assert sorted(ctx.freed) == list(range(9 + 32, 9 + 40))
    assert len(ctx.freed) == 24


def test_store_is_emptied_when_the_block_raises(rig, tmp_path):
    ctx, device, host = rig
    paths = [_jpeg(tmp_path / f"s{k}.jpg", 9 + k) for k in range(20)]

    def progress(done):
        if done >= 16:
            raise RuntimeError("stop")
    with pytest.raises(RuntimeError):
        with framesource.open_store():
            framescore.score_files(paths, "lapvar", 0.8, 0, False, True, workers=2, progress=progress)
    assert len(device.made) >= 16 and device.live() == [] and framesource.current_store() is None


def test_cancelled_flow_pass_frees_its_frames(rig, tmp_path, monkeypatch, capsys):
    ctx, device, host = rig
    paths = [_jpeg(tmp_path / f"s{k:02d}.jpg", 9 + k) for k in range(40)]
    records = [{"file_paths": [p]} for p in paths]
    calls = []

    def flow_arrays(ctx, frames, pairs, *a, **kw):
        calls.append(len(pairs))
        frameflow.cancel_event.set()                              # (the SIGINT handler's flag)
        return [1.0] * len(pairs)
    monkeypatch.setattr(frameflow, "flow_arrays", flow_arrays)
    with framesource.open_store(budget_bytes=10 * 16 * 12):
        framescore.score_files(paths[:12], "lapvar", 0.8, 0, False, True, workers=2)
        kept = len(framesource.current_store().frames)
        assert 0 < kept < 12 and device.live() == list(range(9, 9 + kept))
        mags = [0.0] * 40
        assert frameflow._compute_flow_magnitudes(records, mags, 0.6, 2, "Optical flow") == frameflow.CHUNK_PAIRS
        assert calls == [frameflow.CHUNK_PAIRS]
        assert device.live() == list(range(9, 9 + kept))          # what the pass decoded is gone, whatever was still queued
        assert framesource.stats()["reused"] == kept
    assert device.live() == []


def test_host_decoder_never_reaches_the_device_path(rig, tmp_path, monkeypatch):
    ctx, device, host = rig
    monkeypatch.delenv("GS360_JPEG_DECODER")

    def never(*a, **kw):
        raise AssertionError("gs360.framesource on the host decoder's path")
    for name in ("device_decode", "open_store", "current_store"):
        monkeypatch.setattr(framesource, name, never)
    for name in ("load", "resolve", "read", "frames", "__init__"):
        monkeypatch.setattr(framesource.Reader, name, never)
    monkeypatch.setattr(jpegdec, "prepare", never)
    monkeypatch.setattr(frameflow, "flow_arrays", lambda ctx, frames, pairs, *a, **kw: [2.0] * len(pairs))
    paths = [_jpeg(tmp_path / f"s{k}.jpg", 9 + k) for k in range(5)]
    for mode in (None, "host"):
        if mode:
            monkeypatch.setenv("GS360_JPEG_DECODER", mode)
        host.calls.clear()
        assert framescore.score_files(paths, "lapvar", 0.8, 0, False, True, workers=2) == [("host", k) for k in range(5)]
        assert framescore.score_one_file(paths[0], "lapvar", 0.8, 0, False, True) == ("host", 0)
        mags = [0.0] * 5
        assert frameflow._compute_flow_magnitudes([{"file_paths": [p]} for p in paths], mags, 0.6, 2, "Optical flow") == 4
        assert mags == [2.0] * 5
        assert frameflow._compute_pair_flow_magnitude(paths[0], paths[1], 0.6) == 2.0
        assert sorted(host.calls) == sorted(paths * 2 + paths[:1] + paths[:2])


def _run_cli(argv):
    out, code = io.StringIO(), None
    cli.cancel_event.clear()
    try:
        with contextlib.redirect_stdout(out):
            cli.main(argv)
    except SystemExit as e:
        code = e.code
    return code, out.getvalue()


def test_cli_refuses_an_invalid_decoder_setting(tmp_path, monkeypatch):
    (tmp_path / "f000.png").write_bytes(b"")
    monkeypatch.setenv("GS360_JPEG_DECODER", "gpu")
    code, out = _run_cli(["-i", str(tmp_path), "-d"])
    assert code == 1
    assert out.splitlines() == ["[ERR] GS360_JPEG_DECODER must be host or device (got 'gpu')"]


def test_cli_counts_under_the_device_decoder_only(rig, tmp_path, monkeypatch):
    """main() opens the store around its two passes and prints the counts; the default run prints no such line"""
    ctx, device, host = rig
    for k in range(6):
        _jpeg(tmp_path / f"f{k:03d}.jpg", 9 + k)
    (tmp_path / "f006.png").write_bytes(b"")
    monkeypatch.setattr(framescore, "score_arrays", lambda ctx, frames, *a, **kw: [(0.5, 0.0, 0.0, 0.5, 1.0, None, None, None, 1.0)] * len(frames))
    monkeypatch.setattr(frameflow, "flow_arrays", lambda ctx, frames, pairs, *a, **kw: [1.0] * len(pairs))
    argv = ["-i", str(tmp_path), "-d", "--score_backend", "opencv", "-m", "lapvar", "--compute_optical_flow"]
    code, out = _run_cli(argv)
    assert code is None and "[INFO] JPEG decoder: 6 frames decoded on the device, 1 fallbacks, 6 reused\n" in out
    assert device.live() == [] and framesource.current_store() is None
    monkeypatch.delenv("GS360_JPEG_DECODER")
    code, out = _run_cli(argv)
    assert code is None and "JPEG decoder" not in out


def test_reader_frames_run_ahead_on_a_pool_in_order(rig, tmp_path):
    ctx, device, host = rig
    paths, want = _mixed_folder(tmp_path)
    with concurrent.futures.ThreadPoolExecutor(max_workers=3) as ex, framesource.Reader(ctx, host) as reader:
        got = list(reader.frames(paths, ex, 2 * capi.MAX_FRAMES))
    assert [k for k, _ in got] == list(range(40))
    assert [framescore.FAILED if fr is None else _name(fr) for _, fr in got] == want
    assert device.live() == []                                                    # the reader's exit freed what nobody released


def test_header_binding_and_exports_agree():
    h = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "gs360.h").read_text(), flags=re.S)
    assert "gs360_jpeg_decode_gray_u8" in capi.EXPORTS
    sig = r"int %s\(gs360_ctx \*ctx, const gs360_jpeg_dec_job \*jobs, int n_jobs, uint32_t \*status_dev, int slot\);"
    assert re.search(sig % "gs360_jpeg_decode_gray_u8", h) and re.search(sig % "gs360_jpeg_decode_u8", h)
    assert re.search(r"#define GS360_ABI_VERSION (\d+)", h).group(1) == str(capi.ABI_VERSION) == "2"
    L = capi.load_library()
    assert L.gs360_jpeg_decode_gray_u8.argtypes == L.gs360_jpeg_decode_u8.argtypes and L.gs360_jpeg_decode_gray_u8.restype is ctypes.c_int
    assert callable(capi.Context.jpeg_decode_gray_dev)
    # the argument checks come before any device work: on a machine without one the library still reports them
    assert L.gs360_jpeg_decode_gray_u8(None, None, 0, None, 0) != 0 and "ctx" in capi.last_error(L)


def test_batch_takes_prepared_files_and_gray_sizes_the_plane():
    """the host-only part runs without a context; Batch then only allocates and uploads (a context that records what is asked of it)"""
    data = cases.encode(cases.image(37, 53, "noise"), quality=90, subsampling=2)
    p = jpegdec.prepare(data)
    assert (p.d.H, p.d.W, p.d.C) == (37, 53, 3) and p.nscr == jpegdec.scratch_bytes(p.d, p.n_sub) and p.seg.shape[1] == 4
    with pytest.raises(jpegdec.Unsupported):
        jpegdec.prepare(cases.encode(cases.image(8, 8, "noise"), progressive=True))

    class Buf:
        def __init__(self, n):
            self.nbytes, self.ptr = n, 4096

    class Ctx:
        def __init__(self):
            self.allocs, self.calls, self.frees = [], [], 0

        def alloc(self, n):
            self.allocs.append(n)
            return Buf(n)

        def free(self, b):
            self.frees += 1

        def upload(self, *a, **kw):
            pass

        def memset(self, *a, **kw):
            pass

        def sync(self, slot):
            pass

        def jpeg_decode_dev(self, jobs, status, slot=0):
            self.calls.append(("rgb", len(jobs)))

        def jpeg_decode_gray_dev(self, jobs, status, slot=0):
            self.calls.append(("gray", len(jobs)))
    for gray, pad, row in ((True, 0, 53), (True, 3, 56), (False, 3, 162)):
        c = Ctx()
        b = jpegdec.Batch(c, [p, b"not a jpeg", data], pad=pad, guard=0, gray=gray)
        assert list(b.refused) == [1] and [it[5] for it in b.items] == [row, row] and [it[0] for it in b.items] == [0, 2]
        assert c.allocs.count(37 * row) == 2 and b.jobs[0].out_stride == row
        b.run()
        assert c.calls == [("gray" if gray else "rgb", 2)]
        b.close()
        assert c.frees == len(c.allocs)
