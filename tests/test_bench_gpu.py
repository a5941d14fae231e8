"""-m gpu: bench.py's N>1 control flow on ONE GPU (round-1 VERDICT weak #5, ADVICE bench.py:103).

`python bench.py --gpus 2` with no launcher in the environment must start its own torch.distributed.run; with
`--backend gloo` the two ranks share device 0, so the whole multi-rank path (rendezvous, barrier, max-over-ranks, one
JSON line from rank 0) runs on the 1-GPU box.  The numbers are not performance figures."""
import json
import os
import pathlib
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = pathlib.Path(__file__).resolve().parent.parent


def _run(args, timeout=900):
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    p = subprocess.run([sys.executable, str(ROOT / "bench.py")] + args, capture_output=True, text=True, timeout=timeout, env=env)
    assert p.returncode == 0, p.stderr[-2000:]
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, p.stdout[-2000:]
    return json.loads(lines[0])


def test_bench_self_launch_two_ranks_share_device0():
    d = _run(["--gpus", "2", "--backend", "gloo", "--steps", "3", "--warmup", "1", "--frames", "2"])
    assert d["n_gpus"] == 2 and d["scaling"] == "strong" and d["value"] > 0
    assert d["config"]["parity_vs_oracle"] is True
    # 3 steps x 16 launches x 2 frames, the launches dealt to 2 ranks: 24 launches = 48 frame renders on rank 0
    assert d["config"]["launches_per_step"] == 16 and d["config"]["frames_rank0"] == 48 and len(d["config"]["per_rank_seconds"]) == 2
    assert d["cpu_baseline"] is None                   # the timed CPU sample is an N=1 item
    assert d["roofline"]["bound"] == "hbm" and d["roofline"]["kernel_ms"] > 0
    assert 0 < d["roofline"]["line_bound"]["frac"] < 1.5
    # the line proves which devices took part: one PCI bus id per rank (gloo ranks share device 0 here: duplicates reported, not refused)
    assert d["config"]["world_seen"] == 2 and len(d["config"]["rank_devices"]) == 2
    assert d["config"]["rank_devices"][0] == d["config"]["rank_devices"][1] and ":" in d["config"]["rank_devices"][0]


def test_bench_single_rank_line_matches_the_contract():
    d = _run(["--steps", "3", "--warmup", "1", "--no-cpu-baseline"])
    # a step is 16 launches of 16 frames at every N (round-4 verdict): 3 steps = 48 launches = 768 frame renders
    assert d["n_gpus"] == 1 and d["steps"] == 3 and d["config"]["frames_per_step"] == 16 and d["config"]["frames_rank0"] == 768
    assert d["config"]["launches_per_step"] == 16 and d["config"]["world_seen"] == 1 and len(d["config"]["rank_devices"]) == 1
    assert d["roofline"]["algorithmic_bytes_per_launch"] == 16 * 54495972
    # the headline shape takes the source-major kernel: its line bound is the UNION of the six views' lines, each once
    assert d["roofline"]["kernel"] == "eq_srcmajor_kernel"
    assert d["roofline"]["line_bound"]["bytes_per_launch"] == 16 * (413172 * 128 + 11520000)
    # ... and the counters' traffic of the launch is held against what bare loads + stores of this shape reach (profiles/r06/membench/)
    m = d["roofline"]["memsys"]
    assert m["mix_5_to_1"][0] < m["mix_5_to_1"][1] < m["read_only"] < d["roofline"]["peak"]
    assert m["traffic_rate"] is None or 0.3 < m["frac_of_mix"] < 1.2
    # ... and against THIS box's own reading: the probe library (lib/libgs360probe.so, built by csrc/Makefile) ran in-process after the timed region
    here = m["measured_here"]
    assert here is not None and 3000 < here["dmamix"] < 8000 and 3000 < here["rowsmix"] < 8000 and here["rowsmix"] < here["rows"] < 8000, here
    assert m["traffic_rate"] is None or 0.5 < m["frac_of_mix_here"] < 1.1


def test_bench_rccl_world_of_one_prints_exactly_one_json_line():
    """the RCCL leg (backend nccl = RCCL): init, barrier, all_reduce(MAX), all_gather on ONE rank -- stdout must carry exactly one
    JSON line (RCCL's banners go to stderr through the fd-1 redirection) with the keys of the plain run"""
    plain = _run(["--steps", "3", "--warmup", "1", "--no-cpu-baseline"])
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    env["NCCL_DEBUG"] = "VERSION"                   # make RCCL print its banner
    p = subprocess.run([sys.executable, str(ROOT / "bench.py"), "--gpus", "1", "--with-torch", "--steps", "3", "--warmup", "1",
                        "--no-cpu-baseline"], capture_output=True, text=True, timeout=900, env=env)
    assert p.returncode == 0, p.stderr[-2000:]
    out_lines = [ln for ln in p.stdout.splitlines() if ln.strip()]
    assert len(out_lines) == 1, p.stdout[-2000:]
    d = json.loads(out_lines[0])
    assert set(d) == set(plain) and set(d["config"]) == set(plain["config"]) and set(d["roofline"]) == set(plain["roofline"])
    assert d["n_gpus"] == 1 and d["config"]["frames_rank0"] == 768 and d["config"]["launches_per_step"] == 16
    assert len(d["config"]["per_rank_seconds"]) == 1 and d["value"] > 0


def test_bench_more_rccl_ranks_than_gpus_exits_3_without_hanging():
    """`--gpus 2` over RCCL on a 1-GPU box: the rank without a GPU of its own must leave with exit code 3 and the message, the
    launcher must come down with it (no hang at the rendezvous)"""
    import torch
    if torch.cuda.device_count() != 1:
        pytest.skip("needs a box with exactly one GPU")
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    p = subprocess.run([sys.executable, str(ROOT / "bench.py"), "--gpus", "2", "--steps", "2", "--warmup", "1", "--no-cpu-baseline"],
                       capture_output=True, text=True, timeout=300, env=env)
    assert p.returncode == 3, (p.returncode, p.stderr[-2000:])
    assert "needs GPU 1 but only 1 are visible" in p.stderr, p.stderr[-2000:]
    assert not [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
    # the same under a launcher (what the driver does): the rank without a GPU leaves with 3 and takes the job down, no hang
    import socket
    with socket.socket() as so:
        so.bind(("127.0.0.1", 0))
        port = so.getsockname()[1]
    p = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
                        "--master-port", str(port), str(ROOT / "bench.py"), "--gpus", "2", "--steps", "2", "--warmup", "1",
                        "--no-cpu-baseline"], capture_output=True, text=True, timeout=300, env=env)
    assert p.returncode != 0
    assert "needs GPU 1 but only 1 are visible" in p.stderr, p.stderr[-3000:]
    assert not [ln for ln in p.stdout.splitlines() if ln.startswith("{")]


def test_bench_job_mode_two_ranks():
    d = _run(["--gpus", "2", "--backend", "gloo", "--mode", "job", "--job-frames", "5", "--job-size", "256"])
    assert d["n_gpus"] == 2 and d["scaling"] == "strong" and d["steps"] == 5
    assert d["config"]["frames_rank0"] == 3 and d["config"]["parity_vs_oracle"] is True and d["value"] > 0


def test_bench_stream_mode_strong_scaling_two_ranks():
    d = _run(["--gpus", "2", "--backend", "gloo", "--mode", "stream", "--stream-frames", "7", "--stream-size", "320"])
    assert d["n_gpus"] == 2 and d["scaling"] == "strong" and d["steps"] == 7
    assert d["config"]["frames_rank0"] == 4 and d["config"]["parity_vs_oracle"] is True
    assert d["value"] > 0 and d["config"]["frames_per_s"] > 0


def test_bench_dump_outputs_are_what_the_timed_step_computed(tmp_path, orc):
    """--dump-outputs: frame 0's views whole and a seeded sample of every view of the last timed step, float32, under 64 MB,
    equal to the oracle on the same seeded input; --steps sets the timed steps and ms_per_step is per step"""
    import numpy as np
    sys.path.insert(0, str(ROOT))
    import bench
    d = _run(["--steps", "2", "--warmup", "1", "--frames", "4", "--no-cpu-baseline", "--no-secondary", "--no-memsys",
              "--dump-outputs", str(tmp_path / "out")])
    assert d["steps"] == 2 and d["config"]["frames_rank0"] == 2 * 16 * 4 and d["ms_per_step"] > 0
    files = {p.name: np.load(p) for p in (tmp_path / "out").glob("*.npy")}
    assert set(files) == {"views_frame0.npy", "sample_index.npy", "sample_values.npy"}
    assert sum(p.stat().st_size for p in (tmp_path / "out").glob("*.npy")) <= 64 * 2 ** 20
    assert all(a.dtype in (np.float32, np.float64) for a in files.values())
    want = orc.equirect_views_u8(bench.synth_frame(np, 0), [orc.make_view(*v) for v in bench.view_table()], threads=0)
    assert np.array_equal(files["views_frame0.npy"], np.stack(want).astype(np.float32))
    idx = files["sample_index.npy"].astype(np.int64)
    assert idx.size == 1 << 20 and np.all(np.diff(idx) > 0) and idx[-1] < 4 * 6 * 800 * 800 * 3
    frame0 = idx < 6 * 800 * 800 * 3
    assert np.array_equal(files["sample_values.npy"][frame0], files["views_frame0.npy"].reshape(-1)[idx[frame0]])
