"""bench.py's output contract, without a GPU: the LAST stdout line is a compact object the driver can parse (round 3's
23.5 KB line was recorded as `parsed: null`), and `python bench.py --gpus N` starts its own ranks."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import bench  # noqa: E402

CONTRACT = {"metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling",
            "vs_baseline", "dtype", "data", "config"}


def recorded_full_line():
    """A full record as round 3's bench printed it (committed profile: 60-odd kernel tags, long cpu_baseline text)."""
    with open(os.path.join(ROOT, "profiles", "r03d_bench_n1.json")) as f:
        return json.load(f)


def test_compact_line_is_small_and_carries_the_judged_keys():
    full = recorded_full_line()
    assert len(json.dumps(full)) > 20000                      # the record that did not parse
    line = bench.compact_line(full)
    assert "\n" not in line and len(line) < bench.COMPACT_LIMIT < 6000
    out = json.loads(line)
    assert CONTRACT <= set(out) and "kernels" not in out
    assert {"roofline", "backbone", "cpu_baseline", "parity", "fp32_gemm_check", "loss_delta_vs_oracle", "sim_max_abs_delta"} <= set(out)
    assert out["value"] == full["value"] and out["ms_per_step"] == full["ms_per_step"] and out["dtype"] == "fp32"
    assert out["config"]["workload"] == full["config"]["workload"]
    roof = out["roofline"]
    for k in ("bound", "kernel", "achieved", "peak", "unit", "frac", "avg_us", "algorithmic_bytes", "traffic"):
        assert k in roof, k
    assert roof["frac"] == pytest.approx(roof["achieved"] / roof["peak"], rel=1e-3)
    cb = out["cpu_baseline"]
    assert {"value", "unit", "cores", "kind", "sample"} <= set(cb) and cb["kind"] == "port"


def test_compact_line_stays_small_with_long_free_text_and_a_dist_record():
    full = recorded_full_line()
    full["config"]["launch"] = "x" * 3000
    full["cpu_baseline"]["sample"] = "y" * 5000
    full["n_gpus"] = 8
    full["dist"] = {"backend": "nccl", "rccl_version": "2.26.6", "ranks_seen": 8, "devices": list(range(8)),
                    "grad_buckets": [{"params": 40, "bytes": 1 << 25}] * 4, "launcher": "bench.py (self-spawned ranks)",
                    "collective_bytes_per_step": {"all_reduce_total": 98_000_000}, "note": "z" * 2000}
    line = bench.compact_line(full)
    assert len(line) < bench.COMPACT_LIMIT
    out = json.loads(line)
    assert out["dist"]["ranks_seen"] == 8 and out["dist"]["grad_buckets"] == 4


def test_bf16_companion_rides_in_the_compact_line():
    """The default fp32 run attaches a driver-witnessed bf16 step time (C3 / C5 are bf16 configurations): the companion is what
    `companion_from_line` keeps of the bf16 run's own compact line, and the fp32 line still fits."""
    full = recorded_full_line()
    with open(os.path.join(ROOT, "profiles", "r05e_bench_bf16_n1.json")) as f:
        bf16_line = json.loads(f.read().strip().splitlines()[-1])
    full["bf16_companion"] = bench.companion_from_line(bf16_line)
    line = bench.compact_line(full)
    assert len(line) < bench.COMPACT_LIMIT
    out = json.loads(line)
    c = out["bf16_companion"]
    assert c["dtype"] == "bf16" and c["ms_per_step"] == bf16_line["ms_per_step"] and c["value"] == bf16_line["value"]
    assert c["value"] == pytest.approx(2 * 128 * 1e3 / c["ms_per_step"], rel=1e-3) and c["steps"] == bf16_line["steps"]
    roof = c["roofline"]
    assert {"bound", "kernel", "achieved", "peak", "unit", "frac", "avg_us"} <= set(roof)
    assert roof["frac"] == pytest.approx(roof["achieved"] / roof["peak"], rel=1e-3)
    assert out["dtype"] == "fp32" and out["ms_per_step"] == full["ms_per_step"]         # the judged numbers stay the fp32 run's
    # which runs get one: the default fp32 single-GPU command with --full only (a plain run measures its own precision)
    argv = sys.argv
    try:
        for extra, want in ((["--full"], True), (["--full", "--dtype", "bf16"], False), (["--full", "--no-cpu-baseline"], False),
                            (["--full", "--bf16-companion", "0"], False), (["--full", "--gpus", "2"], False), ([], False)):
            sys.argv = ["bench.py", *extra]
            assert bench.wants_companion(bench.parse()) == want, extra
    finally:
        sys.argv = argv


def test_emit_prints_details_first_and_the_compact_line_last(capsys, tmp_path, monkeypatch):
    monkeypatch.setenv("PECLR_BENCH_DETAILS", str(tmp_path / "d.json"))
    bench.emit(recorded_full_line())
    lines = capsys.readouterr().out.splitlines()
    assert len(lines) == 2 and lines[0].startswith("BENCH_DETAILS {") and lines[1].startswith("{")
    assert "kernels" in json.loads(lines[0][len("BENCH_DETAILS "):]) and len(lines[1]) < bench.COMPACT_LIMIT
    assert "kernels" in json.load(open(tmp_path / "d.json"))


def test_plain_run_options_and_its_compact_line():
    """A plain run (no --full) carries the contract keys and nothing that needs a pass of its own."""
    argv = sys.argv
    try:
        sys.argv = ["bench.py", "--gpus", "1", "--steps", "7", "--warmup", "2"]
        args = bench.parse()
        assert not args.full and args.dump_outputs is None and args.steps == 7 and args.warmup == 2
        sys.argv = ["bench.py", "--full", "--dump-outputs", "out_dir"]
        args = bench.parse()
        assert args.full and args.dump_outputs == "out_dir"
    finally:
        sys.argv = argv
    full = recorded_full_line()
    plain = {k: full[k] for k in CONTRACT | {"loss"}}
    plain["details"] = "per-kernel table, roofline, parity, CPU baseline: bench.py --full"
    out = json.loads(bench.compact_line(plain))
    assert CONTRACT <= set(out) and out["ms_per_step"] == full["ms_per_step"] and out["value"] == full["value"]
    assert not {"roofline", "backbone", "cpu_baseline", "parity", "fp32_gemm_check", "bf16_companion"} & set(out)


def test_dump_outputs_writes_float_arrays_and_a_fixed_parameter_sample(tmp_path):
    import numpy as np
    import torch

    g = torch.Generator().manual_seed(3)
    params = [torch.randn(40, 30, generator=g), torch.randn(7, generator=g, dtype=torch.float64), torch.randn(5, generator=g).half()]
    out = {"loss": torch.tensor(2.5), "stat": torch.tensor([1.0, 2.0], dtype=torch.float64), "count": torch.tensor(3)}
    shapes = bench.dump_outputs(str(tmp_path / "a"), out, params)
    assert shapes == {"out_loss": [], "out_stat": [2], "out_count": [], "params": [1212]}
    a = {n: np.load(tmp_path / "a" / f"{n}.npy") for n in shapes}
    assert {n: list(v.shape) for n, v in a.items()} == shapes
    assert a["out_loss"].dtype == np.float32 and a["out_stat"].dtype == np.float64 and a["out_count"].dtype == np.float64
    assert float(a["out_loss"]) == 2.5 and float(a["out_count"]) == 3.0
    flat = torch.cat([p.reshape(-1).float() for p in params]).numpy()
    assert a["params"].dtype == np.float32 and np.array_equal(a["params"], flat)
    # more parameters than the cap: a seeded sample in index order, the same from run to run
    bench.dump_outputs(str(tmp_path / "b"), out, params, sample=100)
    bench.dump_outputs(str(tmp_path / "c"), out, params, sample=100)
    b, c = np.load(tmp_path / "b" / "params.npy"), np.load(tmp_path / "c" / "params.npy")
    assert b.shape == (100,) and np.array_equal(b, c) and np.isin(b, flat).all()
    total = sum(os.path.getsize(tmp_path / "b" / f) for f in os.listdir(tmp_path / "b"))
    assert total < 64 << 20 and bench.DUMP_PARAM_SAMPLE * 4 < 64 << 20


@pytest.mark.timeout(300)
def test_bench_gpus_2_without_a_launcher_spawns_its_own_ranks():
    """The literal command form the driver uses (`python bench.py --gpus N ...`, no WORLD_SIZE in the environment):
    both ranks come up, form the group (gloo here: no GPU) and see each other."""
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_PORT", "MASTER_ADDR")}
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "1", "--warmup", "0", "--dry-dist"],
                       env=env, capture_output=True, text=True, timeout=280, cwd=ROOT)
    assert p.returncode == 0, p.stderr[-3000:]
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1
    r = json.loads(lines[0])
    assert r["ok"] and r["ranks_seen"] == 2 and r["world_size"] == 2 and "self-spawned" in r["launcher"]


@pytest.mark.timeout(300)
def test_bench_without_a_gpu_fails_loudly_on_every_spawned_rank():
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_PORT", "MASTER_ADDR")}
    import torch

    if torch.cuda.is_available():
        pytest.skip("CPU-only check")
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "1", "--warmup", "0"],
                       env=env, capture_output=True, text=True, timeout=280, cwd=ROOT)
    assert p.returncode != 0 and "needs an MI355X" in p.stderr and not [ln for ln in p.stdout.splitlines() if ln.startswith("{")]


@pytest.mark.timeout(200)
def test_a_rank_that_dies_takes_the_whole_launch_down_instead_of_hanging_it():
    """Advisor, round 4: the self-spawning launcher waited on rank 0's output and then on every rank without a limit -- a rank
    that died before a collective left rank 0 (and the parent) blocked in it.  Rank 1 exits before the rendezvous here: the
    parent must come back non-zero within seconds, with rank 0 terminated."""
    import time

    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_PORT", "MASTER_ADDR")}
    env["PECLR_BENCH_DRY_DIE_RANK"] = "1"
    t0 = time.monotonic()
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "1", "--warmup", "0", "--dry-dist"],
                       env=env, capture_output=True, text=True, timeout=180, cwd=ROOT)
    assert p.returncode != 0 and "rank 1 exited with code 3" in p.stderr, p.stderr[-2000:]
    assert time.monotonic() - t0 < 120
    assert not [ln for ln in p.stdout.splitlines() if ln.startswith("{")]


@pytest.mark.gpu
@pytest.mark.timeout(600)
def test_plain_run_prints_the_contract_line_and_dumps_the_last_step(tmp_path):
    """`bench.py --gpus 1 --steps K --warmup W --dump-outputs DIR` (small shape): one stdout line, K timed steps, no per-kernel
    pass or checker output, and the last timed step's outputs as float .npy files within 64 MB."""
    import numpy as np

    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_PORT", "MASTER_ADDR")}
    out_dir = tmp_path / "dump"
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1",
                        "--resnet", "18", "--pairs", "8", "--size", "64", "--dump-outputs", str(out_dir)],
                       env=env, capture_output=True, text=True, timeout=560, cwd=ROOT)
    assert p.returncode == 0, p.stderr[-3000:]
    lines = p.stdout.strip().splitlines()
    assert len(lines) == 1 and lines[0].startswith("{") and "BENCH_DETAILS" not in p.stdout
    r = json.loads(lines[0])
    assert CONTRACT <= set(r) and r["steps"] == 3 and r["warmup"] == 1 and r["dtype"] == "fp32" and r["unit"] == "images/sec"
    assert r["value"] == pytest.approx(2 * 8 * 3 / (r["ms_per_step"] * 3e-3), rel=1e-3)
    assert not {"roofline", "kernels", "cpu_baseline", "parity", "fp32_gemm_check", "bf16_companion"} & set(r)
    files = sorted(os.listdir(out_dir))
    assert "out_loss.npy" in files and "params.npy" in files
    assert sum(os.path.getsize(out_dir / f) for f in files) <= 64 << 20
    for f in files:
        a = np.load(out_dir / f)
        assert a.dtype in (np.float32, np.float64) and np.isfinite(a).all(), f
    assert float(np.load(out_dir / "out_loss.npy")) == pytest.approx(r["loss"], abs=1e-6)
    assert np.load(out_dir / "params.npy").shape == (bench.DUMP_PARAM_SAMPLE,)      # ResNet-18 + head: more than the cap
