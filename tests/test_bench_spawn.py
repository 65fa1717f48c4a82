"""`python bench.py --gpus 2` exactly as the driver may call it WITHOUT a launcher: bench.py must start the ranks itself
(fresh child processes, before anything touches the GPU), rendezvous over 127.0.0.1, gather, and print one JSON line
from rank 0.  No GPU here, so the device solve is stubbed by the CPU build of the solver header (--stub host_twin, test
infrastructure) and the collective goes over gloo; RCCL itself can only run on a multi-GPU node."""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _run(extra, env_extra=None):
    env = dict(os.environ)
    for k in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)
    env.update(env_extra or {})
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + extra, env=env, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-3000:]
    lines = [l for l in p.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, p.stdout
    return json.loads(lines[0]), p.stderr


def test_bench_spawns_its_own_ranks_weak_scaling():
    r, err = _run(["--gpus", "2", "--steps", "3", "--warmup", "1", "--batch", "96", "--stub", "host_twin", "--backend", "gloo", "--inflight", "2"])
    assert "spawned 2 ranks itself" in err and "no GPU call" in err
    assert r["n_gpus"] == 2 and r["steps"] == 3 and r["scaling"] == "weak"
    assert r["config"]["global_batch"] == 192 and r["config"]["batch_per_gpu"] == 96
    assert r["config"]["gather_checked"] is True and "gloo" in r["config"]["collective_mode"]
    assert "gather to rank 0" in r["config"]["collective_mode"] and r["config"]["batches_per_collective"] == 4     # the defaults
    assert r["config"]["gather_bytes_sent_per_rank_per_batch"] == 8 * 96 * (9 + 1 + 20)
    assert r["converged_fraction"] == 1.0 and r["value"] > 0 and "stub" in r and r["metric"].startswith("STUB")
    r, _ = _run(["--gpus", "2", "--steps", "2", "--warmup", "1", "--batch", "96", "--stub", "host_twin", "--backend", "gloo", "--gather", "all",
                 "--gather-results-only", "--gather-group", "1"])
    assert "all_gather" in r["config"]["collective_mode"] and "results only" in r["config"]["collective_mode"] and r["config"]["gather_checked"] is True
    assert r["config"]["gather_bytes_sent_per_rank_per_batch"] == 8 * 96 * 10


def test_bench_strong_scaling_and_f32_flags():
    """configs[3]-style strong scaling (global batch split over the ranks) and the fp32 packed gather (two int rows)."""
    r, _ = _run(["--gpus", "2", "--steps", "2", "--warmup", "1", "--scaling", "strong", "--global-batch", "128", "--N", "25", "--dt", "0.05",
                 "--config", "config-stable.json", "--stub", "host_twin", "--backend", "gloo"])
    assert r["scaling"] == "strong" and r["config"]["batch_per_gpu"] == 64 and r["config"]["global_batch"] == 128 and r["config"]["N"] == 25
    r, _ = _run(["--gpus", "2", "--steps", "2", "--warmup", "1", "--batch", "64", "--weights-sweep", "--precision", "f32", "--no-traj",
                 "--stub", "host_twin", "--backend", "gloo"])
    assert r["dtype"] == "f32" and r["config"]["gather_checked"] is True and r["converged_fraction"] == 1.0
    assert r["roofline"]["algorithmic_bytes_per_launch"] == 136 * 64


def test_bench_parent_refuses_nothing_but_stays_gpu_free():
    """The spawning parent asserts that neither torch nor the HIP runtime is loaded in it (bench.py:spawn_ranks)."""
    src = open(os.path.join(ROOT, "bench.py")).read()
    head = src[:src.index("def cpu_baseline_legs")]
    assert "import torch" not in head and "libamdhip64" in head


def test_bench_dump_outputs_repeatable_and_steps_exact(tmp_path):
    """--dump-outputs: the last timed batch's results as float .npy files, the same from run to run; --steps is the number of
    batches inside the clock."""
    import numpy as np
    dumps = []
    for k in range(2):
        d, full = tmp_path / ("dump%d" % k), tmp_path / ("full%d.json" % k)
        r, _ = _run(["--gpus", "2", "--steps", "5", "--warmup", "1", "--batch", "64", "--stub", "host_twin", "--backend", "gloo",
                     "--dump-outputs", str(d), "--full-json", str(full)])
        assert r["steps"] == 5
        assert json.load(open(full))["timing"]["batches_in_the_window"] == 5
        dumps.append({f: np.load(d / f) for f in sorted(os.listdir(d))})
    assert sorted(dumps[0]) == ["iters.npy", "out.npy", "status.npy", "traj.npy"]
    assert dumps[0]["out.npy"].shape == (2, 9, 64) and dumps[0]["traj.npy"].shape == (2, 20, 64)
    for f, a in dumps[0].items():
        assert a.dtype in (np.float32, np.float64), f
        assert np.array_equal(a, dumps[1][f], equal_nan=True), f
    assert (dumps[0]["status.npy"] == 0).all() and (dumps[0]["iters.npy"] > 0).all()


def test_bench_full_is_opt_in(tmp_path):
    """A plain run times the headline and nothing else; --full adds the measurements that take runs of their own (with the
    stub: the same batches timed from an empty device, strict_value) and dumps what the plain run dumps."""
    import numpy as np
    lines, dumps = [], []
    for k, extra in enumerate(([], ["--full"])):
        d = tmp_path / ("dump%d" % k)
        r, _ = _run(["--gpus", "1", "--steps", "4", "--warmup", "1", "--batch", "64", "--stub", "host_twin", "--dump-outputs", str(d),
                     "--full-json", str(tmp_path / ("full%d.json" % k))] + extra)
        lines.append(r)
        dumps.append({f: np.load(d / f) for f in sorted(os.listdir(d))})
    assert lines[0]["strict_value"] is None and lines[1]["strict_value"] > 0
    assert lines[0]["steps"] == lines[1]["steps"] == 4 and lines[0]["value"] > 0
    assert sorted(dumps[0]) == sorted(dumps[1]) == ["iters.npy", "out.npy", "status.npy", "traj.npy"]
    for f, a in dumps[0].items():
        assert np.array_equal(a, dumps[1][f], equal_nan=True), f


def test_bench_dump_outputs_sample_under_the_cap(tmp_path):
    """Beyond the size cap the same seeded instances are taken from every array, and their indices are written too."""
    import numpy as np
    import torch
    import bench

    B = 1000
    full = {"out": torch.arange(9 * B, dtype=torch.float64).reshape(1, 9, B), "traj": torch.ones(1, 20, B, dtype=torch.float64),
            "status": torch.zeros(1, B, dtype=torch.int32), "iters": torch.arange(B, dtype=torch.int32).reshape(1, B)}

    class Pipe:
        last_slot = staticmethod(lambda: 0)
        pg = type("PG", (), {"result": staticmethod(lambda slot: full)})

    shapes = [bench.dump_outputs(Pipe, str(tmp_path / d), cap_bytes=64 << 10) for d in ("a", "b")]
    assert shapes[0] == shapes[1]
    idx = np.load(tmp_path / "a" / "instance_index.npy")
    total = sum(os.path.getsize(tmp_path / "a" / f) for f in os.listdir(tmp_path / "a"))
    assert 0 < len(idx) < B and total <= (64 << 10) + 4096          # (+ the .npy headers)
    assert np.array_equal(np.load(tmp_path / "a" / "iters.npy")[0], idx)
    assert np.array_equal(np.load(tmp_path / "a" / "out.npy"), np.load(tmp_path / "b" / "out.npy"))
