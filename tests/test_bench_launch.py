"""bench.py's launcher (CPU, no GPU work): `bench.py --gpus N` run directly
starts N ranks itself, and a launcher-provided WORLD_SIZE must match --gpus."""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _run(args, extra_env=None):
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    env.update(extra_env or {})
    return subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), *args], env=env,
                          capture_output=True, text=True, timeout=120)


def test_gpus_n_spawns_n_ranks():
    r = _run(["--gpus", "3", "--dry-run"])
    assert r.returncode == 0, r.stderr
    lines = [json.loads(s) for s in r.stdout.splitlines() if s.startswith("{")]
    assert sorted(x["rank"] for x in lines) == [0, 1, 2]
    assert sorted(x["local_rank"] for x in lines) == [0, 1, 2]
    assert all(x["world"] == 3 and x["master"] == "127.0.0.1" for x in lines)


def test_single_gpu_runs_in_process():
    r = _run(["--gpus", "1", "--dry-run"])
    assert r.returncode == 0, r.stderr
    lines = [json.loads(s) for s in r.stdout.splitlines() if s.startswith("{")]
    assert lines == [{"rank": 0, "local_rank": 0, "world": 1, "master": lines[0]["master"]}]


_DUMP = """
import sys
import numpy as np
import bench
n = int(sys.argv[2])
rng = np.random.default_rng(1)
bench.dump_outputs(sys.argv[1], {"label": rng.integers(0, 2, n).astype(np.uint8),
                                 "fail_step": rng.integers(-1, 200, n).astype(np.int32),
                                 "obj_qpos": rng.standard_normal((n, 7))})
"""


def _dump(tmp_path, n, cap=None):
    code = _DUMP if cap is None else _DUMP.replace("import bench\n", f"import bench\nbench.DUMP_MAX_BYTES = {cap}\n")
    r = subprocess.run([sys.executable, "-c", code, str(tmp_path), str(n)], cwd=ROOT,
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    import numpy as np
    return {f[:-4]: np.load(os.path.join(tmp_path, f)) for f in sorted(os.listdir(tmp_path))}


def test_dump_outputs_whole_set(tmp_path):
    """--dump-outputs: masks as float32, the rest as float64, values exact"""
    import numpy as np
    d = _dump(tmp_path, 37)
    assert sorted(d) == ["fail_step", "label", "obj_qpos"]
    assert d["label"].dtype == np.float32 and d["fail_step"].dtype == np.float64 and d["obj_qpos"].dtype == np.float64
    rng = np.random.default_rng(1)
    assert np.array_equal(d["label"], rng.integers(0, 2, 37))
    assert np.array_equal(d["fail_step"], rng.integers(-1, 200, 37))
    assert np.array_equal(d["obj_qpos"], rng.standard_normal((37, 7)))


def test_dump_outputs_sample_under_cap(tmp_path):
    """a set over the size cap is cut to one seeded sample of candidates, the
    same rows of every array, and stays under the cap with its index"""
    import numpy as np
    cap = 4096
    d = _dump(tmp_path / "a", 1000, cap)
    assert sum(a.nbytes for a in d.values()) <= cap
    keep = d["sample_index"].astype(int)
    assert 0 < len(keep) < 1000 and np.all(np.diff(keep) > 0)
    rng = np.random.default_rng(1)
    lab, fail, q = rng.integers(0, 2, 1000), rng.integers(-1, 200, 1000), rng.standard_normal((1000, 7))
    assert np.array_equal(d["label"], lab[keep]) and np.array_equal(d["fail_step"], fail[keep])
    assert np.array_equal(d["obj_qpos"], q[keep])
    d2 = _dump(tmp_path / "b", 1000, cap)
    assert all(np.array_equal(d[k], d2[k]) for k in d)


def test_world_size_mismatch_fails():
    r = _run(["--gpus", "2", "--dry-run"], {"WORLD_SIZE": "4", "RANK": "0", "LOCAL_RANK": "0"})
    assert r.returncode == 2
    assert "WORLD_SIZE 4" in r.stderr
