"""bench.py driver contract on the CPU: one JSON line from rank 0, self-launch of N ranks
without torchrun (the reference's `mpirun -np P`, Makefile:36), failure propagation."""
import json
import os
import subprocess
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent


def _bench(*args, env=None, timeout=300):
    e = dict(os.environ, PKD_SKIP_BUILD="1")
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK"):
        e.pop(k, None)
    e.update(env or {})
    return subprocess.run([sys.executable, str(ROOT / "bench.py"), *args], capture_output=True, text=True,
                          timeout=timeout, env=e, cwd=ROOT)


def _one_json(stdout):
    lines = [l for l in stdout.splitlines() if l.strip()]
    assert len(lines) == 1, stdout
    return json.loads(lines[0])


def test_bench_single_cpu():
    r = _bench("--full", "--device", "cpu", "--points", "100000", "--steps", "2", "--warmup", "1")
    assert r.returncode == 0, r.stderr
    j = _one_json(r.stdout)
    assert j["n_gpus"] == 1 and j["steps"] == 2 and j["warmup"] == 1 and j["config"]["n_points"] == 100000
    assert j["config"]["tree_checked"] and j["higher_is_better"] and j["unit"] == "Mpoints/s"


def test_bench_plain_run_dumps_outputs(tmp_path):
    """A plain run (no --full) only times: no tree check. --dump-outputs writes the last timed
    build's tree, the same from run to run, and it is the exact tree of the generated points."""
    import numpy as np
    import parallel_kd_tree_amd as pk
    from parallel_kd_tree_amd import ops
    n = 20_001
    trees = []
    for d in ("a", "b"):
        r = _bench("--device", "cpu", "--points", str(n), "--steps", "2", "--warmup", "0",
                   "--dump-outputs", str(tmp_path / d))
        assert r.returncode == 0, r.stderr
        j = _one_json(r.stdout)
        assert j["steps"] == 2 and j["ms_per_step"] > 0 and not j["config"]["tree_checked"]
        assert abs(j["value"] - n / j["ms_per_step"] / 1e3) <= 1e-3 * j["value"] + 1e-3
        assert sorted(p.name for p in (tmp_path / d).iterdir()) == ["tree_ids.npy", "tree_pts.npy"]
        trees.append((np.load(tmp_path / d / "tree_pts.npy"), np.load(tmp_path / d / "tree_ids.npy")))
    (pa, ia), (pb, ib) = trees
    assert pa.dtype == np.float32 and ia.dtype == np.float64 and pa.shape == (n, 3) and ia.shape == (n,)
    assert np.array_equal(pa, pb) and np.array_equal(ia, ib)
    cp, ci = ops.build_cpu(pk.generate_slice(42, 3, 0, n), None, "exact", 0, 1)
    assert np.array_equal(pa, cp.numpy()) and np.array_equal(ia, ci.numpy().astype(np.float64))


def test_bench_runs_from_a_read_only_tree(monkeypatch, capsys):
    """A tree built by another user cannot be locked or rebuilt by the one who runs the benchmark:
    bench.py then runs the extension that is there, and any other build error still propagates."""
    import errno
    import pytest
    import bench
    from parallel_kd_tree_amd import _build, ops

    def denied(*a, **k):
        raise PermissionError(errno.EACCES, "Permission denied", str(ROOT / "build" / ".build.lock"))
    monkeypatch.delenv("PKD_SKIP_BUILD", raising=False)
    monkeypatch.delenv("PKD_BENCH_TRACE_BUILD", raising=False)
    monkeypatch.setattr(_build, "build", denied)
    # a permission error in a tree that CAN be written is a real failure, not a read-only tree
    with pytest.raises(PermissionError):
        bench._ensure_built("rank 0")
    monkeypatch.setattr(bench, "_tree_writable", lambda: False)
    assert bench._ensure_built("rank 0") is False
    assert "rank 0: build NOT checked, the tree is read-only" in capsys.readouterr().err  # said without being asked

    # no extension to run: an error, never another path
    def missing():
        raise ImportError("parallel_kd_tree_amd native extension is not built")
    with monkeypatch.context() as m:
        m.setattr(ops, "native", missing)
        with pytest.raises(ImportError, match="not built"):
            bench._ensure_built("rank 0")

    def broken(*a, **k):
        raise RuntimeError("command failed (1): hipcc")
    monkeypatch.setattr(_build, "build", broken)
    with pytest.raises(RuntimeError, match="command failed"):
        bench._ensure_built("rank 0")


_READ_ONLY_RUN = """
import errno, sys
import bench
from parallel_kd_tree_amd import _build
def denied(*a, **k):
    raise PermissionError(errno.EACCES, "Permission denied", "build/.build.lock")
_build.build = denied
bench._tree_writable = lambda: False
bench.main(sys.argv[1:])
"""


def test_bench_whole_run_from_a_read_only_tree():
    """The whole run in a process of its own when the build cannot be checked: it exits 0, says so on
    stderr and in the result line (config.build_checked), and still builds and checks its tree."""
    e = dict(os.environ)
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "PKD_SKIP_BUILD", "PKD_BENCH_TRACE_BUILD"):
        e.pop(k, None)
    r = subprocess.run([sys.executable, "-c", _READ_ONLY_RUN, "--full", "--device", "cpu", "--points", "20001",
                        "--steps", "1", "--warmup", "0"], capture_output=True, text=True, timeout=300, env=e, cwd=ROOT)
    assert r.returncode == 0, r.stderr
    cfg = _one_json(r.stdout)["config"]
    assert cfg["build_checked"] is False and cfg["tree_checked"]
    assert "build NOT checked, the tree is read-only" in r.stderr


def test_bench_dump_samples_large_outputs(tmp_path):
    """Above the size limit the dump is a fixed sample of tree slots: the same rows of every array."""
    import numpy as np
    import torch
    import bench
    n = 1000
    pts = torch.arange(n * 3, dtype=torch.float32).reshape(n, 3)
    ids = torch.arange(n, dtype=torch.int32) + 2**24 + 1  # not exact in float32
    for d in ("a", "b"):
        bench._dump_outputs(str(tmp_path / d), {"tree_pts": pts, "tree_ids": ids}, "", 2800)
    rows = np.load(tmp_path / "a" / "sample_rows.npy")
    assert rows.dtype == np.float64 and rows.shape == (86,) and (np.diff(rows) >= 0).all()
    assert rows.min() >= 0 and rows.max() < n and len(set(rows.tolist())) > 50
    assert np.array_equal(rows, np.load(tmp_path / "b" / "sample_rows.npy"))
    sel = rows.astype(np.int64)
    assert np.array_equal(np.load(tmp_path / "a" / "tree_pts.npy"), pts.numpy()[sel])
    assert np.array_equal(np.load(tmp_path / "a" / "tree_ids.npy"), ids.numpy()[sel].astype(np.float64))
    assert sum(p.stat().st_size for p in (tmp_path / "a").iterdir()) <= 2800  # files, headers included


def test_bench_self_launch_two_ranks():
    """No WORLD_SIZE in the env: bench.py spawns its ranks itself; rank 0 alone prints."""
    r = _bench("--full", "--gpus", "2", "--device", "cpu", "--points", "60000", "--steps", "1", "--warmup", "1")
    assert r.returncode == 0, r.stderr
    j = _one_json(r.stdout)
    assert j["n_gpus"] == 2 and j["config"]["parallelism"] == "global2" and j["config"]["tree_checked"]


def test_bench_distributed_dump_holds_the_whole_tree(tmp_path):
    """N > 1: every rank dumps its share and rank 0 the top-tree rows; together they hold every point once."""
    import numpy as np
    n = 20_001
    r = _bench("--gpus", "3", "--device", "cpu", "--points", str(n), "--steps", "1", "--warmup", "0",
               "--dump-outputs", str(tmp_path))
    assert r.returncode == 0, r.stderr
    assert sorted(p.name for p in tmp_path.iterdir()) == sorted(
        ["top_ids.npy", "top_pts.npy", "top_slots.npy"] + [f"tree_{a}_rank{k}.npy" for a in ("ids", "pts") for k in range(3)])
    top_ids, top_pts, top_slots = (np.load(tmp_path / f"top_{a}.npy") for a in ("ids", "pts", "slots"))
    assert top_pts.dtype == np.float32 and top_pts.shape == (len(top_ids), 3) and top_slots.shape == top_ids.shape
    assert len(top_ids) >= 2 and (top_slots >= 0).any()
    ids = [top_ids[top_slots >= 0]]
    for k in range(3):
        ids.append(np.load(tmp_path / f"tree_ids_rank{k}.npy"))
        assert np.load(tmp_path / f"tree_pts_rank{k}.npy").shape == (len(ids[-1]), 3)
    assert np.array_equal(np.sort(np.concatenate(ids)), np.arange(1, n + 1, dtype=np.float64))
    # the boundary rows are the points of those ids
    import parallel_kd_tree_amd as pk
    x = pk.generate_slice(42, 3, 0, n).numpy()
    sel = top_slots >= 0
    assert np.array_equal(top_pts[sel], x[top_ids[sel].astype(np.int64) - 1])


def test_bench_self_launch_four_ranks_pipelined():
    r = _bench("--full", "--gpus", "4", "--device", "cpu", "--points", "40001", "--steps", "1", "--warmup", "0",
               "--pipeline-k", "1")
    assert r.returncode == 0, r.stderr
    j = _one_json(r.stdout)
    assert j["n_gpus"] == 4 and j["config"]["tree_checked"]


def test_bench_three_ranks():
    """A world size that is not a power of two: uneven leaf runs, same checked tree."""
    r = _bench("--full", "--gpus", "3", "--device", "cpu", "--points", "30001", "--steps", "1", "--warmup", "0")
    assert r.returncode == 0, r.stderr
    j = _one_json(r.stdout)
    assert j["n_gpus"] == 3 and j["config"]["parallelism"] == "global3" and j["config"]["tree_checked"]
    assert "(not the headline config)" in j["metric"] and j["config"]["headline"] is False
    # a host rehearsal is labelled as one, never as a GPU measurement
    assert "rehearsal" in j["metric"] and j["config"]["shared_gpu"] is False


def test_bench_headline_rehearsal_is_labelled():
    """The headline config run as a host (gloo) rehearsal: same metric stem, but labelled and
    headline false, so it can never pass for the 100 M x 3D measurement."""
    r = _bench("--full", "--gpus", "2", "--device", "cpu", "--points", "20000", "--steps", "1", "--warmup", "0")
    assert r.returncode == 0, r.stderr
    j = _one_json(r.stdout)
    assert j["config"]["headline"] is False and "rehearsal" in j["metric"] and j["config"]["tree_checked"]


def test_bench_launcher_propagates_rank_failure():
    """A dead rank ends the job with a non-zero status and no JSON line (the other rank,
    blocked in a collective, is stopped by the launcher)."""
    r = _bench("--gpus", "2", "--device", "cpu", "--points", "20000", "--steps", "1", "--warmup", "0",
               env={"PKD_BENCH_FAIL_RANK": "1"}, timeout=200)
    assert r.returncode != 0
    assert r.stdout.strip() == ""
    assert "rank 1 exited with 7" in r.stderr


def test_bench_world_mismatch_rejected():
    r = _bench("--gpus", "2", "--device", "cpu", env={"WORLD_SIZE": "1"})
    assert r.returncode != 0 and "WORLD_SIZE" in r.stderr


def test_bench_builds_in_launcher_before_ranks():
    """The self-launcher brings the build up to date before any rank exists; the ranks then only
    verify signatures (no compile, O(1) work) before they join the communicator."""
    r = _bench("--full", "--gpus", "2", "--device", "cpu", "--points", "20000", "--steps", "1", "--warmup", "0",
               env={"PKD_SKIP_BUILD": "0", "PKD_BENCH_TRACE_BUILD": "1"}, timeout=1200)
    assert r.returncode == 0, r.stderr
    cfg = _one_json(r.stdout)["config"]
    assert cfg["tree_checked"] and cfg["build_checked"]
    lines = [l for l in r.stderr.splitlines() if l.startswith("bench.py:") and ": build " in l]
    assert lines and lines[0].startswith("bench.py: launcher: build"), r.stderr
    ranks = [l for l in lines if l.startswith("bench.py: rank ")]
    assert len(ranks) == 2, r.stderr
    for l in ranks:
        assert "build up to date" in l, l
        ms = float(l.rsplit("(", 1)[1].split(" ms")[0])
        assert ms < 20_000, l
