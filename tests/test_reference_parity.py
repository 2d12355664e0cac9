"""Byte parity with what the REAL reference binaries printed.

tests/golden/reference_outputs.json holds the output of the reference programs, compiled from
their unchanged sources and run at the configurations below by oracle/record_golden.py:

* kdtree_sequential.cpp, unmodified (DEBUG 0): the graded evaluation path (seed on stdin,
  500 000 x 128, Utility.cpp:92-102). At d=128 the reference search is exact, so
  both of our modes must print byte-identical stdout AND stderr.
* kdtree_mpi.cpp compiled against tests/fakempi/mpi.h (file-based stand-ins for its six MPI
  calls) and run as P processes: unmodified at the evaluation config, and with DEBUG 1 (plus
  the scope fix of its `tick` variable, SURVEY F6, without which DEBUG 1 does not compile) at
  low-dimensional configs, where its forest gives different answers than the sequential
  binary that our `--decomp forest --mode reference` must reproduce exactly.
* tests/fixtures/ref_eval_seed*.txt hold the unmodified reference's eval-mode stdout; they
  are checked against the recorded reference output here and used by the GPU tests
  (test_gpu_cli.py).
"""
import json
import os
import socket
import subprocess
import sys
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
FIX = Path(__file__).resolve().parent / "fixtures"
GOLDEN = Path(__file__).resolve().parent / "golden" / "reference_outputs.json"


def _run(cmd, stdin=None, env=None, timeout=600):
    return subprocess.run([str(c) for c in cmd], input=stdin, capture_output=True, text=True, env=env, timeout=timeout)


@pytest.fixture(scope="module")
def ref():
    """The reference programs' recorded output: ref[program][configuration]."""
    return json.loads(GOLDEN.read_text())


def _key(*parts):
    return "_".join(str(p) for p in parts)


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _ours_forest(P, args, extra=()):
    """Our Python CLI, P gloo ranks on the CPU, forest decomposition in reference mode."""
    env = dict(os.environ, PKD_SKIP_BUILD="1", OMP_NUM_THREADS="1")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={P}",
           "--master-addr", "127.0.0.1", "--master-port", str(_free_port()), "-m", "parallel_kd_tree_amd.cli",
           "--device", "cpu", "--decomp", "forest", "--mode", "reference", *extra, *map(str, args)]
    r = subprocess.run(cmd, capture_output=True, text=True, env=env, cwd=ROOT, timeout=900)
    assert r.returncode == 0, r.stderr[-3000:]
    return r.stdout


def _results(stdout):
    return [l for l in stdout.splitlines() if not l.startswith("elapsed time")]


@pytest.mark.slow
@pytest.mark.parametrize("seed", [3, 42])
def test_eval_config_byte_parity(ref, bin_dir, seed):
    want = ref["seq_eval"][_key(seed)]
    for mode in ("exact", "reference"):
        ours = _run([bin_dir / "kdtree_sequential", "--threads", "8", "--mode", mode], stdin=f"{seed}\n")
        assert ours.returncode == 0, ours.stderr
        assert ours.stdout == want["stdout"], mode
        assert ours.stderr == want["stderr"], mode
    fix = FIX / f"ref_eval_seed{seed}.txt"
    assert fix.read_text() == want["stdout"], "fixture differs from the recorded reference output"


@pytest.mark.parametrize("cfg", [(42, 3, 1024), (1, 2, 1), (5, 8, 3000)])
def test_debug_config_byte_parity_exact_points(ref, bin_dir, cfg):
    """Unmodified DEBUG 0 binary cannot take argv; its eval path is covered above. Here the
    same sources with DEBUG 1: reference mode is byte-identical (elapsed time aside)."""
    want = ref["seq_debug"][_key(*cfg)]
    ours = _run([bin_dir / "kdtree_sequential", "--mode", "reference", *cfg])
    assert _results(ours.stdout) == want["stdout"] and ours.stderr == want["stderr"]


@pytest.mark.slow
@pytest.mark.parametrize("P", [2, 4])
def test_mpi_eval_config_parity(ref, P):
    """The unmodified reference MPI driver at its evaluation config (stdin seed, 500k x 128)."""
    assert _results(_ours_forest(P, [7, 128, 500000])) == ref["mpi_eval"][_key(P, 7)]


@pytest.mark.parametrize("P,cfg", [(2, (42, 3, 20000)), (4, (11, 3, 20000)), (4, (5, 2, 7001)), (3, (9, 8, 5000))])
def test_mpi_forest_parity_low_dim(ref, P, cfg):
    """Low dims, where the reference forest's answers differ from the sequential binary's and
    from brute force (F1/F2): ours must print exactly the reference MPI driver's lines."""
    lines = ref["mpi_debug"][_key(P, *cfg)]
    assert lines[0] == "READY" and lines[-1] == "DONE" and len(lines) == 12
    assert _results(_ours_forest(P, cfg)) == lines


@pytest.mark.parametrize("procs,cfg", [(2, (42, 3, 20000)), (1, (7, 2, 9001)), (3, (5, 3, 16003))])
def test_mpi_16_ranks_on_fewer_processes(ref, procs, cfg):
    """The reference's own launch, `mpirun -np 16 --oversubscribe` (Makefile:36), reproduced by
    fewer processes (GPUs): --ranks 16 spreads the 16 logical forest ranks over them, each keeping
    the reference's slicing at P = 16, so reference-mode answers (which depend on P)
    equal the reference MPI driver's at 16 processes, byte for byte."""
    lines = ref["mpi_debug"][_key(16, *cfg)]
    assert lines[0] == "READY" and lines[-1] == "DONE" and len(lines) == 12
    assert _results(_ours_forest(procs, cfg, extra=["--ranks", "16"])) == lines
