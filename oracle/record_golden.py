#!/usr/bin/env python3
"""Record what the reference programs print, for the parity tests.

    python oracle/record_golden.py REFERENCE_DIR

compiles the reference sources found in REFERENCE_DIR (kdtree_sequential.cpp, kdtree_mpi.cpp,
Node.*, Utility.*) into oracle/_ref/ (not committed) with the reference Makefile's flags, runs
them at the configurations the tests use and writes their output to
tests/golden/reference_outputs.json. The tests compare the project's programs with that file, so
they need neither the reference sources nor a compiler for them.

* seq_debug: kdtree_sequential.cpp with DEBUG 1 (seed / dim / points on the command line).
* seq_eval: kdtree_sequential.cpp unmodified (seed on stdin, 500 000 x 128).
* mpi_eval / mpi_debug: kdtree_mpi.cpp against tests/fakempi/mpi.h (file-based stand-ins for
  its six MPI calls), run as P processes; DEBUG 1 also needs the scope fix of its `tick`
  variable, without which it does not compile.
* print: print_tree / print_head_and_leaves of the reference's own tree.
"elapsed time" lines are dropped: they differ from run to run.
"""
import json
import os
import subprocess
import sys
import tempfile
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
OUT = ROOT / "oracle" / "_ref"
GOLDEN = ROOT / "tests" / "golden" / "reference_outputs.json"
GXX = ["g++", "-O3", "-std=c++17", "-mavx"]  # the reference Makefile's flags

SEQ_DEBUG = [(42, 3, 1024), (7, 2, 5000), (3, 8, 20000), (11, 1, 777), (2, 3, 100), (1, 2, 1), (5, 8, 3000)]
SEQ_EVAL = [3, 42]
MPI_EVAL = [(2, 7), (4, 7)]  # processes, seed
MPI_DEBUG = [(2, (42, 3, 20000)), (4, (11, 3, 20000)), (4, (5, 2, 7001)), (3, (9, 8, 5000)),
             (16, (42, 3, 20000)), (16, (7, 2, 9001)), (16, (5, 3, 16003))]
PRINT = [(42, 3, 100), (7, 2, 37), (3, 8, 50), (11, 1, 9), (5, 6, 1), (9, 5, 64)]

PRINT_HARNESS = r"""
#include "Utility.hpp"  // includes Node.hpp (neither header has include guards)
#include <cstdlib>
#include <iostream>
Node* build_tree(Point** point_list, int num_points);
int main(int argc, char** argv) {
  int seed = atoi(argv[1]), dim = atoi(argv[2]), n = atoi(argv[3]);
  float* x = Utility::generate_problem(seed, dim, n);
  Point** pts = new Point*[n];
  for (int i = 0; i < n; ++i) pts[i] = new Point(dim, i + 1, x + i * dim);
  Node* root = build_tree(pts, n);
  Utility::print_tree(root);
  Utility::print_head_and_leaves(root);
  return 0;
}
"""


def key(*parts) -> str:
    return "_".join(str(p) for p in parts)


def results(stdout: str):
    return [l for l in stdout.splitlines() if not l.startswith("elapsed time")]


def cc(args):
    subprocess.run([str(a) for a in args], check=True)


def run(cmd, stdin=None):
    r = subprocess.run([str(c) for c in cmd], input=stdin, capture_output=True, text=True, check=True)
    return r.stdout, r.stderr


def run_mpi(exe, procs, args=(), stdin=None):
    """`procs` processes of the reference MPI driver; rank 0's stdout."""
    with tempfile.TemporaryDirectory() as tmp:
        ps = []
        for r in range(procs):
            env = dict(os.environ, FAKEMPI_RANK=str(r), FAKEMPI_SIZE=str(procs), FAKEMPI_DIR=tmp)
            ps.append(subprocess.Popen([str(exe), *map(str, args)], stdin=subprocess.PIPE, stdout=subprocess.PIPE,
                                       stderr=subprocess.PIPE, text=True, env=env))
        outs = [p.communicate(input=(stdin if r == 0 else "")) for r, p in enumerate(ps)]
        assert all(p.returncode == 0 for p in ps), [o[1] for o in outs]
    return outs[0][0]


def main():
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    ref = Path(sys.argv[1]).resolve()
    OUT.mkdir(parents=True, exist_ok=True)
    common = [ref / "Node.cpp", ref / "Utility.cpp"]
    seq, mpi = ref / "kdtree_sequential.cpp", ref / "kdtree_mpi.cpp"

    cc([*GXX, "-I", ref, seq, *common, "-o", OUT / "sequential"])
    seq_dbg = OUT / "kdtree_sequential_debug.cpp"
    seq_dbg.write_text(seq.read_text().replace("#define DEBUG 0", "#define DEBUG 1", 1))
    cc([*GXX, "-I", ref, seq_dbg, *common, "-o", OUT / "sequential_debug"])
    fake = ["-I", ROOT / "tests" / "fakempi"]
    cc([*GXX, "-I", ref, *fake, mpi, *common, "-o", OUT / "mpi"])
    text = mpi.read_text().replace("#define DEBUG 0", "#define DEBUG 1", 1)
    # F6: `tick` is declared inside the rank-0 block and used in another one
    text = text.replace("auto tick = std::chrono::high_resolution_clock::now();",
                        "tick = std::chrono::high_resolution_clock::now();", 1)
    text = text.replace("int data[3];", "int data[3];\n    auto tick = std::chrono::high_resolution_clock::now();", 1)
    mpi_dbg = OUT / "kdtree_mpi_debug.cpp"
    mpi_dbg.write_text(text)
    cc([*GXX, "-I", ref, *fake, mpi_dbg, *common, "-o", OUT / "mpi_debug"])
    (OUT / "print_harness.cpp").write_text(PRINT_HARNESS)
    cc(["g++", "-O2", "-std=c++17", "-mavx", "-I", ref, "-Dmain=reference_main", "-c", seq, "-o", OUT / "seq_nomain.o"])
    cc(["g++", "-O2", "-std=c++17", "-mavx", "-I", ref, OUT / "print_harness.cpp", OUT / "seq_nomain.o", *common,
        "-o", OUT / "printer"])

    g = {"seq_debug": {}, "seq_eval": {}, "mpi_eval": {}, "mpi_debug": {}, "print": {}}
    for cfg in SEQ_DEBUG:
        out, err = run([OUT / "sequential_debug", *cfg])
        g["seq_debug"][key(*cfg)] = {"stdout": results(out), "stderr": err}
    for seed in SEQ_EVAL:
        out, err = run([OUT / "sequential"], stdin=f"{seed}\n")
        g["seq_eval"][key(seed)] = {"stdout": out, "stderr": err}
    for procs, seed in MPI_EVAL:
        g["mpi_eval"][key(procs, seed)] = results(run_mpi(OUT / "mpi", procs, stdin=f"{seed}\n"))
    for procs, cfg in MPI_DEBUG:
        g["mpi_debug"][key(procs, *cfg)] = results(run_mpi(OUT / "mpi_debug", procs, args=cfg))
    for cfg in PRINT:
        g["print"][key(*cfg)] = run([OUT / "printer", *cfg])[0]
    GOLDEN.parent.mkdir(parents=True, exist_ok=True)
    GOLDEN.write_text(json.dumps(g, indent=1) + "\n")
    print("wrote", GOLDEN)


if __name__ == "__main__":
    main()
