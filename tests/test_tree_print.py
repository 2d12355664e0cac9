"""Tree utilities (Utility.cpp:21-63) and the Point printer (Node.cpp:16-28): byte parity of
print_tree / print_head_and_leaves with the reference's own functions, run on the reference's
own tree (mode="reference" builds the same tree); what they printed is kept in
tests/golden/reference_outputs.json."""
import json
from pathlib import Path

import numpy as np
import pytest
import torch

import parallel_kd_tree_amd as pk
from parallel_kd_tree_amd.utils import tree_print

GOLDEN = Path(__file__).resolve().parent / "golden" / "reference_outputs.json"


@pytest.fixture(scope="module")
def ref_printed():
    """What the reference's print_tree + print_head_and_leaves printed for its own tree, per
    'seed_dim_points' (recorded by oracle/record_golden.py)."""
    return json.loads(GOLDEN.read_text())["print"]


@pytest.mark.parametrize("seed,dim,n", [(42, 3, 100), (7, 2, 37), (3, 8, 50), (11, 1, 9), (5, 6, 1), (9, 5, 64)])
def test_print_parity_with_reference(ref_printed, seed, dim, n):
    want = ref_printed[f"{seed}_{dim}_{n}"]
    x = pk.generate_problem(seed, dim, n)
    t = pk.KDTree.build(x, id_base=1, mode="reference")
    got = tree_print.tree_string(t, "tree") + tree_print.tree_string(t, "head_and_leaves")
    assert got == want


def test_print_tree_shape_and_subtree(capsys):
    x = pk.generate_problem(1, 3, 20)
    t = pk.KDTree.build(x, id_base=1)
    pk.print_tree(t)
    lines = capsys.readouterr().out.splitlines()
    assert len(lines) == 20 and lines[0].startswith("NODE(@depth=0): Point(ID=")
    depth = [len(l) - len(l.lstrip("\t")) for l in lines]
    assert max(depth) == pk.tree_height(20) - 1
    # a Node prints its own subtree with depths relative to it
    sub = tree_print.tree_string(t.root.left, "tree").splitlines()
    assert len(sub) == t.root.left.n and sub[0].startswith("NODE(@depth=0)")
    body = lambda l: (len(l) - len(l.lstrip("\t")), l.split("): ", 1)[1])
    assert [(d + 1, p) for d, p in map(body, sub)] == list(map(body, lines[1:1 + len(sub)]))


def test_point_printer_matches_python_repr(native):
    for dim in (1, 3, 5, 6, 9):
        c = torch.linspace(-3.5, 77.25, dim, dtype=torch.float32)
        p = pk.Point(dim, 17, c.numpy())
        assert native.point_str(17, c) == repr(p)


def test_free_tree():
    t = pk.KDTree.build(pk.generate_problem(1, 2, 10), id_base=1)
    pk.free_tree(t)
    assert t.n == 0 and t.tree_ids.numel() == 0
