"""Exact k-NN on the host: ``ops.knn_cpu`` (the oracle of the GPU kernels) against an oracle that
uses no project code, ``KDTree.knn`` on CPU trees, ``knn_merge`` on host tensors, and the forest
over gloo. Every comparison is bit for bit on the packed (d2, id) rows."""
import numpy as np
import pytest
import torch

import parallel_kd_tree_amd as pk
from parallel_kd_tree_amd import ops
from parallel_kd_tree_amd.ops.query import INF_PACKED

from test_distributed_cpu import run


def numpy_knn(x, ids, q, k):
    """Independent oracle. float32 elementwise IEEE operations, column by column in the
    reference's summation order (bit-equal to sq_dist), packed with the ids, sorted."""
    x = np.ascontiguousarray(x, dtype=np.float32)
    q = np.ascontiguousarray(q, dtype=np.float32)
    ids = np.asarray(ids).astype(np.uint64)
    out = np.full((q.shape[0], k), INF_PACKED, dtype=np.uint64)
    for i in range(q.shape[0]):
        acc = np.zeros(x.shape[0], dtype=np.float32)
        for c in range(x.shape[1]):
            t = x[:, c] - q[i, c]
            acc = acc + t * t
        packed = np.sort((acc.view(np.uint32).astype(np.uint64) << np.uint64(32)) | ids)
        m = min(k, packed.shape[0])
        out[i, :m] = packed[:m]
    return torch.from_numpy(out.view(np.int64))


def problem(n, dim, nq=40, seed=7):
    """n points and nq queries of the reference stream; a quarter of the queries are data points."""
    full = pk.generate_problem(seed, dim, n + nq)
    x, q = full[:n].contiguous(), full[n:].clone()
    hits = nq // 4
    q[:hits] = x[torch.arange(hits) * 7919 % n]
    return x, q


def grid_problem():
    """5 000 points on a 4 x 4 x 4 grid (64 distinct positions) with shuffled distinct ids."""
    g = torch.Generator().manual_seed(5)
    x = torch.randint(0, 4, (5000, 3), generator=g).float()
    ids = (torch.randperm(5000, generator=g) + 100).to(torch.int32)
    q = torch.stack(torch.meshgrid(*[torch.arange(4.0)] * 3, indexing="ij"), -1).reshape(-1, 3)
    return x, ids, q


@pytest.mark.parametrize("n,dim,k", [(1, 3, 1), (2, 3, 4), (65, 2, 64), (5000, 3, 8), (2000, 16, 5)])
def test_knn_cpu_equals_numpy(n, dim, k):
    x, q = problem(n, dim)
    got = ops.knn_cpu(x, None, q, k, id_base=1)
    assert got.dtype == torch.int64 and tuple(got.shape) == (q.shape[0], k)
    assert torch.equal(got, numpy_knn(x.numpy(), np.arange(n) + 1, q.numpy(), k))


def test_duplicates_order_by_id():
    x, ids, q = grid_problem()
    got = ops.knn_cpu(x, ids, q, 16)
    assert torch.equal(got, numpy_knn(x.numpy(), ids.numpy(), q.numpy(), 16))
    d2, gid = ops.unpack(got)
    assert bool((d2 == 0).all()), "every grid position holds more than 16 points: all ties at distance 0"
    assert bool((gid[:, 1:] > gid[:, :-1]).all())


def test_padding_when_k_exceeds_n():
    x, q = problem(5, 3)
    got = ops.knn_cpu(x, None, q, 8)
    assert torch.equal(got, numpy_knn(x.numpy(), np.arange(5), q.numpy(), 8))
    assert bool((got[:, 5:] == INF_PACKED).all()) and bool((got[:, :5] != INF_PACKED).all())
    dist, ids = ops.finalize_knn(got)
    assert bool(torch.isinf(dist[:, 5:]).all()) and bool((ids[:, 5:] == -1).all())
    assert bool((ids[:, :5] >= 0).all())


def test_column0_is_the_1nn_answer():
    x, q = problem(4000, 3)
    tree = pk.KDTree.build(x, id_base=1)
    dist, ids = tree.knn(q, 6)
    d1, i1 = tree.query(q, "brute")
    assert torch.equal(dist[:, 0], d1) and torch.equal(ids[:, 0], i1)
    packed = tree.knn_packed(q, 6)
    assert torch.equal(packed, numpy_knn(x.numpy(), np.arange(4000) + 1, q.numpy(), 6))
    d2, _ = ops.unpack(packed)
    assert torch.equal(dist, ops.query.sqrt_exact(d2))


def test_reference_mode_cpu_tree():
    x, q = problem(1500, 3)
    tree = pk.KDTree.build(x, id_base=1, mode="reference")
    assert torch.equal(tree.knn_packed(q, 7), numpy_knn(x.numpy(), np.arange(1500) + 1, q.numpy(), 7))


def test_knn_merge_cpu():
    x, q = problem(3000, 3)
    whole = ops.knn_cpu(x, None, q, 8)
    acc, chained = None, None
    for lo in (0, 1000, 2000):
        part = ops.knn_cpu(x[lo:lo + 1000], None, q, 8, id_base=lo)
        acc = part if acc is None else ops.knn_merge(acc, part)
        tree = pk.KDTree.build(x[lo:lo + 1000], id_base=lo)
        chained = tree.knn_packed(q, 8, into=chained)
    assert torch.equal(acc, whole)
    assert torch.equal(chained, whole)


@pytest.mark.parametrize("k", [0, 65])
def test_k_out_of_range(k):
    x, q = problem(100, 3)
    with pytest.raises(ValueError):
        ops.knn_cpu(x, None, q, k)
    with pytest.raises(ValueError):
        pk.KDTree.build(x).knn(q, k)
    with pytest.raises(ValueError):
        pk.KDTree.build(x).knn_packed(q, k)


def _forest_knn(rank, world, n, dim, k):
    import parallel_kd_tree_amd as pk
    from parallel_kd_tree_amd import ops
    from parallel_kd_tree_amd.parallel import comm
    from parallel_kd_tree_amd.parallel.forest import ForestTree
    first, cnt = comm.forest_slice(n, world, rank)
    full = pk.generate_problem(5, dim, n + 20)
    f = ForestTree.build(full[first:first + cnt].contiguous(), first, n, id_base=1)
    q = full[n:].clone()
    q[:5] = full[:5]
    got = f.knn_packed(q, k)
    assert torch.equal(got, ops.knn_cpu(full[:n].contiguous(), None, q, k, id_base=1)), f"rank {rank}"


@pytest.mark.parametrize("world,n", [(2, 3000), (3, 3000), (3, 2)])
def test_forest_knn(world, n):
    run(world, _forest_knn, n, 3, 8)
