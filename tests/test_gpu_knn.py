"""Exact k-NN on the GPU (csrc/gpu/knn.hip): the wave-per-query traversal, the slab brute force
and the host oracle ``ops.knn_cpu`` must agree bit for bit on the packed (d2, id) rows, on the
smallest shapes at which each code path can go wrong."""
import pytest
import torch

import parallel_kd_tree_amd as pk
from parallel_kd_tree_amd import ops
from parallel_kd_tree_amd.ops.query import INF_PACKED

pytestmark = pytest.mark.gpu


def problem(n, dim, seed=3, off=200, hits=50):
    """n points of the reference stream; `off` queries off the data plus `hits` data points."""
    full = pk.generate_problem(seed, dim, n + off)
    x = full[:n].contiguous()
    q = torch.cat([full[n:], x[torch.arange(hits) * 7919 % n]]).contiguous()
    return x, q


# (n, dim, depth0, k): 1-2 points; a list exactly full or one short; a whole-tree bucket scan
# (512) against the first real descent (513); several blocks; every compile-time dim path that
# differs (2, 3, 5, 8) and the runtime-dim instance (12)
CASES = [(1, 3, 0, 1), (2, 3, 0, 4), (63, 2, 1, 64), (64, 3, 0, 64), (65, 3, 0, 64), (512, 3, 0, 8), (513, 3, 0, 8),
         (700, 2, 1, 16), (20_000, 3, 0, 1), (20_000, 3, 0, 5), (20_000, 3, 0, 64), (50_000, 8, 0, 16),
         (20_000, 5, 2, 10), (30_000, 12, 0, 8)]


@pytest.mark.parametrize("n,dim,depth0,k", CASES)
def test_traverse_brute_cpu_agree(gpu_device, n, dim, depth0, k):
    x, q = problem(n, dim)
    want = ops.knn_cpu(x, None, q, k, id_base=1)
    tree = pk.KDTree.build(x.to(gpu_device), id_base=1, depth0=depth0).check()
    qd = q.to(gpu_device)
    trav = tree.knn_packed(qd, k, "traverse")
    brute = tree.knn_packed(qd, k, "brute")
    assert trav.dtype == torch.int64 and tuple(trav.shape) == (q.shape[0], k)
    assert torch.equal(trav.cpu(), want), "traversal differs from the host oracle"
    assert torch.equal(brute.cpu(), want), "brute force differs from the host oracle"
    raw = ops.knn_gpu(x.to(gpu_device), None, qd, k, "brute", id_base=1)  # raw points, implicit ids
    assert torch.equal(raw.cpu(), want)


@pytest.mark.parametrize("k", [16, 64])
def test_duplicate_grid(gpu_device, k):
    g = torch.Generator().manual_seed(5)
    x = torch.randint(0, 4, (5000, 3), generator=g).float()
    ids = (torch.randperm(5000, generator=g) + 100).to(torch.int32)
    q = torch.stack(torch.meshgrid(*[torch.arange(4.0)] * 3, indexing="ij"), -1).reshape(-1, 3)
    want = ops.knn_cpu(x, ids, q, k)
    tree = pk.KDTree.build(x.to(gpu_device), ids.to(gpu_device)).check()
    assert torch.equal(tree.knn_packed(q.to(gpu_device), k, "traverse").cpu(), want)
    assert torch.equal(tree.knn_packed(q.to(gpu_device), k, "brute").cpu(), want)
    d2, gid = ops.unpack(want)
    if k == 16:  # every position holds more than 16 points: all ties, ordered by id
        assert bool((d2 == 0).all()) and bool((gid[:, 1:] > gid[:, :-1]).all())


def test_k1_equals_query_packed(gpu_device):
    x = pk.generate_slice(11, 3, 0, 205_000, device=gpu_device)
    tree = pk.KDTree.build(x[:200_000], id_base=1).check()
    q = x[200_000:].contiguous()
    assert torch.equal(tree.knn_packed(q, 1)[:, 0], tree.query_packed(q, "traverse"))


def test_high_dimension_auto_is_brute(gpu_device):
    x, q = problem(3000, 128, off=30, hits=10)
    tree = pk.KDTree.build(x.to(gpu_device), id_base=1)
    assert torch.equal(tree.knn_packed(q.to(gpu_device), 10).cpu(), ops.knn_cpu(x, None, q, 10, id_base=1))


def test_reference_mode_tree(gpu_device):
    x, q = problem(10_000, 3)
    tree = pk.KDTree.build(x.to(gpu_device), id_base=1, mode="reference")
    want = ops.knn_cpu(x, None, q, 9, id_base=1)
    assert torch.equal(tree.knn_packed(q.to(gpu_device), 9, "traverse").cpu(), want)  # always brute force
    dist, ids = tree.knn(q.to(gpu_device), 9)
    wd, wi = ops.finalize_knn(want)
    assert torch.equal(dist.cpu(), wd) and torch.equal(ids.cpu(), wi)


@pytest.mark.parametrize("method", ["traverse", "brute"])
def test_into_and_merge(gpu_device, method):
    x, q = problem(30_000, 3)
    qd = q.to(gpu_device)
    k = 12
    whole = pk.KDTree.build(x.to(gpu_device), id_base=0).knn_packed(qd, k, method)
    assert torch.equal(whole.cpu(), ops.knn_cpu(x, None, q, k))
    trees = [pk.KDTree.build(x[lo:lo + 10_000].to(gpu_device), id_base=lo) for lo in (0, 10_000, 20_000)]
    acc = torch.full((q.shape[0], k), INF_PACKED, dtype=torch.int64, device=gpu_device)
    merged = None
    for t in trees:
        ret = t.knn_packed(qd, k, method, into=acc)
        assert ret.data_ptr() == acc.data_ptr(), "`into` is updated in place and returned"
        part = t.knn_packed(qd, k, method)
        merged = part if merged is None else ops.knn_merge(merged, part)
    assert torch.equal(acc, whole)
    assert torch.equal(merged, whole)


def test_finalize_knn(gpu_device):
    x, q = problem(40, 3)
    tree = pk.KDTree.build(x.to(gpu_device), id_base=1)
    packed = tree.knn_packed(q.to(gpu_device), 64)
    dist, ids = ops.finalize_knn(packed)
    assert dist.dtype == torch.float32 and ids.dtype == torch.int64 and tuple(dist.shape) == tuple(packed.shape)
    d2, want_ids = ops.unpack(packed.cpu())
    assert torch.equal(dist.cpu(), ops.query.sqrt_exact(d2))
    assert torch.equal(ids[:, :40].cpu(), want_ids[:, :40])
    assert bool(torch.isinf(dist[:, 40:]).all()) and bool((ids[:, 40:] == -1).all())
    assert bool(torch.isfinite(dist[:, :40]).all())
    d2k, idk = tree.knn(q.to(gpu_device), 64)
    assert torch.equal(d2k, dist) and torch.equal(idk, ids)


def test_errors(gpu_device):
    x, q = problem(1000, 3)
    tree = pk.KDTree.build(x.to(gpu_device), id_base=1)
    qd = q.to(gpu_device)
    for k in (0, 65):
        with pytest.raises(ValueError):
            tree.knn_packed(qd, k)
        with pytest.raises(ValueError):
            ops.knn_gpu(tree.tree_pts, tree.tree_ids, qd, k, "brute")
    with pytest.raises(ValueError):  # low-level entry point, past the Python checks
        ops.native().knn(tree.tree_pts, tree.tree_ids, 0, qd, 65, "brute", 0, None)
    x40, q40 = problem(500, 40, off=20, hits=5)
    t40 = pk.KDTree.build(x40.to(gpu_device), id_base=1)
    with pytest.raises(ValueError):
        t40.knn_packed(q40.to(gpu_device), 4, "traverse")
    with pytest.raises(ValueError):
        ops.native().knn(t40.tree_pts, t40.tree_ids, 0, q40.to(gpu_device), 4, "traverse", 0, None)
    with pytest.raises(ValueError):  # wrong shape
        tree.knn_packed(qd, 4, into=torch.full((q.shape[0], 5), INF_PACKED, dtype=torch.int64, device=gpu_device))
    with pytest.raises(ValueError):  # wrong device
        tree.knn_packed(qd, 4, into=torch.full((q.shape[0], 4), INF_PACKED, dtype=torch.int64))
