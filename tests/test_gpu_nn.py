"""Exact 1-NN on the GPU (csrc/gpu/query.hip) against host oracles, on every dispatch path.

Exact-mode answers (``k_brute``, ``k_brute_pf``, the MFMA filter's fallback, ``k_nn_wave``,
``k_traverse<false>``) are compared bit for bit, as packed (d2, id) int64 values, with
``ops.knn_cpu(..., k=1)`` (pinned to numpy by tests/test_knn_cpu.py). Reference-mode answers
(``k_traverse<true>``, ``k_ref_visit_all`` / ``k_ref_resolve``) are compared, distance and id,
with the host search on the same tree. ``k_finalize`` is compared with numpy's float32 sqrt
and ``k_check`` with the host invariant checker. Shapes are the smallest at which each path
can still go wrong; the path each case takes is read from nn_brute / nn_traverse /
nn_traverse_reference."""
import numpy as np
import pytest
import torch

import parallel_kd_tree_amd as pk
from parallel_kd_tree_amd import ops
from parallel_kd_tree_amd.ops.query import INF_PACKED

pytestmark = pytest.mark.gpu


# ------------------------------------------------------------------------------ helpers
def oracle(x, ids, q, id_base=0):
    """Packed 1-NN of every query on the host."""
    return ops.knn_cpu(x, ids, q, 1, id_base)[:, 0].contiguous()


def stream(n, dim, nq, seed):
    """n points and nq queries of the reference stream; every fourth query is a data point."""
    full = pk.generate_problem(seed, dim, n + nq)
    x, q = full[:n].contiguous(), full[n:].clone()
    hit = torch.arange(0, nq, 4)
    q[hit] = x[(hit * 7919 + 1) % n]
    return x, q


def shuffled_ids(n, seed):
    """Distinct shuffled ids as int32 bits; up to 15 of them are 0xFFFFFFF0 + i (top bit set)."""
    g = torch.Generator().manual_seed(seed)
    v = torch.randperm(n, generator=g) + 100
    top = min(15, n)
    v[:top] = 0xFFFFFFF0 + torch.arange(top)
    v = v[torch.randperm(n, generator=g)]
    return torch.where(v >= 2 ** 31, v - 2 ** 32, v).to(torch.int32)


def misaligned(t, device):
    """A contiguous device copy of ``t`` that starts 4 B past a 16-B boundary."""
    n, dim = t.shape
    v = torch.empty(n * dim + 1, dtype=torch.float32, device=device)[1:].view(n, dim)
    v.copy_(t)
    assert v.is_contiguous() and v.data_ptr() % 16 == 4
    return v


def same(got, want):
    assert got.dtype == torch.int64 and got.shape == want.shape
    return torch.equal(got.cpu(), want.cpu())


def check_into(whole, halves, want, device):
    """``whole(into)`` answers over all points, ``halves[i](into)`` over two disjoint halves of
    them (with their id_base); all update ``into`` in place when it is given."""
    nq = want.numel()
    wd = want.to(device)
    inf = lambda: torch.full((nq,), INF_PACKED, dtype=torch.int64, device=device)  # noqa: E731
    assert torch.equal(whole(None), wd)
    acc = inf()
    ret = whole(acc)
    assert ret.data_ptr() == acc.data_ptr(), "`into` is updated in place and returned"
    assert torch.equal(acc, wd), "a start of INF_PACKED changes the answer"
    for order in (halves, halves[::-1]):
        acc = inf()
        for h in order:
            h(acc)
        assert torch.equal(acc, wd), "chaining the two halves differs from the whole"
    zero = torch.zeros(nq, dtype=torch.int64, device=device)  # pack(0.0, 0): nothing is smaller
    whole(zero)
    assert not bool(zero.any()), "a start of pack(0.0, 0) was overwritten"
    even = (torch.arange(nq, device=device) % 2) == 0
    mixed = torch.where(even, torch.zeros_like(wd), inf())
    whole(mixed)
    assert torch.equal(mixed, torch.where(even, torch.zeros_like(wd), wd))


# ------------------------------------------------------------------------------ 1. brute force
# k_brute<false>: 1, 3, 5, 7 (tail loop only), 33, 37 (one 32-chunk + tail);
# k_brute<true>: 4, 8, 12 (tail loop only), 36, 40 (one 32-chunk + tail)
@pytest.mark.parametrize("dim", [1, 3, 5, 7, 33, 37, 4, 8, 12, 36, 40])
def test_brute_low_dims(gpu_device, dim):
    for n in (1, 255, 256, 257, 3000):
        x, q = stream(n, dim, 50, seed=dim)
        if n > 10:  # a duplicated row and a query on it: the smaller id wins
            x[n - 3] = x[1]
            q[1] = x[1]
        ids = shuffled_ids(n, n + dim)
        want_raw, want_ids = oracle(x, None, q, 1), oracle(x, ids, q)
        xd, qd = x.to(gpu_device), q.to(gpu_device)
        tree = pk.KDTree.build(xd, ids.to(gpu_device)).check()
        for nq in (1, 15, 16, 17, 50):
            assert same(ops.nn_gpu(xd, None, qd[:nq], "brute", id_base=1), want_raw[:nq]), (n, nq)
            assert same(tree.query_packed(qd[:nq], "brute"), want_ids[:nq]), (n, nq)


# aligned: k_brute<true> (8), k_brute_pf<QT, 32> (32, 64), the MFMA filter (n >= 4096, nq >= 16);
# any misaligned operand: k_brute<false> with 0, 1 or 2 register chunks
@pytest.mark.parametrize("dim", [8, 32, 64])
def test_brute_misaligned_views(gpu_device, dim):
    for n, nq in ((300, 17), (3000, 50), (4200, 20)):
        x, q = stream(n, dim, nq, seed=dim + 1)
        ids = shuffled_ids(n, dim)
        want = oracle(x, ids, q)
        xa, qa, idd = x.to(gpu_device), q.to(gpu_device), ids.to(gpu_device)
        xm, qm = misaligned(x, gpu_device), misaligned(q, gpu_device)
        aligned = ops.nn_gpu(xa, idd, qa, "brute")
        assert same(aligned, want)
        for xs, qs in ((xm, qa), (xa, qm), (xm, qm)):
            got = ops.nn_gpu(xs, idd, qs, "brute")
            assert torch.equal(got, aligned) and same(got, want), (n, nq)


# k_brute_pf<QT, 16>: QT = 1, 2, 4, 8, 10, 16 by nq; dim 16 is the single-chunk edge
@pytest.mark.parametrize("dim", [16, 48, 80])
def test_brute_pf_ch16(gpu_device, monkeypatch, dim):
    _brute_pf(gpu_device, monkeypatch, dim, (1, 2, 3, 4, 5, 8, 9, 10, 11, 16, 17, 40), (16, 17, 40))


# k_brute_pf<QT, 32>: QT = 1, 2, 4, 8, 10; nq 11 and 15 take <16, 16>; dim 32 is the single chunk
@pytest.mark.parametrize("dim", [32, 64, 96])
def test_brute_pf_ch32(gpu_device, monkeypatch, dim):
    _brute_pf(gpu_device, monkeypatch, dim, (1, 2, 3, 5, 9, 10, 11, 15), (16, 17))


def _brute_pf(device, monkeypatch, dim, nqs, nqs_large):
    nqmax = max(nqs + nqs_large)
    for n in (1, 300, 4000, 4100):
        x, q = stream(n, dim, nqmax, seed=dim + n)
        if n > 10:
            x[n - 3] = x[1]
            q[1] = x[1]
        ids = shuffled_ids(n, n + dim)
        want_raw, want_ids = oracle(x, None, q, 1), oracle(x, ids, q)
        xd, qd, idd = x.to(device), q.to(device), ids.to(device)
        if n >= 4096:  # nq >= 16 would take the MFMA filter: switched off, <16, 16> runs
            monkeypatch.setenv("PKD_BRUTE_MFMA", "0")
        for nq in (nqs_large if n >= 4096 else nqs):
            assert same(ops.nn_gpu(xd, None, qd[:nq], "brute", id_base=1), want_raw[:nq]), (n, nq)
            assert same(ops.nn_gpu(xd, idd, qd[:nq], "brute"), want_ids[:nq]), (n, nq)
        monkeypatch.delenv("PKD_BRUTE_MFMA", raising=False)


# (dim, n, nq, MFMA): k_brute<false>, k_brute<true>, k_brute_pf<10, 16>, <16, 16> (two tiles),
# k_brute_pf<8, 32>, the MFMA filter, and <16, 16> at the filter's shape with the filter off
@pytest.mark.parametrize("dim,n,nq,mfma", [(3, 3000, 50, "1"), (8, 3000, 50, "1"), (48, 3000, 10, "1"),
                                           (48, 3000, 20, "1"), (64, 3000, 7, "1"), (64, 4200, 20, "1"),
                                           (64, 4200, 20, "0")])
def test_brute_into(gpu_device, monkeypatch, dim, n, nq, mfma):
    monkeypatch.setenv("PKD_BRUTE_MFMA", mfma)
    x, q = stream(n, dim, nq, seed=dim + 2)
    xd, qd = x.to(gpu_device), q.to(gpu_device)
    h = n // 2
    lo, hi = xd[:h].contiguous(), xd[h:].contiguous()
    check_into(lambda into: ops.nn_gpu(xd, None, qd, "brute", id_base=1, into=into),
               [lambda into: ops.nn_gpu(lo, None, qd, "brute", id_base=1, into=into),
                lambda into: ops.nn_gpu(hi, None, qd, "brute", id_base=1 + h, into=into)],
               oracle(x, None, q, 1), gpu_device)


# ------------------------------------------------------------------------------ 2. traversal
def both_traversals(tree, q, monkeypatch):
    """The default traversal (k_nn_wave up to dim 32, k_traverse<false> above) and the forced
    thread-per-query kernel (k_traverse<false> at every dim)."""
    monkeypatch.delenv("PKD_TRAVERSE", raising=False)
    wave = tree.query_packed(q, "traverse")
    monkeypatch.setenv("PKD_AB", "1")
    monkeypatch.setenv("PKD_TRAVERSE", "thread")
    thread = tree.query_packed(q, "traverse")
    monkeypatch.delenv("PKD_TRAVERSE", raising=False)
    return wave, thread


# k_nn_wave<1..8>, k_nn_wave<0> at its limits 9 and 32 (and 12, 31), k_traverse<false> above;
# n: below, at and above the 512-point bucket and its first two descents; nq 3 and 5 leave a
# partial block of 4 waves
@pytest.mark.parametrize("dim", [1, 2, 3, 4, 5, 6, 7, 8, 9, 12, 31, 32, 33, 40])
def test_traverse_every_dim(gpu_device, monkeypatch, dim):
    for n in (1, 2, 3, 511, 512, 513, 1025, 1026, 20_000):
        x, q = stream(n, dim, 1000, seed=100 + dim)
        want = oracle(x, None, q, 1).to(gpu_device)
        xd, qd = x.to(gpu_device), q.to(gpu_device)
        for depth0 in (0, 1, dim - 1, dim + 2):
            tree = pk.KDTree.build(xd, id_base=1, depth0=depth0).check()
            for nq in (1, 3, 4, 5, 1000):
                wave, thread = both_traversals(tree, qd[:nq], monkeypatch)
                assert torch.equal(wave, want[:nq]), ("default", n, depth0, nq)
                assert torch.equal(thread, want[:nq]), ("thread", n, depth0, nq)


def lattice_queries(dim, lo, hi, step, limit=1000):
    """Every point of the grid lo, lo + step, ..., hi in `dim` dimensions (a seeded sample of
    `limit` of them when there are more)."""
    vals = torch.arange(lo, hi + step / 2, step)
    if len(vals) ** dim <= limit:
        return torch.stack(torch.meshgrid(*[vals] * dim, indexing="ij"), -1).reshape(-1, dim).contiguous()
    g = torch.Generator().manual_seed(dim)
    return vals[torch.randint(0, len(vals), (limit, dim), generator=g)].contiguous()


# about 5000 points on {0..3}^dim with shuffled explicit ids: heavy duplicates at low dims, and
# queries on the half-step grid are exactly equidistant from points on both sides of split
# planes (dax2 == bd), where only `dax2 <= bd` lets the smaller id on the far side win
@pytest.mark.parametrize("dim", [1, 2, 3, 4, 6, 7, 9, 12, 33])
def test_traverse_lattice_ties(gpu_device, monkeypatch, dim):
    g = torch.Generator().manual_seed(40 + dim)
    n = 5003
    x = torch.randint(0, 4, (n, dim), generator=g).float()
    ids = shuffled_ids(n, dim)
    on = lattice_queries(dim, 0.0, 3.0, 1.0)
    half = lattice_queries(dim, -0.5, 3.5, 0.5)
    want_on, want_half = oracle(x, ids, on), oracle(x, ids, half)
    d2, _ = ops.unpack(want_on)
    if dim <= 4:
        assert bool((d2 == 0).all())
    for depth0 in (0, 1):
        tree = pk.KDTree.build(x.to(gpu_device), ids.to(gpu_device), depth0=depth0).check()
        for q, want in ((on, want_on), (half, want_half)):
            wave, thread = both_traversals(tree, q.to(gpu_device), monkeypatch)
            assert same(wave, want), ("default", depth0)
            assert same(thread, want), ("thread", depth0)
            assert same(tree.query_packed(q.to(gpu_device), "brute"), want)


@pytest.mark.parametrize("dim", [3, 5, 12, 33])
@pytest.mark.parametrize("kind", ["identical", "far", "signed_zero"])
def test_traverse_degenerate_data(gpu_device, monkeypatch, dim, kind):
    g = torch.Generator().manual_seed(dim)
    n, nq = 1500, 200
    if kind == "identical":  # all points identical: every plane ties, the smallest id wins
        x, q = stream(n, dim, nq, seed=dim)
        x[:] = x[0].clone()
        q[:3] = x[0]
    elif kind == "far":  # queries far outside the box
        x, q = stream(n, dim, nq, seed=dim)
        q = torch.where(torch.rand(q.shape, generator=g) < 0.5, q + 1e4, q - 1e4)
        q[:4] = torch.tensor([1e4, -1e4, 1e4, -1e4])[:, None].expand(4, dim)
    else:  # coordinates in {-1, -0.0, +0.0, 1}: -0.0 sorts before +0.0 but compares equal
        def signed(shape):
            v = torch.randint(-1, 2, shape, generator=g).float()
            return torch.where(torch.rand(shape, generator=g) < 0.5, -v, v)
        x, q = signed((n, dim)), signed((nq, dim))
        assert bool((torch.signbit(x) & (x == 0)).any()) and bool((~torch.signbit(x) & (x == 0)).any())
    ids = shuffled_ids(n, dim + 1)
    want = oracle(x, ids, q)
    for depth0 in (0, dim + 2):
        tree = pk.KDTree.build(x.to(gpu_device), ids.to(gpu_device), depth0=depth0).check()
        wave, thread = both_traversals(tree, q.to(gpu_device), monkeypatch)
        assert same(wave, want), ("default", depth0)
        assert same(thread, want), ("thread", depth0)


# k_nn_wave<3>, k_nn_wave<0> and k_traverse<false> (forced at 3, by dim at 40)
@pytest.mark.parametrize("dim,mode", [(3, "default"), (12, "default"), (3, "thread"), (40, "default")])
def test_traverse_into(gpu_device, monkeypatch, dim, mode):
    if mode == "thread":
        monkeypatch.setenv("PKD_AB", "1")
        monkeypatch.setenv("PKD_TRAVERSE", "thread")
    n, nq = 3000, 101
    x, q = stream(n, dim, nq, seed=dim + 3)
    xd, qd = x.to(gpu_device), q.to(gpu_device)
    h = n // 2
    whole = pk.KDTree.build(xd, id_base=1).check()
    parts = [pk.KDTree.build(xd[:h].contiguous(), id_base=1, depth0=1).check(),
             pk.KDTree.build(xd[h:].contiguous(), id_base=1 + h, depth0=2).check()]
    check_into(lambda into: whole.query_packed(qd, "traverse", into=into),
               [lambda into, t=t: t.query_packed(qd, "traverse", into=into) for t in parts],
               oracle(x, None, q, 1), gpu_device)


# ------------------------------------------------------------------------------ 3. reference search
def slot_axes(n, dim, depth0):
    """Split axis of every slot of the implicit tree."""
    ax = np.empty(n, dtype=np.int64)
    stack = [(0, n, 0)]
    while stack:
        lo, c, d = stack.pop()
        if c <= 0:
            continue
        ax[lo + c // 2] = (depth0 + d) % dim
        stack += [(lo, c // 2, d + 1), (lo + c // 2 + 1, c - c // 2 - 1, d + 1)]
    return ax


def shortcut_rule(tree_pts, q, depth0):
    """The visit-all shortcut's own rule in plain numpy float32 (sequential sums, separately
    rounded): per query, (gap^2 < min d2 at every slot, number of slots at the minimum, min d2,
    max gap^2)."""
    P, Q = tree_pts.numpy(), q.numpy()
    n, dim = P.shape
    ax = slot_axes(n, dim, depth0)
    pa = P[np.arange(n), ax]
    proved, ties = np.empty(len(Q), dtype=bool), np.empty(len(Q), dtype=np.int64)
    dmin, gmax = np.empty(len(Q), dtype=np.float32), np.empty(len(Q), dtype=np.float32)
    for i in range(len(Q)):
        acc = np.zeros(n, dtype=np.float32)
        for c in range(dim):
            t = P[:, c] - Q[i, c]
            acc = acc + t * t
        gap = Q[i, ax] - pa
        dmin[i], gmax[i] = acc.min(), (gap * gap).max()
        proved[i] = bool(gmax[i] < dmin[i])
        ties[i] = int((acc == dmin[i]).sum())
    return proved, ties, dmin, gmax


def host_search(tree, q):
    """Packed answers of the host reference search on a CPU tree."""
    slots, d2 = ops.nn_cpu(tree.tree_pts, q, tree.depth0)
    ids = tree.tree_ids.to(torch.int64)[slots] & 0xFFFFFFFF
    return (d2.view(torch.int32).to(torch.int64) << 32) | ids


def reference_problem(n, dim, dups):
    """Points (a third of the rows copies of other rows when `dups`) and 400 queries, by index
    % 4: off the data inside the box, a data point, far outside the box (all axis gaps small
    against the distance), off the data."""
    nq = 400
    full = pk.generate_problem(300 + dim, dim, n + nq)
    x, q = full[:n].clone(), full[n:].clone()
    if dups:
        g = torch.Generator().manual_seed(dim)
        x = torch.cat([x[: n - n // 3], x[: n // 3]])[torch.randperm(n, generator=g)].contiguous()
    k = torch.arange(nq)
    q[k % 4 == 1] = x[(k[k % 4 == 1] * 7919) % x.shape[0]]
    q[k % 4 == 2] = q[k % 4 == 2].sign() * 1000 + q[k % 4 == 2]
    return x, q.contiguous()


# dims 3, 8: k_traverse<true> alone; 16, 64: nn_brute + k_ref_visit_all + k_ref_resolve, then
# k_traverse<true> on the selected queries (64-D with 4500 points: the MFMA filter from 16 queries)
@pytest.mark.parametrize("dups", [False, True])
@pytest.mark.parametrize("n,dim,depth0", [(3000, 3, 0), (3000, 8, 1), (3000, 16, 0), (4500, 64, 2)])
def test_reference_search_distance_and_id(gpu_device, n, dim, depth0, dups):
    x, q = reference_problem(n, dim, dups)
    tc = pk.KDTree.build(x, id_base=1, mode="reference", depth0=depth0)
    tg = tc.to(gpu_device)
    want = host_search(tc, q)
    if dim >= 16:  # both resolve routes run: answered by the proof, and handed to the walk
        proved, ties, dmin, gmax = shortcut_rule(tc.tree_pts, q, depth0)
        for nq in (16, 17, 400):
            shortcut = proved[:nq] & (ties[:nq] == 1)
            assert shortcut.any() and (~proved[:nq]).any(), (nq, shortcut.sum(), (~proved[:nq]).sum())
        assert (ties[np.arange(400) % 4 == 1] >= 1).all() and not proved[np.arange(400) % 4 == 1].any()
        if dups:  # proved, but the minimum is not unique: the walk must answer (first visited, not
            # smallest id) -- and for some of them these differ
            tied = proved & (ties > 1)
            assert tied.any()
            brute = oracle(tc.tree_pts, tc.tree_ids, q)
            assert bool((brute[torch.from_numpy(tied)] != want[torch.from_numpy(tied)]).any())
    qd = q.to(gpu_device)
    for nq in (1, 16, 17, 400):
        assert same(tg.query_packed(qd[:nq]), want[:nq]), nq
    dg, ig = tg.query(qd)
    dc, ic = tc.query(q)
    assert torch.equal(dg.cpu().view(torch.int32), dc.view(torch.int32)) and torch.equal(ig.cpu(), ic)
    d2, wid = ops.unpack(want)
    assert torch.equal(ic, wid) and torch.equal(dc, ops.query.sqrt_exact(d2))
    # into: INF_PACKED is no start value at all; distance 0 is never beaten
    acc = torch.full((400,), INF_PACKED, dtype=torch.int64, device=gpu_device)
    assert tg.query_packed(qd, into=acc).data_ptr() == acc.data_ptr() and same(acc, want)
    zero = torch.zeros(400, dtype=torch.int64, device=gpu_device)
    tg.query_packed(qd, into=zero)
    assert not bool(zero.any())
    even = (torch.arange(400, device=gpu_device) % 2) == 0
    mixed = torch.where(even, torch.zeros_like(acc), torch.full_like(acc, INF_PACKED))
    tg.query_packed(qd, into=mixed)
    assert torch.equal(mixed, torch.where(even, torch.zeros_like(acc), want.to(gpu_device)))
    if dim >= 16:
        # a finite incoming best on the queries whose walk provably visits every node: the search
        # replaces it only by a strictly smaller distance. Below the minimum (and above every
        # gap^2) or equal to it, it stays; at twice the minimum the tree's own answer replaces it
        start, expect = np.full(400, INF_PACKED, dtype=np.int64), want.numpy().copy()
        used = set()
        for j, i in enumerate(np.flatnonzero(proved)):
            mid = np.float32((np.float64(gmax[i]) + np.float64(dmin[i])) / 2)
            d_in = (mid, dmin[i], np.float32(2) * dmin[i])[j % 3]
            if not gmax[i] < d_in:
                continue
            start[i] = (int(np.array([d_in], dtype=np.float32).view(np.uint32)[0]) << 32) | 7
            if d_in <= dmin[i]:
                expect[i] = start[i]
            used.add(j % 3)
        assert used == {0, 1, 2}
        acc = torch.from_numpy(start).to(gpu_device)
        tg.query_packed(qd, into=acc)
        assert torch.equal(acc.cpu(), torch.from_numpy(expect))


# ------------------------------------------------------------------------------ 4. finalize
def test_finalize_sqrt_is_correctly_rounded(gpu_device):
    g = torch.Generator().manual_seed(9)
    per = 4200
    expo = torch.arange(0, 255).repeat_interleave(per)  # 0: subnormals; 255 (inf / NaN) apart
    mant = torch.randint(0, 1 << 23, (expo.numel(),), generator=g)
    roots = torch.arange(1, 4097, dtype=torch.float32)
    squares = (roots * roots).view(torch.int32).to(torch.int64)  # exact up to 2^24
    special = torch.tensor([0, 1, 2, 0x007FFFFF, 0x00800000, 0x7F7FFFFF, 0x7F800000, 0x3F800000, 0x3F7FFFFF,
                            0x3F800001, 0x40000000, 0x40800000])
    bits = torch.cat([(expo << 23) | mant, squares - 1, squares, squares + 1, special, torch.tensor([INF_PACKED >> 32])])
    ids = torch.randint(0, 1 << 32, (bits.numel(),), generator=g)
    ids[:6] = torch.tensor([0, 1, 0x7FFFFFFF, 0x80000000, 0xFFFFFFFE, 0xFFFFFFFF])
    ids[-1] = INF_PACKED & 0xFFFFFFFF
    packed = (bits << 32) | ids
    assert packed.numel() >= 1 << 20 and int(packed[-1]) == INF_PACKED and bool((packed >= 0).all())
    dist, got_ids = ops.finalize(packed.to(gpu_device))
    assert dist.dtype == torch.float32 and got_ids.dtype == torch.int64
    d2 = bits.to(torch.int32).view(torch.float32)
    want = ops.query.sqrt_exact(d2)
    assert torch.equal(dist.cpu().view(torch.int32), want.view(torch.int32))
    assert torch.equal(got_ids.cpu(), ids) and bool((got_ids >= 0).all())
    assert float(dist[-1]) == float("inf") and int(got_ids[-1]) == 0xFFFFFFFF
    hd, hi = ops.finalize(packed)  # the host path agrees
    assert torch.equal(hd.view(torch.int32), want.view(torch.int32)) and torch.equal(hi, ids)


# ------------------------------------------------------------------------------ 5. invariant checker
def path_to(n, slot):
    """(lo, count, depth) of every node from the root down to `slot`."""
    out, lo, c, d = [], 0, n, 0
    while True:
        m = lo + c // 2
        out.append((lo, c, d))
        if slot == m:
            return out
        if slot < m:
            c = c // 2
        else:
            lo, c = m + 1, c - c // 2 - 1
        d += 1


def leftmost_leaf(lo, c):
    while c > 1:
        c = c // 2
    return lo


def leaves(n):
    out, stack = [], [(0, n)]
    while stack:
        lo, c = stack.pop()
        if c == 1:
            out.append(lo)
        elif c > 1:
            stack += [(lo, c // 2), (lo + c // 2 + 1, c - c // 2 - 1)]
    return sorted(out)


def both_counts(tp, ti, depth0, device):
    cpu = pk.KDTree(tp, ti, depth0).invariant_violations()
    gpu = pk.KDTree(tp.to(device), ti.to(device), depth0).invariant_violations()
    return cpu, gpu


def swap_rows(tp, ti, a, b):
    tp, ti = tp.clone(), ti.clone()
    tp[[a, b]] = tp[[b, a]]
    ti[[a, b]] = ti[[b, a]]
    return tp, ti


@pytest.mark.parametrize("n,dim,depth0", [(1000, 3, 0), (5000, 5, 2), (700, 2, 1)])
def test_invariant_checker_single_corruptions(gpu_device, n, dim, depth0):
    x = pk.generate_problem(n + dim, dim, n)
    tp, ti = ops.build_cpu(x, shuffled_ids(n, n), "exact", depth0)
    assert both_counts(tp, ti, depth0, gpu_device) == (0, 0)
    lv = leaves(n)
    for leaf in (lv[0], lv[len(lv) // 3], lv[-1]):
        path = path_to(n, leaf)
        lo, c, d = path[-4]  # the ancestor three levels up
        anc = lo + c // 2
        # two leaves under different children of that ancestor
        other = leftmost_leaf(anc + 1, c - c // 2 - 1) if leaf < anc else leftmost_leaf(lo, c // 2)
        assert (other < anc) != (leaf < anc) and len(path_to(n, other)) >= len(path) - 1
        for a, b in ((leaf, other), (leaf, anc)):  # ... and the ancestor with its own leaf
            cpu, gpu = both_counts(*swap_rows(tp, ti, a, b), depth0, gpu_device)
            assert cpu > 0 and gpu > 0, (leaf, a, b, cpu, gpu)
        # one coordinate of the leaf, on an axis that is not its own, crosses the plane of the
        # highest ancestor that splits on that axis (by one float)
        own = (depth0 + path[-1][2]) % dim
        alo, ac, ad = next(p for p in path[:-1] if (depth0 + p[2]) % dim != own)
        am, axis = alo + ac // 2, (depth0 + ad) % dim
        moved = tp.clone()
        moved[leaf, axis] = torch.nextafter(tp[am, axis], torch.tensor(float("inf") if leaf < am else float("-inf")))
        cpu, gpu = both_counts(moved, ti, depth0, gpu_device)
        assert cpu > 0 and gpu > 0, (leaf, am, axis, cpu, gpu)


@pytest.mark.parametrize("n,dim,depth0", [(1000, 3, 0), (5000, 5, 2), (700, 2, 1)])
def test_invariant_checker_id_order_only(gpu_device, n, dim, depth0):
    """Duplicate-key data: two identical rows, one an ancestor of the other, swapped. Every
    coordinate comparison still holds; only the (key, id) order at the ancestor is wrong."""
    g = torch.Generator().manual_seed(n)
    x = torch.randint(0, 4, (n, dim), generator=g).float()
    tp, ti = ops.build_cpu(x, shuffled_ids(n, dim), "exact", depth0)
    assert both_counts(tp, ti, depth0, gpu_device) == (0, 0)
    found = 0
    for leaf in leaves(n):
        for lo, c, _ in path_to(n, leaf)[:-1]:
            anc = lo + c // 2
            if torch.equal(tp[anc], tp[leaf]):
                stp, sti = swap_rows(tp, ti, leaf, anc)
                assert torch.equal(stp, tp) and not torch.equal(sti, ti)
                cpu, gpu = both_counts(stp, sti, depth0, gpu_device)
                assert cpu > 0 and gpu > 0, (leaf, anc, cpu, gpu)
                found += 1
                break
        if found == 3:
            break
    assert found == 3
