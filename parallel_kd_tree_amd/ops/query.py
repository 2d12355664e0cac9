"""Exact 1-NN and k-NN query ops (csrc/gpu/query.hip, csrc/gpu/knn.hip, csrc/cpu/cpu_tree.cpp).

GPU results are packed int64: ``(float_bits(d2) << 32) | id`` so a plain MIN (also across
ranks) is the lexicographic (distance, id) minimum, and a k-NN row is the k smallest packed
values in ascending order.
"""
from __future__ import annotations

from typing import Optional, Tuple

import torch

from . import native

INF_PACKED = (0x7F800000 << 32) | 0xFFFFFFFF


def nn_gpu(points: torch.Tensor, ids: Optional[torch.Tensor], queries: torch.Tensor, method: str = "brute",
           depth0: int = 0, id_base: int = 0, into: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Packed (d2, id) nearest neighbours of ``queries`` among ``points``.

    method='brute' works on any point array; method='traverse' needs an implicit in-order
    tree (``points``, ``ids`` from a build) whose root is at depth ``depth0``. With ``into``
    the results are MIN-accumulated into an existing packed tensor (forest queries).
    """
    return native().nn(points.contiguous(), ids, int(id_base), queries.contiguous(), method, int(depth0), into)


def unpack(packed: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """Packed int64 -> (squared distance float32, id int64)."""
    p = packed.to(torch.int64)
    d2 = (p >> 32).to(torch.int32).view(torch.float32)
    ids = p & 0xFFFFFFFF
    return d2, ids


def finalize(packed: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """Packed -> (distance = correctly rounded sqrtf(d2), id). On the GPU this runs a HIP
    kernel: torch's device sqrt is not correctly rounded, the reference's is."""
    if packed.is_cuda:
        d, i = native().nn_finalize(packed.contiguous())
        return d, i
    d2, ids = unpack(packed)
    return sqrt_exact(d2), ids


def sqrt_exact(d2: torch.Tensor) -> torch.Tensor:
    """Correctly rounded fp32 sqrt on the host. torch's CPU sqrt may use a 0.5001-ulp SIMD
    polynomial on some CPUs; numpy uses the hardware sqrt instruction (IEEE exact)."""
    import numpy as np
    return torch.from_numpy(np.sqrt(d2.detach().cpu().to(torch.float32).numpy()))


KNN_MAX = 64


def _check_k(k: int) -> int:
    k = int(k)
    if not 1 <= k <= KNN_MAX:
        raise ValueError(f"k must be in 1..{KNN_MAX}, got {k}")
    return k


def knn_gpu(points: torch.Tensor, ids: Optional[torch.Tensor], queries: torch.Tensor, k: int, method: str = "brute",
            depth0: int = 0, id_base: int = 0, into: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Packed k nearest neighbours: int64 [nq, k], every row the k smallest packed (d2, id) in
    ascending order (ties on distance -> smaller id), padded with ``INF_PACKED`` where fewer than
    k points exist. Ids must be distinct.

    method='brute' works on any point array and dimension; method='traverse' needs an implicit
    exact-mode tree whose root is at depth ``depth0``, dim <= 32. ``into`` ([nq, k], sorted rows)
    is the starting list: it is updated in place and returned, and prunes the search from the
    first node. The lists chained this way must come from disjoint point sets (forest slices);
    searching the same tree twice into one list duplicates its entries.
    """
    k = _check_k(k)
    if method not in ("brute", "traverse"):
        raise ValueError("method must be 'brute' or 'traverse'")
    if method == "traverse" and points.shape[1] > 32:
        raise ValueError("k-NN traversal needs dim <= 32; use method='brute'")
    if into is not None and (into.dtype != torch.int64 or tuple(into.shape) != (queries.shape[0], k)
                             or into.device != points.device or not into.is_contiguous()):
        raise ValueError("`into` must be a contiguous int64 [nq, k] tensor on the tree's device")
    return native().knn(points.contiguous(), ids, int(id_base), queries.contiguous(), k, method, int(depth0), into)


def knn_cpu(points: torch.Tensor, ids: Optional[torch.Tensor], queries: torch.Tensor, k: int,
            id_base: int = 0) -> torch.Tensor:
    """Exact brute-force k-NN on the host, packed like ``knn_gpu`` (its oracle): any layout."""
    k = _check_k(k)
    return native().knn_cpu(points.detach().cpu().to(torch.float32).contiguous(),
                            None if ids is None else ids.detach().cpu().contiguous(), int(id_base),
                            queries.detach().cpu().to(torch.float32).contiguous(), k)


def knn_merge(a: torch.Tensor, b: torch.Tensor) -> torch.Tensor:
    """The k smallest entries per row of two sorted packed [nq, k] lists (of disjoint point
    sets): a HIP kernel for GPU tensors, a sort on the host."""
    if a.dim() != 2 or a.shape != b.shape:
        raise ValueError("knn_merge needs two [nq, k] tensors of one shape")
    _check_k(a.shape[1])
    return native().knn_merge(a.contiguous(), b.contiguous())


def finalize_knn(packed: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """Packed [nq, k] -> (distance float32 [nq, k] = correctly rounded sqrtf(d2), id int64
    [nq, k]); padding entries become ``inf`` / ``-1``."""
    d, i = finalize(packed.reshape(-1))
    pad = packed.reshape(-1) == INF_PACKED
    i = torch.where(pad.to(i.device), torch.full_like(i, -1), i)
    return d.reshape(packed.shape), i.reshape(packed.shape)


def nn_cpu(tree_pts: torch.Tensor, queries: torch.Tensor, depth0: int = 0, brute: bool = False):
    """Reference-procedure search on a CPU tree: returns (slot int64, d2 float32)."""
    return tuple(native().search_cpu(tree_pts.contiguous(), queries.to(torch.float32).contiguous(), int(depth0),
                                     bool(brute)))
