// Exact k-nearest-neighbour queries on the GPU (the 1-NN kernels are in gpu_query.hpp).
//
// For a query q the answer is the k smallest packed values pack_dist_idx(sq_dist(p, q), id(p))
// over the points p, in ascending order: a row of k u64 whose unsigned order is the
// lexicographic (distance, id) order, so ties on distance go to the smaller id and column 0 is
// the 1-NN answer. Rows with fewer than k points end in kPackedInf. Ids must be distinct. The
// order is total and every path computes distances with sq_dist's sequential no-FMA sum, so
// traversal, brute force and the CPU oracle (knn_brute_cpu) agree bit for bit.
//
// `out` is [nq, k] and is BOTH input and output: every row must hold a sorted list on entry
// (kPackedInf everywhere for a fresh search: nn_init(out, nq * k)), and the search merges its
// points into it. Chaining searches over trees of DISJOINT point sets into one `out` gives the
// answer over their union (forests); searching the same points twice duplicates their entries.
//
// 1 <= k <= kKnnMax; anything else throws std::invalid_argument.
#pragma once
#include <hip/hip_runtime.h>

#include "pkdtree/common.hpp"

namespace pkdtree {

constexpr int kKnnMax = 64;  // one list entry per lane of a wave

// tree_pts/tree_ids: in-order implicit tree of n points whose root is at depth `depth0`
// (exact mode: the search relies on the kd invariant). One wave per query; dim <= 32.
void knn_traverse(const float* tree_pts, const u32* tree_ids, i64 n, int dim, int depth0, const float* queries, i64 nq,
                  int k, u64* out, hipStream_t stream);

// Slabs the brute force splits n rows into for nq queries, and the u64 words of its scratch.
int knn_brute_slabs(i64 n, i64 nq);
inline size_t knn_brute_scratch_words(i64 n, i64 nq, int k) {
  return size_t(nq) * size_t(knn_brute_slabs(n, nq)) * size_t(k);
}

// pts [n, dim] AoS, any layout and any dim; ids [n] or nullptr (id = id_base + row). One wave
// per (query, slab of rows) writes its sorted k-list to scratch [nq, slabs, k]; a second kernel
// merges the slab lists into out. scratch: knn_brute_scratch_words() u64 ordered on `stream`,
// or nullptr for a stream-ordered allocation of this call's own.
void knn_brute(const float* pts, const u32* ids, u32 id_base, i64 n, int dim, const float* queries, i64 nq, int k,
               u64* out, hipStream_t stream, u64* scratch = nullptr);

// out[q] = the k smallest of a[q] and b[q] (sorted [nq, k] lists of disjoint point sets).
// out may be a.
void knn_merge(const u64* a, const u64* b, i64 nq, int k, u64* out, hipStream_t stream);

}  // namespace pkdtree
