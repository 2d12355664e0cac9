// Exact k-NN kernels (see gpu_knn.hpp).
//
// Every kernel gives a query (or a query's slab of rows) one wave and keeps its candidate list
// in registers: lane i holds the i-th smallest packed (d2, id) found so far, lanes >= k hold
// kPackedInf. The entry of lane k-1 is the list's threshold: a value enters the list iff it is
// strictly below it, and its distance is the traversal's pruning bound (+inf until k candidates
// are held).
#include <algorithm>
#include <cstdint>
#include <stdexcept>
#include <string>

#include "device_utils.hpp"
#include "pkdtree/gpu_knn.hpp"
#include "pkdtree/gpu_query.hpp"
#include "pkdtree/hip_check.hpp"
#include "pkdtree/trace.hpp"

namespace pkdtree {

namespace {

constexpr int kBlock = 256;
constexpr int kWaves = kBlock / 64;
constexpr int kWaveStack = 48;  // as k_nn_wave: far children of one root-to-bucket path
constexpr u32 kBucket = 512;    // sub-trees of at most this many points are scanned by the 64 lanes

// Lane `src` (wave-uniform) of a 64-bit value, as a wave-uniform value.
__device__ __forceinline__ u64 readlane_u64(u64 v, int src) {
  const u32 lo = __builtin_amdgcn_readlane(u32(v), src);
  const u32 hi = __builtin_amdgcn_readlane(u32(v >> 32), src);
  return (u64(hi) << 32) | lo;
}

__device__ __forceinline__ u64 readfirstlane_u64(u64 v) {
  const u32 lo = __builtin_amdgcn_readfirstlane(u32(v));
  const u32 hi = __builtin_amdgcn_readfirstlane(u32(v >> 32));
  return (u64(hi) << 32) | lo;
}

// Lane i takes lane i-1's value (DPP wave_shr:1); lane 0 keeps its own.
__device__ __forceinline__ u64 shift_up_one(u64 v) {
  const u32 lo = u32(__builtin_amdgcn_update_dpp(int(u32(v)), int(u32(v)), 0x138, 0xf, 0xf, false));
  const u32 hi = u32(__builtin_amdgcn_update_dpp(int(u32(v >> 32)), int(u32(v >> 32)), 0x138, 0xf, 0xf, false));
  return (u64(hi) << 32) | lo;
}

// Insert the wave-uniform candidate c, which must be strictly below the entry of lane k-1: the
// lanes whose entry is below c keep it, lane pos takes c, the lanes above take their lower
// neighbour's entry (the old entry of lane k-1 falls off), lanes >= k stay at kPackedInf.
__device__ __forceinline__ void knn_insert(u64& L, u64 c, int k) {
  const int pos = __popcll(__ballot(L < c));
  const u64 up = shift_up_one(L);
  const int ln = dev::lane();
  if (ln >= pos && ln < k) L = ln == pos ? c : up;
}

// Offer one value per lane (kPackedInf: none) to the list: the lanes below the threshold are
// inserted one by one in lane order, and after every insert the remaining ones are tested
// against the new threshold, so a value that no longer qualifies is dropped. Returns the
// threshold (entry of lane k-1) after the step.
__device__ __forceinline__ u64 knn_offer(u64& L, u64 v, int k, u64 thr) {
  u64 mask = __ballot(v < thr);
  while (mask) {
    const int src = __builtin_ctzll(mask);
    knn_insert(L, readlane_u64(v, src), k);
    thr = readlane_u64(L, k - 1);
    mask &= mask - 1;
    mask &= __ballot(v < thr);
  }
  return thr;
}

// One WAVE per query, the k-NN counterpart of k_nn_wave (query.hip): the top of the implicit
// tree is walked in lockstep, the far children wait on an LDS stack with their axis distance^2,
// sub-trees of at most kBucket points are scanned by the 64 lanes. Visiting rule: near side
// first, far side iff dax2 <= the distance of the k-th entry (checked again when popped). `<=`
// because a far-side point at exactly the k-th distance with a smaller id belongs in the answer;
// no far-side point can have d2 < dax2 (subtraction, squaring and sums of non-negative terms are
// monotone under rounding), so the rule is exact in fp32. DC: compile-time dim (0: runtime dim
// <= 32, query kept in LDS).
template <int DC>
__global__ __launch_bounds__(kBlock) void k_knn_wave(const float* __restrict__ P, const u32* __restrict__ ids, i64 n,
                                                     int dim_rt, int depth0, const float* __restrict__ queries, i64 nq,
                                                     int k, u64* __restrict__ out) {
  __shared__ u32 st_lo[kWaves][kWaveStack], st_n[kWaves][kWaveStack], st_d[kWaves][kWaveStack];
  __shared__ float st_b[kWaves][kWaveStack];
  __shared__ float qsh[kWaves][DC > 0 ? 1 : 32];
  const int w = threadIdx.x / 64, ln = dev::lane();
  const i64 qi = i64(blockIdx.x) * kWaves + w;
  if (qi >= nq || n <= 0) return;  // wave-uniform
  const int dim = DC > 0 ? DC : dim_rt;
  float qr[DC > 0 ? DC : 1];
  const float* qg = queries + qi * dim;
  if constexpr (DC > 0) {
#pragma unroll
    for (int c = 0; c < DC; ++c) qr[c] = qg[c];
  } else {
    if (ln < dim) qsh[w][ln] = qg[ln];
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_s_waitcnt(0xc07f);
  }
  auto dist = [&](const float* p) -> float {
    if constexpr (DC > 0) {
      float acc = 0.0f;
#pragma unroll
      for (int c = 0; c < DC; ++c) {
        const float t = p[c] - qr[c];
        const float sq = t * t;
        acc = acc + sq;
      }
      return acc;
    } else {
      return sq_dist(p, &qsh[w][0], dim);
    }
  };
  auto qcoord = [&](int axis) -> float {
    if constexpr (DC > 0) {
      float v = qr[0];
#pragma unroll
      for (int c = 1; c < DC; ++c) v = c == axis ? qr[c] : v;
      return v;
    } else {
      return qsh[w][axis];
    }
  };
  u64* row = out + qi * k;
  u64 L = ln < k ? row[ln] : kPackedInf;  // the incoming list (kPackedInf: a fresh search)
  u64 thr = readlane_u64(L, k - 1);
  int sp = 0;
  u32 lo = 0, cnt = u32(n);
  int depth = 0;
  for (;;) {
    while (cnt > 0) {
      if (cnt <= kBucket) {  // the whole sub-tree: 64 rows per step, the next step's rows loaded ahead
        auto rowval = [&](u32 j) -> u64 {
          const u32 r = j + u32(ln);
          if (r >= cnt) return kPackedInf;
          const u32 m = lo + r;
          return pack_dist_idx(dist(P + i64(m) * dim), ids[m]);
        };
        u64 v = rowval(0);
        for (u32 j = 0; j < cnt; j += 64) {
          const u64 nxt = rowval(j + 64);
          thr = knn_offer(L, v, k, thr);
          v = nxt;
        }
        break;
      }
      const u32 m = lo + cnt / 2;
      const float* p = P + i64(m) * dim;
      const u64 c = readfirstlane_u64(pack_dist_idx(dist(p), ids[m]));  // the median row: one candidate
      if (c < thr) {
        knn_insert(L, c, k);
        thr = readlane_u64(L, k - 1);
      }
      const float bd = packed_dist(thr);
      const int axis = (depth0 + depth) % dim;
      const float dax = qcoord(axis) - p[axis];
      const float dax2 = dax * dax;
      const u32 ln_ = cnt / 2, rn = cnt - cnt / 2 - 1;
      u32 near_lo, near_n, far_lo, far_n;
      if (dax < 0) {
        near_lo = lo; near_n = ln_; far_lo = m + 1; far_n = rn;
      } else {
        near_lo = m + 1; near_n = rn; far_lo = lo; far_n = ln_;
      }
      if (far_n > 0 && dax2 <= bd && sp < kWaveStack) {
        st_lo[w][sp] = far_lo;
        st_n[w][sp] = far_n;
        st_d[w][sp] = u32(depth + 1);
        st_b[w][sp] = dax2;
        ++sp;
      }
      lo = near_lo;
      cnt = near_n;
      ++depth;
    }
    bool found = false;
    const float bd = packed_dist(thr);
    while (sp > 0) {
      --sp;
      if (st_b[w][sp] <= bd) {
        lo = st_lo[w][sp];
        cnt = st_n[w][sp];
        depth = int(st_d[w][sp]);
        found = true;
        break;
      }
    }
    if (!found) break;
  }
  if (ln < k) row[ln] = L;
}

// Brute force, one wave per (query, slab of rows): the sorted k-list of the slab's rows goes to
// scratch[(query * slabs + slab) * k ..]. Each lane takes one row per 64-row step (sq_dist's
// sequential sum over any dim; the query's coordinates are wave-uniform loads).
__global__ __launch_bounds__(kBlock) void k_knn_brute_slab(const float* __restrict__ pts, const u32* __restrict__ ids,
                                                           u32 id_base, i64 n, int dim,
                                                           const float* __restrict__ queries, i64 nq, int k, int slabs,
                                                           i64 slab_rows, u64* __restrict__ scratch) {
  const int ln = dev::lane();
  const i64 wi = i64(blockIdx.x) * kWaves + threadIdx.x / 64;
  if (wi >= nq * slabs) return;  // wave-uniform
  const i64 qi = wi / slabs;
  const i64 r0 = (wi - qi * slabs) * slab_rows, r1 = std::min<i64>(n, r0 + slab_rows);
  const float* q = queries + qi * dim;
  u64 L = kPackedInf, thr = kPackedInf;
  for (i64 j = r0; j < r1; j += 64) {
    const i64 r = j + ln;
    u64 v = kPackedInf;
    if (r < r1) v = pack_dist_idx(sq_dist(pts + r * dim, q, dim), ids ? ids[r] : id_base + u32(r));
    thr = knn_offer(L, v, k, thr);
  }
  if (ln < k) scratch[wi * k + ln] = L;
}

// One wave per query: `lists` sorted k-lists at src[(query * lists + l) * k ..] merged into the
// sorted list already in out[query * k ..].
__global__ __launch_bounds__(kBlock) void k_knn_merge(const u64* __restrict__ src, int lists, i64 nq, int k,
                                                      const u64* first, u64* out) {
  const int ln = dev::lane();
  const i64 qi = i64(blockIdx.x) * kWaves + threadIdx.x / 64;
  if (qi >= nq) return;  // wave-uniform
  u64 L = ln < k ? first[qi * k + ln] : kPackedInf;
  u64 thr = readlane_u64(L, k - 1);
  for (int l = 0; l < lists; ++l) {
    const u64 v = ln < k ? src[(qi * lists + l) * k + ln] : kPackedInf;
    thr = knn_offer(L, v, k, thr);
  }
  if (ln < k) out[qi * k + ln] = L;
}

void check_k(int k, const char* who) {
  if (k < 1 || k > kKnnMax)
    throw std::invalid_argument(std::string(who) + ": k must be in 1.." + std::to_string(kKnnMax) + ", got " +
                                std::to_string(k));
}

constexpr i64 kMaxBlocks = 1048576;  // blocks per launch

template <int DC>
void launch_knn_wave(const float* P, const u32* ids, i64 n, int dim, int depth0, const float* q, i64 nq, int k,
                     u64* out, hipStream_t stream) {
  for (i64 q0 = 0; q0 < nq; q0 += kMaxBlocks * kWaves) {
    const i64 m = std::min<i64>(nq - q0, kMaxBlocks * kWaves);
    k_knn_wave<DC><<<int((m + kWaves - 1) / kWaves), kBlock, 0, stream>>>(P, ids, n, dim, depth0, q + q0 * dim, m, k,
                                                                          out + q0 * k);
    PKD_LAUNCH_CHECK();
  }
}

void launch_merge(const u64* src, int lists, i64 nq, int k, const u64* first, u64* out, hipStream_t stream) {
  for (i64 q0 = 0; q0 < nq; q0 += kMaxBlocks * kWaves) {
    const i64 m = std::min<i64>(nq - q0, kMaxBlocks * kWaves);
    k_knn_merge<<<int((m + kWaves - 1) / kWaves), kBlock, 0, stream>>>(src + q0 * lists * k, lists, m, k,
                                                                       first + q0 * k, out + q0 * k);
    PKD_LAUNCH_CHECK();
  }
}

}  // namespace

void knn_traverse(const float* tree_pts, const u32* tree_ids, i64 n, int dim, int depth0, const float* queries, i64 nq,
                  int k, u64* out, hipStream_t stream) {
  check_k(k, "knn_traverse");
  if (dim < 1 || dim > 32) throw std::invalid_argument("knn_traverse: dim must be in 1..32 (use knn_brute)");
  if (n >= (i64(1) << 32)) throw std::invalid_argument("knn_traverse: n must be below 2^32");
  if (nq <= 0 || n <= 0) return;
  TraceRange tr("pkd.knn_traverse");
  switch (dim) {
    case 1: launch_knn_wave<1>(tree_pts, tree_ids, n, dim, depth0, queries, nq, k, out, stream); return;
    case 2: launch_knn_wave<2>(tree_pts, tree_ids, n, dim, depth0, queries, nq, k, out, stream); return;
    case 3: launch_knn_wave<3>(tree_pts, tree_ids, n, dim, depth0, queries, nq, k, out, stream); return;
    case 4: launch_knn_wave<4>(tree_pts, tree_ids, n, dim, depth0, queries, nq, k, out, stream); return;
    case 5: launch_knn_wave<5>(tree_pts, tree_ids, n, dim, depth0, queries, nq, k, out, stream); return;
    case 6: launch_knn_wave<6>(tree_pts, tree_ids, n, dim, depth0, queries, nq, k, out, stream); return;
    case 7: launch_knn_wave<7>(tree_pts, tree_ids, n, dim, depth0, queries, nq, k, out, stream); return;
    case 8: launch_knn_wave<8>(tree_pts, tree_ids, n, dim, depth0, queries, nq, k, out, stream); return;
    default: launch_knn_wave<0>(tree_pts, tree_ids, n, dim, depth0, queries, nq, k, out, stream); return;
  }
}

int knn_brute_slabs(i64 n, i64 nq) {
  if (n <= 0 || nq <= 0) return 1;
  // nq * slabs waves fill the chip (256 CUs x 32 waves); a slab is at least 256 rows
  const i64 want = (8192 + nq - 1) / nq;
  return int(std::max<i64>(1, std::min<i64>(std::min<i64>(want, 1024), n / 256)));
}

void knn_brute(const float* pts, const u32* ids, u32 id_base, i64 n, int dim, const float* queries, i64 nq, int k,
               u64* out, hipStream_t stream, u64* scratch) {
  check_k(k, "knn_brute");
  if (dim < 1) throw std::invalid_argument("knn_brute: dim must be positive");
  if (n >= (i64(1) << 32)) throw std::invalid_argument("knn_brute: n must be below 2^32");
  if (nq <= 0 || n <= 0) return;
  TraceRange tr("pkd.knn_brute");
  const int slabs = knn_brute_slabs(n, nq);
  const i64 slab_rows = ((n + slabs - 1) / slabs + 63) / 64 * 64;
  u64* own = nullptr;
  if (!scratch) {
    PKD_HIP_CHECK(hipMallocAsync(reinterpret_cast<void**>(&own), knn_brute_scratch_words(n, nq, k) * 8, stream));
    scratch = own;
  }
  const i64 per = std::max<i64>(1, kMaxBlocks * kWaves / slabs);  // queries per launch
  for (i64 q0 = 0; q0 < nq; q0 += per) {
    const i64 m = std::min<i64>(nq - q0, per);
    k_knn_brute_slab<<<int((m * slabs + kWaves - 1) / kWaves), kBlock, 0, stream>>>(
        pts, ids, id_base, n, dim, queries + q0 * dim, m, k, slabs, slab_rows, scratch + q0 * slabs * k);
    PKD_LAUNCH_CHECK();
  }
  launch_merge(scratch, slabs, nq, k, out, out, stream);
  if (own) PKD_HIP_CHECK(hipFreeAsync(own, stream));
}

void knn_merge(const u64* a, const u64* b, i64 nq, int k, u64* out, hipStream_t stream) {
  check_k(k, "knn_merge");
  if (nq <= 0) return;
  launch_merge(b, 1, nq, k, a, out, stream);
}

}  // namespace pkdtree
