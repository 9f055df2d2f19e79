// Merges of per-shard top-k lists, the last step of a sharded search (DESIGN.md §3 "Multi-GPU:
// global-threshold protocol").  Packed lists [nparts][nq][k + 1] u64 (select.hip's out_packed) go through
// drt_topk_merge_packed*, which picks merge_packed_count_kernel (2..8 parts that fit 128 KiB of LDS),
// merge_packed_tree_kernel (more parts, still in LDS) or merge_packed_kernel (one part, or anything larger) and
// certifies the merged list; plain (scores, ids) lists go through drt_topk_merge.  No other unit calls into
// this one.  (The merge by exact order keys, drt_merge_exact, is refine.hip's.)
#include "profile.h"
#include "search_internal.h"

namespace drt {

// Tree merge of packed per-shard lists by bitonic networks: all P2 =
// pow2ceil(nparts) lists, padded to KP = pow2ceil(k) keys, sit in LDS.  Each
// round merges list pairs (A, B): the half-cleaner min(A[i], B[KP-1-i]) keeps
// exactly the KP smallest keys of A u B as a bitonic sequence, which a bitonic
// merge (strides KP/2 .. 1) sorts.  Keys are held in registers; strides < 64
// are cross-lane shuffles, strides >= NT are in-thread, the rest go through
// the pair's own LDS slot (consecutive addresses, conflict-free) -- unlike a
// binary-search merge, whose scattered 64-bit LDS reads serialise on banks.
constexpr int kTreeThreads = 512;
constexpr int kTreeMaxE = 16;   // keys per thread in round 0: P2 / 2 * KP <= 16 * 512

template <int US>
__device__ __forceinline__ void tree_inthread(uint64_t (&v)[kTreeMaxE]) {
#pragma unroll
  for (int t = 0; t < kTreeMaxE; ++t) {
    if ((t & US) == 0) {
      const uint64_t a = v[t], b = v[t | US];
      v[t] = a < b ? a : b;
      v[t | US] = a < b ? b : a;
    }
  }
}

template <int KP>
__global__ __launch_bounds__(kTreeThreads) void merge_packed_tree_kernel(const uint64_t* parts, int64_t nq,
                                                                         int nparts, int p2, int k,
                                                                         int64_t n_global, float* out_s,
                                                                         int64_t* out_i, int32_t* status,
                                                                         int kcert) {
  extern __shared__ __attribute__((aligned(16))) uint64_t L[];  // [p2][KP]
  constexpr int NT = kTreeThreads;
  __shared__ int bad;
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int64_t q = blockIdx.x;
  const int64_t ps = (int64_t)(k + 1);
  if (tid == 0) bad = 0;
  __syncthreads();
  {
    uint64_t tmp[2 * kTreeMaxE];
#pragma unroll
    for (int t = 0; t < 2 * kTreeMaxE; ++t) {
      const int e = tid + t * NT;
      const int l = e / KP, i = e & (KP - 1);
      const bool ok = e < p2 * KP && l < nparts && i < k;
      // unconditional load from a clamped address, then select: a guarded load
      // makes hipcc branch around it and drain vmcnt(0) per element
      const uint64_t x = parts[((int64_t)(ok ? l : 0) * nq + q) * ps + (ok ? i : 0)];
      tmp[t] = ok ? x : ~0ull;
    }
#pragma unroll
    for (int t = 0; t < 2 * kTreeMaxE; ++t) {
      const int e = tid + t * NT;
      if (e < p2 * KP) L[e] = tmp[t];
    }
  }
  if (tid < nparts && (parts[((int64_t)tid * nq + q) * ps + k] & 1ull)) bad = 1;
  __syncthreads();
  for (int half = 1; half < p2; half <<= 1) {
    const int npairs = p2 / (2 * half);
    const int total = npairs * KP;             // keys this round (outputs)
    uint64_t v[kTreeMaxE];
    // half-cleaner: pair g, index i -> min(A[i], B[KP - 1 - i])
#pragma unroll
    for (int t = 0; t < kTreeMaxE; ++t) {
      const int e = tid + t * NT;
      const int g = e / KP, i = e & (KP - 1);
      v[t] = ~0ull;
      if (e < total) {
        const uint64_t a = L[(2 * g) * half * KP + i];
        const uint64_t b = L[(2 * g + 1) * half * KP + (KP - 1 - i)];
        v[t] = a < b ? a : b;
      }
    }
    __syncthreads();
    // bitonic merge of each pair's KP keys (ascending).  Stage loop kept rolled:
    // a fully unrolled network is tens of KB of straight-line code that every
    // (single-pass) wave fetches cold, which costs more than the loop overhead.
#pragma unroll 1
    for (int stride = KP / 2; stride > 0; stride >>= 1) {
      if (stride >= NT) {
        switch (stride / NT) {
          case 1: tree_inthread<1>(v); break;
          case 2: tree_inthread<2>(v); break;
          default: tree_inthread<4>(v); break;
        }
      } else if (stride >= 64) {
#pragma unroll
        for (int t = 0; t < kTreeMaxE; ++t) {
          const int e = tid + t * NT;
          if (e < total) L[(2 * (e / KP)) * half * KP + (e & (KP - 1))] = v[t];
        }
        __syncthreads();
#pragma unroll
        for (int t = 0; t < kTreeMaxE; ++t) {
          const int e = tid + t * NT;
          if (e < total) {
            const int pe = e ^ stride;
            const uint64_t b = L[(2 * (pe / KP)) * half * KP + (pe & (KP - 1))];
            const bool lower = (e & stride) == 0;
            v[t] = lower ? (v[t] < b ? v[t] : b) : (v[t] < b ? b : v[t]);
          }
        }
        __syncthreads();
      } else {
#pragma unroll
        for (int t = 0; t < kTreeMaxE; ++t) {
          if ((tid & ~63) + t * NT < total) {   // wave-uniform: total is a multiple of 64
            const uint64_t b = __shfl_xor(v[t], stride, 64);
            const bool lower = (lane & stride) == 0;
            v[t] = lower ? (v[t] < b ? v[t] : b) : (v[t] < b ? b : v[t]);
          }
        }
      }
    }
    // sorted pair result -> slot 2g * half
#pragma unroll
    for (int t = 0; t < kTreeMaxE; ++t) {
      const int e = tid + t * NT;
      if (e < total) L[(2 * (e / KP)) * half * KP + (e & (KP - 1))] = v[t];
    }
    __syncthreads();
  }
  for (int i = tid; i < k; i += NT) {
    const uint64_t x = L[i];
    if (x == ~0ull) {
      out_s[q * k + i] = kPadScore;
      out_i[q * k + i] = -1;
    } else {
      out_s[q * k + i] = desc_key_to_score((uint32_t)(x >> 32));
      out_i[q * k + i] = (int64_t)(x & 0xFFFFFFFFull);
    }
  }
  if (status && tid == 0) status[q] = (bad || (L[kcert - 1] == ~0ull && n_global >= (int64_t)kcert)) ? 1 : 0;
}

// Count merge (round 2, the default where 2 <= nparts <= 8 and nparts * k <= 8192): entry k of
// every packed list carries its valid count in bits 32-63, so ONE work-group per query loads only
// the valid keys of all parts (in the global-threshold regime ~1.3 k / world per part, not k) into
// LDS, then places every key at rank = its index in its part + its lower bounds in the other
// parts (branch-free searches advancing in lock step, so their LDS reads overlap).  The round-2
// rank merge (one work-group per (query, part), all nparts * k keys loaded by each) measured
// 13.4 vs 21.7 us at 128 queries and 57 vs 278 us at 2048 (profiles/r02f_merge_bench.log).
// The count word is checked against the data: the key before it must be real and the key at it
// a pad (~0); a list whose count disagrees (e.g. written by a producer that leaves entry k = flags
// only) is measured instead by a binary search for its first pad key (lists are sorted ascending).
__device__ __forceinline__ int packed_valid_count(const uint64_t* L, int k) {
  const uint64_t w = L[k];
  int c = (int)(w >> 32);
  c = c < k ? c : k;
  const bool ok_lo = c == 0 || L[c - 1] != ~0ull;
  const bool ok_hi = c == k || L[c] == ~0ull;
  if (ok_lo && ok_hi) return c;
  int lo = 0, hi = k;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (L[mid] != ~0ull) lo = mid + 1;
    else hi = mid;
  }
  return lo;
}
constexpr int kCntThreads = 1024;
constexpr int kCntMaxParts = 8;
constexpr int kCntMaxKeys = 16384;   // 128 KiB of LDS
// lcap: entries per list (list stride lcap + 1); k: merged outputs.  lcap < k (capped exchange lists,
// round 6): a list that was truncated (flag bit 1: its shard had more hits than it carries) certifies only
// if its last entry ranks at or below the k-th merged place -- every entry it did not carry is worse.
__global__ __launch_bounds__(kCntThreads) void merge_packed_count_kernel(const uint64_t* parts, int64_t nq,
                                                                         int nparts, int k, int64_t n_global,
                                                                         float* out_s, int64_t* out_i,
                                                                         int32_t* status, int kcert, int lcap) {
  extern __shared__ __attribute__((aligned(16))) uint64_t P[];   // valid prefixes of all parts, concatenated
  __shared__ int cnt[kCntMaxParts], off[kCntMaxParts + 1], flg[kCntMaxParts], trn[kCntMaxParts];
  __shared__ int trunc_bad;
  const int tid = threadIdx.x;
  const int64_t q = blockIdx.x;
  const int64_t ps = (int64_t)(lcap + 1);
  if (tid == 0) trunc_bad = 0;
  if (tid < kCntMaxParts) {
    int c = 0, f = 0, t = 0;
    if (tid < nparts) {
      const uint64_t* L = parts + ((int64_t)tid * nq + q) * ps;
      c = packed_valid_count(L, lcap);
      f = (int)(L[lcap] & 1ull);
      t = lcap < k && (L[lcap] & 2ull) != 0 && c == lcap;
    }
    cnt[tid] = c;
    flg[tid] = f;
    trn[tid] = t;
  }
  __syncthreads();
  if (tid == 0) {
    int o = 0;
    for (int l = 0; l < kCntMaxParts; ++l) {
      off[l] = o;
      o += cnt[l];
    }
    off[kCntMaxParts] = o;
  }
  __syncthreads();
  const int tot = off[kCntMaxParts];
  int maxc = 0;
#pragma unroll
  for (int l = 0; l < kCntMaxParts; ++l) maxc = cnt[l] > maxc ? cnt[l] : maxc;
  const int nsteps = 32 - __builtin_clz((unsigned)maxc | 1u);   // halvings until every len <= 1
  int offs[kCntMaxParts + 1];
#pragma unroll
  for (int l = 0; l <= kCntMaxParts; ++l) offs[l] = off[l];
  auto part_of = [&](int e) {
    int l = 0;
#pragma unroll
    for (int j = 1; j < kCntMaxParts; ++j) l += (e >= offs[j]) ? 1 : 0;
    return l;
  };
  for (int e = tid; e < tot; e += kCntThreads) {
    const int l = part_of(e);
    P[e] = parts[((int64_t)l * nq + q) * ps + (e - offs[l])];
  }
  __syncthreads();
  for (int e = tid; e < tot; e += kCntThreads) {
    const int me = part_of(e);
    const uint64_t x = P[e];
    int base[kCntMaxParts], len[kCntMaxParts];
#pragma unroll
    for (int l = 0; l < kCntMaxParts; ++l) {
      base[l] = offs[l];
      len[l] = (l == me) ? 0 : offs[l + 1] - offs[l];
    }
    // the keys confirmed below x so far bound its rank from below: once that bound reaches k the
    // key is never output, and its searches stop (with the sample's ~4k hits per query over W
    // parts, ~2/3 of the keys of a W = 8 merge; round 4)
    bool out_of_k = false;
    for (int step = 0; step < nsteps; ++step) {
      int lb = e - offs[me];
#pragma unroll
      for (int l = 0; l < kCntMaxParts; ++l) {
        if (len[l] > 1) {
          const int half = len[l] >> 1;
          base[l] = P[base[l] + half - 1] < x ? base[l] + half : base[l];
          len[l] -= half;
        }
        lb += base[l] - offs[l];
      }
      if (lb >= k) {
        out_of_k = true;
        break;
      }
    }
    if (out_of_k) continue;
    int rank = e - offs[me];
#pragma unroll
    for (int l = 0; l < kCntMaxParts; ++l)
      rank += (base[l] - offs[l]) + ((len[l] == 1 && P[base[l]] < x) ? 1 : 0);
    // a truncated list's last carried entry above the k-th merged place: entries it did not carry may
    // belong to the top k -- not certified (the batch is redone exactly)
    if (trn[me] && e == offs[me + 1] - 1 && rank < k - 1) trunc_bad = 1;
    if (rank < k) {
      out_s[q * k + rank] = desc_key_to_score((uint32_t)(x >> 32));
      out_i[q * k + rank] = (int64_t)(x & 0xFFFFFFFFull);
    }
  }
  for (int i = (tot < k ? tot : k) + tid; i < k; i += kCntThreads) {
    out_s[q * k + i] = kPadScore;
    out_i[q * k + i] = -1;
  }
  __syncthreads();
  if (status && tid == 0) {
    int bad = trunc_bad;
    for (int l = 0; l < kCntMaxParts; ++l) bad |= flg[l];
    status[q] = (bad || (tot < kcert && n_global >= (int64_t)kcert)) ? 1 : 0;
  }
}

// Merge of packed per-shard lists [nparts][nq][k + 1] (sorted u64 keys, entry k =
// flags) into (score, id) [nq][k]; status[q] = 1 unless exact: the k-th merged
// entry is real (>= k candidates over all shards, so the global tau was <= the
// k-th score) and no shard overflowed.
__global__ __launch_bounds__(512) void merge_packed_kernel(const uint64_t* parts, int64_t nq, int nparts, int k,
                                                           int64_t n_global, float* out_s, int64_t* out_i,
                                                           int32_t* status, int kcert) {
  __shared__ uint64_t A[kSelMaxK], B[kSelMaxK], Cb[kSelMaxK];
  __shared__ int bad;
  const int tid = threadIdx.x;
  const int64_t q = blockIdx.x;
  const int64_t ps = (int64_t)(k + 1);
  if (tid == 0) bad = 0;
  for (int i = tid; i < k; i += 512) A[i] = parts[q * ps + i];
  __syncthreads();
  if (tid == 0 && (parts[q * ps + k] & 1ull)) bad = 1;
  for (int p = 1; p < nparts; ++p) {
    const uint64_t* src = parts + ((int64_t)p * nq + q) * ps;
    for (int i = tid; i < k; i += 512) B[i] = src[i];
    if (tid == 0 && (src[k] & 1ull)) bad = 1;
    __syncthreads();
    for (int i = tid; i < k; i += 512) {
      int lo = 0, hi = k;   // #B < A[i]
      while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (B[mid] < A[i]) lo = mid + 1;
        else hi = mid;
      }
      if (i + lo < k) Cb[i + lo] = A[i];
      int lo2 = 0, hi2 = k;  // #A <= B[i]
      while (lo2 < hi2) {
        const int mid = (lo2 + hi2) >> 1;
        if (A[mid] <= B[i]) lo2 = mid + 1;
        else hi2 = mid;
      }
      if (i + lo2 < k) Cb[i + lo2] = B[i];
    }
    __syncthreads();
    for (int i = tid; i < k; i += 512) A[i] = Cb[i];
    __syncthreads();
  }
  for (int i = tid; i < k; i += 512) {
    const uint64_t x = A[i];
    if (x == ~0ull) {
      out_s[q * k + i] = kPadScore;
      out_i[q * k + i] = -1;
    } else {
      out_s[q * k + i] = desc_key_to_score((uint32_t)(x >> 32));
      out_i[q * k + i] = (int64_t)(x & 0xFFFFFFFFull);
    }
  }
  if (status && tid == 0) status[q] = (bad || (A[kcert - 1] == ~0ull && n_global >= (int64_t)kcert)) ? 1 : 0;
}

// ---------------------------------------------------------------------------
// Merge of per-shard sorted top-k lists (RCCL all-gather output).
// Pairwise merge by rank: element i of A lands at i + #{B < A[i]},
// element j of B at j + #{A <= B[j]} (total order: score desc, id asc).
// ---------------------------------------------------------------------------
struct MergeEnt {
  uint32_t key;  // desc_key(score)
  int64_t id;
};

__device__ __forceinline__ bool ent_less(uint32_t ka, int64_t ia, uint32_t kb, int64_t ib) {
  return ka < kb || (ka == kb && ia < ib);
}

constexpr int kMergeThreads = 512;

__global__ __launch_bounds__(kMergeThreads) void merge_kernel(const float* scores, const int64_t* ids,
                                                              int64_t nq, int nparts, int k_in,
                                                              int k_out, float* out_s, int64_t* out_i) {
  __shared__ uint32_t ka[kSelMaxK], kb[kSelMaxK], kc[kSelMaxK];
  __shared__ int64_t ia[kSelMaxK], ib[kSelMaxK], ic[kSelMaxK];
  const int tid = threadIdx.x;
  const int64_t q = blockIdx.x;
  // running list A holds up to min(k_out, seen) entries
  int na = k_in < k_out ? k_in : k_out;
  for (int i = tid; i < na; i += kMergeThreads) {
    const int64_t o = (0 * nq + q) * k_in + i;
    ka[i] = desc_key(scores[o]);
    ia[i] = ids[o];
  }
  __syncthreads();
  for (int p = 1; p < nparts; ++p) {
    const int nb = k_in < k_out ? k_in : k_out;
    {
      float sv[kSelMaxK / kMergeThreads];
      int64_t iv[kSelMaxK / kMergeThreads];
#pragma unroll
      for (int u = 0; u < kSelMaxK / kMergeThreads; ++u) {   // clamped loads, issued back to back
        const int i = tid + u * kMergeThreads;
        const int64_t o = ((int64_t)p * nq + q) * k_in + (i < nb ? i : 0);
        sv[u] = scores[o];
        iv[u] = ids[o];
      }
#pragma unroll
      for (int u = 0; u < kSelMaxK / kMergeThreads; ++u) {
        const int i = tid + u * kMergeThreads;
        if (i < nb) {
          kb[i] = desc_key(sv[u]);
          ib[i] = iv[u];
        }
      }
    }
    __syncthreads();
    const int nc = (na + nb) < k_out ? (na + nb) : k_out;
    for (int i = tid; i < na; i += kMergeThreads) {
      // #B strictly less than A[i]
      int lo = 0, hi = nb;
      while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (ent_less(kb[mid], ib[mid], ka[i], ia[i])) lo = mid + 1;
        else hi = mid;
      }
      const int rk = i + lo;
      if (rk < nc) {
        kc[rk] = ka[i];
        ic[rk] = ia[i];
      }
    }
    for (int j = tid; j < nb; j += kMergeThreads) {
      // #A less than or equal to B[j]
      int lo = 0, hi = na;
      while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (!ent_less(kb[j], ib[j], ka[mid], ia[mid])) lo = mid + 1;
        else hi = mid;
      }
      const int rk = j + lo;
      if (rk < nc) {
        kc[rk] = kb[j];
        ic[rk] = ib[j];
      }
    }
    __syncthreads();
    for (int i = tid; i < nc; i += kMergeThreads) {
      ka[i] = kc[i];
      ia[i] = ic[i];
    }
    na = nc;
    __syncthreads();
  }
  for (int i = tid; i < k_out; i += kMergeThreads) {
    const int64_t o = q * k_out + i;
    if (i < na) {
      out_s[o] = desc_key_to_score(ka[i]);
      out_i[o] = ia[i];
    } else {
      out_s[o] = kPadScore;
      out_i[o] = -1;
    }
  }
}

}  // namespace drt

using namespace drt;

extern "C" {

int drt_topk_merge(const float* scores, const int64_t* ids, int64_t nq, int32_t nparts, int32_t k_in,
                   int32_t k_out, float* out_scores, int64_t* out_ids, void* stream) {
  DRT_REQUIRE(nq >= 0 && nparts >= 1 && nparts <= 64 && k_in >= 1 && k_in <= kSelMaxK && k_out >= 1 &&
              k_out <= kSelMaxK && (int64_t)k_out <= (int64_t)k_in * nparts);
  if (nq == 0) return DRT_OK;
  DRT_REQUIRE(scores && ids && out_scores && out_ids);
  const ProfPair pp = prof_begin(PROF_MERGE, (hipStream_t)stream);
  hipLaunchKernelGGL(merge_kernel, dim3((unsigned)nq), dim3(kMergeThreads), 0, (hipStream_t)stream, scores,
                     ids, nq, (int)nparts, (int)k_in, (int)k_out, out_scores, out_ids);
  prof_end(pp, (hipStream_t)stream);
  return hip_status(hipGetLastError());
}

// merge_packed_count_kernel's dynamic LDS goes up to kCntMaxKeys keys: raised once, before its first launch.
static hipError_t merge_count_lds_attr() {
  static bool attr_set = false;
  if (attr_set) return hipSuccess;
  const hipError_t e = hipFuncSetAttribute((const void*)merge_packed_count_kernel,
                                           hipFuncAttributeMaxDynamicSharedMemorySize, kCntMaxKeys * 8);
  attr_set = e == hipSuccess;
  return e;
}

int drt_topk_merge_packed(const uint64_t* parts, int64_t nq, int32_t nparts, int32_t k, int64_t n_global,
                          float* out_scores, int64_t* out_ids, int32_t* status, void* stream) {
  return drt_topk_merge_packed_cert(parts, nq, nparts, k, k, n_global, out_scores, out_ids, status, stream);
}

// Capped exchange lists (round 6): parts [nparts][nq][lcap + 1] with lcap <= k entries each (a shard's top
// lcap hits, flag bit 1 = it had more), merged into the top k; a truncated list whose last carried entry
// ranks above the k-th merged place leaves its query uncertified.  The count merge only (2..8 parts).
int drt_topk_merge_packed_capped(const uint64_t* parts, int64_t nq, int32_t nparts, int32_t lcap, int32_t k,
                                 int32_t k_cert, int64_t n_global, float* out_scores, int64_t* out_ids,
                                 int32_t* status, void* stream) {
  DRT_REQUIRE(nq >= 0 && nparts >= 2 && nparts <= kCntMaxParts && k >= 1 && k <= kSelMaxK && lcap >= 1 &&
              lcap <= k && (int64_t)nparts * lcap <= kCntMaxKeys && n_global >= 0 && k_cert >= 1 && k_cert <= k);
  if (nq == 0) return DRT_OK;
  DRT_REQUIRE(parts && out_scores && out_ids);
  hipStream_t s = (hipStream_t)stream;
  DRT_CHECK_HIP(merge_count_lds_attr());
  const ProfPair pp = prof_begin(PROF_MERGE, s);
  hipLaunchKernelGGL(merge_packed_count_kernel, dim3((unsigned)nq), dim3(kCntThreads), (size_t)nparts * lcap * 8, s,
                     parts, nq, (int)nparts, (int)k, n_global, out_scores, out_ids, status, (int)k_cert, (int)lcap);
  prof_end(pp, s);
  return hip_status(hipGetLastError());
}

int drt_topk_merge_packed_cert(const uint64_t* parts, int64_t nq, int32_t nparts, int32_t k, int32_t k_cert,
                               int64_t n_global, float* out_scores, int64_t* out_ids, int32_t* status,
                               void* stream) {
  DRT_REQUIRE(nq >= 0 && nparts >= 1 && nparts <= 4096 && k >= 1 && k <= kSelMaxK && n_global >= 0 &&
              k_cert >= 1 && k_cert <= k);
  if (nq == 0) return DRT_OK;
  DRT_REQUIRE(parts && out_scores && out_ids);
  hipStream_t s = (hipStream_t)stream;
  const ProfPair pp = prof_begin(PROF_MERGE, s);
  int p2 = 1;
  while (p2 < nparts) p2 <<= 1;
  int kp = 64;
  while (kp < k) kp <<= 1;
  const size_t lds = (size_t)p2 * kp * 8;
  int rc = DRT_OK;
  const size_t cnt_lds = (size_t)nparts * k * 8;
  const bool count_ok = nparts <= kCntMaxParts && (int64_t)nparts * k <= kCntMaxKeys;
  // one part (one GPU): the plain per-query kernel (tools/merge_bench.py: 8 vs 23 us at 2048 queries)
  if (count_ok && nparts > 1) {
    DRT_CHECK_HIP(merge_count_lds_attr());
    hipLaunchKernelGGL(merge_packed_count_kernel, dim3((unsigned)nq), dim3(kCntThreads), cnt_lds, s, parts, nq,
                       (int)nparts, (int)k, n_global, out_scores, out_ids, status, (int)k_cert, (int)k);
  } else if (nparts > 1 && (p2 / 2) * kp <= kTreeMaxE * kTreeThreads && lds <= 128 * 1024) {
#define DRT_TREE(KPV)                                                                                        \
  {                                                                                                          \
    static bool attr_set = false;                                                                            \
    if (!attr_set) {                                                                                         \
      DRT_CHECK_HIP(hipFuncSetAttribute((const void*)merge_packed_tree_kernel<KPV>,                          \
                                        hipFuncAttributeMaxDynamicSharedMemorySize, 128 * 1024));            \
      attr_set = true;                                                                                       \
    }                                                                                                        \
    hipLaunchKernelGGL(merge_packed_tree_kernel<KPV>, dim3((unsigned)nq), dim3(kTreeThreads), lds, s, parts,   \
                       nq, (int)nparts, p2, (int)k, n_global, out_scores, out_ids, status, (int)k_cert);     \
  }
    switch (kp) {
      case 64: DRT_TREE(64) break;
      case 128: DRT_TREE(128) break;
      case 256: DRT_TREE(256) break;
      case 512: DRT_TREE(512) break;
      case 1024: DRT_TREE(1024) break;
      default: DRT_TREE(2048) break;
    }
#undef DRT_TREE
  } else {
    hipLaunchKernelGGL(merge_packed_kernel, dim3((unsigned)nq), dim3(512), 0, s, parts, nq, (int)nparts, (int)k,
                       n_global, out_scores, out_ids, status, (int)k_cert);
  }
  prof_end(pp, s);
  rc = hip_status(hipGetLastError());
  return rc;
}

}  // extern "C"
