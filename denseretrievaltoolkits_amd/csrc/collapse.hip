// Grouped (document-level, MaxP) search on top of the exact row search (DESIGN.md "Grouped search"): the one
// kernel the index needs beyond its top-k to answer "the best k groups, each scored by its best row".
//
//   topk_collapse_kernel  a stable compaction of each query's canonical top-K row list that keeps, of every
//                         group (groups[row id]), only its FIRST entry -- the group's best row, since the list is
//                         in (exact score desc, row id asc) order -- and drops pads and ids outside the map.
//
// Exactness: a group's best row precedes all its other rows and groups are ordered by their best rows, so the
// first-occurrence groups of the top-K list, in list order, are the first groups of the grouped result (the
// prefix property); K = min(k * P_max, ntotal), P_max the largest group's row count, always shows k groups or
// every group there is.  Nothing here ranks: keeping the order is the whole job.
//
// First occurrences are found with an open-addressing table of 64-bit slots (group << 32) | position, capacity
// the power of two >= 2 k_in: every entry claims its group's slot (compare-and-swap on an empty one) or lowers
// the position the slot holds (atomic min: a slot's group never changes once set), so after the pass a slot
// holds its group's smallest position whatever order the entries arrived in.  The list is then walked in rank
// order and an entry is kept iff its group's slot holds its own position.  The table lives in LDS up to
// k_in = kCollapseLdsK and in the workspace (one region per work-group, L2-resident) beyond; a fixed number of
// work-groups loop over the queries, so the workspace does not grow with nq.
#include "drt_common.h"

namespace drt {

constexpr int kCollThreads = 256;
constexpr int kCollWaves = kCollThreads / 64;
constexpr int kCollMaxKIn = 32768;               // the large-k path's limit (MAX_K_LARGE)
constexpr int kCollapseLdsK = 2048;              // longest list whose table stays in LDS (kernels.COLLAPSE_LDS_K)
constexpr int kCollLdsSlots = 2 * kCollapseLdsK; // 4096 slots = 32 KiB
constexpr int kCollLdsGroups = 1024;             // work-groups of the LDS form (4 per CU; no workspace)
constexpr int kCollRegions = 128;                // work-groups = table regions of the workspace form
constexpr size_t kCollMinWorkspace = 256;        // the LDS form uses none: a token size keeps "> 0 = supported"
constexpr unsigned long long kCollEmpty = ~0ull; // no packed word equals it: groups are < 2^31

// slots of a k_in-entry list's table: the power of two >= 2 k_in (load factor <= 1/2), as its log2
__host__ __device__ __forceinline__ int coll_log2_slots(int k_in) {
  int lg = 1;
  while ((1 << lg) < 2 * k_in) ++lg;
  return lg;
}

// Table accesses.  LDS: plain loads and stores between barriers, ds atomics.  Workspace: agent-scope atomics
// throughout -- the atomics execute in L2, so a plain load could be served a line the CU's L1 kept from the
// region's previous query.
template <bool kLds>
__device__ __forceinline__ unsigned long long slot_load(unsigned long long* p) {
  if constexpr (kLds) return *p;
  else return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
template <bool kLds>
__device__ __forceinline__ void slot_store(unsigned long long* p, unsigned long long v) {
  if constexpr (kLds) *p = v;
  else __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
// the slot's value before the exchange (== expected iff it succeeded)
template <bool kLds>
__device__ __forceinline__ unsigned long long slot_cas(unsigned long long* p, unsigned long long expected,
                                                       unsigned long long v) {
  __hip_atomic_compare_exchange_strong(p, &expected, v, __ATOMIC_RELAXED, __ATOMIC_RELAXED,
                                       kLds ? __HIP_MEMORY_SCOPE_WORKGROUP : __HIP_MEMORY_SCOPE_AGENT);
  return expected;
}
template <bool kLds>
__device__ __forceinline__ void slot_min(unsigned long long* p, unsigned long long v) {
  __hip_atomic_fetch_min(p, v, __ATOMIC_RELAXED, kLds ? __HIP_MEMORY_SCOPE_WORKGROUP : __HIP_MEMORY_SCOPE_AGENT);
}

// multiplicative (Fibonacci) hash of a group id to a slot of a 2^lg-slot table, 1 <= lg <= 16
__device__ __forceinline__ uint32_t coll_hash(uint32_t g, int lg) { return (g * 2654435769u) >> (32 - lg); }

// a fixed grid; work-group b takes queries b, b + gridDim.x, ... and owns table region b
template <bool kLds>
__global__ __launch_bounds__(kCollThreads) void topk_collapse_kernel(
    const float* __restrict__ scores, const int64_t* __restrict__ ids, int64_t nq, int k_in,
    const int32_t* __restrict__ groups, int64_t n_rows, int k_out, float* __restrict__ out_scores,
    int32_t* __restrict__ out_groups, int64_t* __restrict__ out_ids, int32_t* __restrict__ out_count,
    unsigned long long* __restrict__ ws) {
  __shared__ unsigned long long lds_tab[kLds ? kCollLdsSlots : 1];
  __shared__ int wcnt[2][kCollWaves];   // per-wave kept counts, double-buffered over the steps
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int lg = coll_log2_slots(k_in);
  const uint32_t nslots = 1u << lg, mask = nslots - 1u;
  unsigned long long* tab = kLds ? lds_tab : ws + (size_t)blockIdx.x * nslots;

  int buf = 0;
  for (int64_t q = blockIdx.x; q < nq; q += gridDim.x) {
    const float* s_in = scores + q * (int64_t)k_in;
    const int64_t* i_in = ids + q * (int64_t)k_in;
    float* s_out = out_scores + q * (int64_t)k_out;
    int32_t* g_out = out_groups + q * (int64_t)k_out;
    int64_t* i_out = out_ids + q * (int64_t)k_out;

    // (the previous query's last table read lies before its last step's barrier)
    for (uint32_t t = tid; t < nslots; t += kCollThreads) slot_store<kLds>(tab + t, kCollEmpty);
    __syncthreads();

    // phase 1: every entry leaves its position in its group's slot unless a smaller one is there
    for (int j = tid; j < k_in; j += kCollThreads) {
      const int64_t id = i_in[j];
      if (id < 0 || id >= n_rows) continue;
      const uint32_t g = (uint32_t)groups[id];
      const unsigned long long key = ((unsigned long long)g << 32) | (uint32_t)j;
      uint32_t slot = coll_hash(g, lg);
      for (;;) {   // ends: at most k_in <= nslots / 2 groups are ever placed
        unsigned long long cur = slot_load<kLds>(tab + slot);
        if (cur == kCollEmpty) cur = slot_cas<kLds>(tab + slot, kCollEmpty, key);
        if (cur == kCollEmpty) break;   // claimed
        if ((uint32_t)(cur >> 32) == g) {
          if (cur > key) slot_min<kLds>(tab + slot, key);
          break;
        }
        slot = (slot + 1u) & mask;
      }
    }
    __syncthreads();

    // phase 2: the stable compaction of the first occurrences, kCollThreads entries per step
    int base = 0;   // first occurrences before this step (uniform over the work-group)
    for (int j0 = 0; j0 < k_in; j0 += kCollThreads, buf ^= 1) {
      const int j = j0 + tid;
      bool keep = false;
      float s = 0.0f;
      int64_t id = -1;
      uint32_t g = 0;
      if (j < k_in) {
        id = i_in[j];
        s = s_in[j];
        if (id >= 0 && id < n_rows) {
          g = (uint32_t)groups[id];
          uint32_t slot = coll_hash(g, lg);
          unsigned long long cur = slot_load<kLds>(tab + slot);
          // phase 1 placed every listed group, so the probe finds it (an empty slot would end it too)
          while ((uint32_t)(cur >> 32) != g && cur != kCollEmpty) {
            slot = (slot + 1u) & mask;
            cur = slot_load<kLds>(tab + slot);
          }
          keep = (uint32_t)cur == (uint32_t)j;
        }
      }
      const unsigned long long m = __ballot(keep);
      const int before = __popcll(m & ((1ull << lane) - 1ull));
      if (lane == 0) wcnt[buf][wave] = __popcll(m);
      __syncthreads();   // (the other buffer was last read before the previous step's barrier)
      int woff = 0, total = 0;
#pragma unroll
      for (int w = 0; w < kCollWaves; ++w) {
        const int c = wcnt[buf][w];
        woff += w < wave ? c : 0;
        total += c;
      }
      const int pos = base + woff + before;   // output slot of this first occurrence
      if (keep && pos < k_out) {
        s_out[pos] = s;
        g_out[pos] = (int32_t)g;
        i_out[pos] = id;
      }
      base += total;
    }
    // the slots no first occurrence reached
    for (int o = (base < k_out ? base : k_out) + tid; o < k_out; o += kCollThreads) {
      s_out[o] = kPadScore;
      g_out[o] = -1;
      i_out[o] = -1;
    }
    if (tid == 0) out_count[q] = base;
  }
}

}  // namespace drt

using namespace drt;

extern "C" {

size_t drt_topk_collapse_workspace(int64_t nq, int32_t k_in) {
  if (nq < 0 || nq > 0x7FFFFFFF || k_in < 1 || k_in > kCollMaxKIn) return 0;
  if (k_in <= kCollapseLdsK) return kCollMinWorkspace;
  const int64_t regions = nq < kCollRegions ? (nq > 0 ? nq : 1) : kCollRegions;
  return (size_t)regions * ((size_t)1 << coll_log2_slots(k_in)) * sizeof(unsigned long long);
}

int drt_topk_collapse(const float* scores, const int64_t* ids, int64_t nq, int32_t k_in, const int32_t* groups,
                      int64_t n_rows, int32_t k_out, float* out_scores, int32_t* out_groups, int64_t* out_ids,
                      int32_t* out_count, void* ws, size_t ws_bytes, void* stream) {
  const size_t need = drt_topk_collapse_workspace(nq, k_in);
  DRT_REQUIRE(need > 0 && n_rows >= 0 && k_out >= 1);
  if (nq == 0) return DRT_OK;
  // groups may be NULL for n_rows == 0: every id is then outside the map and it is never read
  DRT_REQUIRE(scores && ids && (groups || n_rows == 0) && out_scores && out_groups && out_ids && out_count);
  if (k_in <= kCollapseLdsK) {
    const int64_t wgs = nq < kCollLdsGroups ? nq : kCollLdsGroups;
    hipLaunchKernelGGL(topk_collapse_kernel<true>, dim3((unsigned)wgs), dim3(kCollThreads), 0, (hipStream_t)stream,
                       scores, ids, nq, (int)k_in, groups, n_rows, (int)k_out, out_scores, out_groups, out_ids,
                       out_count, (unsigned long long*)nullptr);
  } else {
    DRT_REQUIRE(ws && ws_bytes >= need && ((uintptr_t)ws & 7) == 0);
    const int64_t wgs = nq < kCollRegions ? nq : kCollRegions;   // need = wgs regions
    hipLaunchKernelGGL(topk_collapse_kernel<false>, dim3((unsigned)wgs), dim3(kCollThreads), 0, (hipStream_t)stream,
                       scores, ids, nq, (int)k_in, groups, n_rows, (int)k_out, out_scores, out_groups, out_ids,
                       out_count, (unsigned long long*)ws);
  }
  return hip_status(hipGetLastError());
}

}  // extern "C"
