// Hard-negative mining on top of the exact search (DESIGN.md "Filtered search"): the two kernels the index
// needs beyond its top-k to answer "top-m of the corpus minus a per-query id set".
//
//   topk_exclude_kernel   a stable compaction of each query's canonical top-K list: entries whose id is in
//                         the query's (sorted) exclusion segment, pads, and entries at or above the query's
//                         score ceiling are dropped; survivors skip .. skip + k_out - 1 are written in
//                         their input order.  Replaces the Python skip loop of BM25Negatives.load_passages
//                         (DRT/trainer/sampler.py:69-80).
//   pair_scores_kernel    the exact score (fp64 sum of the bf16 products, rounded once to fp32 -- the
//                         canonical stage's definition, refine.hip) of chosen (query, row) pairs: the
//                         positives' scores a positive-aware ceiling is made from.
//
// Exactness: the input list is the top-K of the whole corpus in (score desc, id asc) order, so its first
// skip + m survivors are the top-(skip + m) of the corpus minus the segment E whenever K >= skip + m + |E|
// (at most |E| entries of the list are dropped).  Nothing here ranks: keeping the order is the whole job.
#include "drt_common.h"

namespace drt {

constexpr int kExclThreads = 256;
constexpr int kExclWaves = kExclThreads / 64;
constexpr int kExclLds = 4096;        // ids of a segment staged in LDS (32 KiB); longer ones stay in HBM
constexpr int kExclMaxKIn = 32768;    // the large-k path's limit (MAX_K_LARGE)

// is x in the ascending array a[0, n)?  (duplicates allowed)
template <typename Ptr>
__device__ __forceinline__ bool sorted_has(Ptr a, int64_t n, int64_t x) {
  int64_t lo = 0, hi = n;
  while (lo < hi) {
    const int64_t mid = lo + ((hi - lo) >> 1);
    if (a[mid] < x) lo = mid + 1;
    else hi = mid;
  }
  return lo < n && a[lo] == x;
}

// grid nq, one work-group per query; the list is walked in rank order, kExclThreads entries per step
__global__ __launch_bounds__(kExclThreads) void topk_exclude_kernel(
    const float* __restrict__ scores, const int64_t* __restrict__ ids, int k_in, const int64_t* __restrict__ excl,
    const int64_t* __restrict__ excl_off, const float* __restrict__ ceiling, int skip, int k_out,
    float* __restrict__ out_scores, int64_t* __restrict__ out_ids, int32_t* __restrict__ out_count) {
  __shared__ int64_t seg[kExclLds];
  __shared__ int wcnt[2][kExclWaves];   // per-wave survivor counts, double-buffered over the steps
  const int64_t q = blockIdx.x;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int64_t e0 = excl_off[q];
  int64_t ne = excl_off[q + 1] - e0;
  if (ne < 0) ne = 0;
  const int64_t* ge = excl + e0;
  const bool in_lds = ne <= kExclLds;
  if (in_lds) {
    for (int i = tid; i < (int)ne; i += kExclThreads) seg[i] = ge[i];
  }
  __syncthreads();
  const bool has_ceil = ceiling != nullptr;
  const float ceil_q = has_ceil ? ceiling[q] : 0.0f;
  const float* s_in = scores + q * (int64_t)k_in;
  const int64_t* i_in = ids + q * (int64_t)k_in;
  float* s_out = out_scores + q * (int64_t)k_out;
  int64_t* i_out = out_ids + q * (int64_t)k_out;

  int base = 0;   // survivors before this step (uniform over the work-group)
  int buf = 0;
  for (int j0 = 0; j0 < k_in; j0 += kExclThreads, buf ^= 1) {
    const int j = j0 + tid;
    bool keep = false;
    float s = 0.0f;
    int64_t id = -1;
    if (j < k_in) {
      id = i_in[j];
      s = s_in[j];
      keep = id >= 0 && (!has_ceil || s < ceil_q);
      if (keep && ne > 0) keep = !(in_lds ? sorted_has(seg, ne, id) : sorted_has(ge, ne, id));
    }
    const unsigned long long m = __ballot(keep);
    const int before = __popcll(m & ((1ull << lane) - 1ull));
    if (lane == 0) wcnt[buf][wave] = __popcll(m);
    __syncthreads();   // (the other buffer was last read before the previous step's barrier)
    int woff = 0, total = 0;
#pragma unroll
    for (int w = 0; w < kExclWaves; ++w) {
      const int c = wcnt[buf][w];
      woff += w < wave ? c : 0;
      total += c;
    }
    const int pos = base + woff + before - skip;   // output slot of this survivor
    if (keep && pos >= 0 && pos < k_out) {
      s_out[pos] = s;
      i_out[pos] = id;
    }
    base += total;
  }
  // the slots no survivor reached
  const int filled = base - skip < 0 ? 0 : (base - skip < k_out ? base - skip : k_out);
  for (int o = filled + tid; o < k_out; o += kExclThreads) {
    s_out[o] = kPadScore;
    i_out[o] = -1;
  }
  if (tid == 0) out_count[q] = base;
}

// one wave per pair, 16-B loads: lane l takes the 8-element chunks l and l + 64 of the two rows
constexpr int kPairThreads = 256;
constexpr int kPairMaxD = 1024;

__global__ __launch_bounds__(kPairThreads) void pair_scores_kernel(
    const __bf16* __restrict__ Q, int64_t nq, const __bf16* __restrict__ P, int64_t n, int d,
    const int32_t* __restrict__ qidx, const int64_t* __restrict__ rows, int64_t npairs, float* __restrict__ out) {
  const int lane = threadIdx.x & 63;
  const int64_t j = (int64_t)blockIdx.x * (kPairThreads / 64) + (threadIdx.x >> 6);
  if (j >= npairs) return;   // wave-uniform
  const int64_t qi = qidx[j], r = rows[j];
  if (qi < 0 || qi >= nq || r < 0 || r >= n) {
    if (lane == 0) out[j] = kPadScore;
    return;
  }
  const __bf16* qr = Q + qi * (int64_t)d;
  const __bf16* pr = P + r * (int64_t)d;
  const int nch = d >> 3;
  double acc = 0.0;
#pragma unroll
  for (int t = 0; t < kPairMaxD / 8 / 64; ++t) {
    const int c = lane + 64 * t;
    if (c < nch) {
      const bf16x8 a = *(const bf16x8*)(qr + 8 * c);
      const bf16x8 b = *(const bf16x8*)(pr + 8 * c);
#pragma unroll
      for (int u = 0; u < 8; ++u) acc = __builtin_fma((double)(float)a[u], (double)(float)b[u], acc);
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) acc += __shfl_xor(acc, o, 64);
  if (lane == 0) out[j] = (float)acc;
}

}  // namespace drt

using namespace drt;

extern "C" {

int drt_topk_exclude(const float* scores, const int64_t* ids, int64_t nq, int32_t k_in, const int64_t* excl,
                     const int64_t* excl_off, const float* ceiling, int32_t skip, int32_t k_out, float* out_scores,
                     int64_t* out_ids, int32_t* out_count, void* stream) {
  DRT_REQUIRE(nq >= 0 && nq <= 0x7FFFFFFF && k_in >= 1 && k_in <= kExclMaxKIn && k_out >= 1 && skip >= 0);
  if (nq == 0) return DRT_OK;
  // excl may be NULL when every segment is empty (it is then never read)
  DRT_REQUIRE(scores && ids && excl_off && out_scores && out_ids && out_count);
  hipLaunchKernelGGL(topk_exclude_kernel, dim3((unsigned)nq), dim3(kExclThreads), 0, (hipStream_t)stream, scores,
                     ids, (int)k_in, excl, excl_off, ceiling, (int)skip, (int)k_out, out_scores, out_ids, out_count);
  return hip_status(hipGetLastError());
}

int drt_pair_scores_bf16(const void* Q, int64_t nq, const void* P, int64_t n, int32_t d, const int32_t* qidx,
                         const int64_t* rows, int64_t npairs, float* out, void* stream) {
  DRT_REQUIRE(nq >= 0 && n >= 0 && npairs >= 0 && d >= 8 && d % 8 == 0 && d <= kPairMaxD);
  if (npairs == 0) return DRT_OK;
  const int64_t blocks = (npairs + kPairThreads / 64 - 1) / (kPairThreads / 64);
  DRT_REQUIRE(blocks <= 0x7FFFFFFF);
  // Q / P may be NULL for nq / n == 0: every pair then answers -FLT_MAX without reading them
  DRT_REQUIRE((Q || nq == 0) && (P || n == 0) && qidx && rows && out);
  hipLaunchKernelGGL(pair_scores_kernel, dim3((unsigned)blocks), dim3(kPairThreads), 0, (hipStream_t)stream,
                     (const __bf16*)Q, nq, (const __bf16*)P, n, (int)d, qidx, rows, npairs, out);
  return hip_status(hipGetLastError());
}

}  // extern "C"
