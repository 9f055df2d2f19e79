// The canonical-order stage of the top-k search (search.hip step 5; DESIGN.md §3 "Canonical order"): the
// fp32 scan order turned into the order of the exact scores.  In file order: the error bound and the refine
// kernels (a candidate list's near-tie window re-ranked by exact sums), the wide resolve (a window wider than
// the list), large k (2048 < k <= 32768) with the merge by exact keys, the row statistics the bound needs,
// then the host side: launch_refine and the resolve drivers' shared helpers (search_internal.h), the C
// entries.  The filter pass of the wide and large paths is search.hip's scan, through launch_scan.
#include "profile.h"
#include "search_internal.h"

namespace drt {

// ---------------------------------------------------------------------------
// Canonical order: exact re-ranking of a top-k candidate list.
//
// The filter scan scores in fp32 on the MFMA (bf16 products are exact in fp32; the sum of d of
// them is rounded), so rows whose exact inner products differ by less than the fp32 summation
// error may come out in either order -- and a row just outside the fp32 top-k may belong inside
// it.  The reference evaluator's answer is defined by the exact products (faiss sums in fp32 too,
// in yet another order); this stage makes the result canonical: the order of the EXACT scores
// (fp64 sums of the bf16 products), ties by ascending id -- what an fp64 CPU evaluator returns.
//
// Error bound of the scan's fp32 score (round 5, measured: tools/mfma_numerics.py,
// profiles/r05b_mfma.json).  Every kernel that produces candidate scores (ip_scan16r_kernel,
// ip_scan16_kernel) accumulates one (query, row) score as a chain of T = d / 32 dependent
// v_mfma_f32_16x16x32_bf16 steps, step t adding the 32 exact bf16 products of elements
// [32t, 32t + 32) to the accumulator S_t.  One step is NOT a sequence of fp32 additions: the 33 terms
// are aligned to the largest one with 3 guard bits below fp32's last bit and the bits below that are
// truncated (32 products of 2^-28 next to a 1 vanish, 2^-26 survive; C = 2^24 plus 32 ones gives
// 2^24 + 32), then the sum is rounded once.  Worst measured error of one step: 7.9 u (|C| + sum |p|)
// (one large product, 31 just under the cut); the model gives < 8 u max|term| + 2 u |result|, so
//     |err step t| <= 10 u (|S_t| + sum_{i in step t} |q_i p_i|),      u = 2^-24.
// By Cauchy-Schwarz on the prefixes, |S_t| <= ||q_[0,32t)|| * max_rows ||p_[0,32t)||, and the products
// sum to at most ||q|| max ||p||, so over the chain
//     eps = 10 u (1 + 1e-3) (sum_{t=1}^{T-1} Qp_t Pp_t + ||q|| Pp_T),
// Qp_t = ||q_[0,32t)|| (per query), Pp_t = max over rows of ||p_[0,32t)|| (row statistics, one value
// per k-step).  Uniformly spread energy gives ~T/2 + 1 = 13 (x 10 u ||q|| max ||p||) at d = 768:
// 15x tighter than the round-4 bound 2.5 d u ||q|| max ||p|| (an fp32 summation in any order) -- the
// C2 leg's untrained-tower embeddings, whose 1000th score has ~100 rows within the old 2 eps, now
// certify (tools/c2_window_probe.py).  Chains of 24 steps measured at most 1.5 u sum_t |S_t|.
// With s_k the k-th candidate's fp32 score, every row of the exact top-k has fp32 score >= B =
// s_k - 2 eps (the k-th exact score is >= s_k - eps), so the candidates are exactly the entries >= B
// of a list that (a) holds every hit >= B -- its last entry is < B, or the hits ended -- and (b) saw
// every row >= B -- the filter threshold tau <= B.  Either failing sets status bit 1; the product then
// runs the wide resolve (drt_ip_topk_resolve_wide): a filter pass at threshold B, the exact sums of
// every row it collects (up to kWideCap per query) and an exact-key selection.  Integer-valued rows
// and queries whose |partial sums| stay below 2^23 are scored exactly in fp32: eps = 0 and the fp32
// order IS the exact order.
//
// refine_delta_kernel  grid (nq, kc / slice): exact sum for each candidate this rank owns
//   (global id in [row_offset, row_offset + n_local)) -> delta = exact - fp32 score (0 where not
//   owned or past the window: shards add their deltas with one all-reduce SUM); cnt[q] = window
//   size (-1 when eps = 0).
// refine_sort_kernel   grid nq: the window by (fp32 score + delta desc, id asc) -> top-k.
// ---------------------------------------------------------------------------
constexpr int kRefThreads = 256;
constexpr int kRefSlice = 64;        // candidates per work-group of refine_delta, one GPU
constexpr int kRefSliceShard = 256;  // ... on a shard of a sharded index (~1/W of them owned)
constexpr int kRefSortThreads = 512;
constexpr int kRefMax = kSelMaxK;

__device__ __forceinline__ uint64_t desc_key64(double x) {
  x = x + 0.0;
  const uint64_t u = __builtin_bit_cast(uint64_t, x);
  const uint64_t ord = (u >> 63) ? ~u : (u | 0x8000000000000000ull);
  return ~ord;
}

template <typename T>
__device__ __forceinline__ T ref_block_sum(T v, T* scr) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) scr[threadIdx.x >> 6] = v;
  __syncthreads();
  T r = 0;
  for (int w = 0; w < (int)(blockDim.x >> 6); ++w) r += scr[w];
  return r;
}

// Row statistics (drt_row_stats_bf16): [0] max_rows ||p||^2, [1] 1.0f while every element is an
// integer, [2 + t] max_rows ||p_[0, 32 (t + 1))||^2 for the k-steps t < ceil(d / 32) (the prefix
// norms of the error bound above).
constexpr int kStatBlocks = 32;   // d <= 1024
constexpr int kStatsLen = 2 + kStatBlocks;

// eps of query q (0: exact in fp32; the bound above).  Every work-group of q computes the same value.
// dscr: >= kStatBlocks + 1 doubles of LDS.
__device__ __forceinline__ float refine_eps(const RefineArgs& a, int64_t q, float* fscr, int* iscr, double* dscr) {
  const __bf16* qr = a.Q + q * (int64_t)a.d;
  const int nb = (a.d + 31) >> 5;
  int nonint = 0;
  for (int i = threadIdx.x; i < a.d; i += blockDim.x) {
    const float v = (float)qr[i];
    nonint |= (v != __builtin_rintf(v)) ? 1 : 0;
  }
  if ((int)threadIdx.x < nb) {   // this k-step's squared query norm, exactly enough in fp64
    double ss = 0.0;
    const int e1 = min(a.d, 32 * (int)threadIdx.x + 32);
    for (int i = 32 * threadIdx.x; i < e1; ++i) {
      const double v = (double)(float)qr[i];
      ss += v * v;
    }
    dscr[threadIdx.x] = ss;
  }
  nonint = ref_block_sum(nonint, iscr);   // (its barriers also publish dscr)
  if (threadIdx.x == 0) {
    double qp2 = 0.0, acc = 0.0;
    for (int t = 0; t < nb; ++t) {
      if (t > 0) acc += __builtin_sqrt(qp2 * (double)a.stats[2 + t - 1]);
      qp2 += dscr[t];
    }
    const double pmax2 = (double)a.stats[0];
    acc += __builtin_sqrt(qp2 * pmax2);
    const bool pint = a.stats[1] != 0.0f;
    const double qn = __builtin_sqrt(qp2) * 1.0001, pmax = __builtin_sqrt(pmax2) * 1.0001;
    float e;
    if (pint && nonint == 0 && qn * pmax < 8388608.0) e = 0.0f;
    else e = (float)(10.0 * 5.9604644775390625e-8 * 1.001 * acc) + 1e-30f;
    dscr[kStatBlocks] = (double)e;
  }
  __syncthreads();
  return (float)dscr[kStatBlocks];
}

// per query: eps, the window C (entries >= B = s_k - 2 eps) and the certificate bits -> cnt[q]
__global__ __launch_bounds__(kRefThreads) void refine_prep_kernel(RefineArgs a) {
  __shared__ float fscr[kRefThreads / 64];
  __shared__ int iscr[kRefThreads / 64];
  __shared__ double dscr[kStatBlocks + 1];
  const int64_t q = blockIdx.x;
  const int tid = threadIdx.x;
  const float eps = refine_eps(a, q, fscr, iscr, dscr);
  const float* cs = a.cs + q * (int64_t)a.kc;
  const int64_t* ci = a.ci + q * (int64_t)a.kc;
  int nval = 0;
  for (int j = tid; j < a.kc; j += kRefThreads) nval += ci[j] >= 0 ? 1 : 0;
  nval = ref_block_sum(nval, iscr);
  const float B = nval < a.k ? -__builtin_inff() : cs[a.k - 1] - 2.0f * eps;
  int C = 0;
  for (int j = tid; j < nval; j += kRefThreads) C += cs[j] >= B ? 1 : 0;
  C = ref_block_sum(C, iscr);
  const bool wide = eps != 0.0f && C == a.kc && nval == a.kc;               // window wider than the list
  // the window reaches below the filter threshold: rows in [B, tau) were never collected, so the
  // exact order of the window cannot be certified from the list.  The fp32 top-k itself is exact
  // (every row >= tau was collected; the select certified k <= hits): it stays in place in the fp32
  // order with status bit 1, and the caller's wide resolve (a filter pass at B) replaces it.
  const bool below = eps != 0.0f && a.tau && nval >= a.k && a.tau[q] > B;
  if (tid == 0) {
    a.cnt[2 * q] = eps == 0.0f ? -1 : ((wide || below) ? -2 : C);
    a.cnt[2 * q + 1] = __builtin_bit_cast(int32_t, eps);
    if (a.status) {
      const int st = (wide || below) ? 2 : 0;
      const int64_t orow = a.qmap ? (int64_t)a.qmap[q] : q;
      if (a.set_status) a.status[orow] = st;
      else if (st) a.status[orow] |= st;
    }
  }
}

// exact sums of the window's candidates this shard owns.  A work-group takes a slice of `slice`
// candidates (64 on one GPU, 256 on a shard of a sharded index), writes delta 0 for the ones another
// shard owns and compacts the owned ones into LDS; its 4 waves then split the owned list, kRefUnroll
// rows at a time with every row load of the group in flight together (one HBM round trip per group
// instead of one per candidate).  Round 4: the waves used to walk the slice itself, so on a W-way
// sharded index ~(W-1)/W of their row slots were idle -- 461 us per 2048-query group at W = 8
// for ~1/8 of the gathers (tools/sim_rank.py, profiles/r04af_*).
constexpr int kRefUnroll = 8;
// exact sums of the compacted owned candidates e0 .. e1 (own_j / own_row in LDS)
__device__ __forceinline__ void refine_delta_rows(const RefineArgs& a, int64_t q, const float* cs, const int64_t* ci,
                                                  float* dq, int lane, int e0, int e1, const int* own_j,
                                                  const int64_t* own_row) {
  // this lane's query elements: 4-element chunks c = lane + 64 t of the row, in fp64
  constexpr int kMaxT = 4;   // d <= 1024
  const int nch = a.d >> 2;
  double qv[kMaxT][4];
  const __bf16* qr = a.Q + q * (int64_t)a.d;
#pragma unroll
  for (int t = 0; t < kMaxT; ++t) {
    const int c = lane + 64 * t;
    const bf16x4 x = c < nch ? *(const bf16x4*)(qr + 4 * c) : bf16x4{};
#pragma unroll
    for (int u = 0; u < 4; ++u) qv[t][u] = (double)(float)x[u];
  }
  for (int eb = e0; eb < e1; eb += kRefUnroll) {
    bool ok[kRefUnroll];
    int jj[kRefUnroll];
    int64_t row[kRefUnroll];
#pragma unroll
    for (int u = 0; u < kRefUnroll; ++u) {
      ok[u] = eb + u < e1;   // wave-uniform
      jj[u] = ok[u] ? own_j[eb + u] : 0;
      row[u] = ok[u] ? own_row[eb + u] : 0;
    }
    bf16x4 x[kRefUnroll][kMaxT];
#pragma unroll
    for (int u = 0; u < kRefUnroll; ++u) {
      const __bf16* pr = a.P + row[u] * (int64_t)a.d;
#pragma unroll
      for (int t = 0; t < kMaxT; ++t) {
        const int c = lane + 64 * t;
        x[u][t] = (ok[u] && c < nch) ? *(const bf16x4*)(pr + 4 * c) : bf16x4{};
      }
    }
    double acc[kRefUnroll];
#pragma unroll
    for (int u = 0; u < kRefUnroll; ++u) {
      acc[u] = 0.0;
#pragma unroll
      for (int t = 0; t < kMaxT; ++t)
#pragma unroll
        for (int e = 0; e < 4; ++e) acc[u] = __builtin_fma(qv[t][e], (double)(float)x[u][t][e], acc[u]);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1)
#pragma unroll
      for (int u = 0; u < kRefUnroll; ++u) acc[u] += __shfl_xor(acc[u], o, 64);
    if (lane == 0) {
#pragma unroll
      for (int u = 0; u < kRefUnroll; ++u)
        if (ok[u]) dq[jj[u]] = (float)(acc[u] - (double)cs[jj[u]]);
    }
  }
}
constexpr int kRefSliceMax = kRefThreads;
__global__ __launch_bounds__(kRefThreads) void refine_delta_kernel(RefineArgs a) {
  __shared__ int own_j[kRefSliceMax];
  __shared__ int64_t own_row[kRefSliceMax];   // the owned candidates' local rows (no dependent id load later)
  __shared__ int n_own;
  const int64_t q = blockIdx.x;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int C = a.cnt[2 * q];
  const int jb = (int)blockIdx.y * a.slice;
  if (C <= jb) return;   // also: exact in fp32 (-1) or window too wide (-2)
  const float* cs = a.cs + q * (int64_t)a.kc;
  const int64_t* ci = a.ci + q * (int64_t)a.kc;
  float* dq = a.delta + q * (int64_t)a.kc;
  if (tid == 0) n_own = 0;
  __syncthreads();
  {
    const int j = jb + tid;
    bool own = false;
    int64_t row = 0;
    if (tid < a.slice && j < C) {
      const int64_t id = ci[j];
      row = id - a.row_offset;
      own = id >= 0 && row >= 0 && row < a.n_local;
      if (!own) dq[j] = 0.0f;   // another shard's row: its delta arrives through the all-reduce
    }
    const uint64_t m = __ballot(own);
    int base = 0;
    if (lane == 0 && m) base = atomicAdd(&n_own, __builtin_popcountll(m));
    base = __shfl(base, 0, 64);
    if (own) {
      const int e = base + (int)__builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
      own_j[e] = j;
      own_row[e] = row;
    }
  }
  __syncthreads();
  const int n = n_own;
  const int per = (n + 3) >> 2;
  const int e0 = wave * per;
  const int e1 = e0 + per < n ? e0 + per : n;
  if (e0 < e1) refine_delta_rows(a, q, cs, ci, dq, lane, e0, e1, own_j, own_row);
}

// One shard (ip_topk / resolve: every candidate is this shard's): each wave takes kRefSlice / 4 window
// entries directly, no compaction (the compaction kernel above measured 71-82 vs 57 us per 10M batch).
__global__ __launch_bounds__(kRefThreads) void refine_delta_local_kernel(RefineArgs a) {
  const int64_t q = blockIdx.x;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int C = a.cnt[2 * q];
  const int j0 = blockIdx.y * kRefSlice + wave * (kRefSlice / 4);
  if (C <= j0) return;   // also: exact in fp32 (-1) or window too wide (-2)
  const int j1 = j0 + kRefSlice / 4 < C ? j0 + kRefSlice / 4 : C;
  const float* cs = a.cs + q * (int64_t)a.kc;
  const int64_t* ci = a.ci + q * (int64_t)a.kc;
  float* dq = a.delta + q * (int64_t)a.kc;
  // this lane's query elements: 4-element chunks c = lane + 64 t of the row, in fp64
  constexpr int kMaxT = 4;   // d <= 1024
  const int nch = a.d >> 2;
  double qv[kMaxT][4];
  const __bf16* qr = a.Q + q * (int64_t)a.d;
#pragma unroll
  for (int t = 0; t < kMaxT; ++t) {
    const int c = lane + 64 * t;
    const bf16x4 x = c < nch ? *(const bf16x4*)(qr + 4 * c) : bf16x4{};
#pragma unroll
    for (int u = 0; u < 4; ++u) qv[t][u] = (double)(float)x[u];
  }
  for (int jb = j0; jb < j1; jb += kRefUnroll) {
    bool own[kRefUnroll];
    int64_t row[kRefUnroll];
#pragma unroll
    for (int u = 0; u < kRefUnroll; ++u) {
      const int j = jb + u;
      const int64_t id = j < j1 ? ci[j] : -1;
      row[u] = id - a.row_offset;
      own[u] = j < j1 && id >= 0 && row[u] >= 0 && row[u] < a.n_local;   // wave-uniform
    }
    bf16x4 x[kRefUnroll][kMaxT];
#pragma unroll
    for (int u = 0; u < kRefUnroll; ++u) {
      const __bf16* pr = a.P + (own[u] ? row[u] : 0) * (int64_t)a.d;
#pragma unroll
      for (int t = 0; t < kMaxT; ++t) {
        const int c = lane + 64 * t;
        x[u][t] = (own[u] && c < nch) ? *(const bf16x4*)(pr + 4 * c) : bf16x4{};
      }
    }
    double acc[kRefUnroll];
#pragma unroll
    for (int u = 0; u < kRefUnroll; ++u) {
      acc[u] = 0.0;
#pragma unroll
      for (int t = 0; t < kMaxT; ++t)
#pragma unroll
        for (int e = 0; e < 4; ++e) acc[u] = __builtin_fma(qv[t][e], (double)(float)x[u][t][e], acc[u]);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1)
#pragma unroll
      for (int u = 0; u < kRefUnroll; ++u) acc[u] += __shfl_xor(acc[u], o, 64);
    if (lane == 0) {
#pragma unroll
      for (int u = 0; u < kRefUnroll; ++u)
        if (jb + u < j1) dq[jb + u] = own[u] ? (float)(acc[u] - (double)cs[jb + u]) : 0.0f;
    }
  }
}

// Row-pair form of refine_delta_local_kernel (round 6) for d % 8 == 0 and 16-B aligned rows: the
// two 32-lane halves of a wave take two candidates and each lane loads 16-B chunks c = hl + 32 t
// (one 1.5 KiB row in 3 loads per lane instead of 3 x 8-B loads over 64 lanes), 8 candidates in
// flight per wave.  Deltas identical (bf16 products are exact in fp64 and every test digest
// matches); 0.73 -> 0.64 ms per 2048-query window over the 10M corpus (profiles/r06k/).
__global__ __launch_bounds__(kRefThreads) void refine_delta_local8_kernel(RefineArgs a) {
  const int64_t q = blockIdx.x;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int C = a.cnt[2 * q];
  const int j0 = blockIdx.y * kRefSlice + wave * (kRefSlice / 4);
  if (C <= j0) return;   // also: exact in fp32 (-1) or window too wide (-2)
  const int j1 = j0 + kRefSlice / 4 < C ? j0 + kRefSlice / 4 : C;
  const float* cs = a.cs + q * (int64_t)a.kc;
  const int64_t* ci = a.ci + q * (int64_t)a.kc;
  float* dq = a.delta + q * (int64_t)a.kc;
  const int half = lane >> 5, hl = lane & 31;
  constexpr int kT = 4;   // d <= 1024: 128 chunks of 8 over 32 lanes
  const int n16 = a.d >> 3;
  double qv[kT][8];
  const __bf16* qr = a.Q + q * (int64_t)a.d;
#pragma unroll
  for (int t = 0; t < kT; ++t) {
    const int c = hl + 32 * t;
    const bf16x8 x = c < n16 ? *(const bf16x8*)(qr + 8 * c) : bf16x8{};
#pragma unroll
    for (int u = 0; u < 8; ++u) qv[t][u] = (double)(float)x[u];
  }
  constexpr int kP = 4;   // row pairs in flight
  for (int jb = j0; jb < j1; jb += 2 * kP) {
    bool own[kP];
    int64_t row[kP];
#pragma unroll
    for (int p = 0; p < kP; ++p) {
      const int j = jb + 2 * p + half;
      const int64_t id = j < j1 ? ci[j] : -1;
      row[p] = id - a.row_offset;
      own[p] = j < j1 && id >= 0 && row[p] >= 0 && row[p] < a.n_local;
    }
    bf16x8 x[kP][kT];
#pragma unroll
    for (int p = 0; p < kP; ++p) {
      const __bf16* pr = a.P + (own[p] ? row[p] : 0) * (int64_t)a.d;
#pragma unroll
      for (int t = 0; t < kT; ++t) {
        const int c = hl + 32 * t;
        x[p][t] = (32 * t < n16 && own[p] && c < n16) ? *(const bf16x8*)(pr + 8 * c) : bf16x8{};
      }
    }
    double acc[kP];
#pragma unroll
    for (int p = 0; p < kP; ++p) {
      acc[p] = 0.0;
#pragma unroll
      for (int t = 0; t < kT; ++t) {
        if (32 * t >= n16) break;
#pragma unroll
        for (int u = 0; u < 8; ++u) acc[p] = __builtin_fma(qv[t][u], (double)(float)x[p][t][u], acc[p]);
      }
    }
#pragma unroll
    for (int o = 16; o > 0; o >>= 1)
#pragma unroll
      for (int p = 0; p < kP; ++p) acc[p] += __shfl_xor(acc[p], o, 64);
    if (hl == 0) {
#pragma unroll
      for (int p = 0; p < kP; ++p) {
        const int j = jb + 2 * p + half;
        if (j < j1) dq[j] = own[p] ? (float)(acc[p] - (double)cs[j]) : 0.0f;
      }
    }
  }
}

static void launch_refine_local(const RefineArgs& ra, hipStream_t s) {
  const dim3 grid((unsigned)ra.nq, (unsigned)((ra.kc + kRefSlice - 1) / kRefSlice));
  const bool rows16 = ra.d % 8 == 0 && ((uintptr_t)ra.P % 16 == 0) && ((uintptr_t)ra.Q % 16 == 0);
  if (rows16) hipLaunchKernelGGL(refine_delta_local8_kernel, grid, dim3(kRefThreads), 0, s, ra);
  else hipLaunchKernelGGL(refine_delta_local_kernel, grid, dim3(kRefThreads), 0, s, ra);
}

// The window ranked by (exact score desc, id asc) without a sort network: the candidates arrive
// sorted by fp32 score and every row's fp32 score is within eps of its exact one, so candidate i
// follows every j with s_j > s_i + 2 eps and precedes every j with s_j < s_i - 2 eps; its rank is
// the count of the former plus the exact comparisons inside the band |s_j - s_i| <= 2 eps (two
// binary searches and ~ band-width compares per candidate; the band is a few dozen entries on
// real-valued data).  Each candidate then writes itself at its rank.
__global__ __launch_bounds__(kRefSortThreads) void refine_sort_kernel(RefineArgs a) {
  __shared__ uint64_t key[kRefMax];
  __shared__ int64_t idv[kRefMax];
  __shared__ float sf[kRefMax];
  const int64_t q = blockIdx.x;
  const int tid = threadIdx.x;
  const int64_t orow = a.qmap ? (int64_t)a.qmap[q] : q;
  const float* cs = a.cs + q * (int64_t)a.kc;
  const int64_t* ci = a.ci + q * (int64_t)a.kc;
  float* os = a.out_s + orow * (int64_t)a.k;
  int64_t* oi = a.out_i + orow * (int64_t)a.k;
  const int C = a.cnt[2 * q];
  if (C < 0) {   // exact in fp32 (or the window did not fit the list: status bit 1): the fp32 order
    for (int j = tid; j < a.k; j += kRefSortThreads) {
      os[j] = cs[j];
      oi[j] = ci[j];
    }
    return;
  }
  const double two_eps = 2.0 * (double)__builtin_bit_cast(float, a.cnt[2 * q + 1]);
  const float* dq = a.delta + q * (int64_t)a.kc;
  for (int j = tid; j < C; j += kRefSortThreads) {
    const float s = cs[j];
    sf[j] = s;
    key[j] = desc_key64((double)s + (double)dq[j]);
    idv[j] = ci[j];
  }
  for (int j = C + tid; j < a.k; j += kRefSortThreads) {   // fewer candidates than k: pads
    os[j] = kPadScore;
    oi[j] = -1;
  }
  __syncthreads();
  for (int i = tid; i < C; i += kRefSortThreads) {
    const double si = (double)sf[i];
    const double up = si + two_eps, dn = si - two_eps;
    int lo = 0, hi = i;   // lo = #{j : s_j > si + 2 eps} (a prefix: sf is non-increasing)
    while (lo < hi) {
      const int mid = (lo + hi) >> 1;
      if ((double)sf[mid] > up) lo = mid + 1;
      else hi = mid;
    }
    int lo2 = i, hi2 = C;  // hi2 = #{j : s_j >= si - 2 eps}
    while (lo2 < hi2) {
      const int mid = (lo2 + hi2) >> 1;
      if ((double)sf[mid] >= dn) lo2 = mid + 1;
      else hi2 = mid;
    }
    const uint64_t ki = key[i];
    const int64_t ii = idv[i];
    int rank = lo;
    for (int j = lo; j < lo2; ++j) {
      const uint64_t kj = key[j];
      rank += (kj < ki || (kj == ki && idv[j] < ii)) ? 1 : 0;
    }
    if (rank < a.k) {
      // the exact score from its order key (desc_key64 is a bijection)
      const uint64_t ord = ~ki;
      const uint64_t u = (ord >> 63) ? (ord & 0x7FFFFFFFFFFFFFFFull) : ~ord;
      os[rank] = (float)__builtin_bit_cast(double, u);
      oi[rank] = ii;
    }
  }
}

// ---------------------------------------------------------------------------
// Wide resolve (status bit 1): the canonical order of a query whose near-tie window did not fit the
// candidate list, or reached below the filter threshold -- degenerate embeddings whose scores crowd
// within the fp32 error of the k-th one.  Per query of a chunk (host: drt_ip_topk_resolve_wide):
//   wide_prep_kernel    B = s_k - 2 eps from the query's fp32 top-k (its output row), counters zeroed;
//   filter scan         every row with fp32 score >= B (the same scan kernel: the same fp32 scores),
//                       up to kWideCap keys (desc fp32 key << 32 | row);
//   wide_exact_kernel   the exact sum (fp64) of each collected row -> 64-bit exact order key;
//   wide_select_kernel  the k smallest (exact key, row) pairs: an 8-bit MSD radix select on the exact
//                       key for rank k, a second one on the rows tied at that key, then each selected
//                       entry's rank by counting -- written in (exact score desc, id asc) order.
// The exact top-k lies inside {fp32 >= B} (see the bound above), so the result is the fp64 evaluator's
// for every query whose collected set fits kWideCap; a larger set keeps bit 1 (fp32 order).
// ---------------------------------------------------------------------------
constexpr int kWideThreads = 1024;
constexpr int kWideSlice = 256;   // collected rows per work-group of wide_exact_kernel

struct WideArgs {
  RefineArgs ra;          // Q (the chunk's queries), d, stats: refine_eps
  const int32_t* qmap;    // chunk query -> output row
  int32_t nb;             // queries in the chunk
  int32_t k;
  float* tau;             // [kQueriesPerWG]
  uint32_t* counts;       // [kQueriesPerWG * kCntStride]
  const uint64_t* keys;   // [kQueriesPerWG][cap] filter hits
  uint64_t* ekeys;        // [kQueriesPerWG][cap] exact order keys
  int64_t cap;
  int64_t id_offset;
  float* out_s;           // [*, k] (rows through qmap)
  int64_t* out_i;
  int32_t* status;
  // large-k path (drt_ip_topk_large): qmap == nullptr maps chunk query j to output row q0 + j; tau_in
  // is a per-output-row lower bound of the k-th fp32 score; sel_* hold each query's selected entries
  int64_t q0;
  const float* tau_in;
  uint64_t* sel_k;
  uint32_t* sel_r;
  uint32_t* sel_n;
  uint64_t* bin_k;        // [*, k] the selected entries regrouped by bin (large_rank_kernel)
  uint32_t* bin_r;
  uint64_t* out_keys;     // optional [*, k]: the exact order key of every output entry (~0: pad) -- what a
                          // sharded index merges by (drt_merge_exact)
};

__device__ __forceinline__ int64_t wide_out_row(const WideArgs& w, int j) {
  return w.qmap ? (int64_t)w.qmap[j] : w.q0 + j;
}

__global__ __launch_bounds__(kRefThreads) void wide_prep_kernel(WideArgs w) {
  __shared__ float fscr[kRefThreads / 64];
  __shared__ int iscr[kRefThreads / 64];
  __shared__ double dscr[kStatBlocks + 1];
  const int j = blockIdx.x;
  if (j >= w.nb) {   // padding queries of the 128-query scan block: inactive
    if (threadIdx.x == 0) {
      w.tau[j] = __builtin_nanf("");
      w.counts[j * kCntStride] = 0u;
    }
    return;
  }
  const float eps = refine_eps(w.ra, j, fscr, iscr, dscr);
  if (threadIdx.x == 0) {
    const int64_t orow = wide_out_row(w, j);
    const float sk = w.tau_in ? w.tau_in[orow] : w.out_s[orow * w.k + w.k - 1];
    w.tau[j] = sk - 2.0f * eps;
    w.counts[j * kCntStride] = 0u;
    if (w.tau_in) w.status[orow] = 2;   // large path: cleared once the query's set is ranked
  }
}

__global__ __launch_bounds__(kRefThreads) void wide_exact_kernel(WideArgs w) {
  const int j = blockIdx.x;
  const uint32_t c = w.counts[j * kCntStride];
  const int64_t h0 = (int64_t)blockIdx.y * kWideSlice;
  if (c > (uint64_t)w.cap || h0 >= (int64_t)c) return;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int d = w.ra.d;
  constexpr int kMaxT = 4;   // d <= 1024
  const int nch = d >> 2;
  double qv[kMaxT][4];
  const __bf16* qr = w.ra.Q + (int64_t)j * d;
#pragma unroll
  for (int t = 0; t < kMaxT; ++t) {
    const int cc = lane + 64 * t;
    const bf16x4 x = cc < nch ? *(const bf16x4*)(qr + 4 * cc) : bf16x4{};
#pragma unroll
    for (int u = 0; u < 4; ++u) qv[t][u] = (double)(float)x[u];
  }
  const uint64_t* kj = w.keys + (int64_t)j * w.cap;
  uint64_t* ej = w.ekeys + (int64_t)j * w.cap;
  const int64_t h1 = std::min<int64_t>((int64_t)c, h0 + kWideSlice);
  for (int64_t hb = h0 + wave * kRefUnroll; hb < h1; hb += 4 * kRefUnroll) {
    bool ok[kRefUnroll];
    int64_t row[kRefUnroll];
#pragma unroll
    for (int u = 0; u < kRefUnroll; ++u) {
      ok[u] = hb + u < h1;   // wave-uniform
      row[u] = ok[u] ? (int64_t)(uint32_t)kj[hb + u] : 0;
    }
    bf16x4 x[kRefUnroll][kMaxT];
#pragma unroll
    for (int u = 0; u < kRefUnroll; ++u) {
      const __bf16* pr = w.ra.P + row[u] * (int64_t)d;
#pragma unroll
      for (int t = 0; t < kMaxT; ++t) {
        const int cc = lane + 64 * t;
        x[u][t] = (ok[u] && cc < nch) ? *(const bf16x4*)(pr + 4 * cc) : bf16x4{};
      }
    }
    double acc[kRefUnroll];
#pragma unroll
    for (int u = 0; u < kRefUnroll; ++u) {
      acc[u] = 0.0;
#pragma unroll
      for (int t = 0; t < kMaxT; ++t)
#pragma unroll
        for (int e = 0; e < 4; ++e) acc[u] = __builtin_fma(qv[t][e], (double)(float)x[u][t][e], acc[u]);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1)
#pragma unroll
      for (int u = 0; u < kRefUnroll; ++u) acc[u] += __shfl_xor(acc[u], o, 64);
    if (lane == 0) {
#pragma unroll
      for (int u = 0; u < kRefUnroll; ++u)
        if (ok[u]) ej[hb + u] = desc_key64(acc[u]);
    }
  }
}

// 8-bit MSD radix select over the entries of `src` that match (prefix, mask) on `key`: the value whose
// ascending rank is `want` (1-based); `want` becomes that value's rank among the entries equal to it.
template <typename KeyFn>
__device__ __forceinline__ uint64_t wide_radix_select(int64_t n, int bits, KeyFn key_of, uint32_t* hist, uint64_t* sh,
                                                      int64_t& want) {
  uint64_t prefix = 0, mask = 0;
  for (int shift = bits - 8; shift >= 0; shift -= 8) {
    for (int b = threadIdx.x; b < 256; b += blockDim.x) hist[b] = 0u;
    __syncthreads();
    for (int64_t h = threadIdx.x; h < n; h += blockDim.x) {
      bool take;
      const uint64_t v = key_of(h, take);
      if (take && (v & mask) == prefix) atomicAdd(&hist[(v >> shift) & 255u], 1u);
    }
    __syncthreads();
    if (threadIdx.x == 0) {
      int64_t cum = 0;
      int dg = 255;
      for (int b = 0; b < 256; ++b) {
        if (cum + (int64_t)hist[b] >= want) {
          dg = b;
          break;
        }
        cum += hist[b];
      }
      sh[0] = prefix | ((uint64_t)dg << shift);
      sh[1] = (uint64_t)(want - cum);
    }
    __syncthreads();
    prefix = sh[0];
    want = (int64_t)sh[1];
    mask |= (uint64_t)0xFF << shift;
    __syncthreads();
  }
  return prefix;
}

__global__ __launch_bounds__(kWideThreads) void wide_select_kernel(WideArgs w) {
  __shared__ uint32_t hist[256];
  __shared__ uint64_t sh[2];
  __shared__ uint64_t sek[kSelMaxK];
  __shared__ uint32_t srow[kSelMaxK];
  __shared__ int ns;
  const int j = blockIdx.x;
  if (j >= w.nb) return;
  const uint32_t c = w.counts[j * kCntStride];
  if (c > (uint64_t)w.cap) return;   // more rows within 2 eps of the k-th than the cap: bit 1 stays
  const int64_t nh = c;
  const uint64_t* kj = w.keys + (int64_t)j * w.cap;
  const uint64_t* ej = w.ekeys + (int64_t)j * w.cap;
  const int64_t keff = std::min<int64_t>(w.k, nh);
  const int64_t orow = w.qmap[j];
  float* os = w.out_s + orow * w.k;
  int64_t* oi = w.out_i + orow * w.k;
  uint64_t kstar = ~0ull;
  uint64_t rstar = ~0ull;
  if (keff > 0) {
    int64_t want = keff;
    kstar = wide_radix_select(nh, 64, [&](int64_t h, bool& take) { take = true; return ej[h]; }, hist, sh, want);
    // rows tied at the k-th exact key: the `want` smallest
    const uint64_t ks = kstar;
    rstar = wide_radix_select(nh, 32, [&](int64_t h, bool& take) {
      take = ej[h] == ks;
      return (uint64_t)(uint32_t)kj[h];
    }, hist, sh, want);
  }
  if (threadIdx.x == 0) ns = 0;
  __syncthreads();
  for (int64_t h = threadIdx.x; h < nh && keff > 0; h += kWideThreads) {
    const uint64_t ek = ej[h];
    const uint64_t row = (uint32_t)kj[h];
    if (ek < kstar || (ek == kstar && row <= rstar)) {
      const int pos = atomicAdd(&ns, 1);
      if (pos < kSelMaxK) {
        sek[pos] = ek;
        srow[pos] = (uint32_t)row;
      }
    }
  }
  __syncthreads();
  const int m = ns < kSelMaxK ? ns : kSelMaxK;
  for (int i = threadIdx.x; i < m; i += kWideThreads) {
    const uint64_t ki = sek[i];
    const uint32_t ri = srow[i];
    int rank = 0;
    for (int t = 0; t < m; ++t) rank += (sek[t] < ki || (sek[t] == ki && srow[t] < ri)) ? 1 : 0;
    if (rank < w.k) {
      const uint64_t ord = ~ki;
      const uint64_t u = (ord >> 63) ? (ord & 0x7FFFFFFFFFFFFFFFull) : ~ord;
      os[rank] = (float)__builtin_bit_cast(double, u);
      oi[rank] = (int64_t)ri + w.id_offset;
    }
  }
  for (int i = m + threadIdx.x; i < w.k; i += kWideThreads) {
    os[i] = kPadScore;
    oi[i] = -1;
  }
  if (threadIdx.x == 0 && m == keff) w.status[orow] &= ~2;
}

// ---------------------------------------------------------------------------
// Large k (2048 < k <= kLargeMaxK; faiss IndexFlatIP answers any k, the reference's retrieve_num is a
// free flag: arguments.py:195, trainer.py:296-297).  The wide resolve's machinery with a threshold
// from outside: the caller passes tau_q <= the query's k-th fp32 score (the host takes the minimum of
// the m-th scores of C disjoint row ranges, C * m >= k), the filter collects every row with fp32
// score >= tau_q - 2 eps (it holds the exact top-k, see the bound above), wide_exact_kernel computes
// their exact sums, large_select_kernel finds the k-th (exact key, row) by the two radix selects and
// compacts the k selected entries, large_rank_kernel ranks each by counting within bins of the exact
// key (below).  Output: the canonical order (exact score desc, id asc), scores = exact sums rounded to
// fp32, rows past n padded like ip_topk; status 0, or 2 when the collected set overflowed kWideCap.
// ---------------------------------------------------------------------------
constexpr int32_t kLargeMaxK = 32768;
constexpr int kLargeThreads = 1024;

__global__ __launch_bounds__(kWideThreads) void large_select_kernel(WideArgs w) {
  __shared__ uint32_t hist[256];
  __shared__ uint64_t sh[2];
  __shared__ uint32_t ns;
  const int j = blockIdx.x;
  if (j >= w.nb) return;
  const uint32_t c = w.counts[j * kCntStride];
  if (c > (uint64_t)w.cap) {
    if (threadIdx.x == 0) w.sel_n[j] = 0xFFFFFFFFu;
    return;
  }
  const int64_t nh = c;
  const uint64_t* kj = w.keys + (int64_t)j * w.cap;
  const uint64_t* ej = w.ekeys + (int64_t)j * w.cap;
  const int64_t keff = std::min<int64_t>(w.k, nh);
  uint64_t kstar = 0, rstar = 0;
  if (keff > 0) {
    int64_t want = keff;
    kstar = wide_radix_select(nh, 64, [&](int64_t h, bool& take) { take = true; return ej[h]; }, hist, sh, want);
    const uint64_t ks = kstar;
    rstar = wide_radix_select(nh, 32, [&](int64_t h, bool& take) {
      take = ej[h] == ks;
      return (uint64_t)(uint32_t)kj[h];
    }, hist, sh, want);
  }
  if (threadIdx.x == 0) ns = 0u;
  __syncthreads();
  uint64_t* sk = w.sel_k + (int64_t)j * w.k;
  uint32_t* sr = w.sel_r + (int64_t)j * w.k;
  for (int64_t h = threadIdx.x; h < nh && keff > 0; h += kWideThreads) {
    const uint64_t ek = ej[h];
    const uint64_t row = (uint32_t)kj[h];
    if (ek < kstar || (ek == kstar && row <= rstar)) {
      const uint32_t pos = atomicAdd(&ns, 1u);
      if (pos < (uint32_t)keff) {
        sk[pos] = ek;
        sr[pos] = (uint32_t)row;
      }
    }
  }
  __syncthreads();
  if (threadIdx.x == 0) w.sel_n[j] = ns == (uint32_t)keff ? ns : 0xFFFFFFFFu;
}

// One work-group per query: rank = the number of selected entries before an entry in (exact key, row)
// order, counted within bins -- a histogram of the exact SCORES (decoded from the keys) over kLargeBins
// equal ranges between the set's max and min score (a monotone map: an entry's bin never exceeds a
// larger key's), the bins' exclusive prefix, the entries regrouped by bin, then each entry compared only
// with its own bin's.  Ties share a bin, so a set of many equal keys degrades towards the all-pairs count.
// (Round 6: the bins were equal ranges of the raw 64-bit key; a set whose scores cross zero or span
// several binades then crowded into a few bins -- the advisor's finding -- and the per-bin counts grew
// towards k^2.)
constexpr int kLargeBins = 4096;

__device__ __forceinline__ double large_key_score(uint64_t key) {   // inverse of desc_key64
  const uint64_t ord = ~key;
  const uint64_t u = (ord >> 63) ? (ord & 0x7FFFFFFFFFFFFFFFull) : ~ord;
  return __builtin_bit_cast(double, u);
}

__device__ __forceinline__ int large_bin(uint64_t key, double smax, double scale) {
  const double x = (smax - large_key_score(key)) * scale;   // >= 0, non-decreasing in the key
  const int b = x < (double)(kLargeBins - 1) ? (int)x : kLargeBins - 1;
  return b > 0 ? b : 0;
}

__global__ __launch_bounds__(kLargeThreads) void large_rank_kernel(WideArgs w) {
  __shared__ uint32_t start[kLargeBins];
  __shared__ uint32_t cursor[kLargeBins];
  __shared__ uint64_t red[2][kLargeThreads / 64];
  __shared__ uint32_t wsum[kLargeThreads / 64];
  const int j = blockIdx.x;
  if (j >= w.nb) return;
  const uint32_t m = w.sel_n[j];
  if (m == 0xFFFFFFFFu) return;   // overflow: status stays 2
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int64_t orow = wide_out_row(w, j);
  const uint64_t* sk = w.sel_k + (int64_t)j * w.k;
  const uint32_t* sr = w.sel_r + (int64_t)j * w.k;
  uint64_t* bk = w.bin_k + (int64_t)j * w.k;
  uint32_t* br = w.bin_r + (int64_t)j * w.k;
  // key range of the set
  uint64_t lo = ~0ull, hi = 0ull;
  for (uint32_t i = tid; i < m; i += kLargeThreads) {
    const uint64_t v = sk[i];
    lo = v < lo ? v : lo;
    hi = v > hi ? v : hi;
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const uint64_t a = __shfl_xor(lo, o, 64), b = __shfl_xor(hi, o, 64);
    lo = a < lo ? a : lo;
    hi = b > hi ? b : hi;
  }
  if (lane == 0) {
    red[0][wave] = lo;
    red[1][wave] = hi;
  }
  for (int b = tid; b < kLargeBins; b += kLargeThreads) start[b] = 0u;
  __syncthreads();
  lo = red[0][0];
  hi = red[1][0];
  for (int q = 1; q < kLargeThreads / 64; ++q) {
    lo = red[0][q] < lo ? red[0][q] : lo;
    hi = red[1][q] > hi ? red[1][q] : hi;
  }
  // lo / hi: the smallest / largest key = the best / worst score of the set
  const double smax = m ? large_key_score(lo) : 0.0, smin = m ? large_key_score(hi) : 0.0;
  const double range = smax - smin;
  const double scale = range > 0.0 ? (double)kLargeBins / (range * (1.0 + 1e-12)) : 0.0;
  // histogram, exclusive prefix (4 bins per thread, wave scan, wave totals)
  for (uint32_t i = tid; i < m; i += kLargeThreads) atomicAdd(&start[large_bin(sk[i], smax, scale)], 1u);
  __syncthreads();
  constexpr int kPer = kLargeBins / kLargeThreads;
  uint32_t c[kPer], tot = 0;
#pragma unroll
  for (int u = 0; u < kPer; ++u) {
    c[u] = start[tid * kPer + u];
    tot += c[u];
  }
  uint32_t inc = tot;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const uint32_t t = __shfl_up(inc, o, 64);
    if (lane >= o) inc += t;
  }
  if (lane == 63) wsum[wave] = inc;
  __syncthreads();
  uint32_t base = inc - tot;
  for (int q = 0; q < wave; ++q) base += wsum[q];
#pragma unroll
  for (int u = 0; u < kPer; ++u) {
    start[tid * kPer + u] = base;
    cursor[tid * kPer + u] = base;
    base += c[u];
  }
  __syncthreads();
  // regroup by bin (positions within a bin are arbitrary: the counts below do not depend on them)
  for (uint32_t i = tid; i < m; i += kLargeThreads) {
    const uint64_t v = sk[i];
    const uint32_t pos = atomicAdd(&cursor[large_bin(v, smax, scale)], 1u);
    bk[pos] = v;
    br[pos] = sr[i];
  }
  __syncthreads();
  float* os = w.out_s + orow * w.k;
  int64_t* oi = w.out_i + orow * w.k;
  for (uint32_t i = tid; i < m; i += kLargeThreads) {
    const uint64_t ki = sk[i];
    const uint32_t ri = sr[i];
    const int b = large_bin(ki, smax, scale);
    const uint32_t b0 = start[b], b1 = cursor[b];   // cursor = end of the bin after the regroup
    uint32_t rank = b0;
    for (uint32_t t = b0; t < b1; ++t) {
      const uint64_t kt = bk[t];
      rank += (kt < ki || (kt == ki && br[t] < ri)) ? 1u : 0u;
    }
    os[rank] = (float)large_key_score(ki);
    oi[rank] = (int64_t)ri + w.id_offset;
    if (w.out_keys) w.out_keys[orow * w.k + rank] = ki;
  }
  for (int64_t i = (int64_t)m + tid; i < w.k; i += kLargeThreads) {
    os[i] = kPadScore;
    oi[i] = -1;
    if (w.out_keys) w.out_keys[orow * w.k + i] = ~0ull;
  }
  if (tid == 0) w.status[orow] = 0;
}

// Merge of per-shard canonical lists by their EXACT order keys (a sharded index at k > 2048, round 6):
// keys / ids [nparts][nq][k], every list sorted by (exact key asc = exact score desc, global id asc),
// pads (~0, -1) last.  An entry's rank in the union = its index in its own list + the entries of every
// other list before it (one binary search each); the first k ranks are written (out pre-filled with pads
// by merge_exact_fill_kernel).  Global ids are unique, so the ranks of real entries are distinct.
constexpr int kMergeExactThreads = 256;
__global__ __launch_bounds__(kMergeExactThreads) void merge_exact_fill_kernel(int64_t n, float* os, int64_t* oi) {
  for (int64_t i = (int64_t)blockIdx.x * kMergeExactThreads + threadIdx.x; i < n;
       i += (int64_t)gridDim.x * kMergeExactThreads) {
    os[i] = kPadScore;
    oi[i] = -1;
  }
}

__global__ __launch_bounds__(kMergeExactThreads) void merge_exact_kernel(const uint64_t* keys, const int64_t* ids,
                                                                        int64_t nq, int nparts, int k, float* os,
                                                                        int64_t* oi) {
  const int64_t q = blockIdx.y;
  const int64_t e = (int64_t)blockIdx.x * kMergeExactThreads + threadIdx.x;
  if (e >= (int64_t)nparts * k) return;
  const int l = (int)(e / k), i = (int)(e % k);
  const int64_t base = ((int64_t)l * nq + q) * k;
  const uint64_t K = keys[base + i];
  if (K == ~0ull) return;
  const int64_t I = ids[base + i];
  int64_t rank = i;
  for (int l2 = 0; l2 < nparts && rank < k; ++l2) {
    if (l2 == l) continue;
    const uint64_t* k2 = keys + ((int64_t)l2 * nq + q) * k;
    const int64_t* i2 = ids + ((int64_t)l2 * nq + q) * k;
    int lo = 0, hi = k;   // entries of list l2 before (K, I)
    while (lo < hi) {
      const int mid = (lo + hi) >> 1;
      const uint64_t km = k2[mid];
      if (km < K || (km == K && i2[mid] < I)) lo = mid + 1;
      else hi = mid;
    }
    rank += lo;
  }
  if (rank < k) {
    os[q * k + rank] = (float)large_key_score(K);
    oi[q * k + rank] = I;
  }
}

// Row statistics for the refine bound (layout above kStatsLen).  One wave per row: lane L holds the
// 4-element chunks c = L + 64 i, whose squares a wave-wide inclusive scan turns into running prefix
// sums; the lane whose chunk ends k-step t (c = 8 t + 7, or the last chunk) keeps the max over its rows
// of the prefix through step t.  Non-negative floats are combined across work-groups by an integer max
// of their bits; the integer flag by AND of the bits of 1.0f / 0.0f.
__global__ __launch_bounds__(256) void row_stats_kernel(const __bf16* P, int64_t n, int32_t d, uint32_t* stats) {
  constexpr int kIt = 4;   // chunks per lane: d <= 1024
  __shared__ float fm[4][kStatBlocks];
  __shared__ int fi[4];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t gw = (int64_t)blockIdx.x * 4 + wave, nw = (int64_t)gridDim.x * 4;
  const int nch = d >> 2;
  float pm[kIt];
#pragma unroll
  for (int i = 0; i < kIt; ++i) pm[i] = 0.0f;
  int nonint = 0;
  for (int64_t r = gw; r < n; r += nw) {
    const __bf16* pr = P + r * (int64_t)d;
    float carry = 0.0f;
#pragma unroll
    for (int it = 0; it < kIt; ++it) {
      if (64 * it >= nch) break;   // wave-uniform
      const int c = lane + 64 * it;
      float ss = 0.0f;
      if (c < nch) {
        const bf16x4 x = *(const bf16x4*)(pr + 4 * c);
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          const float v = (float)x[u];
          ss += v * v;
          nonint |= (v != __builtin_rintf(v)) ? 1 : 0;
        }
      }
#pragma unroll
      for (int o = 1; o < 64; o <<= 1) {
        const float t = __shfl_up(ss, o, 64);
        if (lane >= o) ss += t;
      }
      const float v = carry + ss;
      pm[it] = fmaxf(pm[it], v);
      carry = __shfl(v, 63, 64);
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) nonint |= __shfl_xor(nonint, o, 64);
  const int nb = (d + 31) >> 5;
  for (int b = lane; b < kStatBlocks; b += 64) fm[wave][b] = 0.0f;
  if (lane == 0) fi[wave] = nonint;
  __syncthreads();
#pragma unroll
  for (int it = 0; it < kIt; ++it) {
    const int c = lane + 64 * it;
    if (c < nch && ((c & 7) == 7 || c == nch - 1)) fm[wave][c >> 3] = pm[it];
  }
  __syncthreads();
  if ((int)threadIdx.x < nb) {
    const int b = threadIdx.x;
    const float m = fmaxf(fmaxf(fm[0][b], fm[1][b]), fmaxf(fm[2][b], fm[3][b]));
    atomicMax(stats + 2 + b, __builtin_bit_cast(uint32_t, m));
    if (b == nb - 1) atomicMax(stats, __builtin_bit_cast(uint32_t, m));
  }
  if (threadIdx.x == 0 && (fi[0] | fi[1] | fi[2] | fi[3])) atomicAnd(stats + 1, 0u);
}

__global__ void row_stats_init_kernel(uint32_t* stats) {
  if (threadIdx.x < kStatsLen) stats[threadIdx.x] = threadIdx.x == 1 ? __builtin_bit_cast(uint32_t, 1.0f) : 0u;
}

// Host side.  The first three are what other units call (search_internal.h).
int launch_refine(RefineArgs& ra, hipStream_t s) {
  if (ra.nq == 0) return DRT_OK;
  const ProfPair pp = prof_begin(PROF_SELECT, s);
  hipLaunchKernelGGL(refine_prep_kernel, dim3((unsigned)ra.nq), dim3(kRefThreads), 0, s, ra);
  // the one-GPU entries (ip_topk, resolve): every candidate is this shard's
  launch_refine_local(ra, s);
  hipLaunchKernelGGL(refine_sort_kernel, dim3((unsigned)ra.nq), dim3(kRefSortThreads), 0, s, ra);
  prof_end(pp, s);
  return hip_status(hipGetLastError());
}

int flagged_queries(const int32_t* status, int64_t nq, int32_t mask, int32_t want, hipStream_t s,
                    std::vector<int32_t>& out) {
  std::vector<int32_t> st(nq);
  DRT_CHECK_HIP(hipMemcpyAsync(st.data(), status, nq * 4, hipMemcpyDeviceToHost, s));
  DRT_CHECK_HIP(hipStreamSynchronize(s));
  out.clear();
  for (int64_t i = 0; i < nq; ++i)
    if ((st[i] & mask) == want) out.push_back((int32_t)i);
  return DRT_OK;
}

int gather_queries(const void* Q, int32_t d, const int32_t* idx, int64_t nb, void* qbuf, void* qmap, hipStream_t s) {
  for (int64_t i = 0; i < nb; ++i)
    DRT_CHECK_HIP(hipMemcpyAsync((char*)qbuf + i * d * 2, (const char*)Q + (int64_t)idx[i] * d * 2, d * 2,
                                 hipMemcpyDeviceToDevice, s));
  DRT_CHECK_HIP(hipMemcpyAsync(qmap, idx, nb * 4, hipMemcpyHostToDevice, s));
  return DRT_OK;
}

// What the wide resolve and the large-k path fill alike: the problem, the outputs and the chunk buffers of
// the wide layout at `wp`.  The chunk's queries (ra.Q, nb) and their output rows (qmap, or q0) are the driver's.
static WideArgs wide_args(const WideLayout& l, char* wp, const void* P, int32_t d, int32_t k, int64_t id_offset,
                          const float* stats, float* out_scores, int64_t* out_ids, int32_t* status) {
  WideArgs w{};
  w.ra.d = d;
  w.ra.P = (const __bf16*)P;
  w.ra.stats = stats;
  w.k = k;
  w.tau = (float*)(wp + l.tau);
  w.counts = (uint32_t*)(wp + l.counts);
  w.keys = (const uint64_t*)(wp + l.keys);
  w.ekeys = (uint64_t*)(wp + l.ekeys);
  w.cap = kWideCap;
  w.id_offset = id_offset;
  w.out_s = out_scores;
  w.out_i = out_ids;
  w.status = status;
  return w;
}

// One chunk's collection: wide_prep_kernel (B = s_k - 2 eps, counters zeroed), the filter scan of the n rows at B
// into w.keys, wide_exact_kernel (their exact order keys).  n == 0 (only the large path gets here): prep alone.
static int launch_wide_collect(const WideArgs& w, int64_t n, hipStream_t s) {
  hipLaunchKernelGGL(wide_prep_kernel, dim3((unsigned)kQueriesPerWG), dim3(kRefThreads), 0, s, w);
  DRT_CHECK_HIP(hipGetLastError());
  if (n == 0) return DRT_OK;
  const ScanArgs a = filter_scan_args(w.ra.Q, w.nb, w.ra.P, w.ra.d, n, w.tau, w.counts, (void*)w.keys, w.cap);
  if (const int rc = launch_scan(a, w.ra.d, SCAN_FILTER, s, -1)) return rc;   // (not a headline filter launch)
  hipLaunchKernelGGL(wide_exact_kernel, dim3((unsigned)w.nb, (unsigned)(kWideCap / kWideSlice)), dim3(kRefThreads), 0,
                     s, w);
  return DRT_OK;
}

}  // namespace drt

using namespace drt;

extern "C" {

int drt_row_stats_bf16(const void* P, int64_t n, int32_t d, float* stats, int32_t accumulate, void* stream) {
  DRT_REQUIRE(n >= 0 && d > 0 && d % 4 == 0 && stats != nullptr);
  hipStream_t s = (hipStream_t)stream;
  DRT_REQUIRE(d <= 32 * kStatBlocks);
  if (!accumulate) hipLaunchKernelGGL(row_stats_init_kernel, dim3(1), dim3(64), 0, s, (uint32_t*)stats);
  if (n > 0) {
    DRT_REQUIRE(P != nullptr);
    const int64_t blocks = std::min<int64_t>((n + 3) / 4, 4096);
    hipLaunchKernelGGL(row_stats_kernel, dim3((unsigned)blocks), dim3(256), 0, s, (const __bf16*)P, n, d,
                       (uint32_t*)stats);
  }
  return hip_status(hipGetLastError());
}

int32_t drt_refine_width(int32_t k) {
  if (k < 1 || k > kSelMaxK) return -1;
  return (int32_t)refine_width(k);
}

static int refine_delta_impl(const void* Q, int64_t nq, int32_t d, const void* P, int64_t n_local, int64_t row_offset,
                             const float* cand_s, const int64_t* cand_i, int32_t kc, int32_t k, const float* stats,
                             const float* tau, float* delta, int32_t* cnt, int32_t* status, void* stream,
                             bool local) {
  DRT_REQUIRE(nq >= 0 && d > 0 && d % 64 == 0 && d <= 1024 && k >= 1 && kc >= k && kc <= kSelMaxK && n_local >= 0);
  if (nq == 0) return DRT_OK;
  DRT_REQUIRE(Q && cand_s && cand_i && stats && delta && cnt && (P || n_local == 0));
  RefineArgs ra{};
  ra.Q = (const __bf16*)Q;
  ra.nq = nq;
  ra.d = d;
  ra.P = (const __bf16*)P;
  ra.n_local = n_local;
  ra.row_offset = row_offset;
  ra.cs = cand_s;
  ra.ci = cand_i;
  ra.kc = kc;
  ra.k = k;
  ra.stats = stats;
  ra.tau = tau;
  ra.delta = delta;
  ra.cnt = cnt;
  ra.status = status;
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(refine_prep_kernel, dim3((unsigned)nq), dim3(kRefThreads), 0, s, ra);
  if (local) {   // one shard holds every candidate: waves walk the window directly (no compaction)
    launch_refine_local(ra, s);
  } else {
    ra.slice = kRefSliceShard;   // the sharded protocol's entry: most candidates live on other shards
    hipLaunchKernelGGL(refine_delta_kernel, dim3((unsigned)nq, (unsigned)((kc + ra.slice - 1) / ra.slice)),
                       dim3(kRefThreads), 0, s, ra);
  }
  return hip_status(hipGetLastError());
}

int drt_refine_delta_bf16(const void* Q, int64_t nq, int32_t d, const void* P, int64_t n_local, int64_t row_offset,
                          const float* cand_s, const int64_t* cand_i, int32_t kc, int32_t k, const float* stats,
                          const float* tau, float* delta, int32_t* cnt, int32_t* status, void* stream) {
  return refine_delta_impl(Q, nq, d, P, n_local, row_offset, cand_s, cand_i, kc, k, stats, tau, delta, cnt, status,
                           stream, false);
}

int drt_refine_delta_local_bf16(const void* Q, int64_t nq, int32_t d, const void* P, int64_t n_local,
                                int64_t row_offset, const float* cand_s, const int64_t* cand_i, int32_t kc, int32_t k,
                                const float* stats, const float* tau, float* delta, int32_t* cnt, int32_t* status,
                                void* stream) {
  return refine_delta_impl(Q, nq, d, P, n_local, row_offset, cand_s, cand_i, kc, k, stats, tau, delta, cnt, status,
                           stream, true);
}

int drt_refine_sort(const float* cand_s, const int64_t* cand_i, const float* delta, const int32_t* cnt, int64_t nq,
                    int32_t kc, int32_t k, float* out_scores, int64_t* out_ids, void* stream) {
  DRT_REQUIRE(nq >= 0 && k >= 1 && kc >= k && kc <= kSelMaxK);
  if (nq == 0) return DRT_OK;
  DRT_REQUIRE(cand_s && cand_i && delta && cnt && out_scores && out_ids);
  RefineArgs ra{};
  ra.nq = nq;
  ra.cs = cand_s;
  ra.ci = cand_i;
  ra.kc = kc;
  ra.k = k;
  ra.delta = (float*)delta;
  ra.cnt = (int32_t*)cnt;
  ra.out_s = out_scores;
  ra.out_i = out_ids;
  hipLaunchKernelGGL(refine_sort_kernel, dim3((unsigned)nq), dim3(kRefSortThreads), 0, (hipStream_t)stream, ra);
  return hip_status(hipGetLastError());
}

size_t drt_ip_topk_resolve_wide_workspace(int64_t n, int32_t d) {
  if (n < 0 || d <= 0 || d % 64 || d > 1024) return 0;
  return wide_layout(d).total;
}

int drt_ip_topk_resolve_wide(const void* Q, int64_t nq, const void* P, int64_t n, int32_t d, int32_t k,
                             int64_t id_offset, const float* stats, float* out_scores, int64_t* out_ids,
                             int32_t* status, void* ws, size_t ws_bytes, int64_t* n_resolved, void* stream) {
  DRT_REQUIRE(valid_dims(nq, n, d, k));
  if (n_resolved) *n_resolved = 0;
  if (nq == 0 || n == 0) return DRT_OK;
  const WideLayout l = wide_layout(d);
  DRT_REQUIRE(Q && P && stats && out_scores && out_ids && status && ws && ws_bytes >= l.total);
  hipStream_t s = (hipStream_t)stream;
  std::vector<int32_t> wide;   // order not certified and the fp32 top-k itself certified: status exactly 2
  int rc = flagged_queries(status, nq, 3, 2, s, wide);
  if (rc || wide.empty()) return rc;
  const int64_t B = kQueriesPerWG;
  char* wp = (char*)ws;
  WideArgs w = wide_args(l, wp, P, d, k, id_offset, stats, out_scores, out_ids, status);
  w.ra.Q = (const __bf16*)(wp + l.qbuf);
  w.qmap = (const int32_t*)(wp + l.qmap);
  for (size_t b0 = 0; b0 < wide.size(); b0 += B) {
    w.nb = (int)std::min<int64_t>(B, (int64_t)wide.size() - (int64_t)b0);
    if ((rc = gather_queries(Q, d, wide.data() + b0, w.nb, wp + l.qbuf, wp + l.qmap, s))) return rc;
    if ((rc = launch_wide_collect(w, n, s))) return rc;
    hipLaunchKernelGGL(wide_select_kernel, dim3((unsigned)w.nb), dim3(kWideThreads), 0, s, w);
    DRT_CHECK_HIP(hipGetLastError());
  }
  std::vector<int32_t> left;   // still exactly 2 (only these queries were touched): their sets overflowed the cap
  if ((rc = flagged_queries(status, nq, 3, 2, s, left))) return rc;
  if (n_resolved) *n_resolved = (int64_t)wide.size() - (int64_t)left.size();
  return DRT_OK;
}

size_t drt_ip_topk_large_workspace(int32_t d, int32_t k) {
  if (d <= 0 || d % 64 || d > 1024 || k < 1 || k > kLargeMaxK) return 0;
  return large_layout(d, k).total;
}

int drt_ip_topk_large(const void* Q, int64_t nq, const void* P, int64_t n, int32_t d, int32_t k, int64_t id_offset,
                      const float* stats, const float* tau, float* out_scores, int64_t* out_ids, int32_t* status,
                      void* ws, size_t ws_bytes, void* stream) {
  return drt_ip_topk_large_keys(Q, nq, P, n, d, k, id_offset, stats, tau, out_scores, out_ids, nullptr, status, ws,
                                ws_bytes, stream);
}

int drt_ip_topk_large_keys(const void* Q, int64_t nq, const void* P, int64_t n, int32_t d, int32_t k,
                           int64_t id_offset, const float* stats, const float* tau, float* out_scores,
                           int64_t* out_ids, uint64_t* out_keys, int32_t* status, void* ws, size_t ws_bytes,
                           void* stream) {
  DRT_REQUIRE(nq >= 0 && n >= 0 && n < (int64_t)0xFFFFFFFFll && drt_ip_topk_large_workspace(d, k) > 0);
  if (nq == 0) return DRT_OK;
  const LargeLayout l = large_layout(d, k);
  DRT_REQUIRE(Q && (P || n == 0) && stats && tau && out_scores && out_ids && status && ws && ws_bytes >= l.total);
  hipStream_t s = (hipStream_t)stream;
  const int64_t B = kQueriesPerWG;
  char* wp = (char*)ws;
  WideArgs w = wide_args(l.wide, wp, P, d, k, id_offset, stats, out_scores, out_ids, status);
  w.tau_in = tau;   // (qmap stays null: the queries are read in place, chunk query j -> output row q0 + j)
  w.sel_k = (uint64_t*)(wp + l.sel_k);
  w.sel_r = (uint32_t*)(wp + l.sel_r);
  w.sel_n = (uint32_t*)(wp + l.sel_n);
  w.bin_k = (uint64_t*)(wp + l.bin_k);
  w.bin_r = (uint32_t*)(wp + l.bin_r);
  w.out_keys = out_keys;
  for (int64_t b0 = 0; b0 < nq; b0 += B) {
    w.ra.Q = (const __bf16*)Q + b0 * d;
    w.q0 = b0;
    w.nb = (int)std::min<int64_t>(B, nq - b0);
    if (const int rc = launch_wide_collect(w, n, s)) return rc;
    hipLaunchKernelGGL(large_select_kernel, dim3((unsigned)w.nb), dim3(kWideThreads), 0, s, w);
    hipLaunchKernelGGL(large_rank_kernel, dim3((unsigned)w.nb), dim3(kLargeThreads), 0, s, w);
    DRT_CHECK_HIP(hipGetLastError());
  }
  return DRT_OK;
}

int drt_merge_exact(const uint64_t* keys, const int64_t* ids, int64_t nq, int32_t nparts, int32_t k,
                    float* out_scores, int64_t* out_ids, void* stream) {
  DRT_REQUIRE(nq >= 0 && nparts >= 1 && nparts <= 1024 && k >= 1 && k <= kLargeMaxK);
  if (nq == 0) return DRT_OK;
  DRT_REQUIRE(nq <= 65535 && keys && ids && out_scores && out_ids);
  hipStream_t s = (hipStream_t)stream;
  const int64_t n = nq * (int64_t)k;
  hipLaunchKernelGGL(merge_exact_fill_kernel, dim3((unsigned)std::min<int64_t>((n + 255) / 256, 4096)),
                     dim3(kMergeExactThreads), 0, s, n, out_scores, out_ids);
  const int64_t ents = (int64_t)nparts * k;
  hipLaunchKernelGGL(merge_exact_kernel, dim3((unsigned)((ents + kMergeExactThreads - 1) / kMergeExactThreads),
                                              (unsigned)nq),
                     dim3(kMergeExactThreads), 0, s, keys, ids, nq, (int)nparts, (int)k, out_scores, out_ids);
  return hip_status(hipGetLastError());
}

}  // extern "C"
