// Per-query selection and thresholds of the top-k search (search.hip steps 1 and 3).
//
//   select_kernel       the k best keys of a query's hit list (KEYS64) or dense score row (DENSE32),
//                       sorted by (score desc, row asc), with the certification status; KTH: a threshold.
//   kth_rank_kernel     the sample threshold in one launch: the r-th best key of a dense sample row.
//   kth_partial_kernel, kth_final_kernel   the same for larger samples, and the r-th best of the union
//                       of gathered lists (the distributed threshold).
//   tighten_kernel      the raised threshold after the first of a shard's interleaved filter passes.
// The kernels are launched only here: launch_select and one launcher per threshold kernel, at the end
// of the file, are what search.hip calls (search_internal.h).
#include "profile.h"
#include "search_internal.h"

namespace drt {

// ---------------------------------------------------------------------------
// Per-query selection.
//
// Fast path (every realistic input): one block per query,
//   A  min/max of the scores,
//   B  1024-bin histogram LINEAR IN THE SCORE VALUE (per-wave sub-histograms,
//      so a dense score range does not serialise on a few LDS bins),
//   C  suffix scan -> highest bin b with >= k elements at or above it,
//   D  TOPK: gather every key in bins >= b into LDS (<= 4096 of them),
//      bitonic sort on the 64-bit key (score desc, row asc), emit k;
//      KTH:  tau = min score among bins >= b  (<= the k-th largest: safe).
// Bin membership is one monotone float formula used by every pass, so the
// selected set is always an upper set of the scores (ties stay together).
// Fallback (degenerate data, e.g. >4096 equal scores): MSD radix select on
// the full 64-bit key, 8 bits per pass, then the same sort.
// ---------------------------------------------------------------------------
constexpr int kSelThreads = 512;
constexpr int kSelWaves = kSelThreads / 64;
constexpr int kSelBins = 1024;
constexpr int kSelBuf = 4096;
constexpr int kSelKPT = 16;                          // keys per thread held in registers
constexpr int kSelRegCap = kSelKPT * kSelThreads;    // 8192

template <int INPUT>
__device__ __forceinline__ uint64_t sel_load(const SelectArgs& a, int64_t q, int64_t j) {
  if (INPUT == SEL_KEYS64) return ((const uint64_t*)a.in)[q * a.in_stride + j];
  const uint32_t v = ((const uint32_t*)a.in)[q * a.in_stride + j];
  return ((uint64_t)v << 32) | (uint64_t)(uint32_t)j;
}

__device__ __forceinline__ float key_score(uint64_t x) { return desc_key_to_score((uint32_t)(x >> 32)); }

// bin kSelBins - 1 = best scores
__device__ __forceinline__ int score_bin(float s, float smin, float scale) {
  if (scale == 0.0f) return 0;
  return hist_bin((s - smin) * scale, kSelBins, __builtin_signbit(s) ? 0 : kSelBins - 1);
}

template <typename T, typename Op>
__device__ __forceinline__ T block_reduce(T v, T* scratch, Op op) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = op(v, __shfl_xor(v, o, 64));
  const int w = threadIdx.x >> 6;
  __syncthreads();
  if ((threadIdx.x & 63) == 0) scratch[w] = v;
  __syncthreads();
  T r = scratch[0];
#pragma unroll
  for (int i = 1; i < kSelWaves; ++i) r = op(r, scratch[i]);
  return r;
}

// Block-wide bitonic sort of buf[0..n) ascending (n a power of two, n <= 8 * NT).
// The keys live in registers (element u * NT + tid in v[u]); a compare-exchange
// at stride s runs in-thread (s >= NT), through LDS (64 <= s < NT: two
// barriers) or as a cross-lane shuffle (s < 64, no barrier), so most of the
// log2(n) * (log2(n) + 1) / 2 stages cost no block synchronisation.  Slots past
// n hold the maximum key (they sort last and are never written back).
template <typename T, int NT, int E, int US>
__device__ __forceinline__ void sort_inthread(T (&v)[E], int size, int tid) {
#pragma unroll
  for (int u = 0; u < E; ++u) {
    if ((u & US) == 0 && (u | US) < E) {
      const int i = u * NT + tid;
      const bool up = (i & size) == 0;
      const T a = v[u], b = v[u | US];
      v[u] = up ? (a < b ? a : b) : (a < b ? b : a);
      v[u | US] = up ? (a < b ? b : a) : (a < b ? a : b);
    }
  }
}

template <typename T, int NT, int N>
__device__ __forceinline__ void block_sort_fixed(T* buf, int n) {
  constexpr int E = N / NT;
  const int tid = threadIdx.x;
  const T kMax = ~(T)0;
  T v[E];
#pragma unroll
  for (int u = 0; u < E; ++u) {
    const int i = u * NT + tid;
    v[u] = i < n ? buf[i] : kMax;
  }
  __syncthreads();
#pragma unroll
  for (int size = 2; size <= N; size <<= 1) {
#pragma unroll
    for (int stride = size >> 1; stride > 0; stride >>= 1) {
      if (stride >= NT) {
        if (E >= 2 && stride == NT) sort_inthread<T, NT, E, 1>(v, size, tid);
        else if (E >= 4 && stride == 2 * NT) sort_inthread<T, NT, E, 2>(v, size, tid);
        else if (E >= 8) sort_inthread<T, NT, E, 4>(v, size, tid);
      } else {
        T p[E];
        if (stride >= 64) {
#pragma unroll
          for (int u = 0; u < E; ++u) buf[u * NT + tid] = v[u];
          __syncthreads();
#pragma unroll
          for (int u = 0; u < E; ++u) p[u] = buf[(u * NT + tid) ^ stride];
          __syncthreads();
        } else {
#pragma unroll
          for (int u = 0; u < E; ++u) p[u] = __shfl_xor(v[u], stride, 64);
        }
#pragma unroll
        for (int u = 0; u < E; ++u) {
          const int i = u * NT + tid;
          const bool keep_min = ((i & stride) == 0) == ((i & size) == 0);
          const T a = v[u], b = p[u];
          v[u] = keep_min ? (a < b ? a : b) : (a < b ? b : a);
        }
      }
    }
  }
#pragma unroll
  for (int u = 0; u < E; ++u) {
    const int i = u * NT + tid;
    if (i < n) buf[i] = v[u];
  }
  __syncthreads();
}

template <typename T, int NT>
__device__ __forceinline__ void block_sort(T* buf, int n) {
  if (n <= 1) {
    __syncthreads();
    return;
  }
  if (n <= NT) block_sort_fixed<T, NT, NT>(buf, n);
  else if (n <= 2 * NT) block_sort_fixed<T, NT, 2 * NT>(buf, n);
  else if (n <= 4 * NT) block_sort_fixed<T, NT, 4 * NT>(buf, n);
  else block_sort_fixed<T, NT, 8 * NT>(buf, n);
}

// Bitonic sort of buf[0..n2) ascending (n2 power of two, <= kSelBuf), whole block.
__device__ __forceinline__ void block_bitonic(uint64_t* buf, int n2) { block_sort<uint64_t, kSelThreads>(buf, n2); }

template <int INPUT, int OUTPUT>
__global__ __launch_bounds__(kSelThreads) void select_kernel(SelectArgs a) {
  __shared__ uint32_t hist[kSelWaves][kSelBins];
  __shared__ uint32_t suffix[kSelBins];
  __shared__ float fscr[kSelWaves];
  __shared__ uint64_t uscr[kSelWaves];
  __shared__ uint64_t sh_prefix, sh_mask;
  __shared__ int64_t sh_kk;
  __shared__ int sh_done, sh_bin;
  __shared__ uint32_t sh_nsel, sh_nside;
  __shared__ __attribute__((aligned(16))) uint64_t buf[kSelBuf];

  const int tid = threadIdx.x;
  const int wave = tid >> 6;
  const int64_t q = blockIdx.x;
  int64_t c_raw, c;
  if (INPUT == SEL_KEYS64) {
    c_raw = a.counts[q * kCntStride];
    c = c_raw < a.cap ? c_raw : a.cap;
  } else {
    c_raw = a.n_in;
    c = a.n_in;
  }
  const int64_t kk_total = (int64_t)a.k < c ? (int64_t)a.k : c;

  if (OUTPUT == SEL_KTH && (c < (int64_t)a.k || c == 0)) {
    if (tid == 0) a.tau[q] = -__builtin_inff();  // too few samples: keep everything
    return;
  }

  bool fast_done = false;   // uniform
  int nsel = 0;             // TOPK: entries in buf
  if (c > (int64_t)a.k && c <= kSelRegCap) {
    // every key loaded once (all loads in flight together), passes run on registers
    uint64_t kr[kSelKPT];
    float sc[kSelKPT];
#pragma unroll
    for (int u = 0; u < kSelKPT; ++u) {
      const int64_t j = (int64_t)u * kSelThreads + tid;
      const uint64_t x = sel_load<INPUT>(a, q, j < c ? j : 0);   // clamped: loads issue back to back
      kr[u] = j < c ? x : ~0ull;
    }
    float lo = __builtin_inff(), hi = -__builtin_inff();
#pragma unroll
    for (int u = 0; u < kSelKPT; ++u) {
      sc[u] = key_score(kr[u]);
      if ((int64_t)u * kSelThreads + tid < c) {
        lo = fminf(lo, sc[u]);
        hi = fmaxf(hi, sc[u]);
      }
    }
    lo = block_reduce(lo, fscr, [](float x, float y) { return fminf(x, y); });
    hi = block_reduce(hi, fscr, [](float x, float y) { return fmaxf(x, y); });
    const float range = hi - lo;
    const float scale = hist_scale((float)kSelBins, range);
    for (int i = tid; i < kSelWaves * kSelBins; i += kSelThreads) (&hist[0][0])[i] = 0;
    __syncthreads();
    int bn[kSelKPT];
#pragma unroll
    for (int u = 0; u < kSelKPT; ++u) {
      bn[u] = -1;
      if ((int64_t)u * kSelThreads + tid < c) {
        bn[u] = score_bin(sc[u], lo, scale);
        atomicAdd(&hist[wave][bn[u]], 1u);
      }
    }
    __syncthreads();
    for (int i = tid; i < kSelBins; i += kSelThreads) {
      uint32_t t = 0;
#pragma unroll
      for (int w = 0; w < kSelWaves; ++w) t += hist[w][i];
      suffix[i] = t;
    }
    __syncthreads();
    for (int off = 1; off < kSelBins; off <<= 1) {
      uint32_t v[kSelBins / kSelThreads];
#pragma unroll
      for (int u = 0; u < kSelBins / kSelThreads; ++u) {
        const int i = tid + u * kSelThreads;
        v[u] = suffix[i] + (i + off < kSelBins ? suffix[i + off] : 0u);
      }
      __syncthreads();
#pragma unroll
      for (int u = 0; u < kSelBins / kSelThreads; ++u) suffix[tid + u * kSelThreads] = v[u];
      __syncthreads();
    }
    if (tid == 0) sh_bin = 0;
    __syncthreads();
    for (int i = tid; i < kSelBins; i += kSelThreads) {
      const bool ok = (int64_t)suffix[i] >= kk_total;
      const bool next_ok = (i + 1 < kSelBins) && (int64_t)suffix[i + 1] >= kk_total;
      if (ok && !next_ok) sh_bin = i;
    }
    __syncthreads();
    const int b = sh_bin;
    if (OUTPUT == SEL_KTH) {
      float t = __builtin_inff();
#pragma unroll
      for (int u = 0; u < kSelKPT; ++u)
        if (bn[u] >= b) t = fminf(t, sc[u]);
      t = block_reduce(t, fscr, [](float x, float y) { return fminf(x, y); });
      if (tid == 0) a.tau[q] = t;
      return;
    }
    const uint32_t cnt_sel = suffix[b];
    const uint32_t c_above = (b + 1 < kSelBins) ? suffix[b + 1] : 0u;
    const uint32_t cnt_b = cnt_sel - c_above;
    if (cnt_b <= (uint32_t)(kSelBuf / 2) && kk_total <= kSelBuf / 2) {
      uint64_t* side = buf + kSelBuf / 2;
      if (tid == 0) {
        sh_nsel = 0;
        sh_nside = 0;
      }
      __syncthreads();
#pragma unroll
      for (int u = 0; u < kSelKPT; ++u) {
        if (bn[u] > b) buf[atomicAdd(&sh_nsel, 1u)] = kr[u];
        else if (bn[u] == b) side[atomicAdd(&sh_nside, 1u)] = kr[u];
      }
      __syncthreads();
      const int ns = (int)sh_nside;
      int m2 = 1;
      while (m2 < ns) m2 <<= 1;
      for (int i = ns + tid; i < m2; i += kSelThreads) side[i] = ~0ull;
      __syncthreads();
      block_bitonic(side, m2);
      const int need = (int)kk_total - (int)c_above;
      for (int i = tid; i < need; i += kSelThreads) buf[c_above + i] = side[i];
      __syncthreads();
      nsel = (int)kk_total;
      fast_done = true;
    } else if (cnt_sel <= (uint32_t)kSelBuf) {
      if (tid == 0) sh_nsel = 0;
      __syncthreads();
#pragma unroll
      for (int u = 0; u < kSelKPT; ++u)
        if (bn[u] >= b) buf[atomicAdd(&sh_nsel, 1u)] = kr[u];
      __syncthreads();
      nsel = (int)sh_nsel;
      fast_done = true;
    }
  } else if (c > (int64_t)a.k) {
    // ---- A: score range
    float lo = __builtin_inff(), hi = -__builtin_inff();
    for (int64_t j = tid; j < c; j += kSelThreads) {
      const float s = key_score(sel_load<INPUT>(a, q, j));
      lo = fminf(lo, s);
      hi = fmaxf(hi, s);
    }
    lo = block_reduce(lo, fscr, [](float x, float y) { return fminf(x, y); });
    hi = block_reduce(hi, fscr, [](float x, float y) { return fmaxf(x, y); });
    const float range = hi - lo;
    const float scale = hist_scale((float)kSelBins, range);
    // ---- B: per-wave histograms
    for (int i = tid; i < kSelWaves * kSelBins; i += kSelThreads) (&hist[0][0])[i] = 0;
    __syncthreads();
    for (int64_t j = tid; j < c; j += kSelThreads) {
      const float s = key_score(sel_load<INPUT>(a, q, j));
      atomicAdd(&hist[wave][score_bin(s, lo, scale)], 1u);
    }
    __syncthreads();
    for (int i = tid; i < kSelBins; i += kSelThreads) {
      uint32_t t = 0;
#pragma unroll
      for (int w = 0; w < kSelWaves; ++w) t += hist[w][i];
      suffix[i] = t;
    }
    __syncthreads();
    // ---- C: inclusive suffix sum (Hillis-Steele over 1024 bins)
    for (int off = 1; off < kSelBins; off <<= 1) {
      uint32_t v[kSelBins / kSelThreads];
#pragma unroll
      for (int u = 0; u < kSelBins / kSelThreads; ++u) {
        const int i = tid + u * kSelThreads;
        v[u] = suffix[i] + (i + off < kSelBins ? suffix[i + off] : 0u);
      }
      __syncthreads();
#pragma unroll
      for (int u = 0; u < kSelBins / kSelThreads; ++u) suffix[tid + u * kSelThreads] = v[u];
      __syncthreads();
    }
    // highest bin b with suffix[b] >= kk_total (suffix is non-increasing in b)
    if (tid == 0) sh_bin = 0;
    __syncthreads();
    for (int i = tid; i < kSelBins; i += kSelThreads) {
      const bool ok = (int64_t)suffix[i] >= kk_total;
      const bool next_ok = (i + 1 < kSelBins) && (int64_t)suffix[i + 1] >= kk_total;
      if (ok && !next_ok) sh_bin = i;
    }
    __syncthreads();
    const int b = sh_bin;
    const uint32_t cnt_sel = suffix[b];
    if (OUTPUT == SEL_KTH) {
      // ---- D(KTH): tau = min score in bins >= b  (a lower bound of the k-th largest)
      float t = __builtin_inff();
      for (int64_t j = tid; j < c; j += kSelThreads) {
        const float s = key_score(sel_load<INPUT>(a, q, j));
        if (score_bin(s, lo, scale) >= b) t = fminf(t, s);
      }
      t = block_reduce(t, fscr, [](float x, float y) { return fminf(x, y); });
      if (tid == 0) a.tau[q] = t;
      return;
    }
    const uint32_t c_above = (b + 1 < kSelBins) ? suffix[b + 1] : 0u;   // bins above b: all selected
    const uint32_t cnt_b = cnt_sel - c_above;                             // boundary bin
    if (cnt_b <= (uint32_t)(kSelBuf / 2) && kk_total <= kSelBuf / 2) {
      // ---- D(TOPK): bins > b straight into buf[0, c_above); the boundary bin
      // into buf[kSelBuf/2, ...), sorted alone, its best (kk - c_above) appended:
      // exactly kk keys reach the final sort.
      uint64_t* side = buf + kSelBuf / 2;
      if (tid == 0) {
        sh_nsel = 0;
        sh_nside = 0;
      }
      __syncthreads();
      for (int64_t j = tid; j < c; j += kSelThreads) {
        const uint64_t x = sel_load<INPUT>(a, q, j);
        const int bx = score_bin(key_score(x), lo, scale);
        if (bx > b) buf[atomicAdd(&sh_nsel, 1u)] = x;
        else if (bx == b) side[atomicAdd(&sh_nside, 1u)] = x;
      }
      __syncthreads();
      const int ns = (int)sh_nside;
      int m2 = 1;
      while (m2 < ns) m2 <<= 1;
      for (int i = ns + tid; i < m2; i += kSelThreads) side[i] = ~0ull;
      __syncthreads();
      block_bitonic(side, m2);
      const int need = (int)kk_total - (int)c_above;
      for (int i = tid; i < need; i += kSelThreads) buf[c_above + i] = side[i];
      __syncthreads();
      nsel = (int)kk_total;
      fast_done = true;
    } else if (cnt_sel <= (uint32_t)kSelBuf) {
      // ---- D(TOPK): gather the whole upper set, sort, emit
      if (tid == 0) sh_nsel = 0;
      __syncthreads();
      for (int64_t j = tid; j < c; j += kSelThreads) {
        const uint64_t x = sel_load<INPUT>(a, q, j);
        if (score_bin(key_score(x), lo, scale) >= b) {
          const uint32_t p = atomicAdd(&sh_nsel, 1u);
          if (p < (uint32_t)kSelBuf) buf[p] = x;
        }
      }
      __syncthreads();
      nsel = (int)sh_nsel;
      fast_done = true;
    }
  }

  if (!fast_done) {
    // ---- fallback / small input: MSD radix select on 64-bit keys
    if (tid == 0) {
      sh_prefix = 0;
      sh_mask = 0;
      sh_kk = kk_total;
      sh_done = (c <= (int64_t)a.k) ? 1 : 0;  // everything selected
      if (c <= (int64_t)a.k) {
        sh_prefix = ~0ull;
        sh_mask = ~0ull;
      }
    }
    __syncthreads();
    uint32_t* h0 = &hist[0][0];
    for (int shift = 56; shift >= 0 && !sh_done; shift -= 8) {
      for (int i = tid; i < 256; i += kSelThreads) h0[i] = 0;
      __syncthreads();
      const uint64_t prefix = sh_prefix, mask = sh_mask;
      for (int64_t j = tid; j < c; j += kSelThreads) {
        const uint64_t x = sel_load<INPUT>(a, q, j);
        if ((x & mask) == prefix) atomicAdd(&h0[(x >> shift) & 255], 1u);
      }
      __syncthreads();
      if (tid < 64) {
        const uint32_t b0 = h0[4 * tid], b1 = h0[4 * tid + 1], b2 = h0[4 * tid + 2], b3 = h0[4 * tid + 3];
        const uint32_t s4 = b0 + b1 + b2 + b3;
        uint32_t incl = s4;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
          const uint32_t v = __shfl_up(incl, o, 64);
          if (tid >= o) incl += v;
        }
        const uint32_t excl = incl - s4;
        const int64_t kk = sh_kk;
        if ((int64_t)excl < kk && kk <= (int64_t)incl) {
          uint32_t run = excl;
          const uint32_t bb[4] = {b0, b1, b2, b3};
          int d = 0;
          uint32_t cnt = 0;
#pragma unroll
          for (int t = 0; t < 4; ++t) {
            if ((int64_t)(run + bb[t]) >= kk) {
              d = 4 * tid + t;
              cnt = bb[t];
              break;
            }
            run += bb[t];
          }
          const int64_t rem = kk - run;
          sh_prefix = prefix | ((uint64_t)d << shift);
          sh_mask = mask | (255ull << shift);
          sh_kk = rem;
          if ((int64_t)cnt == rem) sh_done = 1;  // whole bucket selected
        }
      }
      __syncthreads();
    }
    const uint64_t thr = sh_prefix | ~sh_mask;  // every key whose masked value <= prefix
    if (tid == 0) sh_nsel = 0;
    __syncthreads();
    for (int64_t j = tid; j < c; j += kSelThreads) {
      const uint64_t x = sel_load<INPUT>(a, q, j);
      if (x <= thr) {
        const uint32_t p = atomicAdd(&sh_nsel, 1u);
        if (p < (uint32_t)kSelBuf) buf[p] = x;
      }
    }
    __syncthreads();
    nsel = (int)sh_nsel;
  }

  nsel = nsel < kSelBuf ? nsel : kSelBuf;
  int n2 = 1;
  while (n2 < nsel) n2 <<= 1;
  for (int i = nsel + tid; i < n2; i += kSelThreads) buf[i] = ~0ull;
  __syncthreads();
  block_bitonic(buf, n2);

  const int64_t orow = a.qmap ? (int64_t)a.qmap[q] : q;
  if (a.out_packed) {
    uint64_t* op = a.out_packed + orow * (int64_t)(a.k + 1);
    for (int j = tid; j < a.k; j += kSelThreads) {
      if (j < kk_total) {
        const uint64_t x = buf[j];
        op[j] = (x & 0xFFFFFFFF00000000ull) | (uint64_t)(uint32_t)(a.id_offset + (int64_t)(x & 0xFFFFFFFFull));
      } else {
        op[j] = ~0ull;
      }
    }
    if (tid == 0) {
      const uint64_t nval = (uint64_t)(kk_total < a.k ? kk_total : a.k);
      // bit 0: overflow (more hits than the list buffer held); bit 1: truncated (more hits than the k
      // entries written -- what a merge of capped exchange lists certifies against, round 6)
      bool bad = INPUT == SEL_KEYS64 && c_raw > a.cap;
      if (INPUT == SEL_KEYS64 && a.pass0) {
        const uint32_t* t = a.pass0 + q * 4;
        if (t[2] && (int64_t)t[1] + (c_raw - (int64_t)t[0]) < (int64_t)a.k) bad = true;
      }
      op[a.k] = (nval << 32) | (bad ? 1ull : 0ull) | (c_raw > (int64_t)a.k ? 2ull : 0ull);
    }
    return;
  }
  float* os = a.out_scores + orow * a.ldo;
  int64_t* oi = a.out_ids + orow * a.ldo;
  for (int j = tid; j < a.k; j += kSelThreads) {
    if (j < kk_total) {
      const uint64_t x = buf[j];
      os[j] = key_score(x);
      oi[j] = a.id_offset + (int64_t)(x & 0xFFFFFFFFull);
    } else {
      os[j] = kPadScore;
      oi[j] = -1;
    }
  }
  if (a.status && tid == 0) {
    int st = 0;
    if (INPUT == SEL_KEYS64) {
      if (c_raw > a.cap) st = 1;                                                       // overflow
      const int64_t kq = a.k_cert > 0 ? a.k_cert : a.k;
      if (!a.global_tau && c_raw < kq && c_raw < a.n_total) st = 1;                    // threshold too high
    }
    a.status[orow] = st;
  }
}

// ---------------------------------------------------------------------------
// Tightened threshold after the first of a shard's interleaved filter passes
// (drt_ip_topk_filter_passes): tau1[q] = the score of the r-th best key the first pass
// collected (exactly: MSD radix select on the 32-bit score key, 8 bits per step) when it
// collected c0 >= r of them, else tau0[q] (also for an inactive query, tau0 = NaN, and for a
// list that overflowed `cap`).  pass0[q] = {c0, r_eff = first-pass keys scoring >= tau1 (ties
// count), tau1 > tau0, 0}: what the final select certifies the list with (SelectArgs::pass0).
// One block per query; the list (~cap / 4 / passes keys) is read from L2 five times.
// ---------------------------------------------------------------------------
constexpr int kTightThreads = 256;

__global__ __launch_bounds__(kTightThreads) void tighten_kernel(const uint64_t* keys, int64_t cap,
                                                                const uint32_t* counts, const float* tau0, int r,
                                                                float* tau1, uint32_t* pass0) {
  __shared__ uint32_t hist[256];
  __shared__ uint32_t sh_prefix, sh_rem;
  __shared__ uint32_t red[kTightThreads / 64];
  const int tid = threadIdx.x;
  const int64_t q = blockIdx.x;
  const uint32_t c = counts[q * kCntStride];
  const float t0 = tau0[q];
  if (!((int64_t)c <= cap && c >= (uint32_t)r && t0 == t0)) {
    if (tid == 0) {
      tau1[q] = t0;
      pass0[q * 4 + 0] = c;
      pass0[q * 4 + 1] = c;
      pass0[q * 4 + 2] = 0;
      pass0[q * 4 + 3] = 0;
    }
    return;
  }
  const uint64_t* kq = keys + q * cap;
  uint32_t prefix = 0, mask = 0, rem = (uint32_t)r;   // the rem-th smallest key among those matching prefix
  for (int shift = 24; shift >= 0; shift -= 8) {
    hist[tid] = 0;
    __syncthreads();
    for (uint32_t j = tid; j < c; j += kTightThreads) {
      const uint32_t key = (uint32_t)(kq[j] >> 32);
      if ((key & mask) == prefix) atomicAdd(&hist[(key >> shift) & 255], 1u);
    }
    __syncthreads();
    if (tid < 64) {
      const uint32_t bb[4] = {hist[4 * tid], hist[4 * tid + 1], hist[4 * tid + 2], hist[4 * tid + 3]};
      const uint32_t s4 = bb[0] + bb[1] + bb[2] + bb[3];
      uint32_t incl = s4;
#pragma unroll
      for (int o = 1; o < 64; o <<= 1) {
        const uint32_t v = __shfl_up(incl, o, 64);
        if (tid >= o) incl += v;
      }
      uint32_t run = incl - s4;
      if (run < rem && rem <= incl) {   // exactly one lane: at least rem keys match the prefix
        int dgt = 4 * tid;
#pragma unroll
        for (int t = 0; t < 3; ++t) {
          if (dgt == 4 * tid + t && run + bb[t] < rem) {
            run += bb[t];
            ++dgt;
          }
        }
        sh_prefix = prefix | ((uint32_t)dgt << shift);
        sh_rem = rem - run;
      }
    }
    __syncthreads();
    prefix = sh_prefix;
    rem = sh_rem;
    mask |= 255u << shift;
  }
  const float t1 = desc_key_to_score(prefix);
  uint32_t n = 0;
  for (uint32_t j = tid; j < c; j += kTightThreads) n += key_score(kq[j]) >= t1 ? 1u : 0u;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) n += __shfl_xor(n, o, 64);
  if ((tid & 63) == 0) red[tid >> 6] = n;
  __syncthreads();
  if (tid == 0) {
    uint32_t tot = 0;
    for (int w = 0; w < kTightThreads / 64; ++w) tot += red[w];
    tau1[q] = t1;
    pass0[q * 4 + 0] = c;
    pass0[q * 4 + 1] = tot;
    pass0[q * 4 + 2] = t1 > t0 ? 1u : 0u;
    pass0[q * 4 + 3] = 0;
  }
}

// ---------------------------------------------------------------------------
// Sample threshold: tau_q = score of the r-th best sampled key.
// kth_partial: grid (chunks, nq); each block LDS-sorts one 4096-key chunk of
//              the dense sample row and keeps its best r keys.
// kth_final:   grid nq; sorts the chunks' survivors (<= 4096), picks the r-th.
// Padding keys are 0xFFFFFFFF (sort last, never chosen ahead of real keys).
// ---------------------------------------------------------------------------
constexpr int kKthThreads = 512;

__device__ __forceinline__ void block_bitonic_u32(uint32_t* buf, int n2) { block_sort<uint32_t, kKthThreads>(buf, n2); }

// Best r keys of one 4096-key chunk.  Keys live in registers (8 per thread);
// a 256-bin histogram linear in the score value (per-wave sub-histograms)
// finds the bin holding rank r, only the keys in the bins up to it (~r + a
// few) are gathered and sorted.  Degenerate chunks (> 1024 keys tied around
// rank r) fall back to sorting the whole chunk.
constexpr int kKthPer = kKthChunk / kKthThreads;   // 8 keys per thread
constexpr int kKthBins = 256;
constexpr int kKthSel = 1024;

__global__ __launch_bounds__(kKthThreads) void kth_partial_kernel(const uint32_t* in, int64_t stride, int64_t n,
                                                                  int r, uint32_t* part) {
  __shared__ __attribute__((aligned(16))) uint32_t buf[kKthChunk];
  __shared__ uint32_t hist[kKthThreads / 64][kKthBins];
  __shared__ float red[2][kKthThreads / 64];
  __shared__ uint32_t sh_n;
  __shared__ int sh_bin;
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int64_t q = blockIdx.y;
  const int nchunk = gridDim.x;
  const int64_t j0 = (int64_t)blockIdx.x * kKthChunk;
  const int cnt = (int)(n - j0 < kKthChunk ? n - j0 : kKthChunk);
  const uint32_t* src = in + q * stride + j0;

  uint32_t key[kKthPer];
  // thread t holds keys 4t..4t+3 and 2048+4t..2048+4t+3 (two coalesced 16-B loads)
#pragma unroll
  for (int v = 0; v < 2; ++v) {
    const int base = v * (kKthChunk / 2) + 4 * tid;
    if (base + 3 < cnt) {
      const u32x4 x = *(const u32x4*)(src + base);
#pragma unroll
      for (int u = 0; u < 4; ++u) key[4 * v + u] = x[u];
    } else {
#pragma unroll
      for (int u = 0; u < 4; ++u) key[4 * v + u] = base + u < cnt ? src[base + u] : 0xFFFFFFFFu;
    }
  }
  // score range over real keys
  float hi = -__builtin_inff(), lo = __builtin_inff();
#pragma unroll
  for (int e = 0; e < kKthPer; ++e) {
    if (key[e] != 0xFFFFFFFFu) {
      const float sc = desc_key_to_score(key[e]);
      hi = fmaxf(hi, sc);
      lo = fminf(lo, sc);
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    hi = fmaxf(hi, __shfl_xor(hi, o, 64));
    lo = fminf(lo, __shfl_xor(lo, o, 64));
  }
  if (lane == 0) {
    red[0][wave] = hi;
    red[1][wave] = lo;
  }
  for (int i = tid; i < (kKthThreads / 64) * kKthBins; i += kKthThreads) (&hist[0][0])[i] = 0;
  __syncthreads();
#pragma unroll
  for (int w = 0; w < kKthThreads / 64; ++w) {
    hi = fmaxf(hi, red[0][w]);
    lo = fminf(lo, red[1][w]);
  }
  const float range = hi - lo;
  const float scale = hist_scale((float)kKthBins, range);
  // bin 0 = best scores
  int bins[kKthPer];
#pragma unroll
  for (int e = 0; e < kKthPer; ++e) {
    int bb = kKthBins;  // padding
    if (key[e] != 0xFFFFFFFFu) {
      const float sc = desc_key_to_score(key[e]);
      bb = scale == 0.0f ? 0 : hist_bin((hi - sc) * scale, kKthBins, __builtin_signbit(sc) ? kKthBins - 1 : 0);
      atomicAdd(&hist[wave][bb], 1u);
    }
    bins[e] = bb;
  }
  __syncthreads();
  if (tid < 64) {
    uint32_t c4[4];
    uint32_t s4 = 0;
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      uint32_t v = 0;
#pragma unroll
      for (int w = 0; w < kKthThreads / 64; ++w) v += hist[w][4 * tid + t];
      c4[t] = v;
      s4 += v;
    }
    uint32_t incl = s4;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const uint32_t v = __shfl_up(incl, o, 64);
      if (tid >= o) incl += v;
    }
    uint32_t run = incl - s4;
    if (tid == 63 && incl < (uint32_t)r) sh_bin = kKthBins - 1;  // fewer than r real keys: take all
    if (run < (uint32_t)r && (uint32_t)r <= incl) {
#pragma unroll
      for (int t = 0; t < 4; ++t) {
        if (run + c4[t] >= (uint32_t)r) {
          sh_bin = 4 * tid + t;
          break;
        }
        run += c4[t];
      }
    }
  }
  if (tid == 0) sh_n = 0;
  __syncthreads();
  const int b = sh_bin;
  // gather keys of bins <= b
#pragma unroll
  for (int e = 0; e < kKthPer; ++e) {
    if (bins[e] <= b) {
      const uint32_t pos = atomicAdd(&sh_n, 1u);
      if (pos < (uint32_t)kKthSel) buf[pos] = key[e];
    }
  }
  __syncthreads();
  int nsel = (int)sh_n;
  if (nsel > kKthSel) {
    // degenerate: sort the whole chunk
    __syncthreads();
#pragma unroll
    for (int v = 0; v < 2; ++v)
#pragma unroll
      for (int u = 0; u < 4; ++u) buf[v * (kKthChunk / 2) + 4 * tid + u] = key[4 * v + u];
    nsel = kKthChunk;
  }
  int n2 = 1;
  while (n2 < nsel) n2 <<= 1;
  for (int i = nsel + tid; i < n2; i += kKthThreads) buf[i] = 0xFFFFFFFFu;
  __syncthreads();
  block_bitonic_u32(buf, n2);
  uint32_t* o = part + (q * nchunk + blockIdx.x) * r;
  for (int i = tid; i < r; i += kKthThreads) o[i] = i < nsel ? buf[i] : 0xFFFFFFFFu;
}

// Element i of list l for query q lives at part[l * lstride + q * qstride + i], i < r.
// Writes tau[q] (r-th best score; -inf if fewer than r real keys) and/or the
// sorted best r keys best[q * r + i]; zero (optional): zero[q] = 0 (the filter's hit
// counters, so the fused distributed filter needs no separate memset launch).
__global__ __launch_bounds__(kKthThreads) void kth_final_kernel(const uint32_t* part, int nlists, int r,
                                                                int64_t lstride, int64_t qstride, float* tau,
                                                                uint32_t* best, uint32_t* zero, int len) {
  __shared__ uint32_t buf[kKthChunk];
  const int64_t q = blockIdx.x;
  if (zero && threadIdx.x == 0) zero[q * kCntStride] = 0;
  const int tot = nlists * len;   // nlists lists of len keys each (len = r: best-r lists)
  {
    uint32_t tmp[kKthChunk / kKthThreads];
#pragma unroll
    for (int u = 0; u < kKthChunk / kKthThreads; ++u) {
      const int i = threadIdx.x + u * kKthThreads;
      const int ic = i < tot ? i : 0;
      const uint32_t x = part[(int64_t)(ic / len) * lstride + q * qstride + (ic % len)];
      tmp[u] = i < tot ? x : 0xFFFFFFFFu;
    }
#pragma unroll
    for (int u = 0; u < kKthChunk / kKthThreads; ++u) buf[threadIdx.x + u * kKthThreads] = tmp[u];
  }
  __syncthreads();
  int n2 = 1;
  while (n2 < tot) n2 <<= 1;
  block_bitonic_u32(buf, n2);
  if (tau && threadIdx.x == 0) {
    const uint32_t kr = buf[r - 1];
    tau[q] = (kr == 0xFFFFFFFFu) ? -__builtin_inff() : desc_key_to_score(kr);
  }
  if (best)
    for (int i = threadIdx.x; i < r; i += kKthThreads) best[q * r + i] = buf[i];
}

// Sample threshold in ONE launch (one-GPU search, samples up to kRankThreads * kRankPer keys --
// 70,801 at 10M rows and k = 1000): one 1024-thread work-group per query holds the whole sample
// row in registers; round 4: the r-th best of the 1024 per-thread best keys bounds the answer, so only
// those 1024 keys go through the 1024-bin histogram (not every sampled key: 70k LDS atomics per query,
// mostly on the crowded middle bins), the keys no worse than that bound (~r of them) are sorted in
// LDS and tau = the r-th best -- the same key kth_partial + kth_final pick (both exact), without the
// chunk pass, its survivor lists and the second launch.  More than kRankBuf candidates (ties / a
// degenerate score range) fall back to an exact MSD radix select over the candidates.  Also zeroes
// the hit counter.
constexpr int kRankThreads = 1024;
constexpr int kRankPerMax = 80;   // keys per thread (register-resident); smaller samples take 8 / 24
constexpr int kRankBins = 1024;
constexpr int kRankBuf = 2048;
constexpr int64_t kRankMaxKeys = (int64_t)kRankThreads * kRankPerMax;

template <int kRankPer>
__global__ __launch_bounds__(kRankThreads) void kth_rank_kernel(const uint32_t* in, int64_t stride, int64_t n, int r,
                                                                float* tau, uint32_t* zero) {
  __shared__ uint32_t hist[kRankBins];
  __shared__ __attribute__((aligned(16))) uint32_t buf[kRankBuf];
  __shared__ float red[2][kRankThreads / 64];
  __shared__ uint32_t wsum[kRankThreads / 64];
  __shared__ uint32_t sh_n, sh_rem, sh_prefix;
  __shared__ int sh_bin;
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int64_t q = blockIdx.x;
  if (zero && tid == 0) zero[q * kCntStride] = 0;
  const uint32_t* src = in + q * stride;
  constexpr uint32_t kPad = 0xFFFFFFFFu;
  // thread t holds keys j * 4096 + 4t + [0, 4), j < kRankPer / 4 (coalesced 16-B loads; stride % 4 == 0)
  uint32_t key[kRankPer];
#pragma unroll
  for (int j = 0; j < kRankPer / 4; ++j) {
    const int64_t base = (int64_t)j * (4 * kRankThreads) + 4 * tid;
    if (base + 3 < n) {
      const u32x4 x = *(const u32x4*)(src + base);
#pragma unroll
      for (int u = 0; u < 4; ++u) key[4 * j + u] = x[u];
    } else {
#pragma unroll
      for (int u = 0; u < 4; ++u) key[4 * j + u] = base + u < n ? src[base + u] : kPad;
    }
  }
  // Candidates without a histogram of every key: the r best of the 1024 per-thread best keys are r
  // distinct keys, so the r-th best key overall is no worse than the r-th best thread-best, K_r.
  // A 1024-bin histogram of the thread-bests (1024 LDS atomics instead of one per sampled key)
  // brackets K_r by bin b; T = the worst thread-best in bins <= b (>= K_r); every key <= T is a
  // candidate -- the r best keys are among them, typically with few others (the thread-bests of
  // those bins plus the rare second top key of one thread).
  uint32_t best = kPad;
#pragma unroll
  for (int e = 0; e < kRankPer; ++e) best = key[e] < best ? key[e] : best;   // kPad = the largest key
  float hi = -__builtin_inff(), lo = __builtin_inff();
  if (best != kPad) {
    const float sc = desc_key_to_score(best);
    hi = sc;
    lo = sc;
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    hi = fmaxf(hi, __shfl_xor(hi, o, 64));
    lo = fminf(lo, __shfl_xor(lo, o, 64));
  }
  if (lane == 0) {
    red[0][wave] = hi;
    red[1][wave] = lo;
  }
  hist[tid] = 0;
  __syncthreads();
#pragma unroll
  for (int w = 0; w < kRankThreads / 64; ++w) {
    hi = fmaxf(hi, red[0][w]);
    lo = fminf(lo, red[1][w]);
  }
  const float range = hi - lo;
  const float scale = hist_scale((float)kRankBins, range);
  // bin 0 = best scores; monotone in the key
  auto bin_of = [&](uint32_t kk) {
    if (scale == 0.0f) return 0;
    const float sc = desc_key_to_score(kk);
    return hist_bin((hi - sc) * scale, kRankBins, __builtin_signbit(sc) ? kRankBins - 1 : 0);
  };
  if (best != kPad) atomicAdd(&hist[bin_of(best)], 1u);
  __syncthreads();
  {
    const uint32_t v = hist[tid];
    uint32_t incl = v;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const uint32_t t = __shfl_up(incl, o, 64);
      if (lane >= o) incl += t;
    }
    if (lane == 63) wsum[wave] = incl;
    if (tid == 0) {
      sh_n = 0;
      sh_prefix = 0;   // T below (max over the selected thread-bests)
    }
    __syncthreads();
    uint32_t off = 0;
    for (int w = 0; w < wave; ++w) off += wsum[w];
    incl += off;
    const uint32_t excl = incl - v;
    if (excl < (uint32_t)r && (uint32_t)r <= incl) sh_bin = tid;
    // fewer than r thread-bests: every real key is a candidate
    if (tid == kRankThreads - 1 && incl < (uint32_t)r) sh_bin = -1;
  }
  __syncthreads();
  const int b = sh_bin;
  if (b >= 0) {
    // T = the worst (largest) thread-best key in bins <= b
    uint32_t t = (best != kPad && bin_of(best) <= b) ? best : 0u;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      const uint32_t u = __shfl_xor(t, o, 64);
      t = u > t ? u : t;
    }
    if (lane == 0) atomicMax(&sh_prefix, t);
  }
  __syncthreads();
  const uint32_t T = b >= 0 ? sh_prefix : kPad - 1u;
  __syncthreads();
#pragma unroll
  for (int e = 0; e < kRankPer; ++e) {
    if (key[e] <= T) {
      const uint32_t pos = atomicAdd(&sh_n, 1u);
      if (pos < (uint32_t)kRankBuf) buf[pos] = key[e];
    }
  }
  __syncthreads();
  const int nsel = (int)sh_n;
  uint32_t kth;
  if (nsel <= kRankBuf) {
    int n2 = 1;
    while (n2 < nsel) n2 <<= 1;
    for (int i = nsel + tid; i < n2; i += kRankThreads) buf[i] = kPad;
    __syncthreads();
    block_sort<uint32_t, kRankThreads>(buf, n2);
    kth = r <= nsel ? buf[r - 1] : kPad;
  } else {
    // exact MSD radix select (8 bits per pass) of the r-th smallest candidate key
    if (tid == 0) {
      sh_rem = (uint32_t)r;
      sh_prefix = 0;
    }
    uint32_t mask = 0;
    for (int shift = 24; shift >= 0; shift -= 8) {
      if (tid < 256) hist[tid] = 0;
      __syncthreads();
      const uint32_t prefix = sh_prefix;
#pragma unroll
      for (int e = 0; e < kRankPer; ++e)
        if (key[e] <= T && (key[e] & mask) == prefix)
          atomicAdd(&hist[(key[e] >> shift) & 255u], 1u);
      __syncthreads();
      if (tid == 0) {
        uint32_t rem = sh_rem, dgt = 255;
        for (uint32_t dd = 0; dd < 256; ++dd) {
          if (hist[dd] >= rem) {
            dgt = dd;
            break;
          }
          rem -= hist[dd];
        }
        sh_rem = rem;
        sh_prefix = prefix | (dgt << shift);
      }
      mask |= 255u << shift;
      __syncthreads();
    }
    kth = sh_prefix;
  }
  if (tau && tid == 0) tau[q] = (kth == kPad) ? -__builtin_inff() : desc_key_to_score(kth);
}

// ---------------------------------------------------------------------------
// Host launchers (declared in search_internal.h).
// ---------------------------------------------------------------------------
int launch_select(const SelectArgs& a, int input, int output, hipStream_t s) {
  if (a.nq == 0) return DRT_OK;
  dim3 grid((unsigned)a.nq);
  const ProfPair pp = prof_begin(PROF_SELECT, s);
  struct End { const ProfPair& p; hipStream_t s; ~End() { prof_end(p, s); } } end_{pp, s};
  if (input == SEL_KEYS64 && output == SEL_TOPK)
    hipLaunchKernelGGL((select_kernel<SEL_KEYS64, SEL_TOPK>), grid, dim3(kSelThreads), 0, s, a);
  else if (input == SEL_DENSE32 && output == SEL_TOPK)
    hipLaunchKernelGGL((select_kernel<SEL_DENSE32, SEL_TOPK>), grid, dim3(kSelThreads), 0, s, a);
  else if (input == SEL_DENSE32 && output == SEL_KTH)
    hipLaunchKernelGGL((select_kernel<SEL_DENSE32, SEL_KTH>), grid, dim3(kSelThreads), 0, s, a);
  else
    return DRT_EINVAL;
  return hip_status(hipGetLastError());
}

bool kth_rank_fits(int64_t m, int64_t r) { return m <= kRankMaxKeys && r <= kRankBuf; }

// keys per thread sized to the sample (a sample of ~7k keys at 1M rows needs 8, not 80)
void launch_kth_rank(int64_t nq, const uint32_t* in, int64_t stride, int64_t n, int r, float* tau, uint32_t* zero,
                     hipStream_t s) {
  const dim3 grid((unsigned)nq), block(kRankThreads);
  if (n <= (int64_t)kRankThreads * 8)
    hipLaunchKernelGGL(kth_rank_kernel<8>, grid, block, 0, s, in, stride, n, r, tau, zero);
  else if (n <= (int64_t)kRankThreads * 24)
    hipLaunchKernelGGL(kth_rank_kernel<24>, grid, block, 0, s, in, stride, n, r, tau, zero);
  else
    hipLaunchKernelGGL(kth_rank_kernel<kRankPerMax>, grid, block, 0, s, in, stride, n, r, tau, zero);
}

void launch_kth_partial(int64_t nchunk, int64_t nq, const uint32_t* in, int64_t stride, int64_t n, int r,
                        uint32_t* part, hipStream_t s) {
  hipLaunchKernelGGL(kth_partial_kernel, dim3((unsigned)nchunk, (unsigned)nq), dim3(kKthThreads), 0, s, in, stride, n,
                     r, part);
}

void launch_kth_final(int64_t nq, const uint32_t* part, int nlists, int r, int64_t lstride, int64_t qstride,
                      float* tau, uint32_t* best, uint32_t* zero, int len, hipStream_t s) {
  hipLaunchKernelGGL(kth_final_kernel, dim3((unsigned)nq), dim3(kKthThreads), 0, s, part, nlists, r, lstride, qstride,
                     tau, best, zero, len);
}

void launch_tighten(int64_t nq, const uint64_t* keys, int64_t cap, const uint32_t* counts, const float* tau0, int r,
                    float* tau1, uint32_t* pass0, hipStream_t s) {
  hipLaunchKernelGGL(tighten_kernel, dim3((unsigned)nq), dim3(kTightThreads), 0, s, keys, cap, counts, tau0, r, tau1,
                     pass0);
}

}  // namespace drt
