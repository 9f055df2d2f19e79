// Brute-force inner-product top-k over a device-resident corpus shard.
//
// Replaces faiss.IndexFlatIP.search as called by
// BaseFaissIPRetriever.search (DRT/evaluator/index.py:31-33) and the
// filesystem shard exchange of Trainer._index_corpus/_load_index
// (DRT/trainer/trainer.py:220-262).  Algorithm:
//
//   1. sample pass   a strided sample of the shard's rows -> per-query threshold
//                    tau_q = the r-th largest sampled score (a lower bound of
//                    the k-th score with probability 1 - 1e-9; certified in
//                    step 4).  One shard: ip_scan16_kernel<DENSE> writes every
//                    sampled score, kth_rank / kth_partial + kth_final pick
//                    the r-th.  Distributed and grouped (drt_ip_topk_dist_sample):
//                    ip_scan16_kernel<TOPR> keeps each lane's best keys in
//                    registers and kth_final takes the r-th of their union.
//   2. filter pass   streams every shard row once from HBM through LDS
//                    (global_load_lds into a ring of 16-row tiles; at d = 768
//                    5 slots, 6 in ip_scan32r), scores 16 rows x 16 queries per
//                    v_mfma_f32_16x16x32_bf16 (queries resident in VGPRs for
//                    the whole launch) and appends (score, row) keys >= tau_q
//                    to a per-query list.  Kernels (launch_scan_d picks):
//                    ip_scan16r_kernel, 16 queries per wave, the next tile's
//                    fragment reads rolled into this tile's MFMAs (a launch of
//                    up to 128 queries, d <= 768); ip_scan32r_kernel, 32 per
//                    wave (more than 128 queries: a group of batches, whose
//                    query blocks share each tile through L2);
//                    ip_scan16_kernel<FILTER> for d > 768 or strided rows.
//                    A group's filter over a large shard is several launches
//                    into ONE hit list: row chunks
//                    (drt_ip_topk_dist_filter_chunks) or interleaved passes,
//                    tighten_kernel raising the threshold after the first
//                    (drt_ip_topk_filter_passes).
//   3. select        select<KEYS64,TOPK> per query: MSD radix select on the
//                    64-bit key (score desc, row asc) + LDS bitonic sort.
//   4. certify       count_q >= k (or == n) and count_q <= cap  <=> exact.
//                    Otherwise status[q] = 1 and drt_ip_topk_resolve rescans
//                    that query densely (exact by construction).
//   5. canonical order (with row statistics): the refine kernels re-rank each
//                    query's near-tie window by exact scores.
// "Filter scan", "Canonical order", "One-GPU groups in row
// chunks", "One-GPU groups as interleaved passes with a tightened threshold",
// "Multi-GPU: global-threshold protocol".  The select, kth_* and tighten kernels
// of steps 1-3 live in select.hip and are reached through the launchers declared
// in search_internal.h (device code is not relocatable: a kernel is launched only
// from the unit that defines it).  The host side -- plans, the scan launcher, the
// C entry points -- starts at "Host-side planning and launch helpers"; the five
// filter entry points share the filter_* helpers above drt_ip_topk_dist_filter.
#include <algorithm>
#include <cmath>
#include <vector>

#include "profile.h"
#include "search_internal.h"

namespace drt {

constexpr int kHitCap = 1024;       // LDS hit list entries per work-group
enum { SCAN_FILTER = 0, SCAN_DENSE = 1, SCAN_TOPR = 2 };
// SCAN_TOPR (the grouped sample pass, round 6): instead of writing every sampled score, each lane keeps
// the kTopRL best keys of its query over the rows it sees (its 4 rows of every tile of its work-group)
// in registers and writes that list once; the union of a query's lists (4 per work-group column) holds
// every sampled key that beats all but kTopRL - 1 of its list-mates, so its r-th best is the r-th best
// sampled key unless more than kTopRL of the r best fell into one lane's share (then a slightly lower
// threshold: more filter hits, never a wrong result -- the filter's counts certify).  Round 5 wrote a
// [2048, 70.8k] u32 score matrix per group (580 MB) for kth_partial to read back.
constexpr int kTopRL = 4;

struct ScanArgs {
  const __bf16* Q;
  int64_t nq;
  int64_t ldq;
  const __bf16* P;
  int64_t ldp;      // elements between consecutive corpus rows
  int64_t row0;     // logical row i lives at P row (row0 + i * rstride)
  int64_t nrows;
  int64_t rstride;
  const float* tau;   // FILTER: [nq] thresholds (NaN = inactive query)
  uint32_t* counts;   // FILTER: hit counter of query q at counts[q * kCntStride] (zeroed by the caller)
  void* out;          // FILTER: u64 [nq][cap] keys; DENSE: u32 [nq][cap] desc keys
  int64_t cap;
  int64_t exp_hits;   // FILTER: expected hits per query (0: cap / 4); picks the append flavour
  uint32_t row_base;  // FILTER (lean kernels): added to the row of every hit key (a chunk of a longer shard)
  // FILTER (lean kernels): an interleaved pass over the shard -- the launch covers the 16-row tiles t with
  // t % npass == pass (npass <= 1: every tile); nrows stays the shard's row count, hit rows are shard rows
  int32_t npass;
  int32_t pass;
};

// The tiles of an interleaved pass (ScanArgs::npass / pass) out of a shard's `ntiles`.
__host__ __device__ __forceinline__ int pass_tiles(int ntiles, int npass, int pass) {
  return npass <= 1 ? ntiles : (pass < ntiles ? (ntiles - 1 - pass) / npass + 1 : 0);
}

// LDS-DMA of 16 B per lane.  Issued through inline asm on purpose: with the
// builtin, hipcc cannot prove the ring slots disjoint and waits vmcnt(0)
// before the first ds_read of every tile, which drains the prefetch ring.
// The asm form is invisible to hipcc's counters, so the kernel counts its
// own LDS-DMA with s_waitcnt vmcnt(N) (cdna_hip_programming.md §5.7 item 1).
__device__ __forceinline__ void glds16(const void* gsrc, uint32_t lds_addr) {
  uint32_t keep;
  asm volatile(
      "s_mov_b32 %0, m0\n\t"
      "s_mov_b32 m0, %2\n\t"
      "s_nop 0\n\t"
      "global_load_lds_dwordx4 %1, off\n\t"
      "s_mov_b32 m0, %0"
      : "=&s"(keep)
      : "v"(gsrc), "s"(lds_addr)
      : "memory");
}

// The same with the non-temporal policy (the corpus stream is read once per launch).
__device__ __forceinline__ void glds16_nt(const void* gsrc, uint32_t lds_addr) {
  uint32_t keep;
  asm volatile(
      "s_mov_b32 %0, m0\n\t"
      "s_mov_b32 m0, %2\n\t"
      "s_nop 0\n\t"
      "global_load_lds_dwordx4 %1, off nt\n\t"
      "s_mov_b32 m0, %0"
      : "=&s"(keep)
      : "v"(gsrc), "s"(lds_addr)
      : "memory");
}

__device__ __forceinline__ uint32_t lds_addr_of(const void* p) {
  return (uint32_t)(uintptr_t)(const __attribute__((address_space(3))) char*)p;
}

template <int N>
__device__ __forceinline__ void wait_vmcnt() {
  asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N) : "memory");
}

__device__ __forceinline__ void lds_barrier() {
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  __builtin_amdgcn_s_barrier();
}

// Push one filtered hit: LDS list first, direct global append when full.
__device__ __forceinline__ void push_hit(const ScanArgs& a, int q_local,
                                         int64_t q, uint64_t key, uint32_t* hit_n,
                                         uint64_t* hk, uint16_t* hq) {
  const uint32_t p = atomicAdd(hit_n, 1u);
  if (p < (uint32_t)kHitCap) {
    hk[p] = key;
    hq[p] = (uint16_t)q_local;
  } else {
    const uint32_t g = atomicAdd(a.counts + q * kCntStride, 1u);
    if (g < (uint64_t)a.cap) ((uint64_t*)a.out)[q * a.cap + g] = key;
  }
}

// Flush with one global atomic per (work-group, query): LDS counting by query,
// then per-query reservation, then scatter.  qcnt/qoff: 128-entry LDS scratch.
template <int NT>
__device__ __forceinline__ void flush_hits_agg(const ScanArgs& a, int64_t qbase, uint32_t n, const uint64_t* hk,
                                               const uint16_t* hq, uint32_t* qcnt, uint32_t* qoff) {
  n = n < (uint32_t)kHitCap ? n : (uint32_t)kHitCap;
  for (int i = threadIdx.x; i < kQueriesPerWG; i += NT) qcnt[i] = 0;
  lds_barrier();
  uint32_t rank[(kHitCap + NT - 1) / NT];
#pragma unroll
  for (int u = 0; u < (kHitCap + NT - 1) / NT; ++u) {
    const uint32_t i = threadIdx.x + u * NT;
    if (i < n) rank[u] = atomicAdd(&qcnt[hq[i]], 1u);
  }
  lds_barrier();
  for (int q = threadIdx.x; q < kQueriesPerWG; q += NT) {
    const uint32_t c = qcnt[q];
    qoff[q] = (c && qbase + q < a.nq) ? atomicAdd(a.counts + (qbase + q) * kCntStride, c) : 0u;
  }
  lds_barrier();
#pragma unroll
  for (int u = 0; u < (kHitCap + NT - 1) / NT; ++u) {
    const uint32_t i = threadIdx.x + u * NT;
    if (i < n) {
      const int ql = hq[i];
      const uint32_t g = qoff[ql] + rank[u];
      if (g < (uint64_t)a.cap) ((uint64_t*)a.out)[(qbase + ql) * a.cap + g] = hk[i];
    }
  }
}

template <int NT>
__device__ __forceinline__ void flush_hits(const ScanArgs& a, int64_t qbase, uint32_t n,
                                           const uint64_t* hk, const uint16_t* hq) {
  n = n < (uint32_t)kHitCap ? n : (uint32_t)kHitCap;
  for (uint32_t i = threadIdx.x; i < n; i += NT) {
    const int64_t q = qbase + hq[i];
    const uint32_t g = atomicAdd(a.counts + q * kCntStride, 1u);
    if (g < (uint64_t)a.cap) ((uint64_t*)a.out)[q * a.cap + g] = hk[i];
  }
}

// ---------------------------------------------------------------------------
// Production scan: 16-row tiles on v_mfma_f32_16x16x32_bf16, 5-slot LDS ring at d = 768
// (4 x 24 KiB in flight per CU while the waves compute; ip_scan16r keeps all 5 slots in flight).
//   B operand (queries, VGPR-resident): lane l holds Q[q0 + 16 b + (l&15)]
//     [32 s + 8 (l>>4) .. +8] for column block b = 0, 1 and k-step s.
//   A operand (corpus, LDS): lane l reads row (l&15), 16-B chunk 4 s + (l>>4).
//   D: lane l holds query (l&15) of block b, rows 4 (l>>4) + 0..3.
// LDS image per tile: [chunk group g][row 0..15][8 x 16 B], chunk position
// XOR (row >> 1) & 7 -> conflict-free ds_read_b128 (all 4 lane groups).
// ---------------------------------------------------------------------------
constexpr int kT16 = 16;

template <int D, int NW>
struct Scan16Cfg {
  static constexpr int KS = D / 32;                         // 16x16x32 k-steps
  static constexpr int TILE_BYTES = kT16 * D * 2;            // 24 KiB at d = 768
  static constexpr int GLDS_PER_TILE = TILE_BYTES / 1024;
  // every wave issues the same count (vmcnt bookkeeping); the remainder
  // instructions are duplicates of earlier ones (same bytes, same LDS address)
  static constexpr int GLDS_PER_WAVE = (GLDS_PER_TILE + NW - 1) / NW;   // 3 at d = 768 (8 waves)
  static constexpr int HITS_BYTES = kHitCap * 10 + 16 + 2 * kQueriesPerWG * 4;
  static constexpr int NBUF_RAW = (160 * 1024 - HITS_BYTES) / TILE_BYTES;
  // at d = 768 a 5-slot ring (4 tiles = 96 KiB in flight per CU) beat 6 slots in three alternating A/B
  // pairs on one box: 2.654-2.665 vs 2.687-2.704 ms per 10M launch (round 4, profiles/r04am_*)
  static constexpr int NBUF_CAP = TILE_BYTES >= 24 * 1024 ? 5 : 8;
  static constexpr int NBUF = NBUF_RAW > NBUF_CAP ? NBUF_CAP : NBUF_RAW;
  static constexpr int PD = NBUF - 1;
  static constexpr int RING_BYTES = NBUF * TILE_BYTES;
  static constexpr int HIT_KEY_OFF = RING_BYTES;
  static constexpr int HIT_Q_OFF = HIT_KEY_OFF + kHitCap * 8;
  static constexpr int HIT_N_OFF = HIT_Q_OFF + kHitCap * 2;
  static constexpr int QCNT_OFF = HIT_N_OFF + 16;
  static constexpr int LDS_BYTES = QCNT_OFF + 2 * kQueriesPerWG * 4;
  static_assert(D % 64 == 0 && D <= 1024, "d");
  static_assert(NBUF >= 3, "ring too small");
  static_assert(LDS_BYTES <= 160 * 1024, "LDS budget");
};

template <int D, int NW, bool NTL = false>
__device__ __forceinline__ void issue_tile16(const ScanArgs& a, uint32_t buf_lds, int64_t tile, int wave, int lane) {
  using C = Scan16Cfg<D, NW>;
  const int rsub = lane >> 3, pos = lane & 7;
#pragma unroll
  for (int j = 0; j < C::GLDS_PER_WAVE; ++j) {
    int J = j * NW + wave;                   // wave-instruction index in the tile
    // (modulo, not one subtraction: at d = 64 a tile is 2 instructions for 8 waves)
    if (C::GLDS_PER_TILE % NW != 0) J %= C::GLDS_PER_TILE;
    const int g = J >> 1;                    // chunk group (2 instructions each)
    const int row = ((J & 1) << 3) + rsub;   // 0..15
    int64_t li = tile * kT16 + row;
    li = li < a.nrows ? li : a.nrows - 1;
    const int c = pos ^ ((row >> 1) & 7);
    const __bf16* src = a.P + (a.row0 + li * a.rstride) * a.ldp + g * 64 + c * 8;
    if (NTL) glds16_nt(src, __builtin_amdgcn_readfirstlane(buf_lds + J * 1024));
    else glds16(src, __builtin_amdgcn_readfirstlane(buf_lds + J * 1024));
  }
}

// Lean LDS-DMA issue for the filter scan (rows contiguous: row0 0, rstride 1).  A lane's chunks sit at
// fixed byte offsets from the tile's first row, so the tile address is ONE scalar 64-bit base (the
// saddr form of global_load_lds) and the lane offsets are set once per launch -- no per-tile 64-bit
// vector address math -- and the wave's loads of a tile share one m0 save / restore; the steady-state
// ring wait is one constant s_waitcnt.  The last tile of a shard whose row count is not a multiple of
// 16 takes issue_tile16 (row clamp).  Round 4: the per-tile issue was on the barrier-synchronised
// critical path -- 2.707-2.718 -> 2.485-2.510 ms per 10M launch (-8 %) in three alternating A/B
// pairs on one box (profiles/r04at_*; SQ counters before: 51 SALU + ~40 VALU per wave per tile,
// profiles/r04ar_scan_pmc_hits.json); then 32-bit tile / row counters and a tile base advanced by a
// constant stride: 2.44-2.46 -> 2.38-2.40 ms (profiles/r04au_*).
template <int D, int NW>
struct LeanTile {
  using C = Scan16Cfg<D, NW>;
  static constexpr int G = C::GLDS_PER_WAVE;
  uint32_t voff[G];   // per lane: byte offset of its 16-B chunk from the tile's first row
  uint32_t loff[G];   // wave-uniform: LDS byte offset of the instruction's 1 KiB within a slot
  __device__ __forceinline__ void init(const ScanArgs& a, int wave, int lane) {
    const int rsub = lane >> 3, pos = lane & 7;
#pragma unroll
    for (int j = 0; j < G; ++j) {
      int J = j * NW + wave;
      if (C::GLDS_PER_TILE % NW != 0) J %= C::GLDS_PER_TILE;
      const int g = J >> 1;
      const int row = ((J & 1) << 3) + rsub;
      const int c = pos ^ ((row >> 1) & 7);
      voff[j] = (uint32_t)((row * a.ldp + g * 64 + c * 8) * 2);
      loff[j] = (uint32_t)__builtin_amdgcn_readfirstlane(J * 1024);
    }
  }
  // `base` = the tile's first row (the caller advances it by a constant per tile); `partial` = this is
  // the shard's last tile and it is short.  NT: non-temporal loads (a tile is read by one work-group:
  // a single-block launch); a grouped launch's blocks share each tile through L2 and load it plainly.
  template <bool NT>
  __device__ __forceinline__ void issue(const ScanArgs& a, uint32_t slot_lds, const char* base, bool partial,
                                        int64_t tile, int wave, int lane) {
    if (partial) {
      issue_tile16<D, NW, NT>(a, slot_lds, tile, wave, lane);
      return;
    }
#define DRT_LEAN3(POL)                                                                                   \
  {                                                                                                     \
    uint32_t keep;                                                                                      \
    asm volatile(                                                                                       \
        "s_mov_b32 %0, m0\n\t"                                                                          \
        "s_mov_b32 m0, %2\n\t"                                                                          \
        "s_nop 0\n\t"                                                                                   \
        "global_load_lds_dwordx4 %3, %1" POL "\n\t"                                                     \
        "s_mov_b32 m0, %4\n\t"                                                                          \
        "s_nop 0\n\t"                                                                                   \
        "global_load_lds_dwordx4 %5, %1" POL "\n\t"                                                     \
        "s_mov_b32 m0, %6\n\t"                                                                          \
        "s_nop 0\n\t"                                                                                   \
        "global_load_lds_dwordx4 %7, %1" POL "\n\t"                                                     \
        "s_mov_b32 m0, %0"                                                                              \
        : "=&s"(keep)                                                                                   \
        : "s"(base), "s"(slot_lds + loff[0]), "v"(voff[0]), "s"(slot_lds + loff[1]), "v"(voff[1]),      \
          "s"(slot_lds + loff[2]), "v"(voff[2])                                                         \
        : "memory");                                                                                    \
  }
#define DRT_LEAN1(POL, J)                                                                                \
  {                                                                                                     \
    uint32_t keep;                                                                                      \
    asm volatile(                                                                                       \
        "s_mov_b32 %0, m0\n\t"                                                                          \
        "s_mov_b32 m0, %2\n\t"                                                                          \
        "s_nop 0\n\t"                                                                                   \
        "global_load_lds_dwordx4 %3, %1" POL "\n\t"                                                     \
        "s_mov_b32 m0, %0"                                                                              \
        : "=&s"(keep)                                                                                   \
        : "s"(base), "s"(slot_lds + loff[J]), "v"(voff[J])                                              \
        : "memory");                                                                                    \
  }
    if constexpr (G == 3) {
      if constexpr (NT) DRT_LEAN3(" nt")
      else DRT_LEAN3("")
    } else {
#pragma unroll
      for (int j = 0; j < G; ++j) {
        if constexpr (NT) DRT_LEAN1(" nt", j)
        else DRT_LEAN1("", j)
      }
    }
#undef DRT_LEAN3
#undef DRT_LEAN1
  }
};

template <int N>
__device__ __forceinline__ void wait_tiles_younger(int younger) {
  // this wave has `younger` tiles issued after the one it needs; each is N instructions
  switch (younger) {
    case 0: asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); break;
    case 1: asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N) : "memory"); break;
    case 2: asm volatile("s_waitcnt vmcnt(%0)" ::"n"(2 * N) : "memory"); break;
    case 3: asm volatile("s_waitcnt vmcnt(%0)" ::"n"(3 * N < 63 ? 3 * N : 63) : "memory"); break;
    case 4: asm volatile("s_waitcnt vmcnt(%0)" ::"n"(4 * N < 63 ? 4 * N : 63) : "memory"); break;
    case 5: asm volatile("s_waitcnt vmcnt(%0)" ::"n"(5 * N < 63 ? 5 * N : 63) : "memory"); break;
    default: asm volatile("s_waitcnt vmcnt(%0)" ::"n"(6 * N < 63 ? 6 * N : 63) : "memory"); break;
  }
}

template <int D, int MODE, int NW = 8, bool AGG = true>
__global__ __launch_bounds__(NW * 64, 1) void ip_scan16_kernel(ScanArgs a) {
  using C = Scan16Cfg<D, NW>;
  constexpr int QB = 128 / (NW * 16);   // 16-query column blocks per wave
  __shared__ __attribute__((aligned(16))) char smem[C::LDS_BYTES];
  uint64_t* hk = (uint64_t*)(smem + C::HIT_KEY_OFF);
  uint16_t* hq = (uint16_t*)(smem + C::HIT_Q_OFF);
  uint32_t* hit_n = (uint32_t*)(smem + C::HIT_N_OFF);
  uint32_t* qcnt = (uint32_t*)(smem + C::QCNT_OFF);
  uint32_t* qoff = qcnt + kQueriesPerWG;

  const int tid = threadIdx.x;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int lane = tid & 63;
  const int r = lane & 15;      // A row / D column (query within block)
  const int kq = lane >> 4;     // k-quarter (A/B) / row quad (D)

  const int64_t qbase = (int64_t)blockIdx.y * kQueriesPerWG;
  const int64_t ntiles = (a.nrows + kT16 - 1) / kT16;
  const int64_t t0 = blockIdx.x;
  const int64_t tstep = gridDim.x;
  const int64_t my_tiles = t0 < ntiles ? (ntiles - 1 - t0) / tstep + 1 : 0;
  if (my_tiles == 0) return;
  if (MODE == SCAN_FILTER && tid == 0) *hit_n = 0;
  const uint32_t ring = lds_addr_of(smem);

  // queries of this wave: qbase + 16 * QB * wave + 16 * b + r
  int qloc[QB];
  int64_t qg[QB];
  bool qok[QB];
  bf16x8 qf[C::KS][QB];
  float tau[QB];
#pragma unroll
  for (int b = 0; b < QB; ++b) {
    qloc[b] = wave * 16 * QB + 16 * b + r;
    qg[b] = qbase + qloc[b];
    qok[b] = qg[b] < a.nq;
    const int64_t qs = qok[b] ? qg[b] : 0;
#pragma unroll
    for (int s = 0; s < C::KS; ++s) qf[s][b] = *(const bf16x8*)(a.Q + qs * a.ldq + s * 32 + kq * 8);
    tau[b] = __builtin_nanf("");
    if (MODE == SCAN_FILTER) {
      const float tv = a.tau[qs];
      tau[b] = qok[b] ? tv : tau[b];
    }
    if (!qok[b]) {
#pragma unroll
      for (int s = 0; s < C::KS; ++s) qf[s][b] = (bf16x8){};
    }
  }
  // Consume every fragment here so hipcc places its vmcnt waits for these loads
  // in the prologue; otherwise it waits at their first use INSIDE the loop,
  // where the counts it computes ignore the asm LDS-DMA and drain the ring.
#pragma unroll
  for (int s = 0; s < C::KS; ++s)
#pragma unroll
    for (int b = 0; b < QB; ++b) asm volatile("" ::"v"(qf[s][b]));
#pragma unroll
  for (int b = 0; b < QB; ++b) asm volatile("" ::"v"(tau[b]));
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");

  // prologue: PD tiles in flight
#pragma unroll
  for (int p = 0; p < C::PD; ++p)
    if (p < my_tiles) issue_tile16<D, NW>(a, ring + p * C::TILE_BYTES, t0 + p * tstep, wave, lane);

  // A-fragment address: chunk 4s + kq of row r, group s >> 1, position (4(s&1) + kq) ^ sw
  const int sw = (r >> 1) & 7;
  int aoff[2];
#pragma unroll
  for (int m = 0; m < 2; ++m) aoff[m] = r * 128 + (((4 * m + kq) ^ sw) << 4);

  uint32_t topl[QB][MODE == SCAN_TOPR ? kTopRL : 1];
#pragma unroll
  for (int b = 0; b < QB; ++b)
#pragma unroll
    for (int i = 0; i < (MODE == SCAN_TOPR ? kTopRL : 1); ++i) topl[b][i] = 0xFFFFFFFFu;

  // The epilogue (filter / key stores) of tile it runs after the MFMAs of tile it + 1 are
  // issued (two accumulator sets, alternating): its VALU work and the wait for the last MFMA
  // result overlap the next tile's matrix work instead of stalling the wave at every tile.
  auto mma_tile = [&](f32x4 (&acc)[QB], int buf_) {
    const char* tb = smem + buf_ * C::TILE_BYTES;
#pragma unroll
    for (int b = 0; b < QB; ++b) acc[b] = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int s = 0; s < C::KS; ++s) {
      const bf16x8 af = *(const bf16x8*)(tb + (s >> 1) * (kT16 * 128) + aoff[s & 1]);
#pragma unroll
      for (int b = 0; b < QB; ++b) acc[b] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af, qf[s][b], acc[b], 0, 0, 0);
    }
  };
  auto epilogue = [&](const f32x4 (&acc)[QB], int64_t rowbase) {
    if (MODE == SCAN_FILTER) {
      float mx = -__builtin_inff();
#pragma unroll
      for (int b = 0; b < QB; ++b)
        mx = fmaxf(mx, fmaxf(fmaxf(acc[b][0], acc[b][1]), fmaxf(acc[b][2], acc[b][3])) - tau[b]);
      if (__ballot(mx >= 0.0f) != 0ull) {
        if (AGG) {
          // wave-aggregated append: one LDS atomic per wave per tile
          uint32_t m = 0;
#pragma unroll
          for (int b = 0; b < QB; ++b)
#pragma unroll
            for (int j = 0; j < 4; ++j)
              if (acc[b][j] >= tau[b] && rowbase + j < a.nrows) m |= 1u << (4 * b + j);
          const uint32_t c = __builtin_popcount(m);
          uint32_t incl = c;
#pragma unroll
          for (int o = 1; o < 64; o <<= 1) {
            const uint32_t v = __shfl_up(incl, o, 64);
            if (lane >= o) incl += v;
          }
          const uint32_t tot = __shfl(incl, 63, 64);
          uint32_t base = 0;
          if (lane == 0) base = atomicAdd(hit_n, tot);
          base = __shfl(base, 0, 64) + incl - c;
          while (m) {
            const int bit = __builtin_ctz(m);
            m &= m - 1;
            const int b = bit >> 2, j = bit & 3;
            const uint64_t key = ((uint64_t)desc_key(acc[b][j]) << 32) | (uint64_t)(uint32_t)(rowbase + j);
            if (base < (uint32_t)kHitCap) {
              hk[base] = key;
              hq[base] = (uint16_t)qloc[b];
            } else {
              const uint32_t g = atomicAdd(a.counts + qg[b] * kCntStride, 1u);
              if (g < (uint64_t)a.cap) ((uint64_t*)a.out)[qg[b] * a.cap + g] = key;
            }
            ++base;
          }
        } else {
#pragma unroll
          for (int b = 0; b < QB; ++b) {
#pragma unroll
            for (int j = 0; j < 4; ++j) {
              const int64_t row = rowbase + j;
              if (acc[b][j] >= tau[b] && row < a.nrows) {
                const uint64_t key = ((uint64_t)desc_key(acc[b][j]) << 32) | (uint64_t)(uint32_t)row;
                push_hit(a, qloc[b], qg[b], key, hit_n, hk, hq);
              }
            }
          }
        }
      }
    } else if (MODE == SCAN_TOPR) {
      // bubble each of the lane's 4 keys through its sorted list (min / max, no indexing): the list
      // keeps the kTopRL smallest keys (best scores) seen so far; padding rows insert nothing
#pragma unroll
      for (int b = 0; b < QB; ++b) {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          uint32_t x = rowbase + j < a.nrows ? desc_key(acc[b][j]) : 0xFFFFFFFFu;
#pragma unroll
          for (int i = 0; i < kTopRL; ++i) {
            const uint32_t lo = x < topl[b][i] ? x : topl[b][i];
            x = x < topl[b][i] ? topl[b][i] : x;
            topl[b][i] = lo;
          }
        }
      }
    } else {
#pragma unroll
      for (int b = 0; b < QB; ++b) {
        if (!qok[b]) continue;
        uint32_t* o = (uint32_t*)a.out + qg[b] * a.cap;
        u32x4 v;
#pragma unroll
        for (int j = 0; j < 4; ++j) v[j] = desc_key(acc[b][j]);
        if (rowbase + 3 < a.nrows) {
          *(u32x4*)(o + rowbase) = v;
        } else {
#pragma unroll
          for (int j = 0; j < 4; ++j)
            if (rowbase + j < a.nrows) o[rowbase + j] = v[j];
        }
      }
    }
  };

  f32x4 accA[QB], accB[QB];
  int64_t rbA = 0, rbB = 0;
  int buf = 0;
  int nslot = C::PD;   // slot of tile it + PD (== slot of it - 1)
  for (int64_t it = 0; it < my_tiles; ++it) {
    const int64_t tile = t0 + it * tstep;
    const int64_t younger = my_tiles - 1 - it;
    wait_tiles_younger<C::GLDS_PER_WAVE>((int)(younger < C::PD - 1 ? younger : C::PD - 1));
    lds_barrier();

    if (MODE == SCAN_FILTER) {
      const uint32_t n = *hit_n;
      if (n >= (uint32_t)(kHitCap / 2)) {
        if (AGG) flush_hits_agg<NW * 64>(a, qbase, n, hk, hq, qcnt, qoff);
        else flush_hits<NW * 64>(a, qbase, n, hk, hq);
        lds_barrier();
        if (tid == 0) *hit_n = 0;
        lds_barrier();
      }
    }
    if (it + C::PD < my_tiles)
      issue_tile16<D, NW>(a, ring + nslot * C::TILE_BYTES, tile + C::PD * tstep, wave, lane);

    const int64_t rowbase = tile * kT16 + 4 * kq;
    if ((it & 1) == 0) {
      mma_tile(accA, buf);
      if (it > 0) epilogue(accB, rbB);
      rbA = rowbase;
    } else {
      mma_tile(accB, buf);
      epilogue(accA, rbA);
      rbB = rowbase;
    }
    buf = (buf + 1 == C::NBUF) ? 0 : buf + 1;
    nslot = (nslot + 1 == C::NBUF) ? 0 : nslot + 1;
  }

  if (my_tiles & 1) epilogue(accA, rbA);
  else epilogue(accB, rbB);

  if (MODE == SCAN_TOPR) {   // list (work-group column x, row quad kq) of each of the lane's queries
#pragma unroll
    for (int b = 0; b < QB; ++b) {
      if (!qok[b]) continue;
      uint32_t* o = (uint32_t*)a.out + qg[b] * a.cap + ((int64_t)blockIdx.x * 4 + kq) * kTopRL;
#pragma unroll
      for (int i = 0; i < kTopRL; ++i) o[i] = topl[b][i];
    }
  }
  if (MODE == SCAN_FILTER) {
    lds_barrier();
    const uint32_t nf = *hit_n;
    if (AGG) flush_hits_agg<NW * 64>(a, qbase, nf, hk, hq, qcnt, qoff);
    else flush_hits<NW * 64>(a, qbase, nf, hk, hq);
  }
}

// ---------------------------------------------------------------------------
// Production filter scan: the 16-row / 8-wave kernel above with the LDS fragment reads of tile
// t+1 rolled into tile t's MFMA sequence (round 2) and, round 4, PER-WAVE hit lists.
// Fragment s of tile t+1 is read into the register that held fragment s of tile t right after
// that fragment's MFMA, so no LDS latency sits between the per-tile barrier and the matrix work
// (the r02 ablation, tools/scan_ab.py: DMA alone 2.44 ms, DMA + fragment reads 2.39, DMA + MFMA
// on registers 2.47, reads + MFMA 2.80 -> the read-to-MFMA latency after every barrier, in lock
// step on both waves of a SIMD, was the cost).
// Ring: NBUF slots, all in use: at iteration t tile t+1 has landed (it is read during t), tiles
// t+2 .. t+NBUF are in flight, and slot(t) is refilled with tile t+NBUF right after the barrier
// (its fragments were read in t-1 and drained by that barrier's lgkmcnt(0)).
// RAW: every wave waits (vmcnt) for its own share of tile t+1 before the barrier of iteration t;
// reads of t+1 follow that barrier.  WAR: slot(t) is re-issued after the barrier that follows the
// drain of its last reads.
// Hits (round 4): each wave owns a private segment of the LDS hit list and appends with
// ballot + mbcnt (no LDS atomic, no read-back latency in the epilogue); a full segment is flushed
// by its own wave to the global per-query lists (one global atomic per hit, no block barrier).
// The round-2/3 shared list needed an LDS atomic per hit (or per wave-tile) and a block-wide
// flush every 512 hits; with ~4k hits per query that cost 20-35 % of the launch at 1M rows
// (tools/scan_probe.py, profiles/r04b_probe*).
// ---------------------------------------------------------------------------
constexpr int kWaveSeg = kHitCap / 8;   // hit entries per wave segment

__device__ __forceinline__ void wave_flush_hits(const ScanArgs& a, int64_t qw, const uint64_t* hk,
                                                const uint8_t* hq, int n, int lane) {
  for (int i = lane; i < n; i += 64) {
    const uint64_t key = hk[i];
    const int64_t q = qw + hq[i];
    const uint32_t g = atomicAdd(a.counts + q * kCntStride, 1u);
    if (g < (uint64_t)a.cap) ((uint64_t*)a.out)[q * a.cap + g] = key;
  }
}

template <int D, bool NT = true>
__global__ __launch_bounds__(512, 1) void ip_scan16r_kernel(ScanArgs a) {
  constexpr int NW = 8;
  using C = Scan16Cfg<D, NW>;
  constexpr int PD = C::NBUF;   // issue distance: every slot in use
  __shared__ __attribute__((aligned(16))) char smem[C::LDS_BYTES];

  const int tid = threadIdx.x;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int lane = tid & 63;
  const int r = lane & 15;
  const int kq = lane >> 4;
  // this wave's hit segment: kWaveSeg keys + kWaveSeg query indices (within the wave's 16)
  uint64_t* hk = (uint64_t*)(smem + C::HIT_KEY_OFF) + wave * kWaveSeg;
  uint8_t* hq = (uint8_t*)(smem + C::HIT_Q_OFF) + wave * kWaveSeg;

  const int64_t qbase = (int64_t)blockIdx.y * kQueriesPerWG;
  // tile and row indices in 32 bits (rows < 2^32: the hit keys carry 32-bit rows).  An interleaved pass
  // (npass > 1) runs over its own tiles j = 0 .. ntiles - 1, which are the shard's tiles j * tmul + tph
  const int tmul = a.npass > 1 ? a.npass : 1;
  const int tph = a.npass > 1 ? a.pass : 0;
  const int tall = (int)((a.nrows + kT16 - 1) / kT16);
  const int ntiles = pass_tiles(tall, a.npass, a.pass);
  const uint32_t nrows = (uint32_t)a.nrows;
  const int t0 = blockIdx.x;
  const int tstep = gridDim.x;
  const int my_tiles = t0 < ntiles ? (ntiles - 1 - t0) / tstep + 1 : 0;
  if (my_tiles == 0) return;
  // (the shard's short last tile belongs to exactly one pass)
  const int partial_tile = ((a.nrows & (kT16 - 1)) != 0 && (tall - 1) % tmul == tph) ? ntiles - 1 : -1;
  const uint32_t ring = lds_addr_of(smem);
  // the next tile to issue, as a row pointer advanced by a constant (scalar) stride per tile
  const int64_t tile_stride = (int64_t)tstep * tmul * kT16 * a.ldp * 2;
  const char* next_base = (const char*)(a.P + ((int64_t)t0 * tmul + tph) * kT16 * a.ldp);

  // 16 queries per wave: qbase + 16 * wave + r
  const int64_t qw = qbase + wave * 16;
  const int64_t qg = qw + r;
  const bool qok = qg < a.nq;
  const int64_t qs = qok ? qg : 0;
  bf16x8 qf[C::KS];
#pragma unroll
  for (int s = 0; s < C::KS; ++s) qf[s] = *(const bf16x8*)(a.Q + qs * a.ldq + s * 32 + kq * 8);
  float tau = __builtin_nanf("");
  {
    const float tv = a.tau[qs];
    tau = qok ? tv : tau;
  }
  if (!qok) {
#pragma unroll
    for (int s = 0; s < C::KS; ++s) qf[s] = (bf16x8){};
  }
#pragma unroll
  for (int s = 0; s < C::KS; ++s) asm volatile("" ::"v"(qf[s]));
  asm volatile("" ::"v"(tau));
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");

  // prologue: tiles 0 .. PD-1 in flight, tile 0 landed and read into registers
  LeanTile<D, NW> lt;
  lt.init(a, wave, lane);
#pragma unroll
  for (int p = 0; p < PD; ++p) {
    if (p < my_tiles) {
      const int tile = t0 + p * tstep;
      lt.template issue<NT>(a, ring + p * C::TILE_BYTES, next_base, tile == partial_tile, tile * tmul + tph, wave,
                            lane);
      next_base += tile_stride;
    }
  }
  if (wave >= NW / 2) __builtin_amdgcn_s_setprio(1);
  {
    const int last = my_tiles - 1 < PD - 1 ? my_tiles - 1 : PD - 1;
    wait_tiles_younger<C::GLDS_PER_WAVE>((int)last);
  }
  lds_barrier();

  const int sw = (r >> 1) & 7;
  int aoff[2];
#pragma unroll
  for (int m = 0; m < 2; ++m) aoff[m] = r * 128 + (((4 * m + kq) ^ sw) << 4);
  bf16x8 af[C::KS];
#pragma unroll
  for (int s = 0; s < C::KS; ++s) af[s] = *(const bf16x8*)(smem + (s >> 1) * (kT16 * 128) + aoff[s & 1]);

  // MFMAs of the tile whose fragments are in af[], each fragment replaced by the same
  // fragment of the tile in slot `nslot` right after its MFMA (unconditional: on the
  // last tile the reads hit a stale slot and are never used).
  auto mma_roll = [&](f32x4& acc, int nslot) {
    const char* nb = smem + nslot * C::TILE_BYTES;
    acc = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int s = 0; s < C::KS; ++s) {
      acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af[s], qf[s], acc, 0, 0, 0);
      af[s] = *(const bf16x8*)(nb + (s >> 1) * (kT16 * 128) + aoff[s & 1]);
      // pin the order: a read hoisted above earlier MFMAs would keep both tiles' fragments live
      __builtin_amdgcn_sched_barrier(0);
    }
  };
  int wcnt = 0;   // entries in this wave's segment (wave-uniform)
  auto epilogue = [&](const f32x4& acc, uint32_t rowbase) {
    const float mx = fmaxf(fmaxf(acc[0], acc[1]), fmaxf(acc[2], acc[3])) - tau;
    if (__ballot(mx >= 0.0f) == 0ull) return;
    // the tile's four row ballots at once (independent compares / popcounts, no branch per row);
    // the per-row path below only when the segment cannot take them all (round 4: -0.35 % per 10M
    // launch in three alternating A/B pairs, profiles/r04as_*)
    bool hv[4];
    uint64_t mv[4];
    int cv[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      hv[j] = acc[j] >= tau && rowbase + j < nrows;
      mv[j] = __ballot(hv[j]);
      cv[j] = __builtin_popcountll(mv[j]);
    }
    const int tot = cv[0] + cv[1] + cv[2] + cv[3];
    if (wcnt + tot <= kWaveSeg) {
      int base = wcnt;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        if (hv[j]) {
          const int pos = base + (int)__builtin_amdgcn_mbcnt_hi((uint32_t)(mv[j] >> 32),
                                                                __builtin_amdgcn_mbcnt_lo((uint32_t)mv[j], 0u));
          hk[pos] = ((uint64_t)desc_key(acc[j]) << 32) | (uint64_t)(a.row_base + rowbase + j);
          hq[pos] = (uint8_t)r;
        }
        base += cv[j];
      }
      wcnt = base;
      return;
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const bool hit = acc[j] >= tau && rowbase + j < nrows;
      const uint64_t m = __ballot(hit);
      if (m == 0ull) continue;
      const int c = __builtin_popcountll(m);
      if (wcnt + c > kWaveSeg) {
        wave_flush_hits(a, qw, hk, hq, wcnt, lane);
        wcnt = 0;
      }
      if (hit) {
        const int pos = wcnt + (int)__builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32),
                                                              __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
        hk[pos] = ((uint64_t)desc_key(acc[j]) << 32) | (uint64_t)(a.row_base + rowbase + j);
        hq[pos] = (uint8_t)r;
      }
      wcnt += c;
    }
  };

  f32x4 accA, accB;
  uint32_t rbA = 0, rbB = 0;
  int buf = 0;   // slot of tile it (its fragments are in af[])
  // one tile: barrier, ring refill, MFMAs (+ reads of the next tile), deferred epilogue of the
  // previous tile; the loop body runs two of them in sequence (accA / accB) so the fragment
  // registers flow straight through and the accumulators are never selected at run time
  auto iter = [&](int it, f32x4& acc, uint32_t& rb, const f32x4& prev, uint32_t rb_prev) {
    const int tile = t0 + it * tstep;
    if (it + PD <= my_tiles) {   // steady state: tiles it+1 .. it+PD-1 in flight, need it+1
      wait_vmcnt<C::GLDS_PER_WAVE * (PD - 2)>();
    } else if (it + 1 < my_tiles) {
      wait_tiles_younger<C::GLDS_PER_WAVE>(my_tiles - 1 - it - 1);
    }
    lds_barrier();   // tile it+1 landed (every wave's share); slot(it) fully read
    if (it + PD < my_tiles) {
      const int ntile = tile + PD * tstep;
      lt.template issue<NT>(a, ring + buf * C::TILE_BYTES, next_base, ntile == partial_tile, ntile * tmul + tph,
                            wave, lane);
      next_base += tile_stride;
    }
    const int nslot = buf + 1 == C::NBUF ? 0 : buf + 1;
    mma_roll(acc, nslot);
    if (it > 0) epilogue(prev, rb_prev);
    rb = (uint32_t)(tile * tmul + tph) * kT16 + 4 * kq;
    buf = nslot;
  };
  for (int it = 0; it < my_tiles; it += 2) {
    iter(it, accA, rbA, accB, rbB);
    if (it + 1 < my_tiles) iter(it + 1, accB, rbB, accA, rbA);
  }
  if (my_tiles & 1) epilogue(accA, rbA);
  else epilogue(accB, rbB);
  if (wcnt) wave_flush_hits(a, qw, hk, hq, wcnt, lane);
}

// ---------------------------------------------------------------------------
// Grouped filter scan (a launch of more than 128 queries): the same 16-row tiles, ring and MFMA
// step order as ip_scan16r_kernel, but 32 queries per wave (two 16-query B sets held in registers,
// 256 queries per work-group), so one LDS fragment read of the tile's rows feeds TWO MFMAs.
// Round 5 ablations of ip_scan16r on the grouped launch (profiles/r05y): its 16x16x32 MFMA per
// 1 KiB fragment read puts the LDS array (256 B/clk/CU, plus the ring's DMA writes) level with the
// MFMA pipe, the launch ran at 53 % MFMA / 53 % LDS busy, and the corpus DMA alone added 30 % to the
// MFMA-only time.  Here the LDS reads per MFMA and the L2 -> LDS bytes per query are halved (a group's
// tile is loaded by half as many work-groups).  Registers: the 32 queries' fragments (2 x d/32 x 4
// VGPRs) leave room for a short fragment roll only: fragment s + RD of the same tile (or, near the
// end of a tile, of the next one) is read into the register fragment s just left, so a slot is read
// during its own tile and is refilled one tile later (issue distance NB - 1).  A tile's epilogue runs
// after the next tile's MFMAs are issued (two accumulator sets alternate), as in ip_scan16r.
// Every score is the same 24-step 16x16x32 chain as ip_scan16r's: identical values and hits.
// ---------------------------------------------------------------------------
template <int D>
struct Scan32Cfg {
  static constexpr int KS = D / 32;
  static constexpr int RD = KS % 2 == 0 ? 2 : 1;   // fragment roll depth (round 5: 2, 3, 4, 6 within noise)
  static constexpr int TILE_BYTES = kT16 * D * 2;
  static constexpr int HIT_BYTES = kHitCap * 9;
  static constexpr int NB_RAW = (160 * 1024 - HIT_BYTES) / TILE_BYTES;
  static constexpr int NB = NB_RAW > 6 ? 6 : NB_RAW;
  static constexpr int RING_BYTES = NB * TILE_BYTES;
  static constexpr int LDS_BYTES = RING_BYTES + HIT_BYTES;
  static_assert(NB >= 3, "ring too small");
  static_assert(LDS_BYTES <= 160 * 1024, "LDS budget");
};
constexpr int kQueriesPerWG32 = 256;

template <int D>
__global__ __launch_bounds__(512, 1) void ip_scan32r_kernel(ScanArgs a) {
  constexpr int NW = 8;
  using C = Scan16Cfg<D, NW>;   // tile image, DMA split, per-wave issue count
  using C32 = Scan32Cfg<D>;
  constexpr int NB = C32::NB;
  constexpr int PD = NB - 1;    // tiles issued ahead (the slot of tile it-1 is refilled at tile it+1)
  constexpr int KS = C32::KS;
  constexpr int RD = C32::RD;
  constexpr int kSeg = kHitCap / NW;
  __shared__ __attribute__((aligned(16))) char smem[C32::LDS_BYTES];

  const int tid = threadIdx.x;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int lane = tid & 63;
  const int r = lane & 15;
  const int kq = lane >> 4;
  uint64_t* hk = (uint64_t*)(smem + C32::RING_BYTES) + wave * kSeg;
  uint8_t* hq = (uint8_t*)(smem + C32::RING_BYTES + kHitCap * 8) + wave * kSeg;

  const int64_t qbase = (int64_t)blockIdx.y * kQueriesPerWG32;
  // (an interleaved pass: its tiles j = 0 .. ntiles - 1 are the shard's tiles j * tmul + tph, as in ip_scan16r)
  const int tmul = a.npass > 1 ? a.npass : 1;
  const int tph = a.npass > 1 ? a.pass : 0;
  const int tall = (int)((a.nrows + kT16 - 1) / kT16);
  const int ntiles = pass_tiles(tall, a.npass, a.pass);
  const uint32_t nrows = (uint32_t)a.nrows;
  const int t0 = blockIdx.x;
  const int tstep = gridDim.x;
  const int my_tiles = t0 < ntiles ? (ntiles - 1 - t0) / tstep + 1 : 0;
  if (my_tiles == 0) return;
  const int partial_tile = ((a.nrows & (kT16 - 1)) != 0 && (tall - 1) % tmul == tph) ? ntiles - 1 : -1;
  const uint32_t ring = lds_addr_of(smem);
  const int64_t tile_stride = (int64_t)tstep * tmul * kT16 * a.ldp * 2;
  const char* next_base = (const char*)(a.P + ((int64_t)t0 * tmul + tph) * kT16 * a.ldp);

  // 32 queries per wave: qw + 16 b + r, b = 0, 1
  const int64_t qw = qbase + wave * 32;
  bf16x8 qf0[KS], qf1[KS];
  float tau0, tau1;
  {
    const int64_t g0 = qw + r, g1 = qw + 16 + r;
    const bool ok0 = g0 < a.nq, ok1 = g1 < a.nq;
    const int64_t s0 = ok0 ? g0 : 0, s1 = ok1 ? g1 : 0;
#pragma unroll
    for (int s = 0; s < KS; ++s) {
      qf0[s] = *(const bf16x8*)(a.Q + s0 * a.ldq + s * 32 + kq * 8);
      qf1[s] = *(const bf16x8*)(a.Q + s1 * a.ldq + s * 32 + kq * 8);
    }
    const float v0 = a.tau[s0], v1 = a.tau[s1];
    tau0 = ok0 ? v0 : __builtin_nanf("");
    tau1 = ok1 ? v1 : __builtin_nanf("");
    if (!ok0) {
#pragma unroll
      for (int s = 0; s < KS; ++s) qf0[s] = (bf16x8){};
    }
    if (!ok1) {
#pragma unroll
      for (int s = 0; s < KS; ++s) qf1[s] = (bf16x8){};
    }
  }
#pragma unroll
  for (int s = 0; s < KS; ++s) asm volatile("" ::"v"(qf0[s]), "v"(qf1[s]));
  asm volatile("" ::"v"(tau0), "v"(tau1));
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");

  LeanTile<D, NW> lt;
  lt.init(a, wave, lane);
#pragma unroll
  for (int p = 0; p < PD; ++p) {
    if (p < my_tiles) {
      const int tile = t0 + p * tstep;
      lt.template issue<false>(a, ring + p * C::TILE_BYTES, next_base, tile == partial_tile, tile * tmul + tph, wave,
                               lane);
      next_base += tile_stride;
    }
  }
  if (wave >= NW / 2) __builtin_amdgcn_s_setprio(1);
  {
    const int last = my_tiles - 1 < PD - 1 ? my_tiles - 1 : PD - 1;
    wait_tiles_younger<C::GLDS_PER_WAVE>((int)last);
  }
  lds_barrier();

  const int sw = (r >> 1) & 7;
  int aoff[2];
#pragma unroll
  for (int m = 0; m < 2; ++m) aoff[m] = r * 128 + (((4 * m + kq) ^ sw) << 4);
  auto frag = [&](int slot, int s) -> bf16x8 {
    return *(const bf16x8*)(smem + slot * C::TILE_BYTES + (s >> 1) * (kT16 * 128) + aoff[s & 1]);
  };
  bf16x8 af[RD];
#pragma unroll
  for (int s = 0; s < RD; ++s) af[s] = frag(0, s);

  int wcnt = 0;
  auto append = [&](const f32x4& acc, float tau, int ql, uint32_t rowbase) {
    const float mx = fmaxf(fmaxf(acc[0], acc[1]), fmaxf(acc[2], acc[3])) - tau;
    if (__ballot(mx >= 0.0f) == 0ull) return;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const bool hit = acc[j] >= tau && rowbase + j < nrows;
      const uint64_t m = __ballot(hit);
      if (m == 0ull) continue;
      const int c = __builtin_popcountll(m);
      if (wcnt + c > kSeg) {
        wave_flush_hits(a, qw, hk, hq, wcnt, lane);
        wcnt = 0;
      }
      if (hit) {
        const int pos = wcnt + (int)__builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32),
                                                              __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
        hk[pos] = ((uint64_t)desc_key(acc[j]) << 32) | (uint64_t)(a.row_base + rowbase + j);
        hq[pos] = (uint8_t)ql;
      }
      wcnt += c;
    }
  };

  // (one ballot over both query sets' tiles measured slower: 2.95-2.97 vs 2.91 ms, profiles/r05y)
  auto epilogue = [&](const f32x4& p0, const f32x4& p1, uint32_t rowbase) {
    append(p0, tau0, r, rowbase);
    append(p1, tau1, 16 + r, rowbase);
  };

  int buf = 0;   // slot of tile it
  // one tile: wait + barrier, ring refill, MFMAs (+ the rolled reads), then the epilogue of the
  // PREVIOUS tile (its accumulators are complete by then: no wait on this tile's MFMA latency); the
  // loop body runs two tiles so the accumulator sets alternate without run-time selection
  auto iter = [&](int it, f32x4& acc0, f32x4& acc1, uint32_t& rb, const f32x4& prev0, const f32x4& prev1,
                  uint32_t rb_prev) {
    const int tile = t0 + it * tstep;
    // issued so far: tiles .. it + PD - 1; tile it+1 must have landed (its first RD fragments are
    // read near the end of this tile's MFMAs)
    if (it + PD <= my_tiles) {
      wait_vmcnt<C::GLDS_PER_WAVE * (PD - 2)>();
    } else if (it + 1 < my_tiles) {
      wait_tiles_younger<C::GLDS_PER_WAVE>(my_tiles - 1 - it - 1);
    }
    // every wave's share of tile it+1 landed, and every wave issued tile it-1's MFMAs (so its reads of
    // slot(it-1) completed: each MFMA waited for its own fragment) -- that slot is refilled below
    lds_barrier();
    // the refill of slot(it-1) is issued a quarter into this tile's MFMAs (its SALU / address work then
    // overlaps queued matrix work instead of delaying every wave's first MFMA after the barrier: round 5,
    // 2.89-2.91 vs 2.95-2.97 ms per grouped launch in three alternating rounds, profiles/r05y)
    const bool do_dma = it + PD < my_tiles;
    const int ntile = tile + PD * tstep;
    const int pslot = buf == 0 ? NB - 1 : buf - 1;   // slot of tile it-1 (it = 0: the unused slot)
    const int nslot = buf + 1 == NB ? 0 : buf + 1;
    acc0 = (f32x4){0.f, 0.f, 0.f, 0.f};
    acc1 = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int s = 0; s < KS; ++s) {
      acc0 = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af[s % RD], qf0[s], acc0, 0, 0, 0);
      acc1 = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af[s % RD], qf1[s], acc1, 0, 0, 0);
      // fragment s + RD: of this tile, or (the last RD steps) the first ones of tile it+1
      af[s % RD] = s + RD < KS ? frag(buf, s + RD) : frag(nslot, s + RD - KS);
      __builtin_amdgcn_sched_barrier(0);
      if (s == KS / 4 && do_dma) {
        lt.template issue<false>(a, ring + pslot * C::TILE_BYTES, next_base, ntile == partial_tile,
                                 ntile * tmul + tph, wave, lane);
        next_base += tile_stride;
      }
      __builtin_amdgcn_sched_barrier(0);
    }
    if (it > 0) epilogue(prev0, prev1, rb_prev);
    rb = (uint32_t)(tile * tmul + tph) * kT16 + 4 * kq;
    buf = nslot;
  };
  f32x4 a0, a1, b0, b1;
  uint32_t rbA = 0, rbB = 0;
  for (int it = 0; it < my_tiles; it += 2) {
    iter(it, a0, a1, rbA, b0, b1, rbB);
    if (it + 1 < my_tiles) iter(it + 1, b0, b1, rbB, a0, a1, rbA);
  }
  if (my_tiles & 1) epilogue(a0, a1, rbA);
  else epilogue(b0, b1, rbB);
  if (wcnt) wave_flush_hits(a, qw, hk, hq, wcnt, lane);
}

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

struct RefineArgs {
  const __bf16* Q;
  int64_t nq;
  int32_t d;
  const __bf16* P;
  int64_t n_local;
  int64_t row_offset;
  const float* cs;      // [nq][kc] fp32 scores, sorted desc (pads -FLT_MAX)
  const int64_t* ci;    // [nq][kc] global ids (pads -1)
  int32_t kc, k;
  const float* stats;   // row statistics (drt_row_stats_bf16)
  const float* tau;     // [nq] filter thresholds or NULL (every row was scored)
  float* delta;         // [nq][kc]
  int32_t* cnt;         // [nq][2]: window size C (-1: exact in fp32, -2: window wider than the list), eps bits
  int32_t* status;      // [nq] (indexed through qmap) or NULL
  const int32_t* qmap;  // output row of query q, or NULL
  bool set_status;      // status[row] = this stage's bits (the exact rescan clears it) instead of |=
  int32_t slice;        // refine_delta: candidates per work-group (64 or 256; 0 = kRefSlice)
  float* out_s;         // refine_sort: [*, k]
  int64_t* out_i;
};

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

// ---------------------------------------------------------------------------
// Host-side planning and launch helpers.
// ---------------------------------------------------------------------------
struct TopkPlan : PlanHead {   // (the head's offsets: off_tau .. off_part)
  int64_t n, k, nq, nq_pad;
  bool sample;        // false: n <= cap, dense scan of everything
  int64_t cap;        // FILTER capacity per query (or dense width when !sample)
  int64_t m;          // sampled rows
  int64_t stride;     // sample stride
  int64_t r;          // rank of the sampled score used as tau
  int64_t nchunk;     // kth_partial chunks per query
  int64_t kc;         // refine: candidates selected per query (>= k)
  // workspace offsets (bytes) of the canonical-order stage, after the head
  size_t off_cs, off_ci, off_delta, off_rcnt, total;
};

// The candidates of the canonical-order stage after the head: [nq_pad][kc] scores, ids, deltas, [nq_pad][2] counts.
static size_t plan_refine_tail(TopkPlan& p) {
  p.kc = refine_width(p.k);
  WsBump b{p.head_end};
  p.off_cs = b.take((size_t)p.nq_pad * p.kc * 4);
  p.off_ci = b.take((size_t)p.nq_pad * p.kc * 8);
  p.off_delta = b.take((size_t)p.nq_pad * p.kc * 4);
  p.off_rcnt = b.take((size_t)p.nq_pad * 8);
  return b.o;
}

static double poisson_tail_ge(double lam, int64_t r) {
  // P[X >= r], X ~ Poisson(lam), by summing the pmf from r upward.
  double logp = -lam + r * std::log(lam) - std::lgamma((double)r + 1.0);
  double p = std::exp(logp), s = 0.0;
  for (int64_t i = r; i < r + 2000; ++i) {
    s += p;
    p *= lam / (double)(i + 1);
    if (p < 1e-30 * s) break;
  }
  return s;
}


static TopkPlan make_plan(int64_t nq, int64_t n, int64_t k) {
  TopkPlan p{};
  p.n = n;
  p.k = k;
  p.nq = nq;
  p.nq_pad = (nq + kQueriesPerWG - 1) / kQueriesPerWG * kQueriesPerWG;
  const int64_t target = hit_target(k);  // expected hits per query
  p.cap = 4 * target;
  if (n <= p.cap) {
    p.sample = false;
    p.cap = align_up(std::max<int64_t>(n, 4), 4);
    p.m = 0;
    p.stride = 1;
    p.r = 0;
  } else {
    p.sample = true;
    // smallest r with P[miss] = P[Poisson(k r / target) >= r] < 1e-9
    int64_t r = 1;
    while (poisson_tail_ge((double)k * r / (double)target, r) > 1e-9 && r < 100000) ++r;
    p.r = r;
    int64_t m = (r * n + target - 1) / target;
    if (m > n) m = n;
    p.stride = std::max<int64_t>(1, n / m);
    // the kth_final pass keeps chunks * r <= 4096 survivors
    const int64_t m_cap = std::max<int64_t>(1, kKthChunk / r) * kKthChunk;
    if (m > m_cap) m = m_cap;
    p.stride = std::max<int64_t>(1, n / m);
    p.m = (n - p.stride / 2 + p.stride - 1) / p.stride;  // rows stride/2 + i*stride < n
    if (p.m > m_cap) p.m = m_cap;
    if (p.m < r) p.m = std::min<int64_t>(n, r);
    p.nchunk = (p.m + kKthChunk - 1) / kKthChunk;
  }
  // filter hits are u64 keys, a dense scan's scores u32; without a sample m and nchunk are 0
  static_cast<PlanHead&>(p) = plan_head_layout(p.nq_pad, p.cap, p.sample ? 8 : 4, p.m, p.nchunk * p.r);
  p.total = plan_refine_tail(p);
  return p;
}

// Distributed plan: shard of n_local rows out of n_global.  target / cap / r
// come from the GLOBAL plan, so the union of the shards' samples has the same
// sampling fraction r / target as a single-index search; each shard expects
// target * n_local / n_global filter hits.
static TopkPlan make_dist_plan(int64_t nq, int64_t n_local, int64_t n_global, int64_t k) {
  const TopkPlan g = make_plan(nq, n_global, k);
  TopkPlan p{};
  p.n = n_local;
  p.k = k;
  p.nq = nq;
  p.nq_pad = g.nq_pad;
  const int64_t target = hit_target(k);
  p.cap = std::max<int64_t>(g.cap, 4 * target);
  p.sample = g.sample;
  p.r = g.sample ? g.r : 0;
  p.stride = 1;
  p.m = 0;
  p.nchunk = 0;
  if (p.sample && n_local > 0) {
    int64_t m = (p.r * n_local + target - 1) / target;
    if (m > n_local) m = n_local;
    const int64_t m_cap = std::max<int64_t>(1, kKthChunk / p.r) * kKthChunk;
    if (m > m_cap) m = m_cap;
    p.stride = std::max<int64_t>(1, n_local / m);
    p.m = (n_local - p.stride / 2 + p.stride - 1) / p.stride;
    if (p.m > m_cap) p.m = m_cap;
    p.nchunk = (p.m + kKthChunk - 1) / kKthChunk;
  }
  static_cast<PlanHead&>(p) = plan_head_layout(p.nq_pad, p.cap, 8, p.m, p.nchunk * p.r);
  p.total = p.head_end;
  return p;
}

// ScanArgs::exp_hits of a filter launch under a distributed plan `p` of a corpus of n_global rows (it picks
// the append flavour of the wide-row kernel, launch_scan_d).  Two forms, on purpose:
// a launch over `rows` contiguous rows -- the whole shard, or one chunk of it -- expects that run's share
// of the target (without a sample the threshold is -inf: every row hits) ...
static int64_t rows_exp_hits(const TopkPlan& p, int64_t rows, int64_t n_global) {
  return p.sample ? std::max<int64_t>(1, hit_target(p.k) * rows / std::max<int64_t>(1, n_global)) : rows;
}

// ... and one of `npasses` interleaved passes expects the shard's share divided by the passes.
static int64_t pass_exp_hits(const TopkPlan& p, int64_t npasses, int64_t n_global) {
  return p.sample ? std::max<int64_t>(1, hit_target(p.k) * p.n / npasses / std::max<int64_t>(1, n_global))
                  : std::max<int64_t>(1, p.n / npasses);
}

// The part of ScanArgs every launch shares: dense [nq, d] queries and [*, d] corpus rows, addressed as one
// contiguous run from P's first row.  nrows and the mode's outputs are the caller's.
static ScanArgs scan_args(const void* Q, int64_t nq, const void* P, int32_t d) {
  ScanArgs a{};
  a.Q = (const __bf16*)Q;
  a.nq = nq;
  a.ldq = d;
  a.P = (const __bf16*)P;
  a.ldp = d;
  a.row0 = 0;
  a.rstride = 1;
  return a;
}

static int scan_grid_x(int64_t ntiles) {
  int dev = 0, cus = 256;
  if (hipGetDevice(&dev) == hipSuccess) {
    int v = 0;
    if (hipDeviceGetAttribute(&v, hipDeviceAttributeMultiprocessorCount, dev) == hipSuccess && v > 0)
      cus = v;
  }
  const int64_t g = std::min<int64_t>(ntiles, (int64_t)cus);
  return (int)std::max<int64_t>(g, 1);
}

// Grid of the 16-row scans (`qpw` queries per work-group row: 128, or 256 for the 32-queries-per-wave
// filter kernel): several query blocks in one launch (a group of batches) get gridDim.x = CUs / blocks,
// a multiple of 8, so work-groups (x, y) and (x, y') -- the
// same tiles for different query blocks -- sit on the same XCD (work-groups are dealt to XCDs round-robin
// by linear id) and run at the same time: a tile comes from HBM once and from that XCD's L2 for the other
// blocks.  (gridDim.x = CUs ran the blocks one after another, each streaming the whole shard from HBM.)
static dim3 scan16_grid(int64_t nq, int64_t nrows, int qpw = kQueriesPerWG) {
  const unsigned gy = (unsigned)((nq + qpw - 1) / qpw);
  const int64_t ntiles = (nrows + kT16 - 1) / kT16;
  int gx = scan_grid_x(ntiles);
  if (gy > 1 && ntiles >= 8) {
    const int cus = scan_grid_x((int64_t)1 << 40);
    const int share = std::max(8, (cus / (int)gy) & ~7);
    gx = (int)std::min<int64_t>(ntiles, share);
  }
  return dim3(gx, gy);
}

template <int D>
static int launch_scan_d(const ScanArgs& a, int mode, hipStream_t s) {
  if (a.nq == 0 || a.nrows == 0) return DRT_OK;
  // an interleaved pass (the lean filter kernels only) is gridded over its own tiles
  constexpr bool kLean = D <= 768;   // the lean filter kernels (ip_scan16r / ip_scan32r) exist for these rows
  if (a.npass > 1 && (mode != SCAN_FILTER || !kLean || a.row0 != 0 || a.rstride != 1 || a.pass < 0 ||
                      a.pass >= a.npass))
    return DRT_EINVAL;
  const int64_t ntiles = pass_tiles((int)((a.nrows + kT16 - 1) / kT16), a.npass, a.pass);
  if (ntiles == 0) return DRT_OK;
  const dim3 grid = scan16_grid(a.nq, ntiles * kT16);
  const unsigned gy = grid.y;
  if (mode == SCAN_FILTER) {
    // 8 waves (2 per SIMD), 16 queries each; fragment reads of the next tile rolled into this
    // tile's MFMAs, non-temporal corpus loads, s_setprio 1 for waves 4-7 (r02 A/B, tools/scan_ab.py,
    // profiles/r02e_scan_roll.log: 2.59-2.62 vs 2.93 ms per launch for the round-1 loop, ids identical).
    // Hit append: one LDS atomic per hit when hits are rare (+ aggregated flush, one global atomic per
    // (work-group, query): profiles/r02g_scan_flush.log, -3 % per launch), one per wave-tile (popcount +
    // wave scan) when they are dense.  Expected hits per 16x16 wave-tile = 256 * (cap/4) / n; measured
    // crossover (profiles/r01_*): dense below ~3M rows at cap 16384.
    const double eh = a.exp_hits > 0 ? (double)a.exp_hits : (double)a.cap / 4.0;
    const bool dense_hits = eh * 256.0 / (double)a.nrows >= 0.35;
    // d > 768: the rolled reads hold two tiles' fragments beside the queries' (2 x d / 32 x 4 VGPRs +
    // d / 32 x 4): that spills from d = 832, so wider rows take the same loop with the fragments read
    // per k-step (ip_scan16_kernel: same MFMA order, identical results), and the lean kernels are
    // instantiated for d <= 768 only (ip_scan32r's 32 queries' fragments spill from d = 832 as well)
    // (ip_scan16r addresses rows as one contiguous run: row0 0, rstride 1 -- every filter pass)
    bool lean = false;
    if constexpr (kLean) {
      lean = a.row0 == 0 && a.rstride == 1;
      if (lean) {
        // non-temporal corpus loads for a single block; a group's blocks share each tile through L2, and a
        // group of more than 128 queries takes the 32-queries-per-wave kernel (256 per work-group)
        if (gy > 1) {
          const dim3 grid32 = scan16_grid(a.nq, ntiles * kT16, kQueriesPerWG32);
          hipLaunchKernelGGL((ip_scan32r_kernel<D>), grid32, dim3(512), 0, s, a);
        } else {
          hipLaunchKernelGGL((ip_scan16r_kernel<D, true>), grid, dim3(512), 0, s, a);
        }
      }
    }
    if (!lean) {
      if (dense_hits) hipLaunchKernelGGL((ip_scan16_kernel<D, SCAN_FILTER, 8, true>), grid, dim3(512), 0, s, a);
      else hipLaunchKernelGGL((ip_scan16_kernel<D, SCAN_FILTER, 8, false>), grid, dim3(512), 0, s, a);
    }
  } else if (mode == SCAN_TOPR) {
    hipLaunchKernelGGL((ip_scan16_kernel<D, SCAN_TOPR>), grid, dim3(512), 0, s, a);
  } else {
    hipLaunchKernelGGL((ip_scan16_kernel<D, SCAN_DENSE>), grid, dim3(512), 0, s, a);
  }
  return hip_status(hipGetLastError());
}

static int launch_scan_impl(const ScanArgs& a, int d, int mode, hipStream_t s) {
  switch (d) {
    case 64: return launch_scan_d<64>(a, mode, s);
    case 128: return launch_scan_d<128>(a, mode, s);
    case 192: return launch_scan_d<192>(a, mode, s);
    case 256: return launch_scan_d<256>(a, mode, s);
    case 320: return launch_scan_d<320>(a, mode, s);
    case 384: return launch_scan_d<384>(a, mode, s);
    case 448: return launch_scan_d<448>(a, mode, s);
    case 512: return launch_scan_d<512>(a, mode, s);
    case 576: return launch_scan_d<576>(a, mode, s);
    case 640: return launch_scan_d<640>(a, mode, s);
    case 704: return launch_scan_d<704>(a, mode, s);
    case 768: return launch_scan_d<768>(a, mode, s);
    case 832: return launch_scan_d<832>(a, mode, s);
    case 896: return launch_scan_d<896>(a, mode, s);
    case 960: return launch_scan_d<960>(a, mode, s);
    case 1024: return launch_scan_d<1024>(a, mode, s);
    default: return DRT_EINVAL;
  }
}

static int launch_scan(const ScanArgs& a, int d, int mode, hipStream_t s, int family) {
  const ProfPair pp = prof_begin(family, s);
  const int rc = launch_scan_impl(a, d, mode, s);
  prof_end(pp, s);
  return rc;
}

static bool valid_dist_dims(int64_t nq, int64_t n_local, int64_t n_global, int32_t d, int32_t k) {
  return nq >= 0 && n_local >= 0 && n_global >= n_local && d > 0 && d % 64 == 0 && d <= 1024 && k >= 1 &&
         k <= kSelMaxK && n_global < (int64_t)0xFFFFFFFFll;
}

}  // namespace drt

using namespace drt;

extern "C" {

const char* drt_version(void) {
  return "drt-mi355x 0.3 (gfx950; packed top-k lists: entry k = valid count << 32 | flags)";
}

size_t drt_ip_topk_workspace(int64_t nq, int64_t n, int32_t d, int32_t k) {
  if (!valid_dims(nq, n, d, k)) return 0;
  return make_plan(nq, n, k).total;
}

}  // extern "C"

namespace drt {

static int launch_refine(RefineArgs& ra, hipStream_t s) {
  if (ra.nq == 0) return DRT_OK;
  const ProfPair pp = prof_begin(PROF_SELECT, s);
  hipLaunchKernelGGL(refine_prep_kernel, dim3((unsigned)ra.nq), dim3(kRefThreads), 0, s, ra);
  // the one-GPU entries (ip_topk, resolve): every candidate is this shard's
  launch_refine_local(ra, s);
  hipLaunchKernelGGL(refine_sort_kernel, dim3((unsigned)ra.nq), dim3(kRefSortThreads), 0, s, ra);
  prof_end(pp, s);
  return hip_status(hipGetLastError());
}

// One shard's top-k (drt_ip_topk_bf16); with row statistics (stats != NULL) the result is put in
// the canonical exact-score order (refine stage above): the select keeps kc >= k candidates in the
// workspace and the refine kernels write the k outputs.
static int ip_topk_impl(const void* Q, int64_t nq, const void* P, int64_t n, int32_t d, int32_t k,
                        int64_t id_offset, float* out_scores, int64_t* out_ids, int32_t* status, void* ws,
                        size_t ws_bytes, const float* stats, hipStream_t s) {
  DRT_REQUIRE(valid_dims(nq, n, d, k));
  if (nq == 0) return DRT_OK;
  DRT_REQUIRE(Q && out_scores && out_ids && ws);
  const TopkPlan p = make_plan(nq, n, k);
  DRT_REQUIRE(ws_bytes >= p.total);
  char* w = (char*)ws;
  float* tau = (float*)(w + p.off_tau);
  uint32_t* cnt = (uint32_t*)(w + p.off_cnt);
  const bool refine = stats != nullptr && n > 0;

  SelectArgs sa{};
  sa.k = k;
  sa.nq = nq;
  sa.out_scores = out_scores;
  sa.out_ids = out_ids;
  sa.ldo = k;
  sa.id_offset = id_offset;
  sa.status = status;
  if (refine) {   // kc candidates into the workspace, certified at k
    sa.k = (int)p.kc;
    sa.k_cert = k;
    sa.out_scores = (float*)(w + p.off_cs);
    sa.out_ids = (int64_t*)(w + p.off_ci);
    sa.ldo = p.kc;
  }
  RefineArgs ra{};
  ra.Q = (const __bf16*)Q;
  ra.nq = nq;
  ra.d = d;
  ra.P = (const __bf16*)P;
  ra.n_local = n;
  ra.row_offset = id_offset;
  ra.cs = (const float*)(w + p.off_cs);
  ra.ci = (const int64_t*)(w + p.off_ci);
  ra.kc = (int32_t)p.kc;
  ra.k = k;
  ra.stats = stats;
  ra.delta = (float*)(w + p.off_delta);
  ra.cnt = (int32_t*)(w + p.off_rcnt);
  ra.status = status;
  ra.out_s = out_scores;
  ra.out_i = out_ids;

  if (n == 0) {
    sa.in = w + p.off_keys;
    sa.in_stride = p.cap;
    sa.n_in = 0;
    sa.n_total = 0;
    return launch_select(sa, SEL_DENSE32, SEL_TOPK, s);
  }
  DRT_REQUIRE(P != nullptr);

  if (!p.sample) {
    // Small shard: score every row densely, select directly.
    ScanArgs a = scan_args(Q, nq, P, d);
    a.nrows = n;
    a.out = w + p.off_keys;
    a.cap = p.cap;
    int rc = launch_scan(a, d, SCAN_DENSE, s, PROF_SCAN);
    if (rc) return rc;
    sa.in = w + p.off_keys;
    sa.in_stride = p.cap;
    sa.n_in = n;
    sa.n_total = n;
    rc = launch_select(sa, SEL_DENSE32, SEL_TOPK, s);
    if (rc || !refine) return rc;
    ra.tau = nullptr;   // every row was scored
    return launch_refine(ra, s);
  }

  // 1. sample pass -> tau: every stride-th row, densely scored
  ScanArgs smp_a = scan_args(Q, nq, P, d);
  smp_a.row0 = p.stride / 2;
  smp_a.nrows = p.m;
  smp_a.rstride = p.stride;
  smp_a.out = w + p.off_sample;
  smp_a.cap = align_up(p.m, 4);
  int rc = launch_scan(smp_a, d, SCAN_DENSE, s, PROF_SAMPLE);
  if (rc) return rc;
  {
    const ProfPair pp = prof_begin(PROF_SELECT, s);
    const uint32_t* smp = (const uint32_t*)(w + p.off_sample);
    const int64_t ld = (int64_t)align_up(p.m, 4);
    if (kth_rank_fits(p.m, p.r)) {   // one launch: the whole sample row per work-group
      launch_kth_rank(nq, smp, ld, p.m, (int)p.r, tau, cnt, s);
    } else {
      launch_kth_partial(p.nchunk, nq, smp, ld, p.m, (int)p.r, (uint32_t*)(w + p.off_part), s);
      launch_kth_final(nq, (const uint32_t*)(w + p.off_part), (int)p.nchunk, (int)p.r, (int64_t)p.r,
                       (int64_t)(p.nchunk * p.r), tau, nullptr, cnt, (int)p.r, s);   // also zeroes the hit counters
    }
    prof_end(pp, s);
    DRT_CHECK_HIP(hipGetLastError());
  }

  // 2. filter pass (counters zeroed by the threshold kernel above: one launch fewer than a memset)
  ScanArgs a = scan_args(Q, nq, P, d);
  a.nrows = n;
  a.tau = tau;
  a.counts = cnt;
  a.out = w + p.off_keys;
  a.cap = p.cap;
  rc = launch_scan(a, d, SCAN_FILTER, s, PROF_SCAN);
  if (rc) return rc;

  // 3. select + certify (4. canonical order)
  sa.in = w + p.off_keys;
  sa.in_stride = p.cap;
  sa.counts = cnt;
  sa.cap = p.cap;
  sa.n_total = n;
  rc = launch_select(sa, SEL_KEYS64, SEL_TOPK, s);
  if (rc || !refine) return rc;
  ra.tau = tau;
  return launch_refine(ra, s);
}

}  // namespace drt

extern "C" {

int drt_ip_topk_bf16(const void* Q, int64_t nq, const void* P, int64_t n, int32_t d, int32_t k,
                     int64_t id_offset, float* out_scores, int64_t* out_ids, int32_t* status,
                     void* ws, size_t ws_bytes, void* stream) {
  return ip_topk_impl(Q, nq, P, n, d, k, id_offset, out_scores, out_ids, status, ws, ws_bytes, nullptr,
                      (hipStream_t)stream);
}

int drt_ip_topk_exact_bf16(const void* Q, int64_t nq, const void* P, int64_t n, int32_t d, int32_t k,
                           int64_t id_offset, const float* stats, float* out_scores, int64_t* out_ids,
                           int32_t* status, void* ws, size_t ws_bytes, void* stream) {
  DRT_REQUIRE(stats != nullptr);
  return ip_topk_impl(Q, nq, P, n, d, k, id_offset, out_scores, out_ids, status, ws, ws_bytes, stats,
                      (hipStream_t)stream);
}

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

// Dense exact rescan, chunked so the score buffer stays <= ~2 GB: queries per chunk.
static int64_t resolve_chunk(int64_t nbad, int64_t n) {
  const int64_t width = resolve_width(n);
  int64_t chunk = std::max<int64_t>(1, std::min<int64_t>(nbad, (2ll << 30) / (width * 4)));
  return std::min<int64_t>(chunk, kQueriesPerWG);
}

size_t drt_ip_topk_resolve_workspace(int64_t nbad, int64_t n, int32_t d) {
  if (nbad <= 0 || n < 0 || d <= 0 || d % 64 || d > 1024) return 0;
  return resolve_layout(resolve_chunk(nbad, n), n, d).total;
}

}  // extern "C"

namespace drt {

static int resolve_impl(const void* Q, int64_t nq, const void* P, int64_t n, int32_t d, int32_t k, int64_t id_offset,
                        float* out_scores, int64_t* out_ids, int32_t* status, void* ws, size_t ws_bytes,
                        int64_t* n_resolved, const float* stats, hipStream_t s) {
  DRT_REQUIRE(valid_dims(nq, n, d, k));
  if (n_resolved) *n_resolved = 0;
  if (nq == 0 || status == nullptr) return DRT_OK;
  std::vector<int32_t> st(nq);
  DRT_CHECK_HIP(hipMemcpyAsync(st.data(), status, nq * 4, hipMemcpyDeviceToHost, s));
  DRT_CHECK_HIP(hipStreamSynchronize(s));
  std::vector<int32_t> bad;
  for (int64_t i = 0; i < nq; ++i)
    if (st[i] & 1) bad.push_back((int32_t)i);
  if (bad.empty()) return DRT_OK;
  if (n_resolved) *n_resolved = (int64_t)bad.size();

  // the caller's workspace decides the chunk (drt_ip_topk_resolve_workspace(#failed, n, d)
  // bytes holds the whole default chunk); nothing is allocated here
  const int64_t width = resolve_width(n);
  int64_t chunk = resolve_chunk((int64_t)bad.size(), n);
  while (chunk > 1 && resolve_layout(chunk, n, d).total > ws_bytes) chunk >>= 1;
  const bool refine = stats != nullptr && n > 0;
  const int64_t kc = refine_width(k);
  const ResolveLayout l = resolve_layout(chunk, n, d, kc);
  DRT_REQUIRE(ws != nullptr && l.total <= ws_bytes);
  char* wp = (char*)ws;
  void* qbuf = wp + l.qbuf;
  void* sbuf = wp + l.scores;
  void* mbuf = wp + l.qmap;
  float* rcs = (float*)(wp + l.cand_s);
  int64_t* rci = (int64_t*)(wp + l.cand_i);
  float* rdl = (float*)(wp + l.delta);
  int32_t* rcn = (int32_t*)(wp + l.cnt);
  int rc = DRT_OK;
  hipError_t e;
  for (size_t b0 = 0; b0 < bad.size() && rc == DRT_OK; b0 += chunk) {
    const int64_t nb = std::min<int64_t>(chunk, (int64_t)bad.size() - (int64_t)b0);
    for (int64_t i = 0; i < nb; ++i) {
      e = hipMemcpyAsync((char*)qbuf + i * d * 2, (const char*)Q + (int64_t)bad[b0 + i] * d * 2, d * 2,
                         hipMemcpyDeviceToDevice, s);
      if (e != hipSuccess) { rc = (int)e; break; }
    }
    if (rc) break;
    if ((e = hipMemcpyAsync(mbuf, bad.data() + b0, nb * 4, hipMemcpyHostToDevice, s)) != hipSuccess) {
      rc = (int)e;
      break;
    }
    ScanArgs a = scan_args(qbuf, nb, P, d);
    a.nrows = n;
    a.out = sbuf;
    a.cap = width;
    rc = launch_scan(a, d, SCAN_DENSE, s, -1);
    if (rc) break;
    SelectArgs sa{};
    sa.in = sbuf;
    sa.in_stride = width;
    sa.n_in = n;
    sa.n_total = n;
    sa.k = k;
    sa.nq = nb;
    sa.out_scores = out_scores;
    sa.out_ids = out_ids;
    sa.ldo = k;
    sa.id_offset = id_offset;
    sa.status = status;
    sa.qmap = (const int32_t*)mbuf;
    if (refine) {   // kc candidates of the chunk, then the canonical order into the caller's rows
      sa.k = (int)kc;
      sa.k_cert = k;
      sa.out_scores = rcs;
      sa.out_ids = rci;
      sa.ldo = kc;
      sa.status = nullptr;
      sa.qmap = nullptr;
    }
    rc = launch_select(sa, SEL_DENSE32, SEL_TOPK, s);
    if (rc) break;
    if (refine) {
      RefineArgs ra{};
      ra.Q = (const __bf16*)qbuf;
      ra.nq = nb;
      ra.d = d;
      ra.P = (const __bf16*)P;
      ra.n_local = n;
      ra.row_offset = id_offset;
      ra.cs = rcs;
      ra.ci = rci;
      ra.kc = (int32_t)kc;
      ra.k = k;
      ra.stats = stats;
      ra.tau = nullptr;
      ra.delta = rdl;
      ra.cnt = rcn;
      ra.status = status;
      ra.qmap = (const int32_t*)mbuf;
      ra.set_status = true;
      ra.out_s = out_scores;
      ra.out_i = out_ids;
      rc = launch_refine(ra, s);
      if (rc) break;
    }
    if ((e = hipStreamSynchronize(s)) != hipSuccess) { rc = (int)e; break; }
  }
  const hipError_t se = hipStreamSynchronize(s);
  return rc != DRT_OK ? rc : (se == hipSuccess ? DRT_OK : (int)se);
}

}  // namespace drt

extern "C" {

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
  std::vector<int32_t> st(nq);
  DRT_CHECK_HIP(hipMemcpyAsync(st.data(), status, nq * 4, hipMemcpyDeviceToHost, s));
  DRT_CHECK_HIP(hipStreamSynchronize(s));
  std::vector<int32_t> wide;   // order not certified and the fp32 top-k itself certified
  for (int64_t i = 0; i < nq; ++i)
    if ((st[i] & 3) == 2) wide.push_back((int32_t)i);
  if (wide.empty()) return DRT_OK;
  const int64_t B = kQueriesPerWG;
  char* wp = (char*)ws;
  char* qbuf = wp + l.qbuf;
  int32_t* qmap = (int32_t*)(wp + l.qmap);
  float* tau = (float*)(wp + l.tau);
  uint32_t* counts = (uint32_t*)(wp + l.counts);
  uint64_t* keys = (uint64_t*)(wp + l.keys);
  uint64_t* ekeys = (uint64_t*)(wp + l.ekeys);
  for (size_t b0 = 0; b0 < wide.size(); b0 += B) {
    const int nb = (int)std::min<int64_t>(B, (int64_t)wide.size() - (int64_t)b0);
    for (int i = 0; i < nb; ++i)
      DRT_CHECK_HIP(hipMemcpyAsync(qbuf + (int64_t)i * d * 2, (const char*)Q + (int64_t)wide[b0 + i] * d * 2, d * 2,
                                   hipMemcpyDeviceToDevice, s));
    DRT_CHECK_HIP(hipMemcpyAsync(qmap, wide.data() + b0, nb * 4, hipMemcpyHostToDevice, s));
    WideArgs w{};
    w.ra.Q = (const __bf16*)qbuf;
    w.ra.d = d;
    w.ra.P = (const __bf16*)P;
    w.ra.stats = stats;
    w.qmap = qmap;
    w.nb = nb;
    w.k = k;
    w.tau = tau;
    w.counts = counts;
    w.keys = keys;
    w.ekeys = ekeys;
    w.cap = kWideCap;
    w.id_offset = id_offset;
    w.out_s = out_scores;
    w.out_i = out_ids;
    w.status = status;
    hipLaunchKernelGGL(wide_prep_kernel, dim3((unsigned)B), dim3(kRefThreads), 0, s, w);
    DRT_CHECK_HIP(hipGetLastError());
    ScanArgs a = scan_args(qbuf, nb, P, d);
    a.nrows = n;
    a.tau = tau;
    a.counts = counts;
    a.out = keys;
    a.cap = kWideCap;
    const int rc = launch_scan(a, d, SCAN_FILTER, s, -1);   // (not a headline filter launch)
    if (rc) return rc;
    hipLaunchKernelGGL(wide_exact_kernel, dim3((unsigned)nb, (unsigned)(kWideCap / kWideSlice)), dim3(kRefThreads), 0,
                       s, w);
    hipLaunchKernelGGL(wide_select_kernel, dim3((unsigned)nb), dim3(kWideThreads), 0, s, w);
    DRT_CHECK_HIP(hipGetLastError());
  }
  std::vector<int32_t> st2(nq);
  DRT_CHECK_HIP(hipMemcpyAsync(st2.data(), status, nq * 4, hipMemcpyDeviceToHost, s));
  DRT_CHECK_HIP(hipStreamSynchronize(s));
  int64_t nres = 0;
  for (int32_t i : wide) nres += (st2[i] & 2) == 0 ? 1 : 0;
  if (n_resolved) *n_resolved = nres;
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
  float* tauc = (float*)(wp + l.wide.tau);
  uint32_t* counts = (uint32_t*)(wp + l.wide.counts);
  uint64_t* keys = (uint64_t*)(wp + l.wide.keys);
  uint64_t* ekeys = (uint64_t*)(wp + l.wide.ekeys);
  uint64_t* sel_k = (uint64_t*)(wp + l.sel_k);
  uint32_t* sel_r = (uint32_t*)(wp + l.sel_r);
  uint32_t* sel_n = (uint32_t*)(wp + l.sel_n);
  uint64_t* bin_k = (uint64_t*)(wp + l.bin_k);
  uint32_t* bin_r = (uint32_t*)(wp + l.bin_r);
  for (int64_t b0 = 0; b0 < nq; b0 += B) {
    const int nb = (int)std::min<int64_t>(B, nq - b0);
    WideArgs w{};
    w.ra.Q = (const __bf16*)Q + b0 * d;
    w.ra.d = d;
    w.ra.P = (const __bf16*)P;
    w.ra.stats = stats;
    w.qmap = nullptr;
    w.q0 = b0;
    w.tau_in = tau;
    w.nb = nb;
    w.k = k;
    w.tau = tauc;
    w.counts = counts;
    w.keys = keys;
    w.ekeys = ekeys;
    w.cap = kWideCap;
    w.id_offset = id_offset;
    w.out_s = out_scores;
    w.out_i = out_ids;
    w.status = status;
    w.sel_k = sel_k;
    w.sel_r = sel_r;
    w.sel_n = sel_n;
    w.bin_k = bin_k;
    w.bin_r = bin_r;
    w.out_keys = out_keys;
    hipLaunchKernelGGL(wide_prep_kernel, dim3((unsigned)B), dim3(kRefThreads), 0, s, w);
    DRT_CHECK_HIP(hipGetLastError());
    if (n > 0) {
      ScanArgs a = scan_args(w.ra.Q, nb, P, d);
      a.nrows = n;
      a.tau = tauc;
      a.counts = counts;
      a.out = keys;
      a.cap = kWideCap;
      const int rc = launch_scan(a, d, SCAN_FILTER, s, -1);
      if (rc) return rc;
      hipLaunchKernelGGL(wide_exact_kernel, dim3((unsigned)nb, (unsigned)(kWideCap / kWideSlice)), dim3(kRefThreads),
                         0, s, w);
    }
    hipLaunchKernelGGL(large_select_kernel, dim3((unsigned)nb), dim3(kWideThreads), 0, s, w);
    hipLaunchKernelGGL(large_rank_kernel, dim3((unsigned)nb), dim3(kLargeThreads), 0, s, w);
    DRT_CHECK_HIP(hipGetLastError());
  }
  return DRT_OK;
}

int drt_ip_topk_resolve(const void* Q, int64_t nq, const void* P, int64_t n, int32_t d, int32_t k,
                        int64_t id_offset, float* out_scores, int64_t* out_ids, int32_t* status,
                        void* ws, size_t ws_bytes, int64_t* n_resolved, void* stream) {
  return resolve_impl(Q, nq, P, n, d, k, id_offset, out_scores, out_ids, status, ws, ws_bytes, n_resolved, nullptr,
                      (hipStream_t)stream);
}

int drt_ip_topk_resolve_exact(const void* Q, int64_t nq, const void* P, int64_t n, int32_t d, int32_t k,
                              int64_t id_offset, const float* stats, float* out_scores, int64_t* out_ids,
                              int32_t* status, void* ws, size_t ws_bytes, int64_t* n_resolved, void* stream) {
  DRT_REQUIRE(stats != nullptr);
  return resolve_impl(Q, nq, P, n, d, k, id_offset, out_scores, out_ids, status, ws, ws_bytes, n_resolved, stats,
                      (hipStream_t)stream);
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

// ---------------------------------------------------------------------------
// Distributed exact top-k with ONE global threshold (see include/drt.h).
// ---------------------------------------------------------------------------
int32_t drt_ip_topk_sample_rank(int32_t k) {
  if (k < 1 || k > kSelMaxK) return -1;
  const TopkPlan p = make_plan(1, (int64_t)0xFFFFFFFEll, k);
  return (int32_t)p.r;
}

size_t drt_ip_topk_dist_workspace(int64_t nq, int64_t n_local, int64_t n_global, int32_t d, int32_t k) {
  if (!valid_dist_dims(nq, n_local, n_global, d, k)) return 0;
  return make_dist_plan(nq, n_local, n_global, k).total;
}

int drt_ip_topk_dist_sample(const void* Q, int64_t nq, const void* P, int64_t n_local, int64_t n_global, int32_t d,
                            int32_t k, uint32_t* best, void* ws, size_t ws_bytes, void* stream) {
  DRT_REQUIRE(valid_dist_dims(nq, n_local, n_global, d, k));
  if (nq == 0) return DRT_OK;
  DRT_REQUIRE(Q && best && ws);
  const TopkPlan p = make_dist_plan(nq, n_local, n_global, k);
  DRT_REQUIRE(ws_bytes >= p.total);
  const int64_t r = drt_ip_topk_sample_rank(k);
  hipStream_t s = (hipStream_t)stream;
  if (!p.sample || n_local == 0) {
    // global corpus fits one filter pass (or this shard is empty): contribute no sample
    DRT_CHECK_HIP(hipMemsetAsync(best, 0xFF, (size_t)nq * r * 4, s));
    return DRT_OK;
  }
  DRT_REQUIRE(P != nullptr);
  char* w = (char*)ws;
  ScanArgs a = scan_args(Q, nq, P, d);
  a.row0 = p.stride / 2;
  a.nrows = p.m;
  a.rstride = p.stride;
  a.out = w + p.off_sample;
  // top-r sample pass (SCAN_TOPR): 4 lists of kTopRL keys per query and work-group column, their union's
  // r-th best in one kth_final launch -- when the union fits kth_final's 4096 keys and the sample buffer
  const int64_t nlists = 4 * (int64_t)scan16_grid(nq, p.m).x;
  if (nlists * kTopRL <= kKthChunk && nlists * kTopRL <= align_up(p.m, 4)) {
    a.cap = nlists * kTopRL;
    DRT_CHECK_HIP(hipMemsetAsync(a.out, 0xFF, (size_t)nq * a.cap * 4, s));
    int rc = launch_scan(a, d, SCAN_TOPR, s, PROF_SAMPLE);
    if (rc) return rc;
    const ProfPair pp = prof_begin(PROF_SELECT, s);
    launch_kth_final(nq, (const uint32_t*)a.out, (int)nlists, (int)r, (int64_t)kTopRL, (int64_t)a.cap, nullptr, best,
                     nullptr, kTopRL, s);
    prof_end(pp, s);
    return hip_status(hipGetLastError());
  }
  a.cap = align_up(p.m, 4);
  int rc = launch_scan(a, d, SCAN_DENSE, s, PROF_SAMPLE);
  if (rc) return rc;
  const ProfPair pp = prof_begin(PROF_SELECT, s);
  // fewer than r sampled rows: kth_partial pads its list with 0xFFFFFFFF
  launch_kth_partial(p.nchunk, nq, (const uint32_t*)(w + p.off_sample), (int64_t)align_up(p.m, 4), p.m, (int)r,
                     (uint32_t*)(w + p.off_part), s);
  launch_kth_final(nq, (const uint32_t*)(w + p.off_part), (int)p.nchunk, (int)r, (int64_t)r, (int64_t)(p.nchunk * r),
                   nullptr, best, nullptr, (int)r, s);
  prof_end(pp, s);
  return hip_status(hipGetLastError());
}

int drt_ip_topk_dist_tau(const uint32_t* lists, int64_t nq, int32_t nlists, int32_t k, float* tau, void* stream) {
  const int32_t r = drt_ip_topk_sample_rank(k);
  DRT_REQUIRE(r > 0 && nq >= 0 && nlists >= 1 && (int64_t)nlists * r <= kKthChunk);
  if (nq == 0) return DRT_OK;
  DRT_REQUIRE(lists && tau);
  launch_kth_final(nq, lists, (int)nlists, (int)r, (int64_t)nq * r, (int64_t)r, tau, nullptr, nullptr, (int)r,
                   (hipStream_t)stream);
  return hip_status(hipGetLastError());
}

// The filter step: scan the shard against a threshold per query, one select over the hits.  The five entry
// points below differ in where the threshold comes from and in how the shard is cut into scan launches,
// and share the rest through four helpers, called in this order:
//   filter_setup    every check that precedes the first HIP call, the plan, the select's arguments and
//                   the ScanArgs of one launch over the whole shard
//   (the entry's own work before the scan: the fused form's threshold kernel, the passes' copies)
//   filter_begin    a non-empty shard only: the corpus pointer check, the hit counters zeroed
//   launch_scan     once per launch the entry wants: a copy of FilterRun::scan with that launch's
//                   threshold, rows and exp_hits (rows_exp_hits / pass_exp_hits above)
//   filter_select   the select over the hit lists, or over nothing for an empty shard
struct FilterRun {
  TopkPlan p;
  hipStream_t s;
  char* w;         // the workspace
  uint32_t* cnt;   // the hit counters in it
  SelectArgs sel;
  ScanArgs scan;
};

// `thr` is the entry's threshold source (tau, or the sample lists).  DRT_OK with nq == 0: nothing to do.
static int filter_setup(FilterRun& f, const void* Q, int64_t nq, const void* P, int64_t n_local, int64_t n_global,
                        int32_t d, int32_t k, int64_t id_offset, const void* thr, uint64_t* packed, void* ws,
                        size_t ws_bytes, void* stream) {
  DRT_REQUIRE(valid_dist_dims(nq, n_local, n_global, d, k));
  DRT_REQUIRE(id_offset >= 0 && id_offset + n_local <= n_global);
  if (nq == 0) return DRT_OK;
  DRT_REQUIRE(Q && thr && packed && ws);
  f.p = make_dist_plan(nq, n_local, n_global, k);
  DRT_REQUIRE(ws_bytes >= f.p.total);
  f.s = (hipStream_t)stream;
  f.w = (char*)ws;
  f.cnt = (uint32_t*)(f.w + f.p.off_cnt);
  f.sel = SelectArgs{};
  f.sel.in = f.w + f.p.off_keys;
  f.sel.in_stride = f.p.cap;
  f.sel.k = k;
  f.sel.nq = nq;
  f.sel.id_offset = id_offset;
  f.sel.out_packed = packed;
  f.sel.global_tau = true;
  f.scan = scan_args(Q, nq, P, d);
  f.scan.nrows = n_local;
  f.scan.counts = f.cnt;
  f.scan.out = f.w + f.p.off_keys;
  f.scan.cap = f.p.cap;
  return DRT_OK;
}

// zero_counts false: the entry's threshold kernel has zeroed the counters (one launch fewer)
static int filter_begin(const FilterRun& f, bool zero_counts) {
  DRT_REQUIRE(f.scan.P != nullptr);
  if (zero_counts) DRT_CHECK_HIP(hipMemsetAsync(f.cnt, 0, f.p.nq_pad * 4 * kCntStride, f.s));
  return DRT_OK;
}

static int filter_select(FilterRun& f) {
  if (f.p.n == 0) return launch_select(f.sel, SEL_DENSE32, SEL_TOPK, f.s);   // n_in = n_total = 0: empty lists
  f.sel.counts = f.cnt;
  f.sel.cap = f.p.cap;
  f.sel.n_total = f.p.n;
  return launch_select(f.sel, SEL_KEYS64, SEL_TOPK, f.s);
}

// One launch over the whole shard.
int drt_ip_topk_dist_filter(const void* Q, int64_t nq, const void* P, int64_t n_local, int64_t n_global, int32_t d,
                            int32_t k, int64_t id_offset, const float* tau, uint64_t* packed, void* ws,
                            size_t ws_bytes, void* stream) {
  FilterRun f;
  int rc = filter_setup(f, Q, nq, P, n_local, n_global, d, k, id_offset, tau, packed, ws, ws_bytes, stream);
  if (rc || nq == 0) return rc;
  if (n_local > 0) {
    if ((rc = filter_begin(f, true))) return rc;
    ScanArgs a = f.scan;
    a.tau = tau;
    a.exp_hits = rows_exp_hits(f.p, n_local, n_global);
    if ((rc = launch_scan(a, d, SCAN_FILTER, f.s, PROF_SCAN))) return rc;
  }
  return filter_select(f);
}

// dist_filter over a shard in row chunks with ONE hit list and ONE select: chunk c = rows
// [starts[c], starts[c + 1]) (host array, starts[0] = 0, starts[nchunks] = n_local) is one scan launch
// (a grouped launch's query blocks stay in step over a chunk, so each tile comes from HBM once), every
// chunk appends to the same per-query key lists (keys carry shard rows: row_base = the chunk's start),
// and the select runs once over the shard's hits -- the packed lists equal drt_ip_topk_dist_filter's
// over the whole shard.  (Round 5: replaces one select per chunk plus a merge of the chunks' lists.)
// Chunks of a shard whose rows need the strided / wide-row kernels (d > 768) are not supported.
int drt_ip_topk_dist_filter_chunks(const void* Q, int64_t nq, const void* P, int64_t n_local, int64_t n_global,
                                   int32_t d, int32_t k, int64_t id_offset, const float* tau, uint64_t* packed,
                                   const int64_t* starts, int32_t nchunks, void* ws, size_t ws_bytes, void* stream) {
  DRT_REQUIRE(d <= 768 && n_local < ((int64_t)1 << 32));
  DRT_REQUIRE(starts != nullptr && nchunks >= 1 && starts[0] == 0 && starts[nchunks] == n_local);
  for (int c = 0; c < nchunks; ++c) DRT_REQUIRE(starts[c] <= starts[c + 1]);
  FilterRun f;
  int rc = filter_setup(f, Q, nq, P, n_local, n_global, d, k, id_offset, tau, packed, ws, ws_bytes, stream);
  if (rc || nq == 0) return rc;
  if (n_local > 0) {
    if ((rc = filter_begin(f, true))) return rc;
    for (int c = 0; c < nchunks; ++c) {
      const int64_t r0 = starts[c], rows = starts[c + 1] - starts[c];
      if (rows == 0) continue;
      ScanArgs a = f.scan;
      a.P += r0 * d;
      a.nrows = rows;
      a.row_base = (uint32_t)r0;
      a.tau = tau;
      a.exp_hits = rows_exp_hits(f.p, rows, n_global);   // the chunk's rows, not the shard's
      if ((rc = launch_scan(a, d, SCAN_FILTER, f.s, PROF_SCAN))) return rc;
    }
  }
  return filter_select(f);
}

// Rank of the tightened threshold (drt_ip_topk_filter_passes): with C = shard tiles / first-pass tiles, the
// rows at or above the first pass's r-th best score number C r on average over the shard, with standard
// deviation sqrt(C (C - 1) r + (C - 1) r) (the order statistic's relative 1 / sqrt(r) on the tail
// probability, plus the Poisson count of the other passes' rows); the smallest r that keeps the mean 5
// sigma above k.  0: nothing to tighten (one pass, or the first pass holds every tile).
int32_t drt_ip_topk_tighten_rank(int64_t n_local, int32_t npasses, int32_t k) {
  if (n_local <= 0 || npasses <= 1 || k < 1) return 0;
  const int64_t tall = (n_local + kT16 - 1) / kT16;
  const int64_t t0 = (tall + npasses - 1) / npasses;   // tiles t % npasses == 0
  if (t0 >= tall) return 0;
  const double C = (double)tall / (double)t0;
  for (int64_t r = 1; r < ((int64_t)1 << 24); ++r) {
    const double sigma = std::sqrt(C * (C - 1.0) * (double)r + (C - 1.0) * (double)r);
    if (C * (double)r - 5.0 * sigma >= (double)k) return (int32_t)r;
  }
  return 0;
}

size_t drt_ip_topk_filter_passes_workspace(int64_t nq, int64_t n_local, int64_t n_global, int32_t d, int32_t k) {
  if (!valid_dist_dims(nq, n_local, n_global, d, k)) return 0;
  const TopkPlan p = make_dist_plan(nq, n_local, n_global, k);
  return passes_layout(p.total, p.nq_pad).total;
}

// dist_filter over a shard as `npasses` interleaved passes with ONE hit list and ONE select: pass p is
// one scan launch over the 16-row tiles t with t % npasses == p (a strided sample of the shard, like the
// sample pass's rows -- not its first rows, which a corpus ordered by source or topic makes
// unrepresentative).  Pass 0 filters against tau; tighten_kernel then raises each query's threshold to
// tau1 = its r-th best collected score (r > 0; r < 0: drt_ip_topk_tighten_rank; 0: every pass against
// tau) and passes 1.. filter against tau1, appending to the same lists.  A tightened list holds every row
// >= tau1 plus pass-0 rows in [tau, tau1), so the select certifies it by r_eff + (later passes' hits) >=
// k (SelectArgs::pass0): then its best k keys all score >= tau1 and the packed list equals
// drt_ip_topk_dist_filter's over the whole shard; otherwise flag bit 0 is set and the merge leaves the
// query uncertified.  tau1_out [nq] / pass0_out [nq][4] (c0, r_eff, tightened, 0): optional copies.
// d <= 768 (the lean filter kernels).  Meant for a shard that is the whole corpus: under a global
// threshold of several shards a short local list is normal and a local r-th best proves nothing.
int drt_ip_topk_filter_passes(const void* Q, int64_t nq, const void* P, int64_t n_local, int64_t n_global,
                              int32_t d, int32_t k, int64_t id_offset, const float* tau, uint64_t* packed,
                              int32_t npasses, int32_t r, float* tau1_out, uint32_t* pass0_out, void* ws,
                              size_t ws_bytes, void* stream) {
  DRT_REQUIRE(d <= 768 && n_local < ((int64_t)1 << 32) && npasses >= 1 && npasses <= 1024);
  FilterRun f;
  int rc = filter_setup(f, Q, nq, P, n_local, n_global, d, k, id_offset, tau, packed, ws, ws_bytes, stream);
  if (rc || nq == 0) return rc;
  const PassesLayout pl = passes_layout(f.p.total, f.p.nq_pad);
  DRT_REQUIRE(ws_bytes >= pl.total);
  if (r < 0) r = drt_ip_topk_tighten_rank(n_local, npasses, k);
  const int tall = (int)((n_local + kT16 - 1) / kT16);
  const bool tighten = r > 0 && n_local > 0 && pass_tiles(tall, npasses, 0) < tall;
  if (!tighten) {
    if (tau1_out) DRT_CHECK_HIP(hipMemcpyAsync(tau1_out, tau, (size_t)nq * 4, hipMemcpyDeviceToDevice, f.s));
    if (pass0_out) DRT_CHECK_HIP(hipMemsetAsync(pass0_out, 0, (size_t)nq * 16, f.s));
  }
  float* tau1 = tau1_out ? tau1_out : (float*)(f.w + f.p.off_tau);
  uint32_t* pass0 = pass0_out ? pass0_out : (uint32_t*)(f.w + pl.off_pass0);
  if (n_local > 0) {
    if ((rc = filter_begin(f, true))) return rc;
    for (int ps = 0; ps < npasses; ++ps) {
      if (pass_tiles(tall, npasses, ps) == 0) continue;
      ScanArgs a = f.scan;
      a.npass = npasses;
      a.pass = ps;
      a.tau = (tighten && ps > 0) ? tau1 : tau;
      a.exp_hits = pass_exp_hits(f.p, npasses, n_global);   // the shard's share over the passes
      if ((rc = launch_scan(a, d, SCAN_FILTER, f.s, PROF_SCAN))) return rc;
      if (tighten && ps == 0) {
        const ProfPair pp = prof_begin(PROF_SELECT, f.s);
        launch_tighten(nq, (const uint64_t*)f.scan.out, f.p.cap, f.cnt, tau, (int)r, tau1, pass0, f.s);
        prof_end(pp, f.s);
        DRT_CHECK_HIP(hipGetLastError());
      }
    }
  }
  f.sel.pass0 = tighten ? pass0 : nullptr;
  return filter_select(f);
}

// dist_tau + dist_filter in one call: the threshold kernel also zeroes the hit counters,
// so the step is 3 launches (tau, filter scan, select) instead of 4 plus a host round trip.
int drt_ip_topk_dist_filter_lists(const void* Q, int64_t nq, const void* P, int64_t n_local, int64_t n_global,
                                  int32_t d, int32_t k, int64_t id_offset, const uint32_t* lists, int32_t nlists,
                                  float* tau_out, uint64_t* packed, void* ws, size_t ws_bytes, void* stream) {
  const int32_t r = drt_ip_topk_sample_rank(k);
  return drt_ip_topk_dist_filter_lists_at(Q, nq, P, n_local, n_global, d, k, id_offset, lists, nlists,
                                          r > 0 ? nq * r : 0, tau_out, packed, ws, ws_bytes, stream);
}

// The same for the query rows [q0, q0 + nq) of lists gathered for a larger query set: list j of
// this batch starts at lists + j * lists_stride (u32 elements), rows r apart.
int drt_ip_topk_dist_filter_lists_at(const void* Q, int64_t nq, const void* P, int64_t n_local, int64_t n_global,
                                     int32_t d, int32_t k, int64_t id_offset, const uint32_t* lists, int32_t nlists,
                                     int64_t lists_stride, float* tau_out, uint64_t* packed, void* ws,
                                     size_t ws_bytes, void* stream) {
  const int32_t r = drt_ip_topk_sample_rank(k);
  DRT_REQUIRE(r > 0 && nlists >= 1 && (int64_t)nlists * r <= kKthChunk);
  DRT_REQUIRE(nlists == 1 || lists_stride >= nq * r);
  FilterRun f;
  int rc = filter_setup(f, Q, nq, P, n_local, n_global, d, k, id_offset, lists, packed, ws, ws_bytes, stream);
  if (rc || nq == 0) return rc;
  float* tau = tau_out ? tau_out : (float*)(f.w + f.p.off_tau);
  launch_kth_final(nq, lists, (int)nlists, (int)r, lists_stride, (int64_t)r, tau, nullptr,
                   n_local > 0 ? f.cnt : nullptr, (int)r, f.s);
  DRT_CHECK_HIP(hipGetLastError());
  if (n_local > 0) {
    if ((rc = filter_begin(f, false))) return rc;   // counters zeroed by the threshold kernel: no memset
    ScanArgs a = f.scan;
    a.tau = tau;
    a.exp_hits = rows_exp_hits(f.p, n_local, n_global);
    if ((rc = launch_scan(a, d, SCAN_FILTER, f.s, PROF_SCAN))) return rc;
  }
  return filter_select(f);
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
