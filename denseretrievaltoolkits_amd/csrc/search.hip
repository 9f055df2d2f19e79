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
// "Multi-GPU: global-threshold protocol".  This unit holds step 2's three scan
// kernels with launch_scan, the planner and the entries that drive the steps
// (ip_topk, the dense resolve, the drt_ip_topk_dist_* / filter entries, which
// share the filter_* helpers); its host side starts at "Host-side planning and
// launch helpers".  The other kernels are reached through the host launchers of
// search_internal.h (device code is not relocatable: a kernel is launched only
// from the unit that defines it): select.hip has the select, kth_* and tighten
// kernels of steps 1-3; refine.hip step 5, its "Error bound", the wide resolve
// and large k (both call launch_scan here); merge.hip the per-shard list merges.
#include <cmath>
#include <type_traits>

#include "profile.h"
#include "search_internal.h"

namespace drt {

constexpr int kHitCap = 1024;       // LDS hit list entries per work-group
// SCAN_TOPR (the grouped sample pass, round 6): instead of writing every sampled score, each lane keeps
// the kTopRL best keys of its query over the rows it sees (its 4 rows of every tile of its work-group)
// in registers and writes that list once; the union of a query's lists (4 per work-group column) holds
// every sampled key that beats all but kTopRL - 1 of its list-mates, so its r-th best is the r-th best
// sampled key unless more than kTopRL of the r best fell into one lane's share (then a slightly lower
// threshold: more filter hits, never a wrong result -- the filter's counts certify).  Round 5 wrote a
// [2048, 70.8k] u32 score matrix per group (580 MB) for kth_partial to read back.
constexpr int kTopRL = 4;

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

// Loader-half issue for ip_scan32r: FOUR waves (one per SIMD, lw = wave & 3) issue a whole tile, G =
// GLDS_PER_TILE / 4 pieces each (6 at d = 768); called from those waves only.  Piece j of loader wave lw
// is wave-instruction J = 4 j + lw of the tile image: chunk group 2 j + (lw >> 1), row half lw & 1, so a
// lane's source offset for piece j is its offset for piece 0 plus j x 256 B and the LDS destination moves
// by 4 KiB: ONE voff VGPR, the instruction's immediate offset (<= 1,280) and one s_add per piece.  The
// immediate offset of an LDS-DMA load is added to the global AND the LDS address, so piece j's m0 is the
// slot's piece-0 address + j x (4,096 - 256).  Same bytes to the same LDS addresses as LeanTile<D, 8> /
// issue_tile16.  A short last tile takes the same statement with the lane's row clamped to the shard's
// last row (the source only: the LDS position keeps the lane's own row, as in issue_tile16), so every
// tile is G pieces for its loader wave.
// Widths whose piece count is not a multiple of four (d = 64, 192, 320, ...) are not issued this way.
template <int D>
struct HalfTile {
  using C = Scan16Cfg<D, 4>;
  static constexpr bool kOk = C::GLDS_PER_TILE % 4 == 0 && C::GLDS_PER_TILE <= 24;
  static constexpr int G = C::GLDS_PER_TILE / 4;
  uint32_t voff;   // per lane: byte offset of its 16-B chunk of piece 0 from the tile's first row
  uint32_t loff;   // wave-uniform: LDS byte offset of piece 0 within a slot
  __device__ __forceinline__ void init(const ScanArgs& a, int wave, int lane) {
    const int lw = wave & 3;
    const int row = ((lw & 1) << 3) + (lane >> 3);
    const int c = (lane & 7) ^ ((row >> 1) & 7);
    voff = (uint32_t)((row * a.ldp + (lw >> 1) * 64 + c * 8) * 2);
    loff = (uint32_t)__builtin_amdgcn_readfirstlane(lw * 1024);
  }
  // `base` = the tile's first row; `partial` = the shard's last tile and it is short; `tile` = its index
  // in the shard
  __device__ __forceinline__ void issue(const ScanArgs& a, uint32_t slot_lds, const char* base, bool partial,
                                        int tile, int wave, int lane) {
    static_assert(kOk, "loader half: a multiple of four pieces per tile");
    uint32_t v = voff;
    if (partial) {
      const int row = ((wave & 1) << 3) + (lane >> 3);
      const int last = (int)(a.nrows - 1 - (int64_t)tile * kT16);   // 0 .. 14
      if (row > last) v -= (uint32_t)((row - last) * a.ldp * 2);
    }
    const uint32_t l0 = slot_lds + loff;
    uint32_t keep;
#define DRT_HALF_PIECE(LDS, OFF) \
  "s_add_u32 m0, %2, " #LDS "\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %3, %1 offset:" #OFF "\n\t"
#define DRT_HALF_ISSUE(PIECES) \
  asm volatile("s_mov_b32 %0, m0\n\t" PIECES "s_mov_b32 m0, %0" : "=&s"(keep) : "s"(base), "s"(l0), "v"(v) : "memory", "scc")
#define DRT_HP0 DRT_HALF_PIECE(0, 0)
#define DRT_HP1 DRT_HP0 DRT_HALF_PIECE(3840, 256)
#define DRT_HP2 DRT_HP1 DRT_HALF_PIECE(7680, 512)
#define DRT_HP3 DRT_HP2 DRT_HALF_PIECE(11520, 768)
#define DRT_HP4 DRT_HP3 DRT_HALF_PIECE(15360, 1024)
#define DRT_HP5 DRT_HP4 DRT_HALF_PIECE(19200, 1280)
    if constexpr (G == 1) DRT_HALF_ISSUE(DRT_HP0);
    else if constexpr (G == 2) DRT_HALF_ISSUE(DRT_HP1);
    else if constexpr (G == 3) DRT_HALF_ISSUE(DRT_HP2);
    else if constexpr (G == 4) DRT_HALF_ISSUE(DRT_HP3);
    else if constexpr (G == 5) DRT_HALF_ISSUE(DRT_HP4);
    else DRT_HALF_ISSUE(DRT_HP5);
#undef DRT_HP5
#undef DRT_HP4
#undef DRT_HP3
#undef DRT_HP2
#undef DRT_HP1
#undef DRT_HP0
#undef DRT_HALF_ISSUE
#undef DRT_HALF_PIECE
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
// during its own tile (and, its first RD fragments, at the end of the tile before).  A tile's epilogue
// runs after the next tile's MFMAs are issued (two accumulator sets alternate), as in ip_scan16r.
// Every score is the same 24-step 16x16x32 chain as ip_scan16r's: identical values and hits.
// Hit check, per 16-query set and tile: 3 VALU instructions, a hazard pad and a branch when the set has no
//   hit in the tile (s_nop 2, v_max3, v_max in one asm statement, then v_cmp mx >= tau; it was 7 VALU: two
//   canonicalising self-maxima, a subtraction to compare with 0 and the row bound ahead of the branch).
//   The pad is the statement's own, see there: the compiler pads nothing inside an asm statement.  With a
//   hit, each of the lane's four rows is tested acc >= tau and balloted; the row bound (row < nrows) is
//   tested only in the epilogue after the loop, the one place the shard's short last tile can be.  At the
//   product's densities a third (passes 1-7, 233 hits per query) to more than a half (pass 0, 515) of the
//   set-tiles take the four row tests, and the launch time fell there, not on the no-hit side (measured
//   without the pad, HIP events, one job: 0 hits 2.917 -> 2.915 ms, 233 hits 2.971 -> 2.920, 515 hits
//   3.049 -> 2.985; with it and against the parent in profiles/r13a).
// Hit flush: a wave's full segment (kSeg = 128 entries) is flushed by that wave, blocking: one returning
//   atomic per hit, s_waitcnt vmcnt(0), the stores (wave_flush_hits).  About 58 flushes per wave and
//   launch at 233 hits per query.  Splitting the segment into halves whose atomics are issued at overflow
//   and whose stores follow a tile later (the positions kept in a register meanwhile) measured level with
//   the blocking flush or behind it, alone and with the check above; so did 192-entry segments
//   (profiles/r13a/variants_explore.txt).
// Ring protocol: ONE wait + work-group barrier per PAIR of tiles (it, it+1), it even; slot of tile t is
// t mod 6; the tile at loop index j refills slot(j-2) with tile j+4 early in its MFMAs.
//   Who issues a tile (loader half; widths with a multiple of four DMA pieces per tile: d = 128, 256,
//   .. 768): waves 4-7, one per SIMD -- wave w and w+4 share a SIMD, and waves 4-7 are the ones that run
//   at s_setprio 1.  They issue every tile WHOLE (HalfTile: 6 pieces per wave at d = 768), in the
//   prologue and in the loop alike, at k-step KS/12 (2 at d = 768); waves 0-3 issue no DMA at all and
//   keep the SIMD's matrix pipe fed while their partner issues.  Measured at d = 768 (profiles/r12a):
//   ahead of the eight-wave issue in every run; the halves taking turns (tile t by half t & 1), waves
//   0-3 as the loaders, the pieces spread over k-steps and a raised priority for the burst all slower.
//   The short last tile of a shard is issued the same way (HalfTile clamps the source row), so a loader
//   wave has G pieces in flight per tile and the other waves none.
//   The other widths (d = 64, 192, 320, ..: 2, 6, 10, .. pieces) keep the eight-wave issue at k-step
//   KS/4 (LeanTile: every wave GLDS_PER_WAVE pieces of every tile, duplicates for the remainder); for
//   them read "every wave" for "a loader wave" below.
//   At the pair's barrier (before even loop index it) tiles .. it+3 have been issued:
//     a loader wave waits for all but its newest tile, vmcnt(G): it+1 and it+2 have landed, it+3 may
//       stay outstanding; where it+3 does not exist (it+3 >= my_tiles) it waits for everything;
//     waves 0-3 hold no tile: their wait is vmcnt(0) (their own hit stores at most).
//   (it+2 must have landed because the last RD k-steps of it+1 read its first fragments; tile it was
//   certified by the pair before.)  The barrier certifies
//     RAW: every loader's share of tiles it+1 and it+2 has landed;
//     WAR: every wave has issued all MFMAs of tiles it-2 and it-1, hence finished reading those slots
//          (each MFMA waited for its own fragment) -- they are refilled with it+4 (during tile it) and
//          it+5 (during it+1).  Both refills are legal from the barrier on; one per tile keeps the
//          issue spread as it was with a barrier per tile.
//   No barrier between the two tiles of a pair: waves drift by up to two tiles, so their hit checks,
//   append paths and DMA issue fall out of phase and one wave's append no longer holds up the other
//   seven at every tile.
//   Slot census during a pair: it-2, it-1 refilling (tiles it+4, it+5); it, it+1 being read; it+2
//   landed; it+3 in flight = 6.  A tile is issued >= 2 tile times before the barrier that needs it.
//   Prologue: tiles 0 .. 3 issued (by the loader waves), 0 .. 2 waited for by the rule above with it = 0
//   (all but tile 3 where it exists), barrier (= pair 0's).  Every wave of a block runs
//   1 + (my_tiles - 1) / 2 barriers (my_tiles is block-uniform); no DMA is issued for a tile index >=
//   my_tiles (do_dma: it + 4 < my_tiles, in a loader wave); near the end of a block the wait is for
//   everything outstanding.
// ---------------------------------------------------------------------------
template <int D>
struct Scan32Cfg {
  static constexpr int KS = D / 32;
  static constexpr int RD = KS % 2 == 0 ? 2 : 1;   // fragment roll depth (round 5: 2, 3, 4, 6 within noise)
  static constexpr int TILE_BYTES = kT16 * D * 2;
  static constexpr int HIT_BYTES = kHitCap * 9;
  static constexpr int NB_RAW = (160 * 1024 - HIT_BYTES) / TILE_BYTES;
  // 6 slots (what fits at d = 768), all accounted for by the pair protocol above: 2 refilling, 2 being
  // read, 1 landed, 1 in flight
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
  constexpr int PD = NB - 2;    // tiles issued ahead (tile it refills the slot of tile it-2 with tile it+PD)
  static_assert(NB == 6, "the pair protocol's slot census");
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
  // loader half (header comment): waves 4-7 issue every tile whole; the other widths, every wave its share
  constexpr bool HALVES = HalfTile<D>::kOk;
  constexpr int GW = HALVES ? HalfTile<D>::G : C::GLDS_PER_WAVE;   // pieces a loader has in flight per tile
  constexpr int KDMA = HALVES ? KS / 12 : KS / 4;                  // the refill's k-step
  const bool loader = !HALVES || wave >= NW / 2;
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
  HalfTile<D> ht;
  if constexpr (HALVES) ht.init(a, wave, lane);
  else lt.init(a, wave, lane);
  // a loader wave's issue of block tile `tile` into ring slot `slot`
  auto issue = [&](int slot, int tile) {
    if constexpr (HALVES)
      ht.issue(a, ring + slot * C::TILE_BYTES, next_base, tile == partial_tile, tile * tmul + tph, wave, lane);
    else
      lt.template issue<false>(a, ring + slot * C::TILE_BYTES, next_base, tile == partial_tile, tile * tmul + tph,
                               wave, lane);
    next_base += tile_stride;
  };
  // the wait before a pair's barrier (it even; it = 0: the prologue's)
  auto pair_wait = [&](int it) {
    if (loader && it + PD <= my_tiles) wait_vmcnt<GW>();
    else wait_vmcnt<0>();
  };
#pragma unroll
  for (int p = 0; p < PD; ++p) {
    if (p < my_tiles && loader) issue(p, t0 + p * tstep);
  }
  if (wave >= NW / 2) __builtin_amdgcn_s_setprio(1);
  // tiles 0 .. 2 landed (tile 3 may stay outstanding): this is also the first pair's barrier
  pair_wait(0);
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
  // one 16-query set's hits of one tile (header comment, "Hit check").  bound: the tile may be the shard's
  // short last one -- only a block's last tile can be, and its epilogue is the one after the loop
  auto append = [&](const f32x4& acc, float tau, int ql, uint32_t rowbase, auto bound) {
    constexpr bool BOUND = decltype(bound)::value;
    if constexpr (BOUND) {
      const float mx = fmaxf(fmaxf(acc[0], acc[1]), fmaxf(acc[2], acc[3])) - tau;
      if (__ballot(mx >= 0.0f) == 0ull) return;
    } else {
      // v_max3 + v_max + v_cmp.  fmaxf first canonicalises two of the operands (v_max x, x), which an MFMA
      // result never needs (it is no signalling NaN).  Only the prefilter: the row test below decides; a
      // NaN tau (invalid query) fails it as it fails every row.
      // The compiler pads no hazard of an asm statement, so the string opens with the pad for both MFMA
      // hazards it can meet, whichever register mx gets (the counts are the compiler's own for this MFMA on
      // gfx950: s_nop 7 before a VALU read of its result, s_nop 2 before a VALU write over its C operand):
      //   mx may be given a register that the MFMA just ahead read as its C operand: 3 wait states, always;
      //   the accumulators read here were written by the tile before: 8 wait states after its last MFMA.
      //   This tile's 2 KS MFMAs lie between (each k-step is pinned by its sched_barrier, the statement is
      //   volatile and follows them), which is 8 or more from d = 128 on; d = 64 has 4 and takes the long pad
      //   (a long pad at every width measured 0.02 ms per launch at d = 768, profiles/r13a)
      constexpr int kPad = 2 * KS >= 8 ? 2 : 7;
      float mx;
      asm volatile("s_nop %5\n\tv_max3_f32 %0, %1, %2, %3\n\tv_max_f32 %0, %0, %4"
                   : "=&v"(mx)
                   : "v"(acc[0]), "v"(acc[1]), "v"(acc[2]), "v"(acc[3]), "n"(kPad));
      if (__ballot(mx >= tau) == 0ull) return;
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const bool hit = acc[j] >= tau && (!BOUND || rowbase + j < nrows);
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
  auto epilogue = [&](const f32x4& p0, const f32x4& p1, uint32_t rowbase, auto bound) {
    append(p0, tau0, r, rowbase, bound);
    append(p1, tau1, 16 + r, rowbase, bound);
  };

  int buf = 0;   // slot of tile it
  // the pair's one synchronisation point, before its first (even) tile `it`.  Issued so far: tiles
  // .. it+3.  What this wave issued of tiles it+1 and it+2 must have landed (a loader lets its newest
  // tile, it+3, stay outstanding; near the end of the block nothing younger than it+2 was issued: wait
  // for all; waves 0-3 issued none of them).  After the barrier every loader's share of
  // them has landed, and every wave has issued the MFMAs of tiles it-2 and it-1 (so its reads of those
  // two slots completed: each MFMA waited for its own fragment) -- the two slots the pair refills
  auto pair_sync = [&](int it) {
    pair_wait(it);
    lds_barrier();
  };
  // one tile: ring refill, MFMAs (+ the rolled reads), then the epilogue of the PREVIOUS tile (its
  // accumulators are complete by then: no wait on this tile's MFMA latency); the loop body runs the
  // two tiles of a pair so the accumulator sets alternate without run-time selection
  auto iter = [&](int it, f32x4& acc0, f32x4& acc1, uint32_t& rb, const f32x4& prev0, const f32x4& prev1,
                  uint32_t rb_prev) {
    const int tile = t0 + it * tstep;
    // the refill of slot(it-2) with tile it+PD is issued a quarter into this tile's MFMAs (its SALU /
    // address work then overlaps queued matrix work instead of delaying every wave's first MFMA after
    // the barrier: round 5, 2.89-2.91 vs 2.95-2.97 ms per grouped launch in three alternating rounds,
    // profiles/r05y).  Counted from the pair's first tile e, that tile refills slot(e-2) and the
    // second one slot(e-1): both free since the pair's barrier; one refill per tile keeps the issue
    // spread (both in the first tile measured slower, profiles/r11a).  Loader half: the refill is the
    // whole tile from waves 4-7; their SIMD partners issue none and keep issuing MFMAs meanwhile, so it
    // can go earlier: k-step KS/12 (k-steps 0 .. 12 at d = 768 in profiles/r12a; one wave-uniform test
    // per tile, as before)
    const bool do_dma = it + PD < my_tiles && loader;
    const int ntile = tile + PD * tstep;
    const int pslot = buf < 2 ? buf + NB - 2 : buf - 2;   // slot of tile it-2 (it < 2: a slot not yet used)
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
      if (s == KDMA && do_dma) issue(pslot, ntile);
      __builtin_amdgcn_sched_barrier(0);
    }
    if (it > 0) epilogue(prev0, prev1, rb_prev, std::false_type{});
    rb = (uint32_t)(tile * tmul + tph) * kT16 + 4 * kq;
    buf = nslot;
  };
  f32x4 a0, a1, b0, b1;
  uint32_t rbA = 0, rbB = 0;
  for (int it = 0; it < my_tiles; it += 2) {
    if (it > 0) pair_sync(it);   // (the prologue's barrier is pair 0's)
    iter(it, a0, a1, rbA, b0, b1, rbB);
    if (it + 1 < my_tiles) iter(it + 1, b0, b1, rbB, a0, a1, rbA);
  }
  // the block's last tile: the only one that can be the shard's short tile, and its accumulators are fresh
  // from the MFMAs: the compiler's own maximum (it pads the hazard) and the row bound
  if (my_tiles & 1) epilogue(a0, a1, rbA, std::true_type{});
  else epilogue(b0, b1, rbB, std::true_type{});
  if (wcnt) wave_flush_hits(a, qw, hk, hq, wcnt, lane);
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

int launch_scan(const ScanArgs& a, int d, int mode, hipStream_t s, int family) {   // (search_internal.h)
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

// One shard's top-k (drt_ip_topk_bf16); with row statistics (stats != NULL) the result is put in
// the canonical exact-score order (refine.hip): the select keeps kc >= k candidates in the
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
  rc = launch_scan(filter_scan_args(Q, nq, P, d, n, tau, cnt, w + p.off_keys, p.cap), d, SCAN_FILTER, s, PROF_SCAN);
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

static int resolve_impl(const void* Q, int64_t nq, const void* P, int64_t n, int32_t d, int32_t k, int64_t id_offset,
                        float* out_scores, int64_t* out_ids, int32_t* status, void* ws, size_t ws_bytes,
                        int64_t* n_resolved, const float* stats, hipStream_t s) {
  DRT_REQUIRE(valid_dims(nq, n, d, k));
  if (n_resolved) *n_resolved = 0;
  if (nq == 0 || status == nullptr) return DRT_OK;
  std::vector<int32_t> bad;   // not certified: status bit 0
  int rc = flagged_queries(status, nq, 1, 1, s, bad);
  if (rc || bad.empty()) return rc;
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
  for (size_t b0 = 0; b0 < bad.size(); b0 += chunk) {
    const int64_t nb = std::min<int64_t>(chunk, (int64_t)bad.size() - (int64_t)b0);
    if ((rc = gather_queries(Q, d, bad.data() + b0, nb, qbuf, mbuf, s))) return rc;
    ScanArgs a = scan_args(qbuf, nb, P, d);
    a.nrows = n;
    a.out = sbuf;
    a.cap = width;
    if ((rc = launch_scan(a, d, SCAN_DENSE, s, -1))) return rc;
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
    if ((rc = launch_select(sa, SEL_DENSE32, SEL_TOPK, s))) return rc;
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
      if ((rc = launch_refine(ra, s))) return rc;
    }
    DRT_CHECK_HIP(hipStreamSynchronize(s));   // every chunk: the entry returns with the rows rewritten
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
  f.scan = filter_scan_args(Q, nq, P, d, n_local, nullptr, f.cnt, f.w + f.p.off_keys, f.p.cap);   // tau: per launch
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

}  // extern "C"
