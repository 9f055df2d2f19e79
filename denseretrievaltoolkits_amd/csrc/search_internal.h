// What the units of the top-k search share -- search.hip (filter scan, planner, most entries), select.hip (select
// and threshold kernels), refine.hip (canonical order, wide resolve, large k), merge.hip (list merges: the
// constants only) -- and the search workspace layouts.  Device code is not relocatable, so a kernel is launched
// only from the unit that defines it: the units reach each other's kernels through the host launchers here.
#pragma once

#include <algorithm>
#include <vector>

#include "drt_common.h"

// Host functions shared between the units stay out of the library's dynamic symbol table.
#define DRT_INTERNAL __attribute__((visibility("hidden")))

namespace drt {

constexpr int kQueriesPerWG = 128;  // queries per work-group row of the 16-query-per-wave scans: 8 waves x 16
// Per-query hit counters sit one 128-B line apart (index q * kCntStride): every work-group's
// flush increments the counters of all 128 queries of its block, and packed into 4 lines they
// serialised in L2 (r02 A/B: see DESIGN.md §3).
constexpr int kCntStride = 32;
constexpr int kSelMaxK = 2048;       // largest k of the candidate-list kernels (select, merge, refine)
constexpr int kKthChunk = 4096;      // keys one kth_partial / kth_final work-group sorts
constexpr int64_t kWideCap = 65536;  // hit keys per query of the wide resolve and the large-k path

enum { SEL_KEYS64 = 0, SEL_DENSE32 = 1 };
enum { SEL_TOPK = 0, SEL_KTH = 1 };

struct SelectArgs {
  const void* in;
  int64_t in_stride;        // elements per query row of `in`
  const uint32_t* counts;   // KEYS64: [nq] hit counts; DENSE32: nullptr
  int64_t n_in;             // DENSE32: valid entries per query
  int64_t cap;              // KEYS64: capacity per query
  int64_t n_total;          // rows the counts were taken over (certification)
  int k;
  int64_t nq;
  // TOPK output
  float* out_scores;
  int64_t* out_ids;
  int64_t ldo;
  int64_t id_offset;
  int32_t* status;          // may be null
  const int32_t* qmap;      // optional: output row for block q (resolve path)
  // KTH output
  float* tau;
  // distributed protocol: packed output [nq][k + 1] u64 = (desc score key << 32 | global id),
  // entry k = flags (bit 0: overflow); with a global tau a short local list is not a failure
  uint64_t* out_packed;
  bool global_tau;
  int k_cert;               // k of the certification (0: k); the refine stage selects kc >= k entries
  // packed output of a filter whose later passes ran against a tightened threshold (tighten_kernel):
  // [nq][4] u32 = the first pass's hit count c0, r_eff = its hits >= tau1, tightened (tau1 > tau0).  The
  // list then holds every row >= tau1 plus first-pass rows in [tau0, tau1): it is the whole shard's list
  // only if r_eff + (hits of the later passes) >= k -- otherwise flag bit 0 is set (not certified)
  const uint32_t* pass0;
};

// select.hip.  launch_select times itself (PROF_SELECT); the other launchers only enqueue their kernel
// with one work-group per query (kth_partial: per chunk and query) -- timing and the error check stay
// with the caller.  kth_rank_fits: a sample of m keys at rank r fits kth_rank_kernel's single launch;
// otherwise kth_partial + kth_final.
DRT_INTERNAL int launch_select(const SelectArgs& a, int input, int output, hipStream_t s);
DRT_INTERNAL bool kth_rank_fits(int64_t m, int64_t r);
DRT_INTERNAL void launch_kth_rank(int64_t nq, const uint32_t* in, int64_t stride, int64_t n, int r, float* tau,
                                  uint32_t* zero, hipStream_t s);
DRT_INTERNAL void launch_kth_partial(int64_t nchunk, int64_t nq, const uint32_t* in, int64_t stride, int64_t n, int r,
                                     uint32_t* part, hipStream_t s);
DRT_INTERNAL void launch_kth_final(int64_t nq, const uint32_t* part, int nlists, int r, int64_t lstride,
                                   int64_t qstride, float* tau, uint32_t* best, uint32_t* zero, int len,
                                   hipStream_t s);
DRT_INTERNAL void launch_tighten(int64_t nq, const uint64_t* keys, int64_t cap, const uint32_t* counts,
                                 const float* tau0, int r, float* tau1, uint32_t* pass0, hipStream_t s);

// The scan kernels' argument (search.hip).  SCAN_TOPR: the grouped sample pass, see kTopRL there.
enum { SCAN_FILTER = 0, SCAN_DENSE = 1, SCAN_TOPR = 2 };

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

// The part of ScanArgs every launch shares: dense [nq, d] queries and [*, d] corpus rows, addressed as one
// contiguous run from P's first row.  nrows and the mode's outputs are the caller's.
static inline ScanArgs scan_args(const void* Q, int64_t nq, const void* P, int32_t d) {
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

// A SCAN_FILTER launch over the n rows of P: hits >= tau[q] appended to out [nq][cap] through counts.
static inline ScanArgs filter_scan_args(const void* Q, int64_t nq, const void* P, int32_t d, int64_t n,
                                        const float* tau, uint32_t* counts, void* out, int64_t cap) {
  ScanArgs a = scan_args(Q, nq, P, d);
  a.nrows = n;
  a.tau = tau;
  a.counts = counts;
  a.out = out;
  a.cap = cap;
  return a;
}

// search.hip: one scan launch (d picks the instantiation), timed under `family` (a ProfFamily, or -1).
DRT_INTERNAL int launch_scan(const ScanArgs& a, int d, int mode, hipStream_t s, int family);

// The canonical-order kernels' argument (refine.hip).
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

// refine.hip.  launch_refine: the one-GPU canonical order of nq candidate lists (PROF_SELECT).  The dense and
// the wide resolve pick their queries with flagged_queries -- status [nq] read back (synchronises s), `out` =
// the q with (status[q] & mask) == want -- and gather a chunk of them with gather_queries: rows idx[0 .. nb) of
// Q [*, d] into qbuf, one device-to-device copy each, and idx into the device array qmap (the chunk's output
// rows).  Both return the first failing HIP call's status.
DRT_INTERNAL int launch_refine(RefineArgs& ra, hipStream_t s);
DRT_INTERNAL int flagged_queries(const int32_t* status, int64_t nq, int32_t mask, int32_t want, hipStream_t s,
                                 std::vector<int32_t>& out);
DRT_INTERNAL int gather_queries(const void* Q, int32_t d, const int32_t* idx, int64_t nb, void* qbuf, void* qmap,
                                hipStream_t s);

static inline size_t align_up(size_t x, size_t a) { return (x + a - 1) / a * a; }

// Rows per query a threshold is set to let through over the whole corpus (the sample's r-th best score
// stands for the target-th best of all rows); the hit lists hold 4x that (TopkPlan::cap).
static inline int64_t hit_target(int64_t k) { return std::max<int64_t>(4096, 4 * k); }

// Candidates the canonical-order stage selects per query: k plus a window for the entries within
// 2 eps of the k-th score (a few on Gaussian data, <= 120 on the C2 leg's untrained-tower embeddings
// at k = 1000, tools/c2_window_probe.py; up to 2048 in all).  A wider window goes to the wide resolve.
static inline int64_t refine_width(int64_t k) {
  return std::min<int64_t>(kSelMaxK, k + std::max<int64_t>(256, k / 4));
}

static inline bool valid_dims(int64_t nq, int64_t n, int32_t d, int32_t k) {
  return nq >= 0 && n >= 0 && d > 0 && d % 64 == 0 && d <= 1024 && k >= 1 && k <= kSelMaxK &&
         n < (int64_t)0xFFFFFFFFll;
}

// ---------------------------------------------------------------------------
// Workspace layouts, each stated once: the *_workspace query returns layout(...).total, the entry checks
// ws_bytes against the same struct and forms its pointers from it.  All offsets are bytes from the
// workspace's start.  Plain host arithmetic (tools/check_workspace_layouts.hip checks it alone).
// ---------------------------------------------------------------------------

struct WsBump {   // take(bytes): the region's offset; the next one starts at the next multiple of 256
  size_t o = 0;
  size_t take(size_t bytes) {
    const size_t at = o;
    o = align_up(o + bytes, 256);
    return at;
  }
};

// The head every plan shares (make_plan / make_dist_plan): thresholds, hit counters, the per-query key
// lists (`key_bytes` per entry: 8 for filter hits, 4 for a dense score row), the sample's score rows of m
// keys and `part_keys` chunk survivors per query (both 0 without a sample pass).
struct PlanHead {
  size_t off_tau, off_cnt, off_keys, off_sample, off_part, head_end;
};
static inline PlanHead plan_head_layout(int64_t nq_pad, int64_t cap, int key_bytes, int64_t m, int64_t part_keys) {
  WsBump b;
  PlanHead h;
  h.off_tau = b.take((size_t)nq_pad * 4);
  h.off_cnt = b.take((size_t)nq_pad * 4 * kCntStride);
  h.off_keys = b.take((size_t)nq_pad * cap * key_bytes);
  h.off_sample = b.take((size_t)nq_pad * align_up(m, 4) * 4);
  h.off_part = b.take((size_t)nq_pad * part_keys * 4);
  h.head_end = b.o;
  return h;
}

// drt_ip_topk_filter_passes: a distributed plan of `plan_total` bytes plus [nq_pad][4] u32 of pass-0 state.
struct PassesLayout {
  size_t off_pass0, total;
};
static inline PassesLayout passes_layout(size_t plan_total, int64_t nq_pad) {
  WsBump b;
  b.take(plan_total);
  PassesLayout l;
  l.off_pass0 = b.take((size_t)nq_pad * 16);
  l.total = b.o;
  return l;
}

static inline int64_t resolve_width(int64_t n) { return align_up(std::max<int64_t>(n, 4), 4); }

// drt_ip_topk_resolve for chunks of `chunk` failed queries: their rows, a dense score row each, their
// output rows, and one unaligned block for the refine stage -- [chunk][kc] scores, ids, deltas and
// [chunk][2] counts -- sized for the widest kc (the workspace query does not know k): kc moves the inner
// offsets only, never `total`.
struct ResolveLayout {
  size_t qbuf, scores, qmap, cand_s, cand_i, delta, cnt, total;
};
static inline ResolveLayout resolve_layout(int64_t chunk, int64_t n, int32_t d, int64_t kc = kSelMaxK) {
  WsBump b;
  ResolveLayout l;
  l.qbuf = b.take((size_t)chunk * d * 2);
  l.scores = b.take((size_t)chunk * resolve_width(n) * 4);
  l.qmap = b.take((size_t)chunk * 4);
  l.cand_s = b.take((size_t)chunk * kSelMaxK * 16 + chunk * 8);
  l.cand_i = l.cand_s + (size_t)chunk * kc * 4;
  l.delta = l.cand_s + (size_t)chunk * kc * 12;
  l.cnt = l.cand_s + (size_t)chunk * kc * 16;
  l.total = b.o;
  return l;
}

// drt_ip_topk_resolve_wide, one chunk of up to kQueriesPerWG queries: their rows and output rows, the
// chunk's thresholds and hit counters, the filter's hit keys and their exact order keys.
struct WideLayout {
  size_t qbuf, qmap, tau, counts, keys, ekeys, total;
};
static inline WideLayout wide_layout(int32_t d) {
  const size_t B = kQueriesPerWG;
  WsBump b;
  WideLayout l;
  l.qbuf = b.take(B * d * 2);
  l.qmap = b.take(B * 4);
  l.tau = b.take(B * 4);
  l.counts = b.take(B * kCntStride * 4);
  l.keys = b.take(B * kWideCap * 8);
  l.ekeys = b.take(B * kWideCap * 8);
  l.total = b.o;
  return l;
}

// drt_ip_topk_large: the wide layout (qbuf and qmap stay unused: the queries are read in place) followed
// by each query's k selected entries (sel_*) and the same regrouped by bin (bin_*).
struct LargeLayout {
  WideLayout wide;
  size_t sel_k, sel_r, sel_n, bin_k, bin_r, total;
};
static inline LargeLayout large_layout(int32_t d, int32_t k) {
  const size_t B = kQueriesPerWG;
  LargeLayout l;
  l.wide = wide_layout(d);
  WsBump b{l.wide.total};
  l.sel_k = b.take(B * k * 8);
  l.sel_r = b.take(B * k * 4);
  l.sel_n = b.take(B * 4);
  l.bin_k = b.take(B * k * 8);
  l.bin_r = b.take(B * k * 4);
  l.total = b.o;
  return l;
}

}  // namespace drt
