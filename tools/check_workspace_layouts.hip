// Stand-alone check of the workspace layouts of csrc/search_internal.h: host arithmetic only, meant to be
// built with the host sanitizers and run on a machine without a GPU:
//
//   hipcc --cuda-host-only -std=c++17 -O1 -g -Xarch_host -fsanitize=address,undefined \
//         -Xarch_host -fno-sanitize-recover=all -Iinclude tools/check_workspace_layouts.hip -o check_layouts
//   ./check_layouts
//
// Over the grid of tests/test_workspace_sizes_cpu.py every layout is rebuilt and checked against the region
// sizes restated here: regions in order, 256-aligned where the layout says so, none overlapping the next,
// `total` = the 256-aligned end of the last region, and the large-k layout's prefix = the wide layout.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../denseretrievaltoolkits_amd/csrc/search_internal.h"

using namespace drt;

struct Region {
  const char* name;
  size_t off, bytes;
  bool aligned;
};

static long g_checked = 0;

#define CHECK(cond, ...)                                  \
  do {                                                    \
    if (!(cond)) {                                        \
      std::fprintf(stderr, "FAILED %s: ", #cond);         \
      std::fprintf(stderr, __VA_ARGS__);                  \
      std::fprintf(stderr, "\n");                         \
      std::exit(1);                                       \
    }                                                     \
  } while (0)

static void check_regions(const char* what, const std::vector<Region>& r, size_t first, size_t total,
                          bool total_aligned = true) {
  CHECK(r.front().off == first, "%s: %s starts at %zu, not %zu", what, r.front().name, r.front().off, first);
  for (size_t i = 0; i < r.size(); ++i) {
    CHECK(!r[i].aligned || r[i].off % 256 == 0, "%s: %s at %zu", what, r[i].name, r[i].off);
    const size_t end = r[i].off + r[i].bytes;
    CHECK(end >= r[i].off, "%s: %s wraps", what, r[i].name);
    const size_t next = i + 1 < r.size() ? r[i + 1].off : total;
    CHECK(end <= next, "%s: %s [%zu, %zu) runs into the next region at %zu", what, r[i].name, r[i].off, end, next);
    // an aligned successor starts at the 256-aligned end, an inner one right at the end
    const bool next_aligned = i + 1 < r.size() ? r[i + 1].aligned : total_aligned;
    CHECK(next == (next_aligned ? align_up(end, 256) : end), "%s: gap after %s: %zu -> %zu", what, r[i].name, end,
          next);
  }
  ++g_checked;
}

int main() {
  const int64_t NQ[] = {0, 1, 128, 129, 2048};
  const int64_t N[] = {0, 1000, 16384, 16385, 70000, 1250000, 10000000};
  const int32_t D[] = {64, 768, 1024};
  const int32_t K[] = {1, 10, 1000, 2048};
  const int32_t KL[] = {2049, 4096, 32768};
  const size_t B = kQueriesPerWG;

  // the plans' head and the passes' tail, over the capacities / sample sizes make_plan produces on the grid
  for (int64_t nq : NQ) {
    const int64_t nq_pad = (nq + kQueriesPerWG - 1) / kQueriesPerWG * kQueriesPerWG;
    for (int64_t cap : {(int64_t)4, (int64_t)1000, (int64_t)16384, (int64_t)65536, (int64_t)131072})
      for (int key_bytes : {4, 8})
        for (int64_t m : {(int64_t)0, (int64_t)1, (int64_t)29, (int64_t)8851, (int64_t)70801})
          for (int64_t part : {(int64_t)0, (int64_t)29, (int64_t)18 * 29}) {
            const PlanHead h = plan_head_layout(nq_pad, cap, key_bytes, m, part);
            check_regions("plan head",
                          {{"tau", h.off_tau, (size_t)nq_pad * 4, true},
                           {"counts", h.off_cnt, (size_t)nq_pad * 4 * kCntStride, true},
                           {"keys", h.off_keys, (size_t)nq_pad * cap * key_bytes, true},
                           {"sample", h.off_sample, (size_t)nq_pad * ((m + 3) / 4 * 4) * 4, true},
                           {"part", h.off_part, (size_t)nq_pad * part * 4, true}},
                          0, h.head_end);
            const PassesLayout p = passes_layout(h.head_end, nq_pad);
            check_regions("passes", {{"plan", 0, h.head_end, true}, {"pass0", p.off_pass0, (size_t)nq_pad * 16, true}},
                          0, p.total);
          }
  }

  for (int32_t d : D) {
    const WideLayout w = wide_layout(d);
    const std::vector<Region> wide = {{"qbuf", w.qbuf, B * d * 2, true},
                                      {"qmap", w.qmap, B * 4, true},
                                      {"tau", w.tau, B * 4, true},
                                      {"counts", w.counts, B * kCntStride * 4, true},
                                      {"keys", w.keys, B * kWideCap * 8, true},
                                      {"ekeys", w.ekeys, B * kWideCap * 8, true}};
    check_regions("wide", wide, 0, w.total);
    for (int32_t k : KL) {
      const LargeLayout l = large_layout(d, k);
      CHECK(l.wide.qbuf == w.qbuf && l.wide.qmap == w.qmap && l.wide.tau == w.tau && l.wide.counts == w.counts &&
                l.wide.keys == w.keys && l.wide.ekeys == w.ekeys && l.wide.total == w.total,
            "large(d=%d, k=%d): the wide prefix differs from wide_layout", d, k);
      check_regions("large",
                    {{"sel_k", l.sel_k, B * k * 8, true},
                     {"sel_r", l.sel_r, B * k * 4, true},
                     {"sel_n", l.sel_n, B * 4, true},
                     {"bin_k", l.bin_k, B * k * 8, true},
                     {"bin_r", l.bin_r, B * k * 4, true}},
                    w.total, l.total);
    }
    for (int64_t n : N)
      for (int64_t chunk : {(int64_t)1, (int64_t)5, (int64_t)64, (int64_t)128})
        for (int32_t k : K) {
          const int64_t kc = refine_width(k);
          const ResolveLayout r = resolve_layout(chunk, n, d, kc);
          CHECK(r.total == resolve_layout(chunk, n, d).total, "resolve: total depends on kc");
          // the refine block is one region sized for kc = kSelMaxK; its inner offsets are unaligned
          check_regions("resolve",
                        {{"qbuf", r.qbuf, (size_t)chunk * d * 2, true},
                         {"scores", r.scores, (size_t)chunk * resolve_width(n) * 4, true},
                         {"qmap", r.qmap, (size_t)chunk * 4, true},
                         {"refine block", r.cand_s, (size_t)chunk * kSelMaxK * 16 + chunk * 8, true}},
                        0, r.total);
          check_regions("resolve refine block",
                        {{"cand_s", r.cand_s, (size_t)chunk * kc * 4, true},
                         {"cand_i", r.cand_i, (size_t)chunk * kc * 8, false},
                         {"delta", r.delta, (size_t)chunk * kc * 4, false},
                         {"cnt", r.cnt, (size_t)chunk * 8, false}},
                        r.cand_s, r.cnt + (size_t)chunk * 8, false);
          CHECK(r.cnt + (size_t)chunk * 8 <= r.cand_s + (size_t)chunk * kSelMaxK * 16 + chunk * 8,
                "resolve: the refine block overruns its region");
        }
  }
  std::printf("workspace layouts: %ld checked, all consistent\n", g_checked);
  return 0;
}
