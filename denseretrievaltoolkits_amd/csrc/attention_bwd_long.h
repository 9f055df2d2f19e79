// What the attention backward kernels share (arguments, LDS fragment offsets, the per-element work
// of the two phases) and the streamed pair for 160 < L <= 512 with its packed (VL) forms.  Entries:
// csrc/encoder_bwd.hip, and csrc/attention_varlen_long.hip for the VL forms.
#pragma once
#include "drt_common.h"

namespace drt {

constexpr int kAbRow = 128;               // bytes per [.][64] bf16 row  (kAbMaxSeq: drt_common.h)

struct AttnBwdArgs {
  const __bf16* qkv;     // [B*L][3H]
  const __bf16* ctx;     // [B*L][H]  forward output O
  const __bf16* dctx;    // [B*L][H]  dO
  const float* lse;      // [B][heads][L]
  const int64_t* mask;   // [B][L] or null
  __bf16* dqkv;          // [B*L][3H]
  int64_t B, L;
  int heads, H;
  float scale;
  float drop_p;           // attention-probability dropout of the forward (0: none)
  uint64_t seed, site;
  const uint32_t* drop_bits;  // optional keep bits written by the forward ([B][heads][L][ceil(L/32)]);
                              // NULL: the same bits drawn again from the hash
  float* dsum;                // optional [B][3H] (L > 160: [B][ceil(L / 128)][3H]): column sums of dQKV
  const float* relbias;       // RB kernels: [heads][2L-1] fp32, the forward's relative-position bias
  float* dtab;                // RB kernels: [B][heads][2L-1] (L > 160: [B][ceil(L / 128)][heads][2L-1]) fp32,
                              // each work-group's sums of dS along the diagonals k - q
  // VL kernels (packed batches, drt_attention_varlen_backward_bf16): qkv / ctx / dctx / dqkv hold T token rows,
  // lse is [heads][T], drop_bits [heads][T][W], dsum [sequences][3H]; B, L and mask unused
  const int32_t* cu_seqlens;  // [sequences + 1] row offsets
  const int32_t* seq_ids;     // [n_seqs] the sequences this launch covers, or null: 0 .. n_seqs - 1
  int max_len;                // bound of every listed length (<= 32 NB); longer ones are clamped
  int64_t L_pad, T;           // the keep hash's row is (b * heads + head) * L_pad + q (the padded batch's)
  int W;                      // keep words per query in drop_bits
  // streamed VL kernels (drt_attention_varlen_long_backward_bf16): one work-group per (tile, head)
  const int32_t* tiles;       // [n_tiles][2] (sequence, 128-row group); dsum is [n_tiles][3H]; seq_ids unused
};

__device__ __forceinline__ int ab_rc(int row, int chunk) { return row * kAbRow + ((chunk ^ ((row >> 1) & 7)) << 4); }

typedef short ab_v4i16 __attribute__((ext_vector_type(4)));

// Per-lane LDS offsets of the fragment reads, fixed for the kernel: every row block starts at a
// multiple of 32 rows, so the swizzle term (row >> 1) & 7 of a block's row never depends on the
// block (16 blk = 0 mod 8).  A-operand rows (blk * 32 + r, chunk 2 k4 + h): offA[k4]; column-wise
// B operands (ab_tr8p rows blk * 32 + 16 ks + 4 h + q and + 8, col0 = 32 t): offT[t][0 / 1].
// A read of block blk is then img + blk * 4096 (+ ks * 2048) + offset: with NB a template
// argument and the block loops unrolled, one VGPR + an immediate per read.
struct AbOffsets {
  int offA[4];
  int offT[2][2];
};
__device__ __forceinline__ AbOffsets ab_offsets(int lane) {
  AbOffsets o;
  const int r = lane & 31, h = lane >> 5, sw = (r >> 1) & 7;
#pragma unroll
  for (int k4 = 0; k4 < 4; ++k4) o.offA[k4] = r * kAbRow + (((2 * k4 + h) ^ sw) << 4);
  const int i = lane & 15, q = i >> 2, p = i & 3, b4 = (lane >> 4) & 1;
  const int sx = 2 * h + (q >> 1), lo = (p & 1) * 8;
#pragma unroll
  for (int t = 0; t < 2; ++t) {
    const int c = 4 * t + 2 * b4 + (p >> 1);
    o.offT[t][0] = (q + 4 * h) * kAbRow + ((c ^ sx) << 4) + lo;
    o.offT[t][1] = (q + 4 * h + 8) * kAbRow + ((c ^ (sx + 4)) << 4) + lo;
  }
  return o;
}

__device__ __forceinline__ bf16x8 ab_tr8o(const char* img, int off0, int off1) {
  typedef __attribute__((address_space(3))) ab_v4i16 lds_v4;
  const ab_v4i16 x = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_v4*)(img + off0));
  const ab_v4i16 y = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_v4*)(img + off1));
  bf16x8 v;
  __builtin_memcpy(&v, &x, 8);
  __builtin_memcpy((char*)&v + 8, &y, 8);
  return v;
}

// Per-score-element work of the two phases on element PAIRS (v_pk_fma_f32 / v_pk_add_f32 /
// v_pk_mul_f32 issue two fp32 lanes each; exp2 stays per element):
//   P1 (lane = key, 4 queries e0..e0+3): P = exp2(S log2e + (kbias - lse2)), dS = P (keep dP / (1-p) - Dv)
//   P2 (lane = query, 4 keys e0..e0+3):  P = exp2(S log2e + (kb2 - lse2)),   dS = P (keep dP / (1-p) - Dv)
// Same roundings as the per-element form: fma(S, log2e, kbias - lse2) vs fma(S, log2e, kbias) - lse2 can
// differ in the last bit of the exponent argument (checked against torch fp32, not bitwise).
// RB: rbv = the relative-position biases (x log2e) of this lane's key and the four queries; they join
// the key bias before lse2 leaves and before the fma, as in the forward (kb + rb, then fma(S, log2e, .)).
template <bool DROP, bool RB = false>
__device__ __forceinline__ void ab_p1_pairs(const f32x16& sv, const f32x16& dp, int e0, const f32x4& lq,
                                            const f32x4& dq, float kbias, const u32x4& wk, uint32_t lanebit,
                                            float inv, bf16x8 (&pa)[2], bf16x8 (&sa)[2],
                                            const f32x4& rbv = f32x4{}) {
  const f32x2 l2e = {kLog2e, kLog2e}, kb = {kbias, kbias}, iv = {inv, inv};
#pragma unroll
  for (int u = 0; u < 4; u += 2) {
    const int e = e0 + u;
    const f32x2 c = (RB ? kb + f32x2{rbv[u], rbv[u + 1]} : kb) - f32x2{lq[u], lq[u + 1]};
    f32x2 x = __builtin_elementwise_fma(f32x2{sv[e], sv[e + 1]}, l2e, c);
    f32x2 p = {__builtin_amdgcn_exp2f(x[0]), __builtin_amdgcn_exp2f(x[1])};
    f32x2 ds, pd = p;
    const f32x2 nd = -f32x2{dq[u], dq[u + 1]};
    if (DROP) {
      const bool k0 = (wk[u] & lanebit) != 0u, k1 = (wk[u + 1] & lanebit) != 0u;
      pd = f32x2{k0 ? p[0] : 0.f, k1 ? p[1] : 0.f};
      ds = p * __builtin_elementwise_fma(f32x2{k0 ? dp[e] : 0.f, k1 ? dp[e + 1] : 0.f}, iv, nd);
    } else {
      ds = p * (f32x2{dp[e], dp[e + 1]} + nd);
    }
    pa[e >> 3][e & 7] = (__bf16)pd[0];
    pa[e >> 3][(e & 7) + 1] = (__bf16)pd[1];
    sa[e >> 3][e & 7] = (__bf16)ds[0];
    sa[e >> 3][(e & 7) + 1] = (__bf16)ds[1];
  }
}

// wbits: bit u (u < 4) = keep of key e0 + u's pair element for this lane's query
// DSF: also hand back the four fp32 dS (before the bf16 rounding) -- the relative-bias gradient
template <bool DROP, bool DSF = false>
__device__ __forceinline__ void ab_p2_pairs(const f32x16& st, const f32x16& dpt, int e0, const f32x4& kbv, float lq,
                                            float dq, uint32_t wbits, float inv, bf16x8 (&sa)[2],
                                            f32x4* dsf = nullptr) {
  const f32x2 l2e = {kLog2e, kLog2e}, lq2 = {lq, lq}, nd = {-dq, -dq}, iv = {inv, inv};
#pragma unroll
  for (int u = 0; u < 4; u += 2) {
    const int e = e0 + u;
    const f32x2 c = f32x2{kbv[u], kbv[u + 1]} - lq2;
    const f32x2 x = __builtin_elementwise_fma(f32x2{st[e], st[e + 1]}, l2e, c);
    const f32x2 p = {__builtin_amdgcn_exp2f(x[0]), __builtin_amdgcn_exp2f(x[1])};
    f32x2 ds;
    if (DROP) {
      const f32x2 kd = {(wbits >> u) & 1u ? dpt[e] : 0.f, (wbits >> (u + 1)) & 1u ? dpt[e + 1] : 0.f};
      ds = p * __builtin_elementwise_fma(kd, iv, nd);
    } else {
      ds = p * (f32x2{dpt[e], dpt[e + 1]} + nd);
    }
    if (DSF) {
      (*dsf)[u] = ds[0];
      (*dsf)[u + 1] = ds[1];
    }
    sa[e >> 3][e & 7] = (__bf16)ds[0];
    sa[e >> 3][(e & 7) + 1] = (__bf16)ds[1];
  }
}

// ---------------------------------------------------------------------------
// Attention backward for 160 < L <= 512 (BERT's max_position_embeddings; the whole-sequence kernel
// above holds Qs, K, V, dO of the sequence in LDS, which stops at 160 rows): the same two phases,
// each as its own kernel over 128-row groups, with the OTHER side streamed through LDS 32 rows at
// a time (FlashAttention-2 style):
//   dkdv: work-group = (sequence, head, 128 keys), wave = 32 keys (K, V fragments in registers);
//         loop over the query blocks: Qs, dO rows (+ Dv from O, lse, keep words) staged in LDS;
//   dq:   work-group = (sequence, head, 128 queries), wave = 32 queries (Qs, dO in registers);
//         loop over the key blocks: K, V rows and the key bias staged in LDS.
// Every score product, exponential and MFMA operand layout is the phase's of
// attention_bwd_rk_kernel (same arithmetic per element).  The next block's global loads are issued
// before the current block's matrix work (one barrier pair per block).  Dropout needs the forward's
// keep bits (drt_attention_forward_bf16's drop_bits).  dsum: column sums per (sequence, 128-row group)
// [B][G][3H], reduced in a fixed order by the caller (deterministic).
// ---------------------------------------------------------------------------
constexpr int kAblMaxSeq = 512;
constexpr int kAblGroup = 128;   // rows per work-group (4 waves x 32)

// RB: the head's whole bias table (x log2e) in LDS at rbs[k - q + 511] (q, k < 512), zero outside
// the table (the dkdv kernel: its shifted reversed copies); the dq kernel also sums dS along the diagonals into dts (as attention_bwd_rk_kernel) and
// writes its group's 2L-1 sums -- zero where its 128 queries have no entry -- to
// a.dtab[sequence][group][head].
constexpr int kAblRb = 2 * kAblMaxSeq;

// Work-group-wide "every key of sequence b is masked" (256 threads over the L <= 512 mask entries;
// one barrier, before any LDS traffic).  Such a sequence runs as attention_bwd_rk_kernel's: P = 1 / L
// from zeroed Qs / K operands, a zero bias table, key bias 0 and lse = ln L (contract: drt.h).
__device__ __forceinline__ bool abl_dead_sequence(const AttnBwdArgs& a, int64_t b, int L) {
  int anylive = a.mask == nullptr;
  if (a.mask)
    for (int i = threadIdx.x; i < L; i += 256) anylive |= a.mask[b * a.L + i] != 0;
  return !__syncthreads_or(anylive);
}

template <bool RB>
__device__ __forceinline__ void abl_stage_relbias(const AttnBwdArgs& a, int hd, int L, bool dead, float* rbs,
                                                  float* dts) {
  if (!RB) return;
  const float* src = a.relbias + (int64_t)hd * (2 * L - 1);
  for (int i = threadIdx.x; i < kAblRb; i += 256) {
    const int j = i - (kAblMaxSeq - L);              // table entry k - q + L - 1
    rbs[i] = (j >= 0 && j < 2 * L - 1 && !dead) ? src[j] * kLog2e : 0.0f;
    dts[i] = 0.0f;
  }
}
// The dkdv kernel's image: four copies of the reversed table shifted by 0..3 entries, as
// attention_bwd_rk_kernel's rbq (one aligned 16-B read per four queries).
constexpr int kAblRbq = kAblRb + 4;
template <bool RB>
__device__ __forceinline__ void abl_stage_relbias_rev(const AttnBwdArgs& a, int hd, int L, bool dead, float* rbq) {
  if (!RB) return;
  const float* src = a.relbias + (int64_t)hd * (2 * L - 1);
  for (int i = threadIdx.x; i < 4 * kAblRb; i += 256) {
    const int c = i / kAblRb, t = i - c * kAblRb;
    const int ii = kAblRb - 2 - (t + c), j = ii - (kAblMaxSeq - L);
    rbq[c * kAblRbq + t] = (ii >= 0 && j >= 0 && j < 2 * L - 1 && !dead) ? src[j] * kLog2e : 0.0f;
  }
}

// The forward's keep word of (hash row, key block kb) drawn again: bit j = keep of key 32 kb + j, zero
// from key L on (16 pair hashes, as attention_bwd_rk_kernel's staging draws them).
__device__ __forceinline__ uint32_t attn_keep_word(uint64_t seed, uint64_t site, uint64_t row, int kb, int L,
                                                   uint32_t thr) {
  uint32_t x = attn_row_key(seed, site, row) + (uint32_t)(kb * 16) * kAttnPairStep;
  uint32_t w = 0u;
#pragma unroll 1   // a rolled loop: the path is the C-ABI caller's without bits, and must cost no registers
  for (int jj = 0; jj < 16; ++jj, x += kAttnPairStep) {
    const uint32_t hsh = attn_mix(x);
    const int key = kb * 32 + 2 * jj;
    w |= (key < L && (hsh & 0xFFFFu) >= thr) ? 1u << (2 * jj) : 0u;
    w |= (key + 1 < L && (hsh >> 16) >= thr) ? 2u << (2 * jj) : 0u;
  }
  return w;
}

// VL (packed batches, drt_attention_varlen_long_backward_bf16): the grid is one work-group per
// (tile, head), blockIdx.x = tile * heads + head, over a host-built table of (sequence, 128-row group)
// with one entry per group that holds a token -- no work-group of a ragged batch is empty, and the
// work-groups that stream one sequence's rows are adjacent in launch order (their re-reads meet in
// L2).  Rows start at cu[b], the length is cu[b + 1] - cu[b] clamped to max_len, and the loop runs
// over the blocks of THAT sequence; lse is [heads][T], the keep words [heads][T][W], the hash row the
// padded batch's (b * heads + head) * L_pad + q.  Without drop_bits the words are drawn again.  No
// mask, so no dead path; no relative bias.  dsum row = the tile's index in the table.  Every
// per-element operation is the padded kernel's: a sequence alone has the bits of the run at B = 1,
// L = len.  The VL forms are instantiated in csrc/attention_varlen_long.hip, which is compiled without
// the packed FP32 instructions (two scalar fma / add / mul round as one packed one does).
template <bool DROP, bool RB = false, bool VL = false>
__global__ __launch_bounds__(256, 2) void attention_bwd_long_dkdv_kernel(AttnBwdArgs a) {
  __shared__ __attribute__((aligned(16))) float rbq[RB ? 4 * kAblRbq : 4];
  __shared__ __attribute__((aligned(16))) char Qs[32 * kAbRow];
  __shared__ __attribute__((aligned(16))) char Os[32 * kAbRow];
  __shared__ __attribute__((aligned(16))) float lse2[32];
  __shared__ __attribute__((aligned(16))) float dvs[32];
  __shared__ __attribute__((aligned(16))) uint32_t kw[4][32];
  __shared__ __attribute__((aligned(16))) char Out[2][kAblGroup * kAbRow];   // dK, dV rows out
  __shared__ float csum[4][2][64];
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int r = lane & 31, h = lane >> 5;
  const int hd = blockIdx.x % a.heads;
  const int64_t tile = blockIdx.x / a.heads;         // VL: row of the tile table and of dsum
  const int64_t b = VL ? a.tiles[2 * tile] : tile;
  const int grp = VL ? a.tiles[2 * tile + 1] : blockIdx.y;
  const int64_t row0 = VL ? a.cu_seqlens[b] : b * a.L;
  int L = (int)a.L;
  if (VL) {   // clamped to the launch's bound (the keep words hold W * 32 >= max_len keys)
    L = a.cu_seqlens[b + 1] - (int)row0;
    L = L < a.max_len ? L : a.max_len;
    if (grp < 0 || grp * kAblGroup >= L) return;     // the whole work-group, before any barrier
  }
  const int64_t hrow = ((int64_t)b * a.heads + hd) * (VL ? a.L_pad : a.L);   // row of the keep hash
  const int64_t orow = VL ? (int64_t)hd * a.T + row0 : hrow;                  // row of lse / drop_bits
  const int64_t ld = 3 * (int64_t)a.H;
  const int nkw = (L + 31) >> 5;                     // keep words per query row that hold a key
  const int bw = VL ? a.W : nkw;                     // keep words per query row in drop_bits
  const int nqb = nkw;                               // query blocks (VL: of this sequence, not of the launch)
  const __bf16* Qg = a.qkv + row0 * ld + hd * 64;
  const __bf16* Kg = Qg + a.H;
  const __bf16* Vg = Qg + 2 * a.H;
  const __bf16* Og = a.ctx + row0 * a.H + hd * 64;
  const __bf16* dOg = a.dctx + row0 * a.H + hd * 64;
  const int blk = grp * 4 + wave;                    // this wave's key block
  const int key = blk * 32 + r;
  const bool active = blk * 32 < L;                  // wave-uniform
  const int keyc = key < L ? key : L - 1;
  // every key masked: P = 1 / L over zeroed Qs, K (VL: no mask, never)
  const bool dead = VL ? false : abl_dead_sequence(a, b, L);
  bf16x8 kf[4], vf[4];                               // B operands of S = Qs K^T, dP = dO V^T
#pragma unroll
  for (int k4 = 0; k4 < 4; ++k4) {
    kf[k4] = *(const bf16x8*)(Kg + (int64_t)keyc * ld + (2 * k4 + h) * 8);
    vf[k4] = *(const bf16x8*)(Vg + (int64_t)keyc * ld + (2 * k4 + h) * 8);
    if (key >= L) {
      kf[k4] = bf16x8{};
      vf[k4] = bf16x8{};
    }
    if (dead) kf[k4] = bf16x8{};
  }
  const float kbias =
      (key >= L || (!VL && !dead && a.mask && a.mask[b * a.L + key] == 0)) ? -3.402823466e+38f : 0.0f;
  const float dead_lse2 = __log2f((float)L);
  const float inv = DROP ? 1.0f / (1.0f - a.drop_p) : 1.0f;
  const AbOffsets off = ab_offsets(lane);
  const uint32_t lanebit = 1u << r;
  const uint32_t thr = VL && DROP ? attn_drop_threshold(a.drop_p) : 0u;   // VL without drop_bits

  // staging of query block qb: thread (row = tid >> 3, chunk c = tid & 7)
  const int srow = tid >> 3, sc = tid & 7;
  bf16x8 gq, go, goo;
  float glse = 0.f;
  uint32_t gw = 0u;
  auto load = [&](int qb) {
    const int q = qb * 32 + srow;
    gq = go = goo = bf16x8{};
    if (q < L) {
      if (!dead) gq = *(const bf16x8*)(Qg + (int64_t)q * ld + sc * 8);
      go = *(const bf16x8*)(dOg + (int64_t)q * a.H + sc * 8);
      goo = *(const bf16x8*)(Og + (int64_t)q * a.H + sc * 8);
    }
    if (tid < 32) glse = qb * 32 + tid < L ? a.lse[orow + qb * 32 + tid] : 0.f;
    if (DROP && tid < 128) {
      const int w = tid >> 5, qq = qb * 32 + (tid & 31), kb = grp * 4 + w;
      if (VL && !a.drop_bits) {   // the forward's word of (query qq, key block kb), drawn again
        gw = 0u;
        if (qq < L && kb < nkw) gw = attn_keep_word(a.seed, a.site, (uint64_t)(hrow + qq), kb, L, thr);
      } else {
        gw = (qq < L && kb < nkw) ? a.drop_bits[(orow + qq) * bw + kb] : 0u;
      }
    }
  };
  auto store = [&](int qb) {
    float part = 0.f;
    bf16x8 qv = gq;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      qv[j] = (__bf16)((float)qv[j] * a.scale);
      part += (float)go[j] * (float)goo[j];
    }
    *(bf16x8*)(Qs + ab_rc(srow, sc)) = qv;
    *(bf16x8*)(Os + ab_rc(srow, sc)) = go;
    part += __shfl_xor(part, 1, 64);
    part += __shfl_xor(part, 2, 64);
    part += __shfl_xor(part, 4, 64);
    if (sc == 0) dvs[srow] = part;
    // rows past L: lse2 = +inf makes P = 0 (their dO is 0 too)
    if (tid < 32) lse2[tid] = qb * 32 + tid < L ? (dead ? dead_lse2 : glse * kLog2e) : __builtin_inff();
    if (DROP && tid < 128) kw[tid >> 5][tid & 31] = gw;
  };

  f32x16 dK[2], dV[2];
#pragma unroll
  for (int t = 0; t < 2; ++t)
#pragma unroll
    for (int e = 0; e < 16; ++e) {
      dK[t][e] = 0.f;
      dV[t][e] = 0.f;
    }
  abl_stage_relbias_rev<RB>(a, hd, L, dead, rbq);   // visible after the loop's first barrier
  const float* rbq1 = rbq + (RB ? ((kAblMaxSeq - 1 - key) & 3) * kAblRbq + ((kAblMaxSeq - 1 - key) & ~3) : 0);
  load(0);
  for (int qb = 0; qb < nqb; ++qb) {
    store(qb);
    __syncthreads();
    if (qb + 1 < nqb) load(qb + 1);   // in flight during this block's matrix work
    if (active) {
      f32x16 sv, dp;
#pragma unroll
      for (int e = 0; e < 16; ++e) {
        sv[e] = 0.f;
        dp[e] = 0.f;
      }
#pragma unroll
      for (int k4 = 0; k4 < 4; ++k4) {
        const bf16x8 qa = *(const bf16x8*)(Qs + off.offA[k4]);
        sv = __builtin_amdgcn_mfma_f32_32x32x16_bf16(qa, kf[k4], sv, 0, 0, 0);
        const bf16x8 oa = *(const bf16x8*)(Os + off.offA[k4]);
        dp = __builtin_amdgcn_mfma_f32_32x32x16_bf16(oa, vf[k4], dp, 0, 0, 0);
      }
      bf16x8 pa[2], sa[2];
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const int q0 = 8 * g + 4 * h;
        const f32x4 lq = *(const f32x4*)(lse2 + q0);
        const f32x4 dq = *(const f32x4*)(dvs + q0);
        u32x4 wk = {};
        if (DROP) wk = *(const u32x4*)(&kw[wave][q0]);
        f32x4 rbv = {};
        if (RB) rbv = *(const f32x4*)(rbq1 + qb * 32 + q0);
        ab_p1_pairs<DROP, RB>(sv, dp, 4 * g, lq, dq, kbias, wk, lanebit, inv, pa, sa, rbv);
      }
#pragma unroll
      for (int ks = 0; ks < 2; ++ks) {
#pragma unroll
        for (int t = 0; t < 2; ++t) {
          const bf16x8 ob = ab_tr8o(Os + ks * 2048, off.offT[t][0], off.offT[t][1]);
          dV[t] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(pa[ks], ob, dV[t], 0, 0, 0);
          const bf16x8 qb8 = ab_tr8o(Qs + ks * 2048, off.offT[t][0], off.offT[t][1]);
          dK[t] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(sa[ks], qb8, dK[t], 0, 0, 0);
        }
      }
    }
    __syncthreads();
  }
  // rows out through LDS: element (key row 8 (e >> 2) + 4 h + (e & 3) of the wave's block, column
  // 32 t + r); dsum: the wave's column sums of the stored values, then the 4 waves in order
#pragma unroll
  for (int t = 0; t < 2; ++t) {
    float sk = 0.f, sv2 = 0.f;
#pragma unroll
    for (int e = 0; e < 16; ++e) {
      const int row = wave * 32 + 8 * (e >> 2) + 4 * h + (e & 3), col = 32 * t + r;
      const __bf16 vk = (__bf16)dK[t][e];
      const __bf16 vv = (__bf16)(DROP ? dV[t][e] * inv : dV[t][e]);
      *(__bf16*)(Out[0] + ab_rc(row, col >> 3) + (col & 7) * 2) = vk;
      *(__bf16*)(Out[1] + ab_rc(row, col >> 3) + (col & 7) * 2) = vv;
      sk += (float)vk;
      sv2 += (float)vv;
    }
    sk += __shfl_xor(sk, 32, 64);
    sv2 += __shfl_xor(sv2, 32, 64);
    if (h == 0) {
      csum[wave][0][32 * t + r] = sk;
      csum[wave][1][32 * t + r] = sv2;
    }
  }
  __syncthreads();
  for (int i = tid; i < kAblGroup * 8; i += 256) {   // 16 B per lane, 8 lanes per row
    const int row = i >> 3, c = i & 7, kk = grp * kAblGroup + row;
    if (kk < L) {
      *(bf16x8*)(a.dqkv + (row0 + kk) * ld + a.H + hd * 64 + c * 8) = *(const bf16x8*)(Out[0] + ab_rc(row, c));
      *(bf16x8*)(a.dqkv + (row0 + kk) * ld + 2 * a.H + hd * 64 + c * 8) = *(const bf16x8*)(Out[1] + ab_rc(row, c));
    }
  }
  if (a.dsum && tid < 128) {   // [B][G][3H], VL: [n_tiles][3H]
    const int G = (L + kAblGroup - 1) / kAblGroup;
    const int m = tid >> 6, col = tid & 63;   // m: 0 dK, 1 dV
    a.dsum[(VL ? tile : (int64_t)b * G + grp) * 3 * a.H + (1 + m) * a.H + hd * 64 + col] =
        csum[0][m][col] + csum[1][m][col] + csum[2][m][col] + csum[3][m][col];
  }
}

template <bool DROP, bool RB = false, bool VL = false>
__global__ __launch_bounds__(256, 2) void attention_bwd_long_dq_kernel(AttnBwdArgs a) {
  __shared__ float rbs[RB ? kAblRb : 1];
  __shared__ float dts[RB ? kAblRb : 1];
  __shared__ __attribute__((aligned(16))) char Ks[32 * kAbRow];
  __shared__ __attribute__((aligned(16))) char Vs[32 * kAbRow];
  __shared__ __attribute__((aligned(16))) float kb2[32];
  __shared__ __attribute__((aligned(16))) char Out[kAblGroup * kAbRow];
  __shared__ float csum[4][64];
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int r = lane & 31, h = lane >> 5;
  const int hd = blockIdx.x % a.heads;
  const int64_t tile = blockIdx.x / a.heads;         // VL: row of the tile table and of dsum
  const int64_t b = VL ? a.tiles[2 * tile] : tile;
  const int grp = VL ? a.tiles[2 * tile + 1] : blockIdx.y;
  const int64_t row0 = VL ? a.cu_seqlens[b] : b * a.L;
  int L = (int)a.L;
  if (VL) {   // as the dkdv kernel
    L = a.cu_seqlens[b + 1] - (int)row0;
    L = L < a.max_len ? L : a.max_len;
    if (grp < 0 || grp * kAblGroup >= L) return;     // the whole work-group, before any barrier
  }
  const int64_t hrow = ((int64_t)b * a.heads + hd) * (VL ? a.L_pad : a.L);   // row of the keep hash
  const int64_t orow = VL ? (int64_t)hd * a.T + row0 : hrow;                  // row of lse / drop_bits
  const int64_t ld = 3 * (int64_t)a.H;
  const int nkw = (L + 31) >> 5;
  const int bw = VL ? a.W : nkw;                     // keep words per query row in drop_bits
  const int nkb = nkw;                               // key blocks (VL: of this sequence, not of the launch)
  const __bf16* Qg = a.qkv + row0 * ld + hd * 64;
  const __bf16* Kg = Qg + a.H;
  const __bf16* Vg = Qg + 2 * a.H;
  const __bf16* Og = a.ctx + row0 * a.H + hd * 64;
  const __bf16* dOg = a.dctx + row0 * a.H + hd * 64;
  const int blk = grp * 4 + wave;
  const int q = blk * 32 + r;                        // this lane's query (D column)
  const bool active = blk * 32 < L;
  const int qc = q < L ? q : L - 1;
  // every key masked: P = 1 / L over zeroed Qs, K (VL: no mask, never)
  const bool dead = VL ? false : abl_dead_sequence(a, b, L);
  bf16x8 qf[4], of[4];                               // B operands of S^T = K Qs^T, dP^T = V dO^T
  float part = 0.f;
#pragma unroll
  for (int k4 = 0; k4 < 4; ++k4) {
    bf16x8 x = *(const bf16x8*)(Qg + (int64_t)qc * ld + (2 * k4 + h) * 8);
    const bf16x8 o = *(const bf16x8*)(dOg + (int64_t)qc * a.H + (2 * k4 + h) * 8);
    const bf16x8 oo = *(const bf16x8*)(Og + (int64_t)qc * a.H + (2 * k4 + h) * 8);
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      x[j] = (__bf16)((float)x[j] * a.scale);
      part += (float)o[j] * (float)oo[j];
    }
    qf[k4] = q < L && !dead ? x : bf16x8{};
    of[k4] = q < L ? o : bf16x8{};
  }
  part += __shfl_xor(part, 32, 64);                 // Dv over the 64 d (the two lane halves)
  const float dq = part;
  const float lq = q < L ? (dead ? __log2f((float)L) : a.lse[orow + q] * kLog2e) : __builtin_inff();
  const float inv = DROP ? 1.0f / (1.0f - a.drop_p) : 1.0f;
  const AbOffsets off = ab_offsets(lane);
  const uint32_t thr = VL && DROP ? attn_drop_threshold(a.drop_p) : 0u;   // VL without drop_bits

  const int srow = tid >> 3, sc = tid & 7;
  bf16x8 gk, gv;
  float gkb = 0.f;
  uint32_t gw = 0u;
  auto load = [&](int kb) {
    const int kk = kb * 32 + srow;
    gk = gv = bf16x8{};
    if (kk < L) {
      if (!dead) gk = *(const bf16x8*)(Kg + (int64_t)kk * ld + sc * 8);
      gv = *(const bf16x8*)(Vg + (int64_t)kk * ld + sc * 8);
    }
    if (tid < 32) {
      const int k2 = kb * 32 + tid;
      gkb = (k2 >= L || (!VL && !dead && a.mask && a.mask[b * a.L + k2] == 0)) ? -3.402823466e+38f : 0.0f;
    }
    if (DROP) {
      if (VL && !a.drop_bits) gw = q < L ? attn_keep_word(a.seed, a.site, (uint64_t)(hrow + q), kb, L, thr) : 0u;
      else gw = q < L ? a.drop_bits[(orow + q) * bw + kb] : 0u;
    }
  };
  auto store = [&]() {
    *(bf16x8*)(Ks + ab_rc(srow, sc)) = gk;
    *(bf16x8*)(Vs + ab_rc(srow, sc)) = gv;
    if (tid < 32) kb2[tid] = gkb;
  };
  f32x16 dQ[2];
#pragma unroll
  for (int t = 0; t < 2; ++t)
#pragma unroll
    for (int e = 0; e < 16; ++e) dQ[t][e] = 0.f;
  abl_stage_relbias<RB>(a, hd, L, dead, rbs, dts);  // visible after the loop's first barrier
  load(0);
  for (int kb = 0; kb < nkb; ++kb) {
    store();
    const uint32_t wq0 = DROP ? gw >> (4 * h) : 0u;   // bit 8 g + u: key 8 g + 4 h + u of the block
    __syncthreads();
    if (kb + 1 < nkb) load(kb + 1);
    if (active) {
      f32x16 st, dpt;
#pragma unroll
      for (int e = 0; e < 16; ++e) {
        st[e] = 0.f;
        dpt[e] = 0.f;
      }
#pragma unroll
      for (int k4 = 0; k4 < 4; ++k4) {
        const bf16x8 ka = *(const bf16x8*)(Ks + off.offA[k4]);
        st = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ka, qf[k4], st, 0, 0, 0);
        const bf16x8 va = *(const bf16x8*)(Vs + off.offA[k4]);
        dpt = __builtin_amdgcn_mfma_f32_32x32x16_bf16(va, of[k4], dpt, 0, 0, 0);
      }
      bf16x8 sa[2];
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        f32x4 kbv = *(const f32x4*)(kb2 + 8 * g + 4 * h);
        f32x4 dsf;
        const int k0 = kb * 32 + 8 * g + 4 * h;      // this lane's four keys k0 .. k0 + 3
        if (RB) {
          const float* rp = rbs + (kAblMaxSeq - 1 - q) + k0;
          kbv += f32x4{rp[0], rp[1], rp[2], rp[3]};
        }
        ab_p2_pairs<DROP, RB>(st, dpt, 4 * g, kbv, lq, dq, wq0 >> (8 * g), inv, sa, &dsf);
        if (RB && q < L) {
          float* dp2 = dts + (kAblMaxSeq - 1 - q) + k0;
#pragma unroll
          for (int u = 0; u < 4; ++u)
            if (k0 + u < L) __hip_atomic_fetch_add(dp2 + u, dsf[u], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        }
      }
#pragma unroll
      for (int ks = 0; ks < 2; ++ks) {
#pragma unroll
        for (int t = 0; t < 2; ++t) {
          const bf16x8 kt = ab_tr8o(Ks + ks * 2048, off.offT[t][0], off.offT[t][1]);
          dQ[t] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(sa[ks], kt, dQ[t], 0, 0, 0);
        }
      }
    }
    __syncthreads();
  }
  // rows out: element (query row 8 (e >> 2) + 4 h + (e & 3) of the wave's block, column 32 t + r)
#pragma unroll
  for (int t = 0; t < 2; ++t) {
    float sq = 0.f;
#pragma unroll
    for (int e = 0; e < 16; ++e) {
      const int row = wave * 32 + 8 * (e >> 2) + 4 * h + (e & 3), col = 32 * t + r;
      const __bf16 v = (__bf16)(dQ[t][e] * a.scale);
      *(__bf16*)(Out + ab_rc(row, col >> 3) + (col & 7) * 2) = v;
      sq += (float)v;
    }
    sq += __shfl_xor(sq, 32, 64);
    if (h == 0) csum[wave][32 * t + r] = sq;
  }
  __syncthreads();
  for (int i = tid; i < kAblGroup * 8; i += 256) {
    const int row = i >> 3, c = i & 7, qq = grp * kAblGroup + row;
    if (qq < L) *(bf16x8*)(a.dqkv + (row0 + qq) * ld + hd * 64 + c * 8) = *(const bf16x8*)(Out + ab_rc(row, c));
  }
  if (RB) {   // complete since the loop's last barrier
    const int G = (L + kAblGroup - 1) / kAblGroup;
    float* dst = a.dtab + (((int64_t)b * G + grp) * a.heads + hd) * (2 * L - 1);
    for (int i = tid; i < 2 * L - 1; i += 256) dst[i] = dead ? 0.0f : dts[i + kAblMaxSeq - L];
  }
  if (a.dsum && tid < 64) {
    const int G = (L + kAblGroup - 1) / kAblGroup;
    a.dsum[(VL ? tile : (int64_t)b * G + grp) * 3 * a.H + hd * 64 + tid] = csum[0][tid] + csum[1][tid] + csum[2][tid] + csum[3][tid];
  }
}

// Launch of the streamed pair over `grid` -- (sequence, head) x 128-row group, or one work-group per
// (tile, head) of a tile table (VL): the dK / dV kernel (`pick(0)`) then the dQ kernel (`pick(1)`);
// static LDS only.
template <typename Pick>
static int launch_attention_bwd_long(Pick&& pick, AttnBwdArgs& a, dim3 grid, hipStream_t stream) {
  void* args[] = {&a};
  hipLaunchKernel((const void*)pick(0), grid, dim3(256), args, 0, stream);
  hipLaunchKernel((const void*)pick(1), grid, dim3(256), args, 0, stream);
  return hip_status(hipGetLastError());
}

// The checked arguments of the two varlen backwards (drt_attention_varlen_backward_bf16 and its _long_
// form, which differ in `max_seq` and in what `ids` lists: n sequences, or with `tiled` the n rows of a
// tile table, which is then required), in the order the contract (drt.h) states: shapes and drop_p,
// then DRT_OK with *launch = false for an empty input, then pointers, L_pad and W.
inline int varlen_train_bwd_args(AttnBwdArgs& a, bool* launch, int max_seq, bool tiled, const void* qkv,
                                 const void* ctx, const void* dctx, const float* lse, const int32_t* cu_seqlens,
                                 const int32_t* ids, int64_t n, int32_t max_len, int64_t L_pad, int64_t T, int32_t W,
                                 const uint32_t* drop_bits, void* dqkv, float* dsum, int32_t heads, int32_t head_dim,
                                 float scale, float drop_p, uint64_t seed, uint64_t site) {
  *launch = false;
  DRT_REQUIRE(n >= 0 && T >= 0 && max_len >= 1 && max_len <= max_seq && heads > 0 && head_dim == 64);
  DRT_REQUIRE(drop_p >= 0.0f && drop_p < 1.0f);
  DRT_REQUIRE(n * heads < (1ll << 31) && T < (1ll << 31));
  if (n == 0 || T == 0) return DRT_OK;
  DRT_REQUIRE(qkv && ctx && dctx && lse && cu_seqlens && (ids || !tiled) && dqkv && L_pad >= max_len);
  const bool drop = drop_p > 0.0f;
  DRT_REQUIRE(!(drop && drop_bits) || W * 32 >= max_len);
  a = AttnBwdArgs{(const __bf16*)qkv, (const __bf16*)ctx, (const __bf16*)dctx, lse, nullptr, (__bf16*)dqkv, 0, 0,
                  heads, heads * 64, scale, drop_p, seed, site, drop ? drop_bits : nullptr, dsum, nullptr, nullptr,
                  cu_seqlens, tiled ? nullptr : ids, max_len, L_pad, T, W, tiled ? ids : nullptr};
  *launch = true;
  return DRT_OK;
}

}  // namespace drt
