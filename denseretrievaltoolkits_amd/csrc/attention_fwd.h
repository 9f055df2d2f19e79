// The attention forward kernel and its launcher (entries: csrc/encoder.hip, and
// csrc/attention_varlen_long.hip for the packed training forward above 160 tokens).
#pragma once
#include "attention_tile.h"
#include "drt_common.h"

namespace drt {

// ---------------------------------------------------------------------------
// Attention.  One work-group (4 waves) per (sequence b, head hd); wave w owns
// query blocks w, w+4, ... of 32 rows.  K, V^T and the key bias are staged in
// the LDS image that attention_tile.h lays out (AttnLds), shared with the
// head_dim-32 kernel.
// ---------------------------------------------------------------------------
constexpr int kAttnThreads = 256;

struct AttnArgs {
  const __bf16* qkv;      // [B*L][3*H]  (Q | K | V, head-major inside each)
  const int64_t* mask;    // [B][L] attention_mask (1 = token, 0 = pad) or null
  __bf16* ctx;            // [B*L][H]
  int64_t B, L;
  int heads, H;
  float scale;            // 1/sqrt(dh): applied to Q (exact for dh = 64)
  float* lse;             // optional [B][heads][L]: log-sum-exp of each query's scaled, masked
                          // scores (what the attention backward needs to rebuild P)
  float drop_p;           // training: dropout of the attention probabilities (DROP kernels)
  uint64_t seed, site;    //   keep = attn_keep(attn_row_key(seed, site, (b * heads + head) * L + q), key)
  uint32_t* drop_bits;    // optional [B][heads][L][ceil(L / 32)]: the keep mask, bit (key & 31) of word
                          //   (query, key >> 5) -- the backward reads it instead of re-hashing
  const float* relbias;   // RB kernels: [heads][2 L - 1] fp32, entry (head, key - query + L - 1) is added
                          //   to the score of (query, key) before the softmax (T5's relative-position bias)
  // VL kernels (packed batches, drt_attention_varlen_forward_bf16): qkv / ctx hold T = cu[B] token rows
  const int32_t* cu_seqlens;  // [B + 1] row offsets of the sequences; B, L, mask, lse and the dropout fields unused
  const int32_t* seq_ids;     // [n_seqs] the sequences this launch covers, or null: 0 .. n_seqs - 1
  int max_len;                // bound of every listed length (the launch's LDS image); longer ones are clamped
  // VL training forward (drt_attention_varlen_train_forward_bf16): lse is [heads][T], drop_bits [heads][T][W]
  // (row cu[b] + q of head h), and the keep hash takes the padded batch's row (b * heads + h) * L_pad + q
  int64_t L_pad, T;
  int W;
  // RB x VL (drt_attention_varlen_relbias_forward_bf16): relbias is ONE centred table [heads][2 S - 1],
  // S = bias_len >= max_len; entry (head, key - query + S - 1) serves every sequence of the batch
  int bias_len;
};

// Attention forward, one work-group per (sequence, head): K (swizzled rows), V^T and the key bias
// in LDS, one 32-query block per wave (S^T tiles of 32 keys: rows = keys, lane = query), online
// softmax in registers, P as the B operand of O^T += V^T P^T.  NB = blocks of 32 (Lp = 32 NB) as a
// template argument for L <= 160 (every LDS offset a per-lane constant + an immediate, key loop
// unrolled, O leaves through LDS as whole-row 16-B stores); NB = 0: any L <= 512 (inference), a
// wave loops over its query blocks and stores directly.
// Round 3: scores in log2 units, s2 = fma(s, log2e, kb) with the key bias kb = 0 / -FLT_MAX (finite:
// a row with every key masked gets HF's uniform softmax over its L keys, no NaN; the padding keys
// L..Lp-1 get -inf, which key 0's finite score keeps out of any inf - inf); the running max is
// lazy (kLazy, attention_tile.h: why that is exact); dropout draws the keep decisions from the pairwise hash (drt_common.h), zeroes dropped P,
// writes the keep words for the backward when asked (drop_bits), and moves 1 / (1 - p) into the
// final 1 / l.  (Drawing the words in a separate one-thread-per-word pass for the forward to read
// measured slower: 272 vs 178 us at 1024 x 128, profiles/r03r_attn_probe.log "bits" vs "hash".)
// lse = (m + log2 l) ln 2 (natural log, what the backward rebuilds P from).
// NW waves: 4, or 5 for 5 query blocks (129 <= L <= 160: the recipe's 156-token passages, the
// reranker's 160-token pairs; with 4, wave 0 ran two blocks while three idled).
constexpr float kLn2 = 0.6931471805599453f;

// Register budget: 4 waves per SIMD (<= 128 VGPRs) -- at 5 query blocks the LDS (42 KiB) admits 3
// work-groups of 5 waves per CU, i.e. 4 waves on three of the SIMDs.
// RB (T5, modeling_t5.py T5Attention): the head's 2 Lp relative-position biases sit in LDS behind
// kb[], pre-multiplied by log2 e (entries past 2 L - 2 are 0); query q reads them at key + L - 1 - q,
// so the 32 query rows of each half of a wave read consecutive banks.  The bias joins kb before the
// fma: a masked key stays at -FLT_MAX (the bias is absorbed, as in HF's fp32 sum), a padding key at
// -inf, and an all-zero table leaves every bit of the !RB kernel's result.
// VL (packed inference batches, csrc/packed.hip): the work-group's sequence is seq_ids[blockIdx.x / heads]
// (or that index itself), its rows start at cu[b] and its length is cu[b + 1] - cu[b], read per
// work-group; no mask (a packed sequence has no masked keys: kb is 0 below len, -inf in the tile
// padding).  NB is the launch's length class: every listed len <= 32 NB.  The training form
// (lse given, DROP) writes lse as [heads][T] and the keep words as [heads][T][W], W = the batch's
// word count whatever this launch's class is, and hashes the keeps with the PADDED batch's row
// (b * heads + head) * L_pad + q: for one (p, seed, site) every real (q, key) keeps what the padded
// forward keeps.
// VL = 1: the inference form (no lse, no dropout), VL = 2: the training form.  VL = 2 at NB = 0
// (drt_attention_varlen_long_train_forward_bf16, max_len 161 .. 512): Lp and the query-block loop are
// those of the work-group's own sequence inside an LDS image sized by the launch's max_len; a query's
// keep words are stored tile by tile, the first ceil(len / 32) of its W.  That form
// is instantiated in csrc/attention_varlen_long.hip, which is compiled without the packed FP32
// instructions; two scalar operations round as one packed one does.
// RB x VL = 1 (packed T5 towers, drt_attention_varlen_relbias_forward_bf16): the bucket of a bias depends
// on key - query alone, so one centred table of a fixed span S (AttnArgs::bias_len) serves every
// sequence, length class and batch.  A work-group stages the 2 len - 1 entries its sequence can reach
// into the same rb image (sized by the launch's max_len, zero tail); the per-query read and the tile
// body are the padded RB form's, so a sequence of n tokens gets the ctx bits of the padded kernel at
// B = 1, L = n with the L = n table.  Instantiated in csrc/encoder.hip only (packed FP32 on, as the
// padded RB kernels).
template <int NB, bool DROP, bool RB = false, int VL = 0>
__global__ __launch_bounds__(NB == 5 ? 320 : 256) __attribute__((amdgpu_waves_per_eu(4, 8)))
void attention_fwd_kernel(AttnArgs a) {
  constexpr int NW = NB == 5 ? 5 : 4;
  constexpr int NT = NW * 64;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int64_t b = VL ? (a.seq_ids ? a.seq_ids[blockIdx.x / a.heads] : blockIdx.x / a.heads) : blockIdx.x / a.heads;
  const int64_t row0 = VL ? a.cu_seqlens[b] : b * a.L;
  int Lv = 0;
  if (VL) {   // clamped to the launch's bound: a wrong table cannot run past the LDS image
    Lv = a.cu_seqlens[b + 1] - (int)row0;
    Lv = Lv < a.max_len ? Lv : a.max_len;
    if (Lv <= 0) return;                    // the whole work-group: no barrier is left waiting
  }
  const int L = VL ? Lv : (int)a.L;
  const int Lp = NB ? NB * 32 : AttnLds::padded(L);  // keys padded to the 32-key tile
  const int nqb = Lp / 32;
  const AttnLds lds(Lp);
  const int vts = lds.vts;
  char* Ks = smem;
  char* Vt = Ks + lds.ks_bytes;
  float* kb = (float*)(Vt + lds.vt_bytes);
  float* rb = (float*)((char*)kb + lds.kb_bytes);

  const int tid = threadIdx.x;
  const int wave = tid >> 6, lane = tid & 63;
  const int r = lane & 31, h = lane >> 5;
  const int hd = blockIdx.x % a.heads;
  const int64_t hrow = ((int64_t)b * a.heads + hd) * (VL ? a.L_pad : (int64_t)L);   // row of the keep hash
  const int64_t orow = VL ? (int64_t)hd * a.T + row0 : hrow;                        // row of lse / drop_bits
  const int bw = VL ? a.W : nqb;                                                    // keep words per query
  const int64_t ld = 3 * (int64_t)a.H;
  const __bf16* Qg = a.qkv + row0 * ld + hd * kHeadDim;
  const __bf16* Kg = Qg + a.H;
  const __bf16* Vg = Qg + 2 * a.H;

  // ---- stage K (swizzled rows) and V^T, key bias.  Passes of NT / 2 keys: thread (key group
  // kg = tid >> 3, 16-B chunk c = tid & 7) owns keys 4 kg .. 4 kg + 3 of chunk c, issues all 8
  // global loads of the pass before any LDS store, and writes V^T as 8 ds_write_b64 (4 keys
  // of one d per store) instead of 32 ds_write_b16.  The first Q block's fragments are
  // requested before the pass so their latency overlaps the staging.
  const int c8 = tid & 7, kg = tid >> 3;
  int qrow0 = wave * 32 + (lane & 31);
  qrow0 = qrow0 < L ? qrow0 : L - 1;
  bf16x8 q0[4];
#pragma unroll
  for (int st = 0; st < 4; ++st) q0[st] = *(const bf16x8*)(Qg + (int64_t)qrow0 * ld + st * 16 + (lane >> 5) * 8);
  for (int kp = 0; kp < Lp; kp += NT / 2) {
    u32x4 kv[4], vv[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int key = kp + kg * 4 + u;
      kv[u] = u32x4{0u, 0u, 0u, 0u};
      vv[u] = u32x4{0u, 0u, 0u, 0u};
      if (key < L) {
        // non-temporal: K / V rows are read once per (sequence, head) -- kept out of L2 for the
        // GEMM panels and the ctx rows the next projection reads (round 6: encode +0.4-0.8 % in three
        // alternating rounds, profiles/r06y/)
        kv[u] = __builtin_nontemporal_load((const u32x4*)(Kg + (int64_t)key * ld + c8 * 8));
        vv[u] = __builtin_nontemporal_load((const u32x4*)(Vg + (int64_t)key * ld + c8 * 8));
      }
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int key = kp + kg * 4 + u;
      if (key < Lp) *(u32x4*)(Ks + key * 128 + ((c8 ^ ((key >> 1) & 7)) << 4)) = kv[u];
    }
    const int key0 = kp + kg * 4;
    if (key0 < Lp) {
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        uint16_t e[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) e[u] = ((const uint16_t*)&vv[u])[j];
        const uint32_t lo = (uint32_t)e[0] | ((uint32_t)e[1] << 16), hi = (uint32_t)e[2] | ((uint32_t)e[3] << 16);
        *(uint2*)(Vt + (c8 * 8 + j) * vts + key0 * 2) = make_uint2(lo, hi);
      }
    }
  }
  for (int i = tid; i < Lp; i += NT) {
    float bv = 0.0f;
    if (i >= L) bv = -__builtin_inff();   // tile padding: P exactly 0, in a row of masked keys too
    else if (!VL && a.mask && a.mask[b * a.L + i] == 0) bv = -3.402823466e+38f;  // (1 - mask) * finfo.min
    kb[i] = bv;
  }
  if (RB) {
    // entry i of the image: the bias of key - query = i - (L - 1).  Padded: the head's [2 L - 1] table whole.
    // VL: the window of the head's centred span-S table that this sequence reaches, entries S - L ..
    // S + L - 2 (L <= max_len <= S, so the window never leaves the head's row)
    const float* src = VL ? a.relbias + (int64_t)hd * (2 * a.bias_len - 1) + (a.bias_len - L)
                          : a.relbias + (int64_t)hd * (2 * L - 1);
    for (int i = tid; i < 2 * Lp; i += NT) rb[i] = i < 2 * L - 1 ? src[i] * kLog2e : 0.0f;
  }
  __syncthreads();

  // per-lane LDS offsets (a 32-key tile starts at a multiple of 32 rows: its swizzle term never
  // depends on the tile)
  const int sw = (r >> 1) & 7;
  int offK[4];
#pragma unroll
  for (int st = 0; st < 4; ++st) offK[st] = r * 128 + ((((2 * st) | h) ^ sw) << 4);
  const int offV0 = r * vts + 8 * h, offV1 = (32 + r) * vts + 8 * h;
  const float inv = DROP ? 1.0f / (1.0f - a.drop_p) : 1.0f;
  const uint32_t thr = DROP ? attn_drop_threshold(a.drop_p) : 0u;
  bf16x8 oo[2][2];                           // NB: this wave's O block, [t][g / 2] (bf16)
  // VL: a sequence shorter than its class skips the query blocks and key tiles that hold no token
  const int nqv = VL ? (L + 31) >> 5 : nqb;

  for (int qb = wave; qb < nqb && (!VL || qb < nqv); qb += NW) {
    // Q fragment (B operand, B[k=d][col=q] = Q[q][d]) scaled by 1/sqrt(dh)
    const int qq = qb * 32 + r;
    const int qrow = qq < L ? qq : L - 1;
    bf16x8 qf[4];
#pragma unroll
    for (int s = 0; s < 4; ++s) {
      bf16x8 v = qb == wave ? q0[s] : *(const bf16x8*)(Qg + (int64_t)qrow * ld + s * 16 + h * 8);
#pragma unroll
      for (int j = 0; j < 8; ++j) v[j] = (__bf16)((float)v[j] * a.scale);
      qf[s] = v;
    }
    const uint32_t rowkey = DROP ? attn_row_key(a.seed, a.site, (uint64_t)(hrow + qq)) : 0u;
    const float* rbq = rb + (L - 1 - qrow);    // RB: this query's bias of key k is rbq[k], k < Lp
    uint32_t words[NB ? NB : 1];               // keep words of this query (stored once, after the last tile)
    if (VL && DROP) {                          // the tiles a short sequence skips hold no kept key
#pragma unroll
      for (int j = 0; j < (NB ? NB : 1); ++j) words[j] = 0u;
    }
    f32x16 o[2];
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
      for (int e = 0; e < 16; ++e) o[t][e] = 0.0f;
    float m = -__builtin_inff(), l = 0.0f;

    auto tile = [&](int kt) {
      // S^T tile: rows = keys kt.., cols = queries
      f32x16 s;
#pragma unroll
      for (int e = 0; e < 16; ++e) s[e] = 0.0f;
#pragma unroll
      for (int st = 0; st < 4; ++st) {
        const bf16x8 kf = *(const bf16x8*)(Ks + kt * 128 + offK[st]);
        s = __builtin_amdgcn_mfma_f32_32x32x16_bf16(kf, qf[st], s, 0, 0, 0);
      }
      // element pairs on the packed FP32 path (v_pk_fma_f32 / v_pk_add_f32: two elements per issue)
      float mt = -__builtin_inff();
      const f32x2 l2e = {kLog2e, kLog2e};
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        f32x4 kbv = *(const f32x4*)(kb + kt + 8 * g + 4 * h);
        if (RB) {   // 4-B reads: the offset L - 1 - q is aligned to nothing wider
          const float* rp = rbq + kt + 8 * g + 4 * h;
          kbv += f32x4{rp[0], rp[1], rp[2], rp[3]};
        }
        const f32x2 lo = __builtin_elementwise_fma(f32x2{s[4 * g], s[4 * g + 1]}, l2e, f32x2{kbv[0], kbv[1]});
        const f32x2 hi = __builtin_elementwise_fma(f32x2{s[4 * g + 2], s[4 * g + 3]}, l2e, f32x2{kbv[2], kbv[3]});
        s[4 * g] = lo[0];
        s[4 * g + 1] = lo[1];
        s[4 * g + 2] = hi[0];
        s[4 * g + 3] = hi[1];
        mt = fmaxf(fmaxf(mt, fmaxf(s[4 * g], s[4 * g + 1])), fmaxf(s[4 * g + 2], s[4 * g + 3]));
      }
      mt = fmaxf(mt, __shfl_xor(mt, 32, 64));
      const bool grow = mt > m + kLazy;
      if (__builtin_amdgcn_ballot_w64(grow) != 0ull) {   // rare after the first tile
        const float mn = grow ? mt : m;
        const float alpha = __builtin_amdgcn_exp2f(m - mn);
#pragma unroll
        for (int t = 0; t < 2; ++t)
#pragma unroll
          for (int e = 0; e < 16; ++e) o[t][e] *= alpha;
        l *= alpha;
        m = mn;
      }
      const f32x2 mm = {m, m};
      f32x2 psum = {0.0f, 0.0f};
#pragma unroll
      for (int e = 0; e < 16; e += 2) {
        f32x2 v = f32x2{s[e], s[e + 1]} - mm;
        v[0] = __builtin_amdgcn_exp2f(v[0]);
        v[1] = __builtin_amdgcn_exp2f(v[1]);
        psum += v;
        s[e] = v[0];
        s[e + 1] = v[1];
      }
      float ps = psum[0] + psum[1];
      ps += __shfl_xor(ps, 32, 64);
      l += ps;
      if (DROP) {   // this lane's keys kt + 8 g + 4 h + {0,1,2,3}: pairs kt / 2 + 4 g + 2 h + {0, 1}
        const uint32_t pbase = rowkey + (uint32_t)((kt >> 1) + 2 * h) * kAttnPairStep;
        uint32_t m16 = 0;
#pragma unroll
        for (int g = 0; g < 4; ++g)
#pragma unroll
          for (int u2 = 0; u2 < 2; ++u2) {
            const uint32_t hsh = attn_mix(pbase + (uint32_t)(4 * g + u2) * kAttnPairStep);
#pragma unroll
            for (int w = 0; w < 2; ++w) {
              const int e = 4 * g + 2 * u2 + w;
              const int kr = 8 * g + 4 * h + 2 * u2 + w;
              const bool keep = kt + kr < L && (w ? hsh >> 16 : hsh & 0xFFFFu) >= thr;
              m16 |= keep ? 1u << kr : 0u;
              s[e] = keep ? s[e] : 0.0f;
            }
          }
        if (a.drop_bits) {   // this query's 32 keep bits of the key tile: the two lane halves' 16 each
          const uint32_t word = m16 | __shfl_xor(m16, 32, 64);
          if (NB) words[NB ? (kt / 32) % NB : 0] = word;
          else if (h == 0 && qq < L) a.drop_bits[(orow + qq) * bw + kt / 32] = word;
        }
      }
      // O^T += V^T P^T over the 32 keys (2 k-steps of 16)
#pragma unroll
      for (int ks = 0; ks < 2; ++ks) {
        const bf16x8 pf = pv_fragment(s, ks);
#pragma unroll
        for (int t = 0; t < 2; ++t) {
          const bf16x8 vf = vt_operand(Vt + (t ? offV1 : offV0) + (kt + 16 * ks) * 2);
          o[t] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(vf, pf, o[t], 0, 0, 0);
        }
      }
    };
    if (NB) {
#pragma unroll
      for (int j = 0; j < (NB ? NB : 1); ++j)
        if (!VL || j < nqv) tile(32 * j);
      if (DROP && a.drop_bits && h == 0 && qq < L) {   // the row's words: contiguous over the wave's queries
        uint32_t* dst = a.drop_bits + (orow + qq) * bw;
        if (NB == 4 && !VL) {
          *(u32x4*)dst = u32x4{words[0], words[NB > 1 ? 1 : 0], words[NB > 2 ? 2 : 0], words[NB > 3 ? 3 : 0]};
        } else {
#pragma unroll
          for (int j = 0; j < (NB ? NB : 1); ++j) dst[j] = words[j];
        }
      }
    } else {
      for (int kt = 0; kt < Lp; kt += 32) tile(kt);
    }
    // O^T[d][q]: lane holds query r; d = 32t + (e&3) + 8(e>>2) + 4h
    if (VL != 1 && qq < L && a.lse && h == 0) a.lse[orow + qq] = (m + __log2f(l)) * kLn2;
    const float sc = inv / l;
    if (NB) {
#pragma unroll
      for (int t = 0; t < 2; ++t)
#pragma unroll
        for (int e = 0; e < 16; ++e) oo[t][e >> 3][e & 7] = (__bf16)(o[t][e] * sc);
    } else if (qq < L) {
      __bf16* orow = a.ctx + (row0 + qq) * a.H + hd * kHeadDim;
#pragma unroll
      for (int t = 0; t < 2; ++t)
#pragma unroll
        for (int g = 0; g < 4; ++g) {
          bf16x4 v;
#pragma unroll
          for (int u = 0; u < 4; ++u) v[u] = (__bf16)(o[t][4 * g + u] * sc);
          *(bf16x4*)(orow + 32 * t + 8 * g + 4 * h) = v;
        }
    }
  }
  if (NB) {
    // O through LDS (the K image, dead once every wave is past its last tile): rows of 128 B
    __syncthreads();
    if (wave < nqv) {
#pragma unroll
      for (int t = 0; t < 2; ++t)
#pragma unroll
        for (int g = 0; g < 4; ++g) {
          bf16x4 v;
#pragma unroll
          for (int u = 0; u < 4; ++u) v[u] = oo[t][g >> 1][(g & 1) * 4 + u];
          const int qr = wave * 32 + r, d0 = 32 * t + 8 * g + 4 * h;   // 4 consecutive d of row qr
          *(bf16x4*)(Ks + qr * 128 + (((d0 >> 3) ^ ((qr >> 1) & 7)) << 4) + (d0 & 7) * 2) = v;
        }
    }
    __syncthreads();
#pragma unroll
    for (int it = 0; it < (Lp * 8 + NT - 1) / NT; ++it) {
      const int i = tid + it * NT;
      const int row = i >> 3, c = i & 7;
      if (i < Lp * 8 && row < L)
        *(bf16x8*)(a.ctx + (row0 + row) * a.H + hd * kHeadDim + c * 8) =
            *(const bf16x8*)(Ks + row * 128 + ((c ^ ((row >> 1) & 7)) << 4));
    }
  }
}

// Launch of attention_fwd_kernel for sequences of at most `len` tokens (L, or a varlen launch's
// max_len), one work-group per (sequence, head) group: the one place that knows the length class NB
// and its block size (the LDS image and its opt-in: launch_attention_lds).  `pick(NB)` names the
// caller's instantiation of the class (NB = 0: len > 160), so a new instantiation is one more entry
// in its caller's table and no launch code.
template <typename Pick>
static int launch_attention_fwd(Pick&& pick, AttnArgs& a, int len, bool rb, int64_t groups, void* stream) {
  const int nqb = AttnLds::padded(len) / 32;
  const int nb = nqb <= 5 ? nqb : 0;
  return launch_attention_lds((const void*)pick(nb), a, len, rb, groups, nb == 5 ? 320 : 256, stream);
}

// The checked arguments of the two varlen training forwards (drt_attention_varlen_train_forward_bf16 and
// its _long_ form, which differ in `max_seq`), in the order the contract (drt.h) states: shapes and
// drop_p, then DRT_OK with *launch = false for an empty input, then pointers, L_pad and W.
inline int varlen_train_fwd_args(AttnArgs& a, bool* launch, int max_seq, const void* qkv, const int32_t* cu_seqlens,
                                 const int32_t* seq_ids, int64_t n_seqs, int32_t max_len, int64_t L_pad, int64_t T,
                                 int32_t W, void* ctx, float* lse, uint32_t* drop_bits, int32_t heads,
                                 int32_t head_dim, float scale, float drop_p, uint64_t seed, uint64_t site) {
  *launch = false;
  DRT_REQUIRE(n_seqs >= 0 && T >= 0 && max_len >= 1 && max_len <= max_seq && heads > 0 && head_dim == kHeadDim);
  DRT_REQUIRE(drop_p >= 0.0f && drop_p < 1.0f);
  DRT_REQUIRE(n_seqs * heads < (1ll << 31) && T < (1ll << 31));
  if (n_seqs == 0 || T == 0) return DRT_OK;
  DRT_REQUIRE(qkv && cu_seqlens && ctx && L_pad >= max_len);
  const bool drop = drop_p > 0.0f;
  DRT_REQUIRE(!(drop && drop_bits) || W * 32 >= max_len);
  a = AttnArgs{(const __bf16*)qkv, nullptr, (__bf16*)ctx, 0, 0, heads, heads * head_dim, scale, lse, drop_p, seed, site,
               drop ? drop_bits : nullptr, nullptr, cu_seqlens, seq_ids, max_len, L_pad, T, W};
  *launch = true;
  return DRT_OK;
}

}  // namespace drt
