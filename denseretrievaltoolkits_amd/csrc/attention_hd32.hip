// Attention forward at head_dim 32 (MiniLM-class BERT towers: hidden 384, 12 heads), inference only:
// drt_attention_hd32_forward_bf16 over a padded [B, L] rectangle with an optional key mask and
// drt_attention_hd32_varlen_forward_bf16 over a packed batch (contracts: drt.h).  No lse, no dropout,
// no relative bias, no backward.  The head_dim-64 kernel (attention_fwd.h) is untouched.
//
// A head's Q / K / V row is 64 B, half of the 128 B the 64-wide kernel stages per token, so the unit
// of work is a PAIR of adjacent heads: one work-group per (sequence, head pair) reads 128 contiguous
// bytes per token and matrix -- the 64-wide kernel's 8 x 16-B chunk loads, its swizzled K rows
// ([key][8 x 16 B], chunks 0..3 head A's d 0..31, chunks 4..7 head B's) and its V^T image (Vt[d][key],
// rows 0..31 head A, 32..63 head B), hence its LDS image and launch: AttnLds and launch_attention_lds
// (attention_tile.h).
//
// Products: v_mfma_f32_32x32x16_bf16 for both.  S^T = K Q^T of a 32-key x 32-query tile is two k-steps
// (d = 32) into one accumulator whose lane holds its query's scores, and that accumulator, converted
// to bf16, IS the B operand of O^T += V^T P^T (two k-steps over the tile's 32 keys into a single
// 32 d x 32 q accumulator): P never leaves the registers.  (16x16x32 covers d in one k-step but its
// accumulator keeps 4 keys per lane where its B operand wants 8: P would need a cross-lane move per tile.)
//
// Per 32 x 32 tile the MFMA work is half of the 64-wide kernel's (4 instead of 8 instructions) while
// the softmax VALU work (16 fma, 16 exp2, max, sum, 16 converts per lane) is the same, so the kernel is
// VALU-bound and the question is how the pair's two heads share the waves.  Waves are split by head:
// wave w runs head w & 1 of the pair over the query blocks w >> 1, w >> 1 + slots, ... (4 waves = 2
// slots; 6 waves = 3 slots at 3 or 5 query blocks, where two slots would leave a last round to one
// wave pair), 76 VGPRs (86 varlen), no scratch; the MFMAs of one wave issue under the exp2 / convert sequences
// of the others on its SIMD.  The other form built -- a wave owning one query block of BOTH heads, the
// two heads as two independent chains in one loop body, 126 VGPRs, 4 waves per SIMD -- tied at
// 512 x 128 and lost 4 to 9 % at 512 x 32, 256 x 160 and 64 x 512, and is gone.
//
// Shared with the 64-wide kernel through attention_tile.h: the LDS plan, the launch, kLazy / kMaxSeq and the
// operands of the P V k-step (pv_fragment, vt_operand).  The staging pass, the key-bias fill, the varlen
// prologue and the softmax tile below are still that kernel's text, copied: a change to one belongs in both.
// Kept from the 64-wide kernel: the online softmax in log2 units with the lazy rescale (kLazy), the
// key bias kb = 0 / -FLT_MAX (masked: finite, so a row of masked keys is HF's uniform softmax) / -inf
// (tile padding), non-temporal K / V loads, Q scaled as bf16(fp32 q * scale), 16-B ctx stores: the
// two lane halves of an O^T accumulator hold the two 8-B halves of each 16-B piece of a query's row,
// so they trade one half each (a cross-half shuffle) and every lane stores two whole 16-B pieces: a
// head's 64-B row leaves in two consecutive instructions of one wave.
#include "attention_tile.h"
#include "drt_common.h"

namespace drt {

struct Attn32Args {
  const __bf16* qkv;          // [rows][3 H]  (Q | K | V, head-major inside each)
  const int64_t* mask;        // padded: [B][L] attention_mask (1 = token, 0 = pad) or null
  __bf16* ctx;                // [rows][H]
  int64_t L;                  // padded: rows = B L
  int heads, H;               // H = heads * 32, heads even
  float scale;
  const int32_t* cu_seqlens;  // varlen: [B + 1] row offsets
  const int32_t* seq_ids;     // varlen: the sequences of this launch, or null: 0 .. n_seqs - 1
  int max_len;                // varlen: bound of every listed length (sizes the LDS image); longer ones are clamped
};

template <bool VL>
__global__ __launch_bounds__(384) __attribute__((amdgpu_waves_per_eu(4, 8)))
void attention_hd32_kernel(Attn32Args a) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int pairs = a.heads >> 1;
  const int64_t g = blockIdx.x / pairs;
  const int64_t b = VL ? (a.seq_ids ? a.seq_ids[g] : g) : g;
  const int64_t row0 = VL ? a.cu_seqlens[b] : b * a.L;
  int L = (int)a.L;
  if (VL) {   // clamped to the launch's bound: a wrong table cannot run past the LDS image
    L = a.cu_seqlens[b + 1] - (int)row0;
    L = L < a.max_len ? L : a.max_len;
    if (L <= 0) return;                     // the whole work-group: no barrier is left waiting
  }
  const int Lp = AttnLds::padded(L);        // keys padded to the 32-key tile
  const int nqb = Lp >> 5;
  const AttnLds lds(Lp);
  const int vts = lds.vts;
  char* Ks = smem;
  char* Vt = Ks + lds.ks_bytes;
  float* kb = (float*)(Vt + lds.vt_bytes);

  const int tid = threadIdx.x, NT = blockDim.x;
  const int wave = tid >> 6, lane = tid & 63;
  const int r = lane & 31, h = lane >> 5;
  const int pair = blockIdx.x % pairs;
  const int64_t ld = 3 * (int64_t)a.H;
  const __bf16* Qg = a.qkv + row0 * ld + pair * 64;
  const __bf16* Kg = Qg + a.H;
  const __bf16* Vg = Qg + 2 * a.H;
  // this wave's head of the pair and its query blocks qb0, qb0 + slots, ...
  const int hx = wave & 1, qb0 = wave >> 1, slots = NT >> 7;

  // ---- stage K (swizzled rows), V^T and the key bias exactly as the 64-wide kernel does: passes of
  // NT / 2 keys, thread (key group kg, 16-B chunk c8) owns keys 4 kg .. 4 kg + 3 of chunk c8, all 8
  // global loads of a pass before any LDS store, V^T as 8 ds_write_b64.  (Its Q prefetch ahead of
  // the passes is not kept.)
  const int c8 = tid & 7, kg = tid >> 3;
  for (int kp = 0; kp < Lp; kp += NT / 2) {
    u32x4 kv[4], vv[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int key = kp + kg * 4 + u;
      kv[u] = u32x4{0u, 0u, 0u, 0u};
      vv[u] = u32x4{0u, 0u, 0u, 0u};
      if (key < L) {   // non-temporal: K / V rows are read once per (sequence, head pair)
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
  __syncthreads();

  // per-lane LDS offsets (a tile starts at a multiple of 32 keys: its swizzle term never depends on it)
  const int sw = (r >> 1) & 7;
  int offK[2];
#pragma unroll
  for (int st = 0; st < 2; ++st) offK[st] = r * 128 + ((((4 * hx + 2 * st) | h) ^ sw) << 4);
  const int offV = (hx * kHd32 + r) * vts + 8 * h;

  for (int qb = qb0; qb < nqb; qb += slots) {
    const int qq = qb * 32 + r;
    const int qrow = qq < L ? qq : L - 1;
    // Q fragments (B operand, B[k = d][col = q]) scaled by `scale`: the fp32 product rounded to bf16
    bf16x8 qf[2];
#pragma unroll
    for (int st = 0; st < 2; ++st) {
      bf16x8 v = *(const bf16x8*)(Qg + (int64_t)qrow * ld + hx * kHd32 + st * 16 + h * 8);
#pragma unroll
      for (int j = 0; j < 8; ++j) v[j] = (__bf16)((float)v[j] * a.scale);
      qf[st] = v;
    }
    f32x16 o;
#pragma unroll
    for (int e = 0; e < 16; ++e) o[e] = 0.0f;
    float m = -__builtin_inff(), l = 0.0f;

    for (int kt = 0; kt < Lp; kt += 32) {
      // S^T tile: rows = keys kt.., cols = queries; the lane holds keys kt + 8 g + 4 h + {0, 1, 2, 3}
      // of query r in s[4 g ..]
      f32x16 s;
#pragma unroll
      for (int e = 0; e < 16; ++e) s[e] = 0.0f;
#pragma unroll
      for (int st = 0; st < 2; ++st) {
        const bf16x8 kf = *(const bf16x8*)(Ks + kt * 128 + offK[st]);
        s = __builtin_amdgcn_mfma_f32_32x32x16_bf16(kf, qf[st], s, 0, 0, 0);
      }
      // scores in log2 units, element pairs on the packed FP32 path
      const f32x2 l2e = {kLog2e, kLog2e};
      float mt = -__builtin_inff();
#pragma unroll
      for (int gq = 0; gq < 4; ++gq) {
        const f32x4 kbv = *(const f32x4*)(kb + kt + 8 * gq + 4 * h);
        const f32x2 lo = __builtin_elementwise_fma(f32x2{s[4 * gq], s[4 * gq + 1]}, l2e, f32x2{kbv[0], kbv[1]});
        const f32x2 hi = __builtin_elementwise_fma(f32x2{s[4 * gq + 2], s[4 * gq + 3]}, l2e, f32x2{kbv[2], kbv[3]});
        s[4 * gq] = lo[0];
        s[4 * gq + 1] = lo[1];
        s[4 * gq + 2] = hi[0];
        s[4 * gq + 3] = hi[1];
        mt = fmaxf(fmaxf(mt, fmaxf(lo[0], lo[1])), fmaxf(hi[0], hi[1]));
      }
      mt = fmaxf(mt, __shfl_xor(mt, 32, 64));
      const bool grow = mt > m + kLazy;
      if (__builtin_amdgcn_ballot_w64(grow) != 0ull) {   // rare after the first tile
        const float mn = grow ? mt : m;
        const float alpha = __builtin_amdgcn_exp2f(m - mn);
#pragma unroll
        for (int e = 0; e < 16; ++e) o[e] *= alpha;
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
      // O^T += V^T P^T over the tile's 32 keys: 2 k-steps of 16; the V^T fragment follows the key
      // order of the S^T accumulator (keys 16 ks + 4 h + {0..3} and + 8)
#pragma unroll
      for (int ks = 0; ks < 2; ++ks) {
        const bf16x8 pf = pv_fragment(s, ks);
        o = __builtin_amdgcn_mfma_f32_32x32x16_bf16(vt_operand(Vt + offV + (kt + 16 * ks) * 2), pf, o, 0, 0, 0);
      }
    }

    // O^T[d][q]: the lane holds query r's d = 8 gq + 4 h + {0..3} in o[4 gq ..], i.e. half h of the 16-B
    // piece gq of the head's row.  The halves of a lane pair (r, 0) / (r, 1) trade: h = 0 gives its
    // half of the odd pieces for the partner's half of the even ones, and then stores pieces 0 and 2,
    // h = 1 pieces 1 and 3.  Every lane takes part in the shuffles; only real queries store.
    __bf16* crow = a.ctx + (row0 + qrow) * a.H + pair * 64 + hx * kHd32;
    const float sc = 1.0f / l;
    uint2 piece[4];
#pragma unroll
    for (int gq = 0; gq < 4; ++gq) {
      bf16x4 v;
#pragma unroll
      for (int u = 0; u < 4; ++u) v[u] = (__bf16)(o[4 * gq + u] * sc);
      piece[gq] = __builtin_bit_cast(uint2, v);
    }
#pragma unroll
    for (int c = 0; c < 2; ++c) {
      const uint2 send = h ? piece[2 * c] : piece[2 * c + 1];
      uint2 recv;
      recv.x = __shfl_xor(send.x, 32, 64);
      recv.y = __shfl_xor(send.y, 32, 64);
      const uint2 own = h ? piece[2 * c + 1] : piece[2 * c];
      const u32x4 out = h ? u32x4{recv.x, recv.y, own.x, own.y} : u32x4{own.x, own.y, recv.x, recv.y};
      if (qq < L) *(u32x4*)(crow + 8 * (2 * c + h)) = out;
    }
  }
}

// One work-group per (sequence, head pair) group; `len` (L, or a varlen launch's max_len) sizes the
// LDS image and picks the wave count: 4 (two query-block slots per head), or 6 at 3 or 5 query blocks.
template <bool VL>
static int launch_attention_hd32(Attn32Args& a, int len, int64_t groups, void* stream) {
  const int nqb = AttnLds::padded(len) / 32;
  const int waves = nqb == 3 || nqb == 5 ? 6 : 4;
  return launch_attention_lds((const void*)attention_hd32_kernel<VL>, a, len, false, groups, waves * 64, stream);
}

}  // namespace drt

using namespace drt;

extern "C" {

int drt_attention_hd32_forward_bf16(const void* qkv, const int64_t* mask, void* ctx, int64_t B, int64_t L,
                                    int32_t heads, float scale, void* stream) {
  DRT_REQUIRE(B >= 0 && L > 0 && L <= kMaxSeq && heads > 0 && heads % 2 == 0);
  DRT_REQUIRE(B * (heads / 2) < (1ll << 31));
  if (B == 0) return DRT_OK;
  DRT_REQUIRE(qkv && ctx && (uintptr_t)qkv % 16 == 0 && (uintptr_t)ctx % 16 == 0);
  Attn32Args a{(const __bf16*)qkv, mask, (__bf16*)ctx, L, heads, heads * kHd32, scale, nullptr, nullptr, 0};
  return launch_attention_hd32<false>(a, (int)L, B * (heads / 2), stream);
}

int drt_attention_hd32_varlen_forward_bf16(const void* qkv, const int32_t* cu_seqlens, const int32_t* seq_ids,
                                           int64_t n_seqs, int32_t max_len, void* ctx, int32_t heads, float scale,
                                           void* stream) {
  DRT_REQUIRE(n_seqs >= 0 && max_len > 0 && max_len <= kMaxSeq && heads > 0 && heads % 2 == 0);
  DRT_REQUIRE(n_seqs * (heads / 2) < (1ll << 31));
  if (n_seqs == 0) return DRT_OK;
  DRT_REQUIRE(qkv && cu_seqlens && ctx && (uintptr_t)qkv % 16 == 0 && (uintptr_t)ctx % 16 == 0);
  Attn32Args a{(const __bf16*)qkv, nullptr, (__bf16*)ctx, 0, heads, heads * kHd32, scale, cu_seqlens, seq_ids, max_len};
  return launch_attention_hd32<true>(a, max_len, n_seqs * (heads / 2), stream);
}

}  // extern "C"
