// One-step T5 decoder kernels (HF T5ForConditionalGeneration with a single decoder token:
// transformers/models/t5/modeling_t5.py, T5LayerCrossAttention in eval mode).  With one query per
// sequence the cross-attention is taken in absorbed form, so the encoder output E [B, L, D] is read
// once and no K / V projection of it is ever formed:
//
//   head_expand   qt[b, h, :] = sum_j q[b, 64 h + j] Wk[64 h + j, :]      (the query through Wk)
//   cross_pool    p = softmax_l(qt[b, h, :] . E[b, l, :] + key mask);  pooled[b, h, :] = sum_l p_l E[b, l, :]
//   head_reduce   ctx[b, 64 h + j] = Wv[64 h + j, :] . pooled[b, h, :]     (the pooled row through Wv)
//
// T5 scales no score and the cross-attention has no position bias.  The norms, the other
// projections and the FFN are the kernels of t5.hip and gemm.hip.
#include "drt_common.h"

namespace drt {

// ---------------------------------------------------------------------------------------------
// cross_pool: one work-group of 4 waves per sequence, online softmax over 32-key tiles.
//
// Wave w owns the D / 4 columns [w WC, (w + 1) WC) of E for both products, so its slice of a tile
// lives in a wave-private LDS image (no work-group barrier guards it) that the wave fills from
// registers: the loads of tile t + 1 are issued before the arithmetic of tile t and written after it.
//   scores   S^T[key, head] = E qt^T with v_mfma_f32_16x16x32_bf16: A = 16 keys x 32 columns of the
//            image (ds_read_b128 along d), B = qt (registers, heads padded to 16 with zeros).  Each
//            wave sums its own columns; the four partial tiles meet in LDS (one barrier per tile, two
//            alternating slabs) and every wave adds them in wave order -> the same bits in every wave.
//   softmax  the S^T output has the head on the lane (l & 15) and keys 4 g + r (g = l >> 4) of both
//            16-key halves in registers: max and sum over a head's 32 keys are 8 registers and two
//            xor-shuffles.  fp32 running max / sum per head, replicated in the four lane groups.
//   pooling  O[head, d] += P E: that register layout IS the A operand with the k order
//            j < 4: key 4 g + j, j >= 4: key 16 + 4 g + (j - 4); the B operand takes the image's rows
//            in the same order, column-wise, with two ds_read_b64_tr_b16.  fp32 accumulators of
//            16 heads x WC columns per wave (4 per lane and 16-column slice).
// Image rows are WC * 2 + 32 bytes: 32 or 160 mod 256, so the 8 rows x 32 B of a transposed read's
// 32-lane half fall in distinct banks.
// Mask: a masked key and the tile padding past L score -inf; a sequence with no live key gets the
// uniform softmax over its L keys (qt is replaced by zero and every key < L counts as live).  Rows
// past L are staged as zeros, so P = 0 meets only finite values.
// ---------------------------------------------------------------------------------------------
constexpr int kCpKeys = 32;
constexpr int kCpMaxSeq = 512;

typedef short cp_v4i16 __attribute__((ext_vector_type(4)));

template <int DQ>
struct CpGeom {
  static constexpr int D = 256 * DQ;
  static constexpr int WC = 64 * DQ;           // columns per wave
  static constexpr int KS = WC / 32;           // score k-steps per wave
  static constexpr int NT = WC / 16;           // pooled 16-column slices per wave
  static constexpr int RS = WC * 2 + 32;       // image row stride, bytes
  static constexpr int CH = WC / 8;            // 16-B chunks per image row
  static constexpr int NLD = kCpKeys * CH / 64;  // 16-B loads per lane and tile
  static constexpr int IMG = kCpKeys * RS;     // bytes per wave image
  static constexpr int PART = 4 * IMG;         // offset of the partial-score slabs [2][4 waves][2][64] f32x4
  static constexpr int ALIVE = PART + 2 * 4 * 2 * 64 * 16;   // offset of the live-key bytes [512]
  static constexpr int BYTES = ALIVE + kCpMaxSeq;
};

template <int DQ>
__global__ __launch_bounds__(256) void t5_cross_pool_kernel(const __bf16* qt, const __bf16* enc, const int64_t* mask,
                                                            __bf16* pooled, int L, int heads) {
  typedef CpGeom<DQ> G;
  __shared__ __attribute__((aligned(16))) char lds[G::BYTES];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int i16 = lane & 15, g = lane >> 4;
  const int64_t b = blockIdx.x;
  char* img = lds + w * G::IMG;
  f32x4* part = (f32x4*)(lds + G::PART);
  unsigned char* alive = (unsigned char*)(lds + G::ALIVE);

  // live keys: thread t decides keys t and t + 256
  bool in[2], mk[2];
  int any = 0;
#pragma unroll
  for (int u = 0; u < 2; ++u) {
    const int l = tid + 256 * u;
    in[u] = l < L;
    mk[u] = in[u] && (mask == nullptr || mask[b * L + l] != 0);
    any |= mk[u];
  }
  const bool dead = !__syncthreads_or(any);
#pragma unroll
  for (int u = 0; u < 2; ++u) alive[tid + 256 * u] = (in[u] && (mk[u] || dead)) ? 1 : 0;

  // this wave's columns of qt as the scores' B operand: lane (head i16, g) holds columns 32 ks + 8 g .. + 7
  bf16x8 qf[G::KS];
#pragma unroll
  for (int ks = 0; ks < G::KS; ++ks) {
    bf16x8 v = {0, 0, 0, 0, 0, 0, 0, 0};
    if (i16 < heads && !dead)
      v = *(const bf16x8*)(qt + (b * heads + i16) * G::D + w * G::WC + ks * 32 + g * 8);
    qf[ks] = v;
  }

  const __bf16* esrc = enc + b * (int64_t)L * G::D + w * G::WC;
  const int ntiles = (L + kCpKeys - 1) / kCpKeys;
  u32x4 nx[G::NLD];

  auto stage_load = [&](int k0) {
#pragma unroll
    for (int i = 0; i < G::NLD; ++i) {
      const int idx = i * 64 + lane, row = idx / G::CH, c = idx % G::CH;
      const int key = k0 + row < L ? k0 + row : L - 1;      // clamped: every load is in bounds
      nx[i] = *(const u32x4*)(esrc + (int64_t)key * G::D + c * 8);
    }
  };
  auto stage_write = [&](int k0) {
#pragma unroll
    for (int i = 0; i < G::NLD; ++i) {
      const int idx = i * 64 + lane, row = idx / G::CH, c = idx % G::CH;
      const u32x4 z = {0u, 0u, 0u, 0u};
      *(u32x4*)(img + row * G::RS + c * 16) = k0 + row < L ? nx[i] : z;
    }
  };

  stage_load(0);
  stage_write(0);

  f32x4 acc[G::NT];
#pragma unroll
  for (int nt = 0; nt < G::NT; ++nt) acc[nt] = f32x4{0.f, 0.f, 0.f, 0.f};
  float m = -__builtin_inff(), lsum = 0.f;

  const int offA = i16 * G::RS + g * 16;                              // + ks * 64 (+ 16 RS: second half)
  const int offT = (4 * g + (i16 >> 2)) * G::RS + 8 * (i16 & 3);      // + nt * 32 (+ 16 RS)
  typedef __attribute__((address_space(3))) cp_v4i16 lds_v4;

  for (int t = 0; t < ntiles; ++t) {
    const int k0 = t * kCpKeys;
    if (t + 1 < ntiles) stage_load(k0 + kCpKeys);
    asm volatile("" ::: "memory");

    // partial scores over this wave's columns
    f32x4 s0 = {0.f, 0.f, 0.f, 0.f}, s1 = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int ks = 0; ks < G::KS; ++ks) {
      const bf16x8 a0 = *(const bf16x8*)(img + offA + ks * 64);
      const bf16x8 a1 = *(const bf16x8*)(img + offA + ks * 64 + 16 * G::RS);
      s0 = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a0, qf[ks], s0, 0, 0, 0);
      s1 = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a1, qf[ks], s1, 0, 0, 0);
    }
    f32x4* slab = part + (t & 1) * 512;
    slab[(w * 2 + 0) * 64 + lane] = s0;
    slab[(w * 2 + 1) * 64 + lane] = s1;
    __syncthreads();
    s0 = slab[0 * 64 + lane];
    s1 = slab[1 * 64 + lane];
#pragma unroll
    for (int ww = 1; ww < 4; ++ww) {
      s0 += slab[(ww * 2 + 0) * 64 + lane];
      s1 += slab[(ww * 2 + 1) * 64 + lane];
    }

    // online softmax of head i16 over keys k0 + 4 g + r and k0 + 16 + 4 g + r
    const uint32_t al0 = *(const uint32_t*)(alive + k0 + 4 * g);
    const uint32_t al1 = *(const uint32_t*)(alive + k0 + 16 + 4 * g);
    float mt = -__builtin_inff();
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      s0[r] = ((al0 >> (8 * r)) & 1u) ? s0[r] : -__builtin_inff();
      s1[r] = ((al1 >> (8 * r)) & 1u) ? s1[r] : -__builtin_inff();
      mt = fmaxf(mt, fmaxf(s0[r], s1[r]));
    }
    mt = fmaxf(mt, __shfl_xor(mt, 16, 64));
    mt = fmaxf(mt, __shfl_xor(mt, 32, 64));
    const float mn = fmaxf(m, mt);
    const float ms = mn == -__builtin_inff() ? 0.f : mn;        // no live key yet: P = exp2(-inf) = 0
    const float alpha = m == -__builtin_inff() ? 0.f : __builtin_amdgcn_exp2f((m - ms) * kLog2e);
    m = mn;
    float ps = 0.f;
    bf16x8 pf;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const float p0 = __builtin_amdgcn_exp2f((s0[r] - ms) * kLog2e);
      const float p1 = __builtin_amdgcn_exp2f((s1[r] - ms) * kLog2e);
      ps += p0 + p1;
      pf[r] = (__bf16)p0;
      pf[4 + r] = (__bf16)p1;
    }
    ps += __shfl_xor(ps, 16, 64);
    ps += __shfl_xor(ps, 32, 64);
    lsum = lsum * alpha + ps;

    // the accumulators hold heads 4 g + r: their rescale factors sit on lanes 4 g + r
    float ar[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) ar[r] = __shfl(alpha, 4 * g + r, 64);
#pragma unroll
    for (int nt = 0; nt < G::NT; ++nt) {
      const cp_v4i16 x = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_v4*)(img + offT + nt * 32));
      const cp_v4i16 y = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_v4*)(img + offT + nt * 32 + 16 * G::RS));
      bf16x8 ef;
      __builtin_memcpy(&ef, &x, 8);
      __builtin_memcpy((char*)&ef + 8, &y, 8);
      f32x4 a = acc[nt];
#pragma unroll
      for (int r = 0; r < 4; ++r) a[r] *= ar[r];
      acc[nt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(pf, ef, a, 0, 0, 0);
    }

    // the wave's own image: its reads above are issued, LDS runs a wave's operations in order
    asm volatile("" ::: "memory");
    if (t + 1 < ntiles) stage_write(k0 + kCpKeys);
    asm volatile("" ::: "memory");
  }

#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int head = 4 * g + r;
    const float inv = 1.0f / __shfl(lsum, head, 64);
    if (head < heads) {
      __bf16* o = pooled + (b * heads + head) * G::D + w * G::WC + i16;
#pragma unroll
      for (int nt = 0; nt < G::NT; ++nt) o[nt * 16] = (__bf16)(acc[nt][r] * inv);
    }
  }
}

// ---------------------------------------------------------------------------------------------
// head_expand: qt[b, h, c] = sum_{j < 64} q[b, 64 h + j] Wk[64 h + j, c], per head a [B, 64] x [64, D]
// product on v_mfma_f32_16x16x32_bf16.  One work-group per (head, 256 columns of Wk, 64 rows of b):
// the head's [64, 256] slice of Wk is staged once in LDS ([j][256] rows of 512 + 32 bytes, the pool
// kernel's image) and read column-wise with ds_read_b64_tr_b16 as the B operand, in the k order
// e < 4: j = 32 s + 4 g + e, e >= 4: j = 32 s + 16 + 4 g + (e - 4) per k-step s; each wave takes 16 rows
// of b, whose q values in that same order (two 8-B loads per k-step) are the A operand.  fp32
// accumulation, one rounding.
// ---------------------------------------------------------------------------------------------
constexpr int kHeCols = 256;
constexpr int kHeRS = kHeCols * 2 + 32;

__global__ __launch_bounds__(256) void t5_head_expand_kernel(const __bf16* q, const __bf16* Wk, __bf16* qt, int64_t B,
                                                             int heads, int D) {
  __shared__ __attribute__((aligned(16))) char img[64 * kHeRS];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, i16 = lane & 15, g = lane >> 4;
  const int h = blockIdx.x, d0 = blockIdx.y * kHeCols;
  const int64_t b0 = (int64_t)blockIdx.z * 64 + w * 16;
  const int I = heads * 64;
  u32x4 st[8];
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    const int idx = i * 256 + tid, row = idx >> 5, c = idx & 31;
    st[i] = *(const u32x4*)(Wk + (int64_t)(h * 64 + row) * D + d0 + c * 8);
  }
  const int64_t br = b0 + i16 < B ? b0 + i16 : B - 1;      // clamped: the surplus rows are not stored
  bf16x8 af[2];
#pragma unroll
  for (int s = 0; s < 2; ++s) {
    const bf16x4 lo = *(const bf16x4*)(q + br * I + h * 64 + 32 * s + 4 * g);
    const bf16x4 hi = *(const bf16x4*)(q + br * I + h * 64 + 32 * s + 16 + 4 * g);
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      af[s][e] = lo[e];
      af[s][4 + e] = hi[e];
    }
  }
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    const int idx = i * 256 + tid, row = idx >> 5, c = idx & 31;
    *(u32x4*)(img + row * kHeRS + c * 16) = st[i];
  }
  __syncthreads();
  if (b0 >= B) return;
  typedef __attribute__((address_space(3))) cp_v4i16 lds_v4;
  const int offT = (4 * g + (i16 >> 2)) * kHeRS + 8 * (i16 & 3);
#pragma unroll 4
  for (int nt = 0; nt < kHeCols / 16; ++nt) {
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int s = 0; s < 2; ++s) {
      const cp_v4i16 x = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_v4*)(img + s * 32 * kHeRS + offT + nt * 32));
      const cp_v4i16 y =
          __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_v4*)(img + s * 32 * kHeRS + offT + nt * 32 + 16 * kHeRS));
      bf16x8 wf;
      __builtin_memcpy(&wf, &x, 8);
      __builtin_memcpy((char*)&wf + 8, &y, 8);
      acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af[s], wf, acc, 0, 0, 0);
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int64_t b = b0 + 4 * g + r;
      if (b < B) qt[(b * heads + h) * D + d0 + nt * 16 + i16] = (__bf16)acc[r];
    }
  }
}

// ---------------------------------------------------------------------------------------------
// head_reduce: ctx[b, 64 h + j] = Wv[64 h + j, :] . pooled[b, h, :], per head a [B, D] x [D, 64] product
// on v_mfma_f32_16x16x32_bf16.  Both operands run along d in memory, so the fragments are plain 16-B
// global loads (A: pooled row b0 + (l & 15), B: Wv row 64 h + 16 w + (l & 15), columns 32 s + 8 g .. + 7)
// and nothing goes through LDS.  One work-group per (head, 16 rows of b), wave w takes j = 16 w ..
// 16 w + 15; two accumulators alternate over the D / 32 k-steps and are added at the end.  fp32
// accumulation, one rounding.
// ---------------------------------------------------------------------------------------------
template <int DQ>
__global__ __launch_bounds__(256) void t5_head_reduce_kernel(const __bf16* pooled, const __bf16* Wv, __bf16* ctx,
                                                             int64_t B, int heads) {
  constexpr int D = 256 * DQ, KS = D / 32;
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, i16 = lane & 15, g = lane >> 4;
  const int h = blockIdx.x;
  const int64_t b0 = (int64_t)blockIdx.y * 16;
  const int64_t br = b0 + i16 < B ? b0 + i16 : B - 1;      // clamped: the surplus rows are not stored
  const __bf16* pa = pooled + (br * heads + h) * D + g * 8;
  const __bf16* pw = Wv + (int64_t)(h * 64 + w * 16 + i16) * D + g * 8;
  f32x4 acc[2] = {{0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}};
#pragma unroll
  for (int ks = 0; ks < KS; ++ks) {
    const bf16x8 af = *(const bf16x8*)(pa + ks * 32);
    const bf16x8 wf = *(const bf16x8*)(pw + ks * 32);
    acc[ks & 1] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af, wf, acc[ks & 1], 0, 0, 0);
  }
  const int I = heads * 64;
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int64_t b = b0 + 4 * g + r;
    if (b < B) ctx[b * I + h * 64 + w * 16 + i16] = (__bf16)(acc[0][r] + acc[1][r]);
  }
}

static bool t5_dec_shape_ok(int64_t B, int32_t heads, int32_t D) {
  return B >= 0 && B <= 0x7FFFFFFF / 16 && heads >= 1 && heads <= 16 && D > 0 && D % 256 == 0 && D <= 1024;
}

}  // namespace drt

using namespace drt;

extern "C" {

int drt_t5_cross_pool_bf16(const void* qt, const void* enc, const int64_t* mask, void* pooled, int64_t B, int64_t L,
                           int32_t heads, int32_t D, void* stream) {
  DRT_REQUIRE(t5_dec_shape_ok(B, heads, D) && L >= 1 && L <= kCpMaxSeq);
  if (B == 0) return DRT_OK;
  DRT_REQUIRE(qt && enc && pooled);
  DRT_REQUIRE((uintptr_t)qt % 16 == 0 && (uintptr_t)enc % 16 == 0);
  hipStream_t s = (hipStream_t)stream;
  const __bf16* q = (const __bf16*)qt;
  const __bf16* e = (const __bf16*)enc;
  __bf16* o = (__bf16*)pooled;
  const dim3 grid((unsigned)B), block(256);
  switch (D / 256) {
    case 1: hipLaunchKernelGGL(t5_cross_pool_kernel<1>, grid, block, 0, s, q, e, mask, o, (int)L, (int)heads); break;
    case 2: hipLaunchKernelGGL(t5_cross_pool_kernel<2>, grid, block, 0, s, q, e, mask, o, (int)L, (int)heads); break;
    case 3: hipLaunchKernelGGL(t5_cross_pool_kernel<3>, grid, block, 0, s, q, e, mask, o, (int)L, (int)heads); break;
    case 4: hipLaunchKernelGGL(t5_cross_pool_kernel<4>, grid, block, 0, s, q, e, mask, o, (int)L, (int)heads); break;
    default: return DRT_EINVAL;
  }
  return hip_status(hipGetLastError());
}

int drt_t5_head_expand_bf16(const void* q, const void* Wk, void* qt, int64_t B, int32_t heads, int32_t D,
                            void* stream) {
  DRT_REQUIRE(t5_dec_shape_ok(B, heads, D));
  if (B == 0) return DRT_OK;
  DRT_REQUIRE(q && Wk && qt);
  DRT_REQUIRE((uintptr_t)Wk % 16 == 0 && (uintptr_t)q % 8 == 0);
  const int64_t groups = (B + 63) / 64;
  DRT_REQUIRE(groups <= 65535);
  hipLaunchKernelGGL(t5_head_expand_kernel, dim3((unsigned)heads, (unsigned)(D / kHeCols), (unsigned)groups), dim3(256),
                     0, (hipStream_t)stream, (const __bf16*)q, (const __bf16*)Wk, (__bf16*)qt, B, (int)heads, (int)D);
  return hip_status(hipGetLastError());
}

int drt_t5_head_reduce_bf16(const void* pooled, const void* Wv, void* ctx, int64_t B, int32_t heads, int32_t D,
                            void* stream) {
  DRT_REQUIRE(t5_dec_shape_ok(B, heads, D));
  if (B == 0) return DRT_OK;
  DRT_REQUIRE(pooled && Wv && ctx);
  DRT_REQUIRE((uintptr_t)pooled % 16 == 0 && (uintptr_t)Wv % 16 == 0);
  const int64_t groups = (B + 15) / 16;
  DRT_REQUIRE(groups <= 65535);
  hipStream_t s = (hipStream_t)stream;
  const __bf16* p = (const __bf16*)pooled;
  const __bf16* wv = (const __bf16*)Wv;
  __bf16* o = (__bf16*)ctx;
  const dim3 grid((unsigned)heads, (unsigned)groups), block(256);
  switch (D / 256) {
    case 1: hipLaunchKernelGGL(t5_head_reduce_kernel<1>, grid, block, 0, s, p, wv, o, B, (int)heads); break;
    case 2: hipLaunchKernelGGL(t5_head_reduce_kernel<2>, grid, block, 0, s, p, wv, o, B, (int)heads); break;
    case 3: hipLaunchKernelGGL(t5_head_reduce_kernel<3>, grid, block, 0, s, p, wv, o, B, (int)heads); break;
    case 4: hipLaunchKernelGGL(t5_head_reduce_kernel<4>, grid, block, 0, s, p, wv, o, B, (int)heads); break;
    default: return DRT_EINVAL;
  }
  return hip_status(hipGetLastError());
}

}  // extern "C"
