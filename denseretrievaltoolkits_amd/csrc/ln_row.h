// Row LayerNorm helpers shared by the encoder kernels and the GEMM's fused split-K + LayerNorm
// finish (one wave per row, H = 64 * EPL, EPL a multiple of 4 and <= 16).
#pragma once
#include <type_traits>

#include "drt_common.h"

namespace drt {

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

template <int EPL>
__device__ __forceinline__ void ln_row(float (&x)[EPL], const float* gamma, const float* beta, float eps, int lane,
                                       int H, __bf16* out_row) {
  float s = 0.f;
#pragma unroll
  for (int e = 0; e < EPL; ++e) s += x[e];
  const float mean = wave_sum(s) / (float)H;
  float v = 0.f;
#pragma unroll
  for (int e = 0; e < EPL; ++e) {
    const float d = x[e] - mean;
    v += d * d;
  }
  const float var = wave_sum(v) / (float)H;
  const float rstd = rsqrtf(var + eps);
  // element e of lane: column c = (e / 4) * 256 + lane * 4 + (e % 4)   (4-wide chunks)
#pragma unroll
  for (int e4 = 0; e4 < EPL / 4; ++e4) {
    const int c = e4 * 256 + lane * 4;
    bf16x4 o;
#pragma unroll
    for (int u = 0; u < 4; ++u) o[u] = (__bf16)((x[e4 * 4 + u] - mean) * rstd * gamma[c + u] + beta[c + u]);
    *(bf16x4*)(out_row + c) = o;
  }
}

// One row of BertEmbeddings (modeling_bert.py:68-108) for the wave: out row t = LayerNorm(word[id] +
// type[tt] + position[pos]), fp32; shared by embed_ln_kernel (encoder.hip: t = b L + pos) and
// embed_ln_packed_kernel (packed.hip: t the packed row of token (b, pos)), which differ only in how
// they find (id, tt, pos) -- so packed and padded rows agree bit for bit.
template <int EPL>
__device__ __forceinline__ void embed_ln_row(int64_t id, int64_t tt, int64_t pos, int64_t t, const float* wemb,
                                             const float* pemb, const float* temb, const float* gamma,
                                             const float* beta, float eps, int lane, int H, __bf16* out, __bf16* pre) {
  const float* w = wemb + id * H;
  const float* p = pemb + pos * H;
  const float* y = temb + tt * H;
  float x[EPL];
#pragma unroll
  for (int e4 = 0; e4 < EPL / 4; ++e4) {
    const int c = e4 * 256 + lane * 4;
    const f32x4 a = *(const f32x4*)(w + c);
    const f32x4 b = *(const f32x4*)(p + c);
    const f32x4 d = *(const f32x4*)(y + c);
#pragma unroll
    for (int u = 0; u < 4; ++u) x[e4 * 4 + u] = (a[u] + d[u]) + b[u];  // (word + type) + position, as HF
    if (pre) {   // training forward: the pre-LN sum, input of the LayerNorm backward
      bf16x4 o;
#pragma unroll
      for (int u = 0; u < 4; ++u) o[u] = (__bf16)x[e4 * 4 + u];
      *(bf16x4*)(pre + t * H + c) = o;
    }
  }
  ln_row<EPL>(x, gamma, beta, eps, lane, H, out + t * H);
}

// ln_row with gamma / beta already in registers (g[e], b[e] of column (e / 4) * 256 + lane * 4 + e % 4):
// the same arithmetic in the same order, for kernels that normalise many rows per wave.
template <int EPL>
__device__ __forceinline__ void ln_row_gb(float (&x)[EPL], const float (&g)[EPL], const float (&b)[EPL], float eps,
                                          int lane, int H, __bf16* out_row) {
  float s = 0.f;
#pragma unroll
  for (int e = 0; e < EPL; ++e) s += x[e];
  const float mean = wave_sum(s) / (float)H;
  float v = 0.f;
#pragma unroll
  for (int e = 0; e < EPL; ++e) {
    const float d = x[e] - mean;
    v += d * d;
  }
  const float var = wave_sum(v) / (float)H;
  const float rstd = rsqrtf(var + eps);
#pragma unroll
  for (int e4 = 0; e4 < EPL / 4; ++e4) {
    const int c = e4 * 256 + lane * 4;
    bf16x4 o;
#pragma unroll
    for (int u = 0; u < 4; ++u) o[u] = (__bf16)((x[e4 * 4 + u] - mean) * rstd * g[e4 * 4 + u] + b[e4 * 4 + u]);
    *(bf16x4*)(out_row + c) = o;
  }
}

// Work-groups of the row-looping norms (layernorm_bf16_kernel, rmsnorm_bf16_kernel): 8 per CU
// (32 waves), at most one per 4 rows.
inline unsigned ln_rows_grid(int64_t M) {
  static int cus = 0;
  if (cus == 0) {
    int dev = 0, v = 0;
    cus = (hipGetDevice(&dev) == hipSuccess &&
           hipDeviceGetAttribute(&v, hipDeviceAttributeMultiprocessorCount, dev) == hipSuccess && v > 0)
              ? v
              : 256;
  }
  const int64_t need = (M + 3) / 4, cap = (int64_t)cus * 8;
  return (unsigned)(need < cap ? need : cap);
}

// Host dispatch on the elements per lane of a row kernel: calls f(std::integral_constant<int, EPL>)
// for H = 64 * EPL with EPL in {4, 8, 12, 16} (the instantiations every row kernel has), so
// `kernel<decltype(E)::value>` names the kernel inside f; DRT_EINVAL for any other H.
template <typename F>
inline int dispatch_epl(int64_t H, F&& f) {
  switch (H / 64) {
    case 4: f(std::integral_constant<int, 4>{}); return DRT_OK;
    case 8: f(std::integral_constant<int, 8>{}); return DRT_OK;
    case 12: f(std::integral_constant<int, 12>{}); return DRT_OK;
    case 16: f(std::integral_constant<int, 16>{}); return DRT_OK;
    default: return DRT_EINVAL;
  }
}

}  // namespace drt
