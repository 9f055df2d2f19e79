// Row LayerNorm helpers shared by the encoder kernels and the GEMM's fused split-K + LayerNorm
// finish (one wave per row, H = 64 * EPL, EPL <= 16).
#pragma once
#include <type_traits>

#include "drt_common.h"

namespace drt {

// The row layout, stated once: a lane's EPL elements are EPL / W chunks of W consecutive columns,
// element e = column (e / W) * 64 W + lane * W + e % W.  W = 4 when EPL is a multiple of 4 (256-column
// chunks: 16-B fp32 loads, 8-B bf16 stores -- H = 256 .. 1024), else 2 (EPL = 6, H = 384: three
// 128-column chunks of 8-B fp32 loads and 4-B bf16 stores).  The sums run over e in order whatever W is.
template <int EPL>
struct RowChunks {
  static_assert(EPL % 2 == 0 && EPL <= 16, "row kernels: an even number of elements per lane, H <= 1024");
  static constexpr int W = EPL % 4 == 0 ? 4 : 2, N = EPL / W, STRIDE = 64 * W;
};
template <int W>
using f32v = float __attribute__((ext_vector_type(W)));
template <int W>
using bf16v = __bf16 __attribute__((ext_vector_type(W)));

// x[e] = (float)row[column of e]: the lane's part of an fp32 or bf16 row
template <int EPL, typename T>
__device__ __forceinline__ void row_load(const T* row, int lane, float (&x)[EPL]) {
  using RC = RowChunks<EPL>;
  typedef T vec __attribute__((ext_vector_type(RC::W)));
#pragma unroll
  for (int j = 0; j < RC::N; ++j) {
    const vec a = *(const vec*)(row + j * RC::STRIDE + lane * RC::W);
#pragma unroll
    for (int u = 0; u < RC::W; ++u) x[j * RC::W + u] = (float)a[u];
  }
}

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
  using RC = RowChunks<EPL>;
#pragma unroll
  for (int j = 0; j < RC::N; ++j) {
    const int c = j * RC::STRIDE + lane * RC::W;
    bf16v<RC::W> o;
#pragma unroll
    for (int u = 0; u < RC::W; ++u) o[u] = (__bf16)((x[j * RC::W + u] - mean) * rstd * gamma[c + u] + beta[c + u]);
    *(bf16v<RC::W>*)(out_row + c) = o;
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
  using RC = RowChunks<EPL>;
  float x[EPL];
#pragma unroll
  for (int j = 0; j < RC::N; ++j) {
    const int c = j * RC::STRIDE + lane * RC::W;
    const f32v<RC::W> a = *(const f32v<RC::W>*)(w + c);
    const f32v<RC::W> b = *(const f32v<RC::W>*)(p + c);
    const f32v<RC::W> d = *(const f32v<RC::W>*)(y + c);
#pragma unroll
    for (int u = 0; u < RC::W; ++u) x[j * RC::W + u] = (a[u] + d[u]) + b[u];  // (word + type) + position, as HF
    if (pre) {   // training forward: the pre-LN sum, input of the LayerNorm backward
      bf16v<RC::W> o;
#pragma unroll
      for (int u = 0; u < RC::W; ++u) o[u] = (__bf16)x[j * RC::W + u];
      *(bf16v<RC::W>*)(pre + t * H + c) = o;
    }
  }
  ln_row<EPL>(x, gamma, beta, eps, lane, H, out + t * H);
}

// ln_row with gamma / beta already in registers (g[e], b[e] of element e's column, RowChunks):
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
  using RC = RowChunks<EPL>;
#pragma unroll
  for (int j = 0; j < RC::N; ++j) {
    const int c = j * RC::STRIDE + lane * RC::W;
    bf16v<RC::W> o;
#pragma unroll
    for (int u = 0; u < RC::W; ++u) o[u] = (__bf16)((x[j * RC::W + u] - mean) * rstd * g[j * RC::W + u] + b[j * RC::W + u]);
    *(bf16v<RC::W>*)(out_row + c) = o;
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

// The same plus H = 384 (EPL = 6, MiniLM-class towers): the inference row entries only -- drt_embed_ln,
// drt_embed_ln_packed and the two LayerNorms.
template <typename F>
inline int dispatch_epl_or_384(int64_t H, F&& f) {
  if (H == 384) {
    f(std::integral_constant<int, 6>{});
    return DRT_OK;
  }
  return dispatch_epl(H, f);
}

}  // namespace drt
