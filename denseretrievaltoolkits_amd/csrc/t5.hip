// T5 encoder forward kernels (HF T5EncoderModel in eval mode: transformers/models/t5/modeling_t5.py
// T5Stack embedding, T5LayerNorm, T5DenseGatedActDense).  The projections are the bf16 GEMMs of
// gemm.hip (ReLU: epilogue flag bit 3) and the attention is the RB instantiation of encoder.hip's
// kernel (drt_attention_forward_bf16 with relbias).
//
//   t5_embed     shared.weight[ids] -> the bf16 residual stream (no position / type table, no norm)
//   rmsnorm      x * rsqrt(mean(x^2) + eps) * w, fp32 statistics, no mean, no bias
//   gated_gelu   gelu_new(X[:, :F]) * X[:, F:] of the [wi_0; wi_1] GEMM's output
#include "drt_common.h"
#include "ln_row.h"

namespace drt {

// One wave per token, 16 B of the fp32 row per lane and step.
__global__ __launch_bounds__(256) void t5_embed_kernel(const int64_t* ids, int64_t T, const float* table, int H,
                                                       __bf16* out) {
  const int lane = threadIdx.x & 63;
  const int64_t t = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (t >= T) return;
  const float* w = table + ids[t] * H;
  for (int c = lane * 4; c < H; c += 256) {
    const f32x4 a = *(const f32x4*)(w + c);
    bf16x4 o;
#pragma unroll
    for (int u = 0; u < 4; ++u) o[u] = (__bf16)a[u];
    *(bf16x4*)(out + t * H + c) = o;
  }
}

// T5LayerNorm over the bf16 residual stream.  The row-looping shape of layernorm_bf16_kernel: one
// round of work-groups, each wave normalising rows t, t + waves, ... with the weight in registers
// and the next row's loads issued before the current row's reduction.  out may alias X.
template <int EPL>
__global__ __launch_bounds__(256) void rmsnorm_bf16_kernel(const __bf16* X, int64_t M, int H, const float* weight,
                                                           float eps, __bf16* out) {
  const int lane = threadIdx.x & 63;
  const int64_t t0 = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  const int64_t nw = (int64_t)gridDim.x * 4;
  if (t0 >= M) return;
  float g[EPL];
#pragma unroll
  for (int e4 = 0; e4 < EPL / 4; ++e4) {
    const f32x4 gv = *(const f32x4*)(weight + e4 * 256 + lane * 4);
#pragma unroll
    for (int u = 0; u < 4; ++u) g[e4 * 4 + u] = gv[u];
  }
  bf16x4 cur[EPL / 4];
#pragma unroll
  for (int e4 = 0; e4 < EPL / 4; ++e4) cur[e4] = *(const bf16x4*)(X + t0 * H + e4 * 256 + lane * 4);
  for (int64_t t = t0; t < M; t += nw) {
    const int64_t tn = t + nw;
    bf16x4 nxt[EPL / 4];
    if (tn < M) {
#pragma unroll
      for (int e4 = 0; e4 < EPL / 4; ++e4) nxt[e4] = *(const bf16x4*)(X + tn * H + e4 * 256 + lane * 4);
    }
    float x[EPL];
    float ss = 0.f;
#pragma unroll
    for (int e4 = 0; e4 < EPL / 4; ++e4)
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        x[e4 * 4 + u] = (float)cur[e4][u];
        ss += x[e4 * 4 + u] * x[e4 * 4 + u];
      }
    const float rstd = rsqrtf(wave_sum(ss) / (float)H + eps);
#pragma unroll
    for (int e4 = 0; e4 < EPL / 4; ++e4) {
      bf16x4 o;
#pragma unroll
      for (int u = 0; u < 4; ++u) o[u] = (__bf16)(x[e4 * 4 + u] * rstd * g[e4 * 4 + u]);   // HF: w * (x * rstd)
      *(bf16x4*)(out + t * H + e4 * 256 + lane * 4) = o;
    }
#pragma unroll
    for (int e4 = 0; e4 < EPL / 4; ++e4) cur[e4] = nxt[e4];
  }
}

// transformers ACT2FN["gelu_new"] = NewGELUActivation (T5 v1.1's gated-gelu)
__device__ __forceinline__ float gelu_new(float a) {
  return 0.5f * a * (1.0f + tanhf(0.7978845608028654f * (a + 0.044715f * a * a * a)));
}

// out[m, f] = gelu_new(X[m, f]) * X[m, F + f]: 8 columns (16 B of each half) per thread.
__global__ __launch_bounds__(256) void gated_gelu_new_kernel(const __bf16* X, int64_t M, int64_t F, __bf16* out) {
  const int64_t f8 = F / 8;
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= M * f8) return;
  const int64_t m = i / f8, f = (i % f8) * 8;
  const bf16x8 a = *(const bf16x8*)(X + m * 2 * F + f);
  const bf16x8 b = *(const bf16x8*)(X + m * 2 * F + F + f);
  bf16x8 o;
#pragma unroll
  for (int u = 0; u < 8; ++u) o[u] = (__bf16)(gelu_new((float)a[u]) * (float)b[u]);
  *(bf16x8*)(out + m * F + f) = o;
}

}  // namespace drt

using namespace drt;

extern "C" {

int drt_t5_embed_bf16(const int64_t* ids, int64_t B, int64_t L, const float* table, int32_t H, void* out,
                      void* stream) {
  DRT_REQUIRE(B >= 0 && L > 0 && H > 0 && H % 4 == 0);
  const int64_t T = B * L;
  if (T == 0) return DRT_OK;
  DRT_REQUIRE(ids && table && out);
  hipLaunchKernelGGL(t5_embed_kernel, dim3((unsigned)((T + 3) / 4)), dim3(256), 0, (hipStream_t)stream, ids, T, table,
                     (int)H, (__bf16*)out);
  return hip_status(hipGetLastError());
}

int drt_rmsnorm_bf16(const void* X, int64_t M, int32_t H, const float* weight, float eps, void* out, void* stream) {
  DRT_REQUIRE(M >= 0 && H > 0 && H % 256 == 0 && H <= 1024);
  if (M == 0) return DRT_OK;
  DRT_REQUIRE(X && weight && out);
  hipStream_t s = (hipStream_t)stream;
  const dim3 grid(ln_rows_grid(M));
  if (const int rc = dispatch_epl(H, [&](auto E) {
        hipLaunchKernelGGL(rmsnorm_bf16_kernel<decltype(E)::value>, grid, dim3(256), 0, s, (const __bf16*)X, M, H,
                           weight, eps, (__bf16*)out);
      }))
    return rc;
  return hip_status(hipGetLastError());
}

int drt_gated_gelu_new_bf16(const void* X, int64_t M, int64_t F, void* out, void* stream) {
  DRT_REQUIRE(M >= 0 && F > 0 && F % 8 == 0);
  if (M == 0) return DRT_OK;
  DRT_REQUIRE(X && out);
  DRT_REQUIRE((uintptr_t)X % 16 == 0 && (uintptr_t)out % 16 == 0);
  const int64_t units = M * (F / 8);
  hipLaunchKernelGGL(gated_gelu_new_kernel, dim3((unsigned)((units + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                     (const __bf16*)X, M, F, (__bf16*)out);
  return hip_status(hipGetLastError());
}

}  // extern "C"
