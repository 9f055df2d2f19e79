// Backward kernels of the T5 encoder tower (HF T5EncoderModel under autograd, modeling_t5.py:
// T5LayerNorm, T5DenseActDense / T5DenseGatedActDense, the shared embedding) for the bf16
// activations the training forward stores (model/t5_train_tower.py).  The projections' gradients
// are the GEMMs of gemm.hip, the attention backward with the relative-position bias is the RB
// instantiation of encoder_bwd.hip's kernels (drt_attention_backward_bf16 with relbias).
//
//   rmsnorm_bwd         y = x r g, r = rsqrt(mean x^2 + eps):
//                       dx = g dy r - x r^3 mean(g dy x) (+ a residual gradient),
//                       per-block dgamma partials (dgamma = sum_rows dy x r, fixed order)
//   gated_gelu_new_bwd  f = gelu_new(a) b:  da = dy b gelu_new'(a),  db = dy gelu_new(a)
//   relu_bwd            f = max(pre, 0):    dpre = dy (f > 0)
//                       (both with the inner dropout HF applies to f before wo: dy is first
//                       dropped with the mask of (p, seed, site) over the [T, F] index)
//   t5_embedding_bwd    dshared[ids[t]] += d[t]   (no position / type table, no padding_idx)
#include "drt_common.h"
#include "ln_row.h"

namespace drt {

__device__ __forceinline__ float t5b_wave_sum(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

constexpr int kRmsBwdBlocks = 1024;   // grid of the row pass = rows of the dgamma partials

// One wave per row (grid-stride over rows), H = 64 * EPL; lane owns columns
// (e / 4) * 256 + lane * 4 + e % 4, as layernorm_bwd_kernel.  r is recomputed from the stored bf16
// row exactly as rmsnorm_bf16_kernel computed it.  Each block leaves its dgamma partial sums in
// part[blockIdx.x][0..H) (fixed order over its rows and its 4 waves).
template <int EPL>
__global__ __launch_bounds__(256) void rmsnorm_bwd_kernel(const __bf16* dy, const __bf16* x, const float* gamma,
                                                          float eps, int64_t M, int H, const __bf16* dres, __bf16* dx,
                                                          float* part) {
  __shared__ float red[4][EPL * 64];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  float dg[EPL], gm[EPL];
#pragma unroll
  for (int e = 0; e < EPL; ++e) {
    dg[e] = 0.f;
    gm[e] = gamma[(e >> 2) * 256 + lane * 4 + (e & 3)];
  }
  for (int64_t t = (int64_t)blockIdx.x * 4 + wave; t < M; t += (int64_t)gridDim.x * 4) {
    float xv[EPL], gv[EPL];
    float ss = 0.f, sgx = 0.f;
#pragma unroll
    for (int e4 = 0; e4 < EPL / 4; ++e4) {
      const int c = e4 * 256 + lane * 4;
      const bf16x4 a = *(const bf16x4*)(x + t * H + c);
      const bf16x4 b = *(const bf16x4*)(dy + t * H + c);
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int e = e4 * 4 + u;
        xv[e] = (float)a[u];
        gv[e] = (float)b[u];            // dy for now
        ss += xv[e] * xv[e];
      }
    }
    const float r = rsqrtf(t5b_wave_sum(ss) / (float)H + eps);
#pragma unroll
    for (int e = 0; e < EPL; ++e) {
      dg[e] += gv[e] * xv[e] * r;
      gv[e] *= gm[e];                   // g dy
      sgx += gv[e] * xv[e];
    }
    const float k = t5b_wave_sum(sgx) / (float)H * r * r * r;   // r^3 mean(g dy x)
#pragma unroll
    for (int e4 = 0; e4 < EPL / 4; ++e4) {
      const int c = e4 * 256 + lane * 4;
      bf16x4 rs = {};
      if (dres) rs = *(const bf16x4*)(dres + t * H + c);
      bf16x4 o;
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int e = e4 * 4 + u;
        o[u] = (__bf16)(gv[e] * r - xv[e] * k + (dres ? (float)rs[u] : 0.f));
      }
      *(bf16x4*)(dx + t * H + c) = o;
    }
  }
#pragma unroll
  for (int e = 0; e < EPL; ++e) red[wave][e * 64 + lane] = dg[e];
  __syncthreads();
  for (int i = threadIdx.x; i < EPL * 64; i += 256) {
    const int e = i >> 6, ln = i & 63;
    const int col = (e >> 2) * 256 + ln * 4 + (e & 3);
    part[(int64_t)blockIdx.x * H + col] = ((red[0][i] + red[1][i]) + red[2][i]) + red[3][i];
  }
}

__device__ __forceinline__ float t5b_keep_scale(float v, bool drop, uint32_t thr, float inv, uint64_t seed,
                                                uint64_t site, uint64_t idx) {
  if (!drop) return v;
  return drop_hash24(seed, site, idx) >= thr ? v * inv : 0.0f;
}

// gelu_new(a) = 0.5 a (1 + tanh(u)), u = c (a + 0.044715 a^3);
// gelu_new'(a) = 0.5 (1 + tanh u) + 0.5 a (1 - tanh^2 u) c (1 + 3 * 0.044715 a^2)
// dy [M, F], X = (a | b) [M, 2F] -> dX [M, 2F] = (da | db); 8 columns of each half per thread.
__global__ __launch_bounds__(256) void gated_gelu_new_bwd_kernel(const __bf16* dy, const __bf16* X, int64_t M,
                                                                 int64_t F, float p, uint64_t seed, uint64_t site,
                                                                 __bf16* dX) {
  const int64_t f8 = F / 8;
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= M * f8) return;
  const int64_t m = i / f8, f = (i % f8) * 8;
  const bf16x8 g = *(const bf16x8*)(dy + m * F + f);
  const bf16x8 a = *(const bf16x8*)(X + m * 2 * F + f);
  const bf16x8 b = *(const bf16x8*)(X + m * 2 * F + F + f);
  const bool drop = p > 0.0f;
  const uint32_t thr = drop_threshold(p);
  const float inv = 1.0f / (1.0f - p);
  bf16x8 oa, ob;
#pragma unroll
  for (int u = 0; u < 8; ++u) {
    const float d = t5b_keep_scale((float)g[u], drop, thr, inv, seed, site, (uint64_t)(m * F + f + u));
    const float av = (float)a[u], bv = (float)b[u];
    const float th = tanhf(0.7978845608028654f * (av + 0.044715f * av * av * av));
    const float gl = 0.5f * av * (1.0f + th);
    const float dgl = 0.5f * (1.0f + th) +
                      0.5f * av * (1.0f - th * th) * 0.7978845608028654f * (1.0f + 0.134145f * av * av);
    oa[u] = (__bf16)(d * bv * dgl);
    ob[u] = (__bf16)(d * gl);
  }
  *(bf16x8*)(dX + m * 2 * F + f) = oa;
  *(bf16x8*)(dX + m * 2 * F + F + f) = ob;
}

// dpre = dropout(dy) (f > 0) over n = M * F elements, 8 per thread (n % 8 == 0).
__global__ __launch_bounds__(256) void relu_bwd_kernel(const __bf16* dy, const __bf16* fo, int64_t n, float p,
                                                       uint64_t seed, uint64_t site, __bf16* dx) {
  const int64_t i8 = ((int64_t)blockIdx.x * 256 + threadIdx.x) * 8;
  if (i8 >= n) return;
  const bf16x8 g = *(const bf16x8*)(dy + i8);
  const bf16x8 fv = *(const bf16x8*)(fo + i8);
  const bool drop = p > 0.0f;
  const uint32_t thr = drop_threshold(p);
  const float inv = 1.0f / (1.0f - p);
  bf16x8 o;
#pragma unroll
  for (int u = 0; u < 8; ++u) {
    const float d = t5b_keep_scale((float)g[u], drop, thr, inv, seed, site, (uint64_t)(i8 + u));
    o[u] = (__bf16)((float)fv[u] > 0.0f ? d : 0.0f);
  }
  *(bf16x8*)(dx + i8) = o;
}

// One block per token; fp32 atomics (the ids are spread over the vocabulary), as
// embedding_bwd_word_kernel without a padding row.
__global__ __launch_bounds__(256) void t5_embedding_bwd_kernel(const int64_t* ids, const __bf16* d, int H,
                                                               int64_t vocab, float* dshared) {
  const int64_t t = (int64_t)blockIdx.x;
  const int64_t id = ids[t];
  if (id < 0 || id >= vocab) return;   // an id outside the table has no row to add to
  for (int c = threadIdx.x; c < H; c += 256) atomicAdd(dshared + id * H + c, (float)d[t * H + c]);
}

}  // namespace drt

using namespace drt;

extern "C" {

size_t drt_rmsnorm_bwd_workspace(int64_t M, int32_t H) {
  if (M <= 0 || H <= 0) return 0;
  return (size_t)kRmsBwdBlocks * (size_t)H * sizeof(float) + drt_colsum_workspace(kRmsBwdBlocks, H);
}

int drt_rmsnorm_bwd_bf16(const void* dy, const void* x, const float* gamma, float eps, int64_t M, int32_t H,
                         const void* dres, void* dx, float* dgamma, void* ws, size_t ws_bytes, void* stream) {
  DRT_REQUIRE(M > 0 && H > 0 && H % 256 == 0 && H <= 1024);
  DRT_REQUIRE(dy && x && gamma && dx && dgamma && ws && ws_bytes >= drt_rmsnorm_bwd_workspace(M, H));
  hipStream_t s = (hipStream_t)stream;
  float* part = (float*)ws;
  int rc = dispatch_epl(H, [&](auto E) {
    hipLaunchKernelGGL(rmsnorm_bwd_kernel<decltype(E)::value>, dim3(kRmsBwdBlocks), dim3(256), 0, s, (const __bf16*)dy,
                       (const __bf16*)x, gamma, eps, M, (int)H, (const __bf16*)dres, (__bf16*)dx, part);
  });
  if (rc == DRT_OK) rc = hip_status(hipGetLastError());
  if (rc) return rc;
  // the blocks' partials in block order (drt_colsum_f32: fixed order, deterministic)
  return drt_colsum_f32(part, kRmsBwdBlocks, H, dgamma, part + (size_t)kRmsBwdBlocks * H,
                        drt_colsum_workspace(kRmsBwdBlocks, H), stream);
}

int drt_gated_gelu_new_bwd_bf16(const void* dy, const void* X, int64_t M, int64_t F, float drop_p, uint64_t seed,
                                uint64_t site, void* dX, void* stream) {
  DRT_REQUIRE(M >= 0 && F > 0 && F % 8 == 0 && drop_p >= 0.0f && drop_p < 1.0f);
  if (M == 0) return DRT_OK;
  DRT_REQUIRE(dy && X && dX);
  DRT_REQUIRE((uintptr_t)dy % 16 == 0 && (uintptr_t)X % 16 == 0 && (uintptr_t)dX % 16 == 0);
  const int64_t units = M * (F / 8);
  hipLaunchKernelGGL(gated_gelu_new_bwd_kernel, dim3((unsigned)((units + 255) / 256)), dim3(256), 0,
                     (hipStream_t)stream, (const __bf16*)dy, (const __bf16*)X, M, F, drop_p, seed, site, (__bf16*)dX);
  return hip_status(hipGetLastError());
}

int drt_relu_bwd_bf16(const void* dy, const void* f, int64_t n, float drop_p, uint64_t seed, uint64_t site, void* dx,
                      void* stream) {
  DRT_REQUIRE(n >= 0 && n % 8 == 0 && drop_p >= 0.0f && drop_p < 1.0f);
  if (n == 0) return DRT_OK;
  DRT_REQUIRE(dy && f && dx);
  DRT_REQUIRE((uintptr_t)dy % 16 == 0 && (uintptr_t)f % 16 == 0 && (uintptr_t)dx % 16 == 0);
  hipLaunchKernelGGL(relu_bwd_kernel, dim3((unsigned)((n + 2047) / 2048)), dim3(256), 0, (hipStream_t)stream,
                     (const __bf16*)dy, (const __bf16*)f, n, drop_p, seed, site, (__bf16*)dx);
  return hip_status(hipGetLastError());
}

int drt_t5_embedding_bwd(const int64_t* ids, const void* d, int64_t B, int64_t L, int32_t H, int64_t vocab,
                         float* dshared, void* stream) {
  DRT_REQUIRE(B >= 0 && L > 0 && H > 0 && vocab > 0);
  if (B == 0) return DRT_OK;
  DRT_REQUIRE(ids && d && dshared);
  hipLaunchKernelGGL(t5_embedding_bwd_kernel, dim3((unsigned)(B * L)), dim3(256), 0, (hipStream_t)stream, ids,
                     (const __bf16*)d, (int)H, vocab, dshared);
  return hip_status(hipGetLastError());
}

}  // extern "C"
