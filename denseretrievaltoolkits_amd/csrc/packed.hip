// Padding-free ("packed") inference and training: the kernels around the varlen attention of encoder.hip.
// A packed batch holds the T = sum of len_b real tokens of B sequences as one [T, H] matrix;
// cu_seqlens (int32 [B + 1], cu[0] = 0, cu[B] = T) says where each sequence starts.  The GEMMs and
// LayerNorm take any row count, so only the kernels that know about (sequence, position) differ:
//
//   embed_ln_packed   packed row t = token (b, t - cu[b]) of the padded ids [B, L]; the row itself is
//                     embed_ln_row (ln_row.h), the function embed_ln_kernel (encoder.hip) calls
//   pool_packed       first / mean / max over a sequence's len rows (max gives 0 when len < L: the
//                     reference's max(hidden * mask), utils.py:233-240, sees a zero at every pad)
//   unpack_rows       [T, H] -> [B * L, H] with zeros at the pad positions
//   pack_rows         [B * L, H] -> [T, H], the inverse (and the unpack's backward); rows past T of
//                     the output are zeroed (the training tower rounds its row count up to 32)
#include "drt_common.h"
#include "ln_row.h"

namespace drt {

// the sequence of packed row t: the largest b with cu[b] <= t (cu is non-decreasing; empty
// sequences share their start with the next one and are skipped)
__device__ inline int seq_of_row(const int32_t* cu, int B, int t) {
  int lo = 0, hi = B;   // invariant: cu[lo] <= t < cu[hi]
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (cu[mid] <= t) lo = mid;
    else hi = mid;
  }
  return lo;
}

template <int EPL>
__global__ __launch_bounds__(256) void embed_ln_packed_kernel(const int64_t* ids, const int64_t* type_ids,
                                                              const int32_t* cu, int B, int64_t L, int T,
                                                              const float* wemb, const float* pemb, const float* temb,
                                                              const float* gamma, const float* beta, float eps, int H,
                                                              __bf16* out, __bf16* pre = nullptr) {
  const int lane = threadIdx.x & 63;
  const int64_t t = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (t >= T) return;
  const int b = seq_of_row(cu, B, (int)t);
  int64_t pos = t - cu[b];
  pos = pos < L ? pos : L - 1;               // a table with len > L cannot read past the sequence's ids
  const int64_t src = (int64_t)b * L + pos;
  const int64_t id = ids[src];
  const int64_t tt = type_ids ? type_ids[src] : 0;
  embed_ln_row<EPL>(id, tt, pos, t, wemb, pemb, temb, gamma, beta, eps, lane, H, out, pre);
}

__global__ __launch_bounds__(256) void pool_packed_kernel(const __bf16* hidden, const int32_t* cu, int64_t L, int H,
                                                          int mode, float* out, __bf16* out_bf16) {
  const int64_t b = blockIdx.x;
  const int64_t r0 = cu[b];
  const int64_t len = cu[b + 1] - r0;
  for (int c = threadIdx.x; c < H; c += 256) {
    float v;
    if (len <= 0) {
      v = 0.0f;                               // no rows to read (plan_packing never makes one)
    } else if (mode == 0) {
      v = (float)hidden[r0 * H + c];
    } else if (mode == 1) {
      float s = 0.f;
      for (int64_t l = 0; l < len; ++l) s += (float)hidden[(r0 + l) * H + c];
      v = s / (float)len;
    } else {
      float mx = len < L ? 0.0f : -__builtin_inff();   // a pad position contributes hidden * 0
      for (int64_t l = 0; l < len; ++l) mx = fmaxf(mx, (float)hidden[(r0 + l) * H + c]);
      v = mx;
    }
    out[b * H + c] = v;
    if (out_bf16) out_bf16[b * H + c] = (__bf16)v;
  }
}

// one wave per padded row, 16-B pieces
__global__ __launch_bounds__(256) void unpack_rows_kernel(const __bf16* packed, const int32_t* cu, int64_t B, int64_t L,
                                                          int H, __bf16* out) {
  const int lane = threadIdx.x & 63;
  const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= B * L) return;
  const int64_t b = row / L, pos = row % L;
  const int64_t r0 = cu[b];
  const int64_t len = cu[b + 1] - r0;
  const bool real = pos < len;
  const __bf16* src = packed + (r0 + pos) * H;
  for (int c = lane * 8; c < H; c += 512) {
    u32x4 v = u32x4{0u, 0u, 0u, 0u};
    if (real) v = *(const u32x4*)(src + c);
    *(u32x4*)(out + row * H + c) = v;
  }
}

// one wave per packed row, 16-B pieces; rows cu[B] .. rows - 1 are zeroed
__global__ __launch_bounds__(256) void pack_rows_kernel(const __bf16* padded, const int32_t* cu, int B, int64_t L,
                                                        int H, int64_t rows, __bf16* out) {
  const int lane = threadIdx.x & 63;
  const int64_t t = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (t >= rows) return;
  const __bf16* src = nullptr;
  if (t < cu[B]) {
    const int b = seq_of_row(cu, B, (int)t);
    const int64_t pos = t - cu[b];
    if (pos < L) src = padded + ((int64_t)b * L + pos) * H;   // a table with len > L reads nothing
  }
  for (int c = lane * 8; c < H; c += 512) {
    u32x4 v = u32x4{0u, 0u, 0u, 0u};
    if (src) v = *(const u32x4*)(src + c);
    *(u32x4*)(out + t * H + c) = v;
  }
}

}  // namespace drt

using namespace drt;

extern "C" {

int drt_embed_ln_pre_packed(const int64_t* ids, const int64_t* type_ids, const int32_t* cu_seqlens, int64_t B,
                            int64_t L, int64_t T, const float* word_emb, const float* pos_emb, const float* type_emb,
                            const float* gamma, const float* beta, float eps, int32_t H, void* out, void* pre,
                            void* stream) {
  DRT_REQUIRE(B >= 0 && L > 0 && T >= 0 && H > 0 && H % 256 == 0 && H <= 1024);
  DRT_REQUIRE(B < (1ll << 31) && T < (1ll << 31) && T <= B * L);
  if (B == 0 || T == 0) return DRT_OK;
  DRT_REQUIRE(ids && cu_seqlens && word_emb && pos_emb && type_emb && gamma && beta && out);
  hipStream_t s = (hipStream_t)stream;
  dim3 grid((unsigned)((T + 3) / 4));
  if (const int rc = dispatch_epl(H, [&](auto E) {
        hipLaunchKernelGGL(embed_ln_packed_kernel<decltype(E)::value>, grid, dim3(256), 0, s, ids, type_ids, cu_seqlens,
                           (int)B, L, (int)T, word_emb, pos_emb, type_emb, gamma, beta, eps, (int)H, (__bf16*)out,
                           (__bf16*)pre);
      }))
    return rc;
  return hip_status(hipGetLastError());
}

int drt_embed_ln_packed(const int64_t* ids, const int64_t* type_ids, const int32_t* cu_seqlens, int64_t B, int64_t L,
                        int64_t T, const float* word_emb, const float* pos_emb, const float* type_emb,
                        const float* gamma, const float* beta, float eps, int32_t H, void* out, void* stream) {
  return drt_embed_ln_pre_packed(ids, type_ids, cu_seqlens, B, L, T, word_emb, pos_emb, type_emb, gamma, beta, eps, H,
                                 out, nullptr, stream);
}

int drt_pool_packed_bf16(const void* hidden, const int32_t* cu_seqlens, int64_t B, int64_t L, int32_t H, int32_t mode,
                         float* out, void* out_bf16, void* stream) {
  DRT_REQUIRE(B >= 0 && B < (1ll << 31) && L > 0 && H > 0 && mode >= 0 && mode <= 2);
  if (B == 0) return DRT_OK;
  DRT_REQUIRE(hidden && cu_seqlens && out);
  hipLaunchKernelGGL(pool_packed_kernel, dim3((unsigned)B), dim3(256), 0, (hipStream_t)stream, (const __bf16*)hidden,
                     cu_seqlens, L, (int)H, (int)mode, out, (__bf16*)out_bf16);
  return hip_status(hipGetLastError());
}

int drt_unpack_rows_bf16(const void* packed, const int32_t* cu_seqlens, int64_t B, int64_t L, int32_t H, void* out,
                         void* stream) {
  DRT_REQUIRE(B >= 0 && L > 0 && H > 0 && H % 8 == 0 && B * L < (1ll << 33));
  if (B == 0) return DRT_OK;
  DRT_REQUIRE(packed && cu_seqlens && out);
  DRT_REQUIRE((uintptr_t)packed % 16 == 0 && (uintptr_t)out % 16 == 0);
  hipLaunchKernelGGL(unpack_rows_kernel, dim3((unsigned)((B * L + 3) / 4)), dim3(256), 0, (hipStream_t)stream,
                     (const __bf16*)packed, cu_seqlens, B, L, (int)H, (__bf16*)out);
  return hip_status(hipGetLastError());
}

int drt_pack_rows_bf16(const void* padded, const int32_t* cu_seqlens, int64_t B, int64_t L, int32_t H, void* out,
                       int64_t out_rows, void* stream) {
  DRT_REQUIRE(B >= 0 && B < (1ll << 31) && L > 0 && H > 0 && H % 8 == 0 && out_rows >= 0 && out_rows < (1ll << 31));
  if (B == 0 || out_rows == 0) return DRT_OK;
  DRT_REQUIRE(padded && cu_seqlens && out);
  DRT_REQUIRE((uintptr_t)padded % 16 == 0 && (uintptr_t)out % 16 == 0);
  hipLaunchKernelGGL(pack_rows_kernel, dim3((unsigned)((out_rows + 3) / 4)), dim3(256), 0, (hipStream_t)stream,
                     (const __bf16*)padded, cu_seqlens, (int)B, L, (int)H, out_rows, (__bf16*)out);
  return hip_status(hipGetLastError());
}

}  // extern "C"
