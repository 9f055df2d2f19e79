// What the attention forward kernels share: attention_fwd_kernel (head_dim 64, attention_fwd.h) and
// attention_hd32_kernel (head_dim 32 as head pairs, attention_hd32.hip) stage 128 B of K and of V per
// key into the same LDS image and are launched over it the same way.
#pragma once
#include "drt_common.h"

namespace drt {

constexpr int kHeadDim = 64;
constexpr int kHd32 = 32;
constexpr int kMaxSeq = 512;
// Online softmax: the running max moves only when a tile's max exceeds it by more than kLazy (P <= 2^8
// in bf16 / fp32 is exact to the same relative precision), so the O rescale is a rare wave-uniform
// branch instead of 32 multiplies per tile.
constexpr float kLazy = 8.0f;

// The LDS image of a launch whose keys pad to Lp (a multiple of the 32-key tile): four regions, each
// starting where the one before it ends.  K as swizzled [key][8 x 16 B] rows (A operand of
// S^T = K Q^T), V transposed as Vt[d][key] with a padded row stride (A operand of O^T = V^T P^T), the
// key bias, and the 2 Lp staged relative biases of the RB kernels.
struct AttnLds {
  int vts;        // Vt row stride (bytes): conflict-free ds_read_b64
  int ks_bytes;   // Lp rows of 128 B
  int vt_bytes;   // 64 rows of vts B
  int kb_bytes;   // Lp floats
  int rb_bytes;   // RB: 2 Lp floats
  __host__ __device__ constexpr explicit AttnLds(int Lp_)
      : vts(Lp_ * 2 + 8), ks_bytes(Lp_ * 128), vt_bytes(64 * vts), kb_bytes(Lp_ * 4), rb_bytes(Lp_ * 8) {}
  __host__ __device__ static constexpr int padded(int len) { return (len + 31) & ~31; }
  __host__ __device__ static constexpr size_t bytes(int len, bool relbias) {
    const AttnLds p(padded(len));
    return (size_t)p.ks_bytes + p.vt_bytes + p.kb_bytes + (relbias ? p.rb_bytes : 0);
  }
};
static_assert(AttnLds::bytes(160, false) == 42112);   // the 42 KiB of the 64-wide kernel's register budget
static_assert(AttnLds::bytes(512, false) == 133632 && AttnLds::bytes(512, true) == 137728);
static_assert(AttnLds::bytes(224, false) == 58752 && AttnLds::bytes(224, false) <= kDefaultLdsBytes);
static_assert(AttnLds::bytes(225, false) == 67072 && AttnLds::bytes(225, false) > kDefaultLdsBytes);

// Device pieces take and return their vectors BY VALUE: with a `const f32x16&` parameter the element reads
// are memory accesses until the caller's loops are unrolled, and the kernels come out with other
// registers (pv_fragment by reference: 76 -> 88 VGPRs in the 32-wide kernel).  By value, every kernel
// keeps its bytes.
// O^T += V^T P^T, one k-step of 16 keys.  pv_fragment: the B operand, P of keys 16 ks .. of the tile as
// bf16.  vt_operand: the A operand in the key order of the S^T accumulator (keys 4 h + {0..3} and + 8 of
// the k-step): two ds_read_b64 of the V^T row at vrow (row d, the k-step's first key, + 8 h bytes).
__device__ __forceinline__ bf16x8 pv_fragment(f32x16 s, int ks) {
  bf16x8 pf;
#pragma unroll
  for (int j = 0; j < 8; ++j) pf[j] = (__bf16)s[8 * ks + j];
  return pf;
}

__device__ __forceinline__ bf16x8 vt_operand(const char* vrow) {
  const bf16x4 v0 = *(const bf16x4*)(vrow);
  const bf16x4 v1 = *(const bf16x4*)(vrow + 16);
  bf16x8 vf;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    vf[j] = v0[j];
    vf[4 + j] = v1[j];
  }
  return vf;
}

// Launch of an attention forward kernel over the LDS image of sequences of at most `len` tokens (L, or
// a varlen launch's max_len; `rb`: with the staged relative bias), one work-group of `threads` per group.
// An image above the default limit (len > 224) needs the kernel's opt-in first.
template <typename Args>
static int launch_attention_lds(const void* kernel, Args& a, int len, bool rb, int64_t groups, int threads,
                                void* stream) {
  const size_t lds = AttnLds::bytes(len, rb);
  if (lds > kDefaultLdsBytes) DRT_CHECK_HIP(allow_large_lds(kernel));
  void* args[] = {&a};
  (void)hipLaunchKernel(kernel, dim3((unsigned)groups), dim3(threads), args, lds, (hipStream_t)stream);
  return hip_status(hipGetLastError());
}

}  // namespace drt
