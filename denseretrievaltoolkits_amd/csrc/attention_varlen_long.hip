// Padding-free BERT training for sequences of 161 .. 512 tokens: the packed (VL) instantiations of
// the attention forward at NB = 0 and of the streamed backward pair, and their two C entries
// (contract: include/drt.h, "Padding-free BERT training").  This unit alone is compiled without the
// packed FP32 instructions (build_native.py): the kernels' fp32 pair operations become two scalar ones
// with the same roundings, so the results keep the bits of the padded kernels' arithmetic.
#include "attention_bwd_long.h"
#include "attention_fwd.h"
#include "drt_common.h"

using namespace drt;

extern "C" {

// The training forward over a packed batch up to 512 tokens (contract: drt.h): above 160 the VL = 2
// form of the NB = 0 kernel -- each wave loops over the query blocks of ITS sequence, the LDS image is
// sized by the launch's max_len, lse and keep words land in the packed layouts.  A launch whose max_len
// is a whole-sequence class goes to drt_attention_varlen_train_forward_bf16 (same arguments): its
// instantiations live in one unit only.  What drt_attention_varlen_long_backward_bf16 can differentiate.
int drt_attention_varlen_long_train_forward_bf16(const void* qkv, const int32_t* cu_seqlens, const int32_t* seq_ids,
                                                 int64_t n_seqs, int32_t max_len, int64_t L_pad, int64_t T, int32_t W,
                                                 void* ctx, float* lse, uint32_t* drop_bits, int32_t heads,
                                                 int32_t head_dim, float scale, float drop_p, uint64_t seed,
                                                 uint64_t site, void* stream) {
  if (max_len <= kAbMaxSeq)   // every check is that entry's own, at its tighter bound
    return drt_attention_varlen_train_forward_bf16(qkv, cu_seqlens, seq_ids, n_seqs, max_len, L_pad, T, W, ctx, lse,
                                                   drop_bits, heads, head_dim, scale, drop_p, seed, site, stream);
  AttnArgs a;
  bool launch;
  const int rc = varlen_train_fwd_args(a, &launch, kMaxSeq, qkv, cu_seqlens, seq_ids, n_seqs, max_len, L_pad, T, W, ctx,
                                       lse, drop_bits, heads, head_dim, scale, drop_p, seed, site);
  if (!launch) return rc;
  const bool drop = drop_p > 0.0f;
  using Kernel = void (*)(AttnArgs);
  static constexpr Kernel kernels[2] = {attention_fwd_kernel<0, false, false, 2>,   // [drop]; NB = 0
                                        attention_fwd_kernel<0, true, false, 2>};
  return launch_attention_fwd([&](int) { return kernels[drop]; }, a, max_len, false, n_seqs * heads, stream);
}

// The attention backward over the long sequences of a packed batch (contract: drt.h): the VL
// instantiations of the streamed pair over the caller's tile table.  dsum rows are per tile, so this
// launch and the short sequences' (drt_attention_varlen_backward_bf16) fill one matrix that the
// caller sums once.
int drt_attention_varlen_long_backward_bf16(const void* qkv, const void* ctx, const void* dctx, const float* lse,
                                            const int32_t* cu_seqlens, const int32_t* tiles, int64_t n_tiles,
                                            int32_t max_len, int64_t L_pad, int64_t T, int32_t W,
                                            const uint32_t* drop_bits, void* dqkv, float* dsum, int32_t heads,
                                            int32_t head_dim, float scale, float drop_p, uint64_t seed, uint64_t site,
                                            void* stream) {
  AttnBwdArgs a;
  bool launch;
  const int rc = varlen_train_bwd_args(a, &launch, kAblMaxSeq, true, qkv, ctx, dctx, lse, cu_seqlens, tiles, n_tiles,
                                       max_len, L_pad, T, W, drop_bits, dqkv, dsum, heads, head_dim, scale, drop_p, seed,
                                       site);
  if (!launch) return rc;
  const bool drop = drop_p > 0.0f;
  using Kernel = void (*)(AttnBwdArgs);
  // [dkdv, dq][drop]
  static constexpr Kernel vl[2][2] = {
      {attention_bwd_long_dkdv_kernel<false, false, true>, attention_bwd_long_dkdv_kernel<true, false, true>},
      {attention_bwd_long_dq_kernel<false, false, true>, attention_bwd_long_dq_kernel<true, false, true>}};
  return launch_attention_bwd_long([&](int k) { return vl[k][drop]; }, a, dim3((unsigned)(n_tiles * heads)),
                                   (hipStream_t)stream);
}

}  // extern "C"
