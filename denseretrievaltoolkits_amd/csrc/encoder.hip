// BERT bi-encoder forward kernels (DRModel.encode, DRT/model/biencoder.py:127-151,
// over HF BertModel: transformers/models/bert/modeling_bert.py embeddings :53-107,
// self-attention :139-204, sublayer outputs :282-352).
//
//   embed_ln        word + position + token-type embedding, LayerNorm (fp32 math)
//   layernorm       LayerNorm of an fp32 [M, H] row (GEMM epilogue already added
//                   bias + residual), bf16 out
//   attention       per (sequence, head): softmax(Q K^T / sqrt(dh) + key mask) V
//                   with v_mfma_f32_32x32x16_bf16, online softmax over 32-key
//                   tiles; S^T = K Q^T keeps each query's scores lane-local and
//                   the S^T accumulator feeds the P.V MFMA directly as its B
//                   operand (no LDS round trip for P); the RB instantiations add T5's
//                   relative-position bias to the scores (drt_attention_forward_bf16, relbias);
//                   the VL instantiations read each sequence's rows from a sequence-offset
//                   table (packed batches, drt_attention_varlen_forward_bf16; csrc/packed.hip), with
//                   lse and dropout for training (drt_attention_varlen_train_forward_bf16), or with
//                   the bias window of one span-S table (packed T5 towers,
//                   drt_attention_varlen_relbias_forward_bf16)
//   pool            first / masked-mean / masked-max pooling (utils.py:233-240)
//   l2norm          F.normalize(reps, dim=1) (biencoder.py:149-150)
#include "attention_fwd.h"
#include "drt_common.h"
#include "ln_row.h"

namespace drt {

template <int EPL>
__global__ __launch_bounds__(256) void embed_ln_kernel(const int64_t* ids, const int64_t* type_ids, int64_t T,
                                                       int64_t L, const float* wemb, const float* pemb,
                                                       const float* temb, const float* gamma, const float* beta,
                                                       float eps, int H, __bf16* out, __bf16* pre = nullptr) {
  const int lane = threadIdx.x & 63;
  const int64_t t = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (t >= T) return;
  const int64_t id = ids[t];
  const int64_t pos = t % L;
  const int64_t tt = type_ids ? type_ids[t] : 0;
  embed_ln_row<EPL>(id, tt, pos, t, wemb, pemb, temb, gamma, beta, eps, lane, H, out, pre);
}

// erf GELU, elementwise (the training forward keeps FFN1's pre-activation for the backward)
__global__ __launch_bounds__(256) void gelu_kernel(const __bf16* x, int64_t n, __bf16* y) {
  const int64_t i8 = ((int64_t)blockIdx.x * 256 + threadIdx.x) * 8;
  if (i8 >= n) return;
  if (i8 + 8 <= n) {   // 16-B pieces
    const bf16x8 xv = *(const bf16x8*)(x + i8);
    bf16x8 o;
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      const float v = (float)xv[u];
      o[u] = (__bf16)(0.5f * v * (1.0f + erff(v * 0.70710678118654752f)));
    }
    *(bf16x8*)(y + i8) = o;
  } else {
    for (int64_t i = i8; i < n; ++i) {
      const float v = (float)x[i];
      y[i] = (__bf16)(0.5f * v * (1.0f + erff(v * 0.70710678118654752f)));
    }
  }
}

// Embedding backward (BertEmbeddings, modeling_bert.py:68-108): the gradient of the pre-LN sum
// goes to the word / position / token-type tables (fp32, caller zeroes them).
// Word rows: one block per token, fp32 atomics (the row ids are spread over the vocabulary).
__global__ __launch_bounds__(256) void embedding_bwd_word_kernel(const int64_t* ids, const __bf16* d, int H,
                                                                 int64_t padding_idx, float* dword) {
  const int64_t t = (int64_t)blockIdx.x;
  const int64_t id = ids[t];
  if (id == padding_idx) return;   // nn.Embedding(padding_idx): the row stays 0
  for (int c = threadIdx.x; c < H; c += 256) atomicAdd(dword + id * H + c, (float)d[t * H + c]);
}

// Token-type rows with type ids (BERT: 2 rows, every token adds to one of them -- per-token atomics
// were T-way contended): a block sums one column slab over a chunk of kTypeChunk tokens per type
// in registers and adds once per (chunk, element).  Grid (column slabs, token chunks).
constexpr int kTypeChunk = 1024;
constexpr int kMaxTypes = 4;
__global__ __launch_bounds__(256) void embedding_bwd_type_kernel(const int64_t* type_ids, const __bf16* d, int64_t T,
                                                                 int H, int ntypes, float* dtype) {
  const int c = blockIdx.x * 256 + threadIdx.x;
  if (c >= H) return;
  const int64_t t0 = (int64_t)blockIdx.y * kTypeChunk;
  const int64_t t1 = t0 + kTypeChunk < T ? t0 + kTypeChunk : T;
  float s[kMaxTypes] = {0.f, 0.f, 0.f, 0.f};
  for (int64_t t = t0; t < t1; ++t) {
    const int64_t tt = type_ids[t];
    const float g = (float)d[t * H + c];
#pragma unroll
    for (int y = 0; y < kMaxTypes; ++y) s[y] += tt == y ? g : 0.0f;
  }
#pragma unroll
  for (int y = 0; y < kMaxTypes; ++y)
    if (y < ntypes && s[y] != 0.0f) atomicAdd(dtype + (int64_t)y * H + c, s[y]);
}

// Position rows: every sequence adds to rows 0..L-1, so per-element atomics from every token were
// B-way contended (and the single token-type row T-way: 2.1 ms per passage tower at B 1024, L 128).
// Here a block sums a chunk of kPosChunk sequences for one position and column slab in registers
// and adds once (B / kPosChunk atomics per element).
constexpr int kPosChunk = 64;
__global__ __launch_bounds__(256) void embedding_bwd_pos_kernel(const __bf16* d, int64_t B, int64_t L, int H,
                                                                float* dpos) {
  const int64_t p = blockIdx.x;
  const int c = blockIdx.y * 256 + threadIdx.x;
  if (c >= H) return;
  const int64_t b0 = (int64_t)blockIdx.z * kPosChunk;
  const int64_t b1 = b0 + kPosChunk < B ? b0 + kPosChunk : B;
  float s = 0.f;
  for (int64_t b = b0; b < b1; ++b) s += (float)d[(b * L + p) * H + c];
  atomicAdd(dpos + p * H + c, s);
}

// Token type 0 without type ids: every token adds to row 0, i.e. dtype[0] += sum of the rows
// dpos[0..L-1] this call produced (dpos arrives zeroed).
__global__ __launch_bounds__(256) void embedding_bwd_type0_kernel(const float* dpos, int64_t L, int H, float* dtype) {
  const int c = blockIdx.x * 256 + threadIdx.x;
  if (c >= H) return;
  float s = 0.f;
  for (int64_t p = 0; p < L; ++p) s += dpos[p * H + c];
  dtype[c] += s;
}

template <int EPL>
__global__ __launch_bounds__(256) void layernorm_f32_kernel(const float* X, int64_t M, int H, const float* gamma,
                                                            const float* beta, float eps, __bf16* out) {
  const int lane = threadIdx.x & 63;
  const int64_t t = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (t >= M) return;
  float x[EPL];
  row_load<EPL>(X + t * H, lane, x);
  ln_row<EPL>(x, gamma, beta, eps, lane, H, out + t * H);
}

// Same LayerNorm over bf16 pre-LN sums (the encoder's default: the GEMM epilogue
// adds bias + residual in fp32 and rounds once, halving the bytes of both sides).
// Round 6: one round of work-groups, each wave normalising rows t, t + waves, ... with gamma / beta
// held in registers (loaded once per wave instead of once per row: 2 x EPL / 4 16-B loads per row
// were twice the row's own loads through the vector memory pipe) and the next row's loads issued
// before the current row's reductions.  Same per-row arithmetic (ln_row_gb): bit-identical.
template <int EPL>
__global__ __launch_bounds__(256) void layernorm_bf16_kernel(const __bf16* X, int64_t M, int H, const float* gamma,
                                                             const float* beta, float eps, __bf16* out) {
  const int lane = threadIdx.x & 63;
  const int64_t t0 = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  const int64_t nw = (int64_t)gridDim.x * 4;
  if (t0 >= M) return;
  using RC = RowChunks<EPL>;
  float g[EPL], b[EPL];
  row_load<EPL>(gamma, lane, g);
  row_load<EPL>(beta, lane, b);
  bf16v<RC::W> cur[RC::N];
#pragma unroll
  for (int j = 0; j < RC::N; ++j) cur[j] = *(const bf16v<RC::W>*)(X + t0 * H + j * RC::STRIDE + lane * RC::W);
  for (int64_t t = t0; t < M; t += nw) {
    const int64_t tn = t + nw;
    bf16v<RC::W> nxt[RC::N];
    if (tn < M) {
#pragma unroll
      for (int j = 0; j < RC::N; ++j) nxt[j] = *(const bf16v<RC::W>*)(X + tn * H + j * RC::STRIDE + lane * RC::W);
    }
    float x[EPL];
#pragma unroll
    for (int j = 0; j < RC::N; ++j)
#pragma unroll
      for (int u = 0; u < RC::W; ++u) x[j * RC::W + u] = (float)cur[j][u];
    ln_row_gb<EPL>(x, g, b, eps, lane, H, out + t * H);
#pragma unroll
    for (int j = 0; j < RC::N; ++j) cur[j] = nxt[j];
  }
}

// ---------------------------------------------------------------------------
// Pooling (utils.py:233-240, biencoder.py:139-146) and L2 normalisation.
// mode 0 = first ([CLS]), 1 = mean over mask, 2 = max of hidden*mask.
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(256) void pool_kernel(const __bf16* hidden, const int64_t* mask, int64_t B, int64_t L,
                                                   int H, int mode, float* out, __bf16* out_bf16) {
  const int64_t b = blockIdx.x;
  for (int c = threadIdx.x; c < H; c += 256) {
    float v;
    if (mode == 0) {
      v = (float)hidden[(b * L) * H + c];
    } else if (mode == 1) {
      float s = 0.f, cnt = 0.f;
      for (int64_t l = 0; l < L; ++l) {
        const float mk = mask ? (float)mask[b * L + l] : 1.0f;
        s += (float)hidden[(b * L + l) * H + c] * mk;
        cnt += mk;
      }
      v = s / fmaxf(cnt, 1e-9f);
    } else {
      float mx = -__builtin_inff();
      for (int64_t l = 0; l < L; ++l) {
        const float mk = mask ? (float)mask[b * L + l] : 1.0f;
        mx = fmaxf(mx, (float)hidden[(b * L + l) * H + c] * mk);
      }
      v = mx;
    }
    out[b * H + c] = v;
    if (out_bf16) out_bf16[b * H + c] = (__bf16)v;
  }
}

__global__ __launch_bounds__(256) void l2norm_kernel(float* x, int64_t B, int H, __bf16* out_bf16) {
  __shared__ float red[4];
  const int64_t b = blockIdx.x;
  float s = 0.f;
  for (int c = threadIdx.x; c < H; c += 256) {
    const float v = x[b * H + c];
    s += v * v;
  }
  s = wave_sum(s);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
  __syncthreads();
  const float tot = red[0] + red[1] + red[2] + red[3];
  const float den = fmaxf(sqrtf(tot), 1e-12f);  // F.normalize eps
  for (int c = threadIdx.x; c < H; c += 256) {
    const float v = x[b * H + c] / den;
    x[b * H + c] = v;
    if (out_bf16) out_bf16[b * H + c] = (__bf16)v;
  }
}

}  // namespace drt

using namespace drt;

extern "C" {

int drt_gelu_bf16(const void* x, int64_t n, void* y, void* stream) {
  DRT_REQUIRE(n >= 0);
  if (n == 0) return DRT_OK;
  DRT_REQUIRE(x && y);
  DRT_REQUIRE((uintptr_t)x % 16 == 0 && (uintptr_t)y % 16 == 0);
  hipLaunchKernelGGL(gelu_kernel, dim3((unsigned)((n + 2047) / 2048)), dim3(256), 0, (hipStream_t)stream,
                     (const __bf16*)x, n, (__bf16*)y);
  return hip_status(hipGetLastError());
}

int drt_embedding_bwd(const int64_t* ids, const int64_t* type_ids, int32_t ntypes, const void* d, int64_t B, int64_t L,
                      int32_t H, int64_t padding_idx, float* dword, float* dpos, float* dtype, void* stream) {
  DRT_REQUIRE(B >= 0 && L > 0 && H > 0 && ntypes >= 1 && (type_ids == nullptr || ntypes <= kMaxTypes));
  if (B == 0) return DRT_OK;
  DRT_REQUIRE(ids && d && dword && dpos && dtype);
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(embedding_bwd_word_kernel, dim3((unsigned)(B * L)), dim3(256), 0, s, ids, (const __bf16*)d,
                     (int)H, padding_idx, dword);
  const unsigned cy = (unsigned)((H + 255) / 256), cz = (unsigned)((B + kPosChunk - 1) / kPosChunk);
  hipLaunchKernelGGL(embedding_bwd_pos_kernel, dim3((unsigned)L, cy, cz), dim3(256), 0, s, (const __bf16*)d, B, L,
                     (int)H, dpos);
  if (!type_ids) {
    hipLaunchKernelGGL(embedding_bwd_type0_kernel, dim3(cy), dim3(256), 0, s, (const float*)dpos, L, (int)H, dtype);
  } else {
    const int64_t T = B * L;
    hipLaunchKernelGGL(embedding_bwd_type_kernel, dim3(cy, (unsigned)((T + kTypeChunk - 1) / kTypeChunk)), dim3(256),
                       0, s, type_ids, (const __bf16*)d, T, (int)H, (int)ntypes, dtype);
  }
  return hip_status(hipGetLastError());
}

// drt_embed_ln (h384: H = 384 too, the inference entry) and drt_embed_ln_pre
static int embed_ln_entry(bool h384, const int64_t* ids, const int64_t* type_ids, int64_t B, int64_t L,
                          const float* word_emb, const float* pos_emb, const float* type_emb, const float* gamma,
                          const float* beta, float eps, int32_t H, void* out, void* pre, void* stream) {
  DRT_REQUIRE(B >= 0 && L > 0 && H > 0 && (H % 256 == 0 || (h384 && H == 384)) && H <= 1024);
  const int64_t T = B * L;
  if (T == 0) return DRT_OK;
  DRT_REQUIRE(ids && word_emb && pos_emb && type_emb && gamma && beta && out);
  hipStream_t s = (hipStream_t)stream;
  dim3 grid((unsigned)((T + 3) / 4));
  if (const int rc = dispatch_epl_or_384(H, [&](auto E) {
        hipLaunchKernelGGL(embed_ln_kernel<decltype(E)::value>, grid, dim3(256), 0, s, ids, type_ids, T, L, word_emb,
                           pos_emb, type_emb, gamma, beta, eps, (int)H, (__bf16*)out, (__bf16*)pre);
      }))
    return rc;
  return hip_status(hipGetLastError());
}

int drt_embed_ln_pre(const int64_t* ids, const int64_t* type_ids, int64_t B, int64_t L, const float* word_emb,
                     const float* pos_emb, const float* type_emb, const float* gamma, const float* beta, float eps,
                     int32_t H, void* out, void* pre, void* stream) {
  return embed_ln_entry(false, ids, type_ids, B, L, word_emb, pos_emb, type_emb, gamma, beta, eps, H, out, pre, stream);
}

int drt_embed_ln(const int64_t* ids, const int64_t* type_ids, int64_t B, int64_t L, const float* word_emb,
                 const float* pos_emb, const float* type_emb, const float* gamma, const float* beta, float eps,
                 int32_t H, void* out, void* stream) {
  return embed_ln_entry(true, ids, type_ids, B, L, word_emb, pos_emb, type_emb, gamma, beta, eps, H, out, nullptr,
                        stream);
}

int drt_layernorm_f32_bf16(const float* X, int64_t M, int32_t H, const float* gamma, const float* beta, float eps,
                           void* out, void* stream) {
  DRT_REQUIRE(M >= 0 && H > 0 && (H % 256 == 0 || H == 384) && H <= 1024);
  if (M == 0) return DRT_OK;
  DRT_REQUIRE(X && gamma && beta && out);
  hipStream_t s = (hipStream_t)stream;
  dim3 grid((unsigned)((M + 3) / 4));
  if (const int rc = dispatch_epl_or_384(H, [&](auto E) {
        hipLaunchKernelGGL(layernorm_f32_kernel<decltype(E)::value>, grid, dim3(256), 0, s, X, M, H, gamma, beta, eps,
                           (__bf16*)out);
      }))
    return rc;
  return hip_status(hipGetLastError());
}

int drt_layernorm_bf16(const void* X, int64_t M, int32_t H, const float* gamma, const float* beta, float eps,
                       void* out, void* stream) {
  DRT_REQUIRE(M >= 0 && H > 0 && (H % 256 == 0 || H == 384) && H <= 1024);
  if (M == 0) return DRT_OK;
  DRT_REQUIRE(X && gamma && beta && out);
  hipStream_t s = (hipStream_t)stream;
  dim3 grid(ln_rows_grid(M));
  if (const int rc = dispatch_epl_or_384(H, [&](auto E) {
        hipLaunchKernelGGL(layernorm_bf16_kernel<decltype(E)::value>, grid, dim3(256), 0, s, (const __bf16*)X, M, H,
                           gamma, beta, eps, (__bf16*)out);
      }))
    return rc;
  return hip_status(hipGetLastError());
}

// The attention forward (contract: drt.h): every instantiation of attention_fwd_kernel.  relbias
// (T5Attention, modeling_t5.py: scores = q k^T + position_bias, no 1 / sqrt(d) -- the caller
// passes scale = 1) selects the RB kernels, drop_p > 0 the DROP ones; lse and drop_bits are
// written when given.  At drop_p = 0 the training forward runs the inference kernels: the same
// ctx bits.
int drt_attention_forward_bf16(const void* qkv, const int64_t* mask, const float* relbias, void* ctx, float* lse,
                               uint32_t* drop_bits, int64_t B, int64_t L, int32_t heads, int32_t head_dim, float scale,
                               float drop_p, uint64_t seed, uint64_t site, void* stream) {
  DRT_REQUIRE(B >= 0 && L > 0 && L <= kMaxSeq && heads > 0 && head_dim == kHeadDim);
  DRT_REQUIRE(drop_p >= 0.0f && drop_p < 1.0f);
  if (B == 0) return DRT_OK;
  DRT_REQUIRE(qkv && ctx);
  AttnArgs a{(const __bf16*)qkv, mask, (__bf16*)ctx, B, L, heads, heads * head_dim, scale, lse, drop_p, seed, site,
             drop_bits, relbias};
  using Kernel = void (*)(AttnArgs);
#define DRT_AF_ROW(NB)                                                          \
  {{attention_fwd_kernel<NB, false, false>, attention_fwd_kernel<NB, false, true>}, \
   {attention_fwd_kernel<NB, true, false>, attention_fwd_kernel<NB, true, true>}}
  // [NB][drop][rb]; NB = 0: 161 <= L <= 512 (the backward's streamed kernels)
  static constexpr Kernel kernels[6][2][2] = {DRT_AF_ROW(0), DRT_AF_ROW(1), DRT_AF_ROW(2),
                                              DRT_AF_ROW(3), DRT_AF_ROW(4), DRT_AF_ROW(5)};
#undef DRT_AF_ROW
  const bool drop = drop_p > 0.0f, rb = relbias != nullptr;
  return launch_attention_fwd([&](int nb) { return kernels[nb][drop][rb]; }, a, (int)L, rb, B * heads, stream);
}

// The forward over a packed batch (contract: drt.h): the VL instantiations, one work-group per
// (listed sequence, head).  max_len picks the instantiation and sizes the LDS image, so a launch
// over one length class keeps that class's occupancy whatever the batch's longest sequence is.
int drt_attention_varlen_forward_bf16(const void* qkv, const int32_t* cu_seqlens, const int32_t* seq_ids,
                                      int64_t n_seqs, int32_t max_len, void* ctx, int32_t heads, int32_t head_dim,
                                      float scale, void* stream) {
  DRT_REQUIRE(n_seqs >= 0 && max_len > 0 && max_len <= kMaxSeq && heads > 0 && head_dim == kHeadDim);
  DRT_REQUIRE(n_seqs * heads < (1ll << 31));
  if (n_seqs == 0) return DRT_OK;
  DRT_REQUIRE(qkv && cu_seqlens && ctx);
  AttnArgs a{(const __bf16*)qkv, nullptr, (__bf16*)ctx, 0, 0, heads, heads * head_dim, scale, nullptr, 0.0f, 0, 0,
             nullptr, nullptr, cu_seqlens, seq_ids, max_len};
  using Kernel = void (*)(AttnArgs);
  static constexpr Kernel kernels[6] = {
      attention_fwd_kernel<0, false, false, 1>, attention_fwd_kernel<1, false, false, 1>,
      attention_fwd_kernel<2, false, false, 1>, attention_fwd_kernel<3, false, false, 1>,
      attention_fwd_kernel<4, false, false, 1>, attention_fwd_kernel<5, false, false, 1>};
  return launch_attention_fwd([&](int nb) { return kernels[nb]; }, a, max_len, false, n_seqs * heads, stream);
}

// The forward over a packed batch with T5's relative-position bias (contract: drt.h): the RB x VL
// instantiations.  relbias is the tower's one centred table of span bias_len; a work-group stages its
// sequence's window of it (attention_fwd.h), so the LDS image carries the rb region of max_len keys.
int drt_attention_varlen_relbias_forward_bf16(const void* qkv, const int32_t* cu_seqlens, const int32_t* seq_ids,
                                              int64_t n_seqs, int32_t max_len, const float* relbias, int32_t bias_len,
                                              void* ctx, int32_t heads, int32_t head_dim, float scale, void* stream) {
  DRT_REQUIRE(n_seqs >= 0 && max_len > 0 && max_len <= kMaxSeq && heads > 0 && head_dim == kHeadDim);
  DRT_REQUIRE(bias_len >= max_len && bias_len <= kMaxSeq);
  DRT_REQUIRE(n_seqs * heads < (1ll << 31));
  if (n_seqs == 0) return DRT_OK;
  DRT_REQUIRE(qkv && cu_seqlens && relbias && ctx);
  AttnArgs a{(const __bf16*)qkv, nullptr, (__bf16*)ctx, 0, 0, heads, heads * head_dim, scale, nullptr, 0.0f, 0, 0,
             nullptr, relbias, cu_seqlens, seq_ids, max_len, 0, 0, 0, bias_len};
  using Kernel = void (*)(AttnArgs);
  static constexpr Kernel kernels[6] = {
      attention_fwd_kernel<0, false, true, 1>, attention_fwd_kernel<1, false, true, 1>,
      attention_fwd_kernel<2, false, true, 1>, attention_fwd_kernel<3, false, true, 1>,
      attention_fwd_kernel<4, false, true, 1>, attention_fwd_kernel<5, false, true, 1>};
  return launch_attention_fwd([&](int nb) { return kernels[nb]; }, a, max_len, true, n_seqs * heads, stream);
}

// The training forward over a packed batch (contract: drt.h): VL x {plain, DROP} at the five
// whole-sequence classes -- what the varlen backward (encoder_bwd.hip) can differentiate.  At
// drop_p = 0 it is the inference entry's arithmetic with lse switched on (its own instantiation, so
// the inference kernels keep their registers).
int drt_attention_varlen_train_forward_bf16(const void* qkv, const int32_t* cu_seqlens, const int32_t* seq_ids,
                                            int64_t n_seqs, int32_t max_len, int64_t L_pad, int64_t T, int32_t W,
                                            void* ctx, float* lse, uint32_t* drop_bits, int32_t heads,
                                            int32_t head_dim, float scale, float drop_p, uint64_t seed, uint64_t site,
                                            void* stream) {
  AttnArgs a;
  bool launch;
  const int rc = varlen_train_fwd_args(a, &launch, kAbMaxSeq, qkv, cu_seqlens, seq_ids, n_seqs, max_len, L_pad, T, W,
                                       ctx, lse, drop_bits, heads, head_dim, scale, drop_p, seed, site);
  if (!launch) return rc;
  const bool drop = drop_p > 0.0f;
  using Kernel = void (*)(AttnArgs);
  static constexpr Kernel kernels[5][2] = {
      {attention_fwd_kernel<1, false, false, 2>, attention_fwd_kernel<1, true, false, 2>},
      {attention_fwd_kernel<2, false, false, 2>, attention_fwd_kernel<2, true, false, 2>},
      {attention_fwd_kernel<3, false, false, 2>, attention_fwd_kernel<3, true, false, 2>},
      {attention_fwd_kernel<4, false, false, 2>, attention_fwd_kernel<4, true, false, 2>},
      {attention_fwd_kernel<5, false, false, 2>, attention_fwd_kernel<5, true, false, 2>}};
  // max_len <= kAbMaxSeq: NB is 1 .. 5
  return launch_attention_fwd([&](int nb) { return kernels[nb - 1][drop]; }, a, max_len, false, n_seqs * heads, stream);
}

// The earlier names (drt.h, "Earlier attention names"): argument subsets of the entry above.
int drt_attention_bf16(const void* qkv, const int64_t* mask, void* ctx, int64_t B, int64_t L, int32_t heads,
                       int32_t head_dim, float scale, void* stream) {
  return drt_attention_forward_bf16(qkv, mask, nullptr, ctx, nullptr, nullptr, B, L, heads, head_dim, scale, 0.0f, 0, 0,
                                    stream);
}

int drt_attention_fwd_lse_bf16(const void* qkv, const int64_t* mask, void* ctx, float* lse, int64_t B, int64_t L,
                               int32_t heads, int32_t head_dim, float scale, void* stream) {
  return drt_attention_forward_bf16(qkv, mask, nullptr, ctx, lse, nullptr, B, L, heads, head_dim, scale, 0.0f, 0, 0,
                                    stream);
}

int drt_attention_train_fwd_bits_bf16(const void* qkv, const int64_t* mask, void* ctx, float* lse,
                                      uint32_t* drop_bits, int64_t B, int64_t L, int32_t heads, int32_t head_dim,
                                      float scale, float drop_p, uint64_t seed, uint64_t site, void* stream) {
  return drt_attention_forward_bf16(qkv, mask, nullptr, ctx, lse, drop_bits, B, L, heads, head_dim, scale, drop_p, seed,
                                    site, stream);
}

int drt_attention_relbias_bf16(const void* qkv, const int64_t* mask, const float* relbias, void* ctx, int64_t B,
                               int64_t L, int32_t heads, int32_t head_dim, float scale, void* stream) {
  DRT_REQUIRE(relbias || B == 0);
  return drt_attention_forward_bf16(qkv, mask, relbias, ctx, nullptr, nullptr, B, L, heads, head_dim, scale, 0.0f, 0, 0,
                                    stream);
}

int drt_attention_relbias_train_fwd_bits_bf16(const void* qkv, const int64_t* mask, const float* relbias, void* ctx,
                                              float* lse, uint32_t* drop_bits, int64_t B, int64_t L, int32_t heads,
                                              int32_t head_dim, float scale, float drop_p, uint64_t seed,
                                              uint64_t site, void* stream) {
  DRT_REQUIRE(relbias || B == 0);
  return drt_attention_forward_bf16(qkv, mask, relbias, ctx, lse, drop_bits, B, L, heads, head_dim, scale, drop_p, seed,
                                    site, stream);
}

int drt_pool_bf16(const void* hidden, const int64_t* mask, int64_t B, int64_t L, int32_t H, int32_t mode,
                  float* out, void* out_bf16, void* stream) {
  DRT_REQUIRE(B >= 0 && L > 0 && H > 0 && mode >= 0 && mode <= 2);
  if (B == 0) return DRT_OK;
  DRT_REQUIRE(hidden && out);
  hipLaunchKernelGGL(pool_kernel, dim3((unsigned)B), dim3(256), 0, (hipStream_t)stream, (const __bf16*)hidden, mask,
                     B, L, H, mode, out, (__bf16*)out_bf16);
  return hip_status(hipGetLastError());
}

int drt_l2_normalize_f32(float* x, int64_t B, int32_t H, void* out_bf16, void* stream) {
  DRT_REQUIRE(B >= 0 && H > 0);
  if (B == 0) return DRT_OK;
  DRT_REQUIRE(x);
  hipLaunchKernelGGL(l2norm_kernel, dim3((unsigned)B), dim3(256), 0, (hipStream_t)stream, x, B, H, (__bf16*)out_bf16);
  return hip_status(hipGetLastError());
}

}  // extern "C"
