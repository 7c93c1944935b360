/*
 * nomic_api.h — C launch API of the Nomic-BERT encoder kernels (gfx950).
 * All tensors are device pointers, bf16 stored as uint16.  Row counts that
 * feed nomic_gemm must be padded to a multiple of 128 in the A buffer.
 */
#ifndef SPLINTER_NOMIC_API_H
#define SPLINTER_NOMIC_API_H
#include <stdint.h>
#include "arena_api.h"

#ifdef __cplusplus
extern "C" {
#endif

/* GEMM epilogues */
#define NOMIC_EPI_STORE    0   /* out = bf16(acc)                                   */
#define NOMIC_EPI_RESIDUAL 1   /* out = bf16(acc + res)                             */
#define NOMIC_EPI_SWIGLU   2   /* W rows interleaved [up16|gate16] (pack_upgate): out = up*silu(gate) */
#define NOMIC_EPI_ROPE     3   /* qkv projection, W rows per head [d0-15|d32-47|d16-31|d48-63]
                                  (pack_qkv); NEOX RoPE on cols < rope_cols; out in natural order */
#define NOMIC_EPI_F32      4   /* out = acc as fp32                                 */

/* Any other mode, RESIDUAL without res and ROPE without rope / pos are refused (non-zero), not launched. */
int nomic_gemm(int mode, const void *A, long lda, const void *W, long ldw, long M, int N, int K,
               void *out, long ldo, const void *res, long ldr, const float *rope, const int32_t *pos,
               int rope_cols, hipStream_t stream);
/* GEMM kernel selection: 0 = auto, 384 = 256x384 register-epilogue kernel (STORE / SWIGLU / ROPE,
 * N a multiple of 384, K a multiple of 32 and >= 64, 16-B aligned output rows), 256 = launch-per-tile
 * 256x256 phased kernel, 128 = 128x128 (where the shape allows; otherwise the next one that does).
 * Returns the previous setting. */
int nomic_gemm_set_variant(int variant);
/* K per LDS stage of the 256x384 kernel: 64 (default; env NOMIC_GEMM384_BK=32 turns it off) runs the
 * 64-wide loop, one barrier per two MFMA K-steps, where K is a multiple of 64; 32, and any other K,
 * run the 32-wide loop.  The output bits are the same.  Returns the previous setting. */
int nomic_gemm384_set_bk(int bk);
/* Tail split of the 256x256 kernel (default on; env NOMIC_GEMM_TAIL_SPLIT=0 turns it off): when the
 * last round of the grid would fill at most half the CUs (0 < tiles % CUs <= CUs / 2), its tiles
 * run as two 128-row half-tile workgroups each, in the same launch; the output bits do not change.
 * Returns the previous setting. */
int nomic_gemm_set_tail_split(int on);
/* workgroups the 256x256 kernel launches for an [M, N] output under the current setting: tiles,
 * plus one per split tile (0: N is no multiple of 256) */
long nomic_gemm256_grid(long M, int N);

/* x[t] = LN(tok[ids[t]] + type_row) ; bf16 out [T, 768] */
int nomic_embed_ln(const int32_t *ids, long T, const void *tok_emb, const void *type_row,
                   const void *gamma, const void *beta, float eps, void *out, hipStream_t stream);
/* in-place (or out-of-place) LayerNorm over 768 columns, bf16 */
int nomic_layernorm(const void *x, long T, const void *gamma, const void *beta, float eps, void *out,
                    hipStream_t stream);
/* attention kernel: 2 = swapped-product 128-row kernel (default), 1 = 64-row kernel */
int nomic_attention_set_variant(int variant);
/* varlen non-causal attention; qkv [T, 3*H*64] (q|k|v), out [T, H*64].
 * qblocks: [nqb] int32 pairs (seq index, q start offset in the sequence) of
 * 128-row query blocks (q starts are multiples of 128)                    */
int nomic_attention(const void *qkv, void *out, const int32_t *cu_seqlens, const int32_t *qblocks,
                    int nqb, int heads, float scale, hipStream_t stream);
/* mean over each sequence's tokens -> fp32 [B, 768]; if slots != NULL also
 * write each vector into arena slot slots[b] (>= 0) under the seqlock, after
 * checking the slot still holds hashes[b]; status[b] gets 0 / -11 / -2.     */
int nomic_mean_pool(const void *x, const int32_t *cu_seqlens, int B, float *pooled, int normalize,
                    spl_arena_t arena, const int64_t *slots, const uint64_t *hashes, int32_t *status,
                    hipStream_t stream);
/* GGUF tensor dequantisation to bf16 (ggml type ids) */
int nomic_dequant(int ggml_type, const void *src, long nelems, void *dst_bf16, hipStream_t stream);

#ifdef __cplusplus
}
#endif
#endif
