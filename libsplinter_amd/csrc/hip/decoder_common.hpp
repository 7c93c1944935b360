// decoder_common.hpp — helpers shared by decoder_kernels.hip (one generation) and decoder_batch.hip
// (up to 16 generations per step): wave reductions, the device state record, the
// sampler's workspace layout and draw, the split-L geometry of the decode attention and the host's
// shape dispatch.  The kernel bodies the two files share are in decoder_body_*.hpp.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>
#include <cmath>
#include <cstdlib>
#include <type_traits>

#include "bf16_util.hpp"

namespace {

// Device state of a generation (int32): [0] pos = tokens already in the KV cache, [1] token = the
// token the next step consumes (the last sampled one), [2] step = sampler draws so far.  The batched
// step (decoder_batch.hip) keeps one 8-word record per sequence slot: the same three words, then
// [3] active (0 / 1), [4] [5] the slot's sampler seed (low, high half), [6] [7] reserved (zero).
enum { ST_POS = 0, ST_TOK = 1, ST_STEP = 2, ST_ACTIVE = 3, ST_SEED_LO = 4, ST_SEED_HI = 5, ST_WORDS = 8 };

// what a sampler leaves in its record: the drawn token, pos += inc_pos, one more draw; the token also goes
// to host_tok (pinned, may be null)
__device__ __forceinline__ void state_commit(int32_t* st, int t, int inc_pos, int32_t* host_tok) {
  st[ST_TOK] = t;
  st[ST_POS] += inc_pos;
  st[ST_STEP] += 1;
  if (host_tok) __hip_atomic_store(host_tok, t, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
}

// Batched prompt prefill (dec_rope_kv_seg, dec_attn_prefill_kv_seg): up to 16 segments of the packed token
// matrix.  Segment i owns rows row0 .. row0 + n - 1, the tokens at absolute positions pos0 .. pos0 + n - 1
// of the prompt in cache slot `slot` (the slot's cache at + slot * seq_stride elements).  The launchers
// validate the host array and pass this table BY VALUE in the kernel arguments: no device table, no copy,
// and a kernel touches no row the validated table does not name.
constexpr int kMaxSegs = 16;
struct PrefillSegs {
  int nseg;
  int row0[kMaxSegs], n[kMaxSegs], pos0[kMaxSegs], slot[kMaxSegs];
  long seq_stride;
};
struct PrefillSeg {
  int row0, n, pos0, slot;
};

// segs: int32 [nseg][4] = {row0, n, pos0, slot}.  False: a segment is empty, leaves the T rows, the nslots
// slots or the n_ctx cache rows, two segments share token rows or a slot, or there are not 1..16 of them
inline bool prefill_segs_build(const int32_t* segs, int nseg, long T, int nslots, int n_ctx, long seq_stride,
                               PrefillSegs& tb) {
  if (!segs || nseg < 1 || nseg > kMaxSegs || T <= 0 || nslots <= 0 || n_ctx <= 0) return false;
  tb = PrefillSegs{};
  tb.nseg = nseg;
  tb.seq_stride = seq_stride;
  for (int i = 0; i < nseg; ++i) {
    const long row0 = segs[4 * i], n = segs[4 * i + 1], pos0 = segs[4 * i + 2], slot = segs[4 * i + 3];
    if (n < 1 || row0 < 0 || row0 + n > T || slot < 0 || slot >= nslots || pos0 < 0 || pos0 + n > n_ctx) return false;
    for (int j = 0; j < i; ++j)
      if (slot == tb.slot[j] || (row0 < (long)tb.row0[j] + tb.n[j] && tb.row0[j] < row0 + n)) return false;
    tb.row0[i] = (int)row0;
    tb.n[i] = (int)n;
    tb.pos0[i] = (int)pos0;
    tb.slot[i] = (int)slot;
  }
  return true;
}

// segment i of the table with i uniform over the workgroup: selects over the unrolled table, so the by-value
// argument is read with constant offsets and never copied to scratch
__device__ __forceinline__ PrefillSeg prefill_seg_at(const PrefillSegs& tb, int i) {
  PrefillSeg s{0, 0, 0, 0};
#pragma unroll
  for (int j = 0; j < kMaxSegs; ++j)
    if (j == i) s = PrefillSeg{tb.row0[j], tb.n[j], tb.pos0[j], tb.slot[j]};
  return s;
}

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}
__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
  return v;
}

// decode attention geometry: waves of the walking kernels, the single-workgroup key limit of the
// grouped kernel, and the flash-decoding split limits
constexpr int kDecWaves = 16;
constexpr int kSmallL = 512;
constexpr int kSplitWaves = 4;
constexpr int kMaxSplits = 32;

// splits for a cache of (up to) L keys: the single-workgroup kernel up to 512 keys, then one split per
// 256 keys, at most kMaxSplits (sweep over 4..32 splits at H 32 / KVH 8 / hd 128:
// profiles/r2_decode_splits.jsonl)
inline int decode_splits(int L) {
  static const int env = [] {
    const char* e = getenv("SPL_DEC_SPLITS");
    return e && *e ? atoi(e) : -1;
  }();
  if (env >= 1) return env < kMaxSplits ? env : kMaxSplits;
  if (L <= 512) return 1;
  const int sp = (L + 255) / 256;
  return sp > kMaxSplits ? kMaxSplits : sp;
}

// host dispatch: the runtime shape as compile-time constants: f(ic<D>) for d = head dim / 64 in 1..4, and
// f(ic<D>, ic<G>) with g = heads per workgroup in {1, 2, 4, 8}
template <int V>
using ic = std::integral_constant<int, V>;

template <class F>
void with_d(int d, F f) {
  switch (d) {
    case 1: f(ic<1>{}); break;
    case 2: f(ic<2>{}); break;
    case 3: f(ic<3>{}); break;
    default: f(ic<4>{}); break;
  }
}
template <class F>
void with_d_g(int d, int g, F f) {
  with_d(d, [&](auto D) {
    switch (g) {
      case 2: f(D, ic<2>{}); break;
      case 4: f(D, ic<4>{}); break;
      case 8: f(D, ic<8>{}); break;
      default: f(D, ic<1>{}); break;
    }
  });
}

// counter-based uniform in [0, 1): splitmix64 of (seed, draw index)
__device__ __forceinline__ double uniform01(uint64_t seed, uint64_t n) {
  uint64_t z = seed + (n + 1) * 0x9E3779B97F4A7C15ull;
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  z ^= z >> 31;
  return (double)(z >> 11) * (1.0 / 9007199254740992.0);
}

constexpr int kSampThreads = 1024;
constexpr int kSampRegs = 4;  // logits per thread: vocabularies up to 4096 tokens, longer ones run k_sb_*

__device__ float block_reduce(float v, float* sh, bool is_max) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  v = is_max ? wave_max(v) : wave_sum(v);
  __syncthreads();
  if (lane == 0) sh[wave] = v;
  __syncthreads();
  float r = sh[0];
  for (int w = 1; w < kSampThreads / 64; ++w) r = is_max ? fmaxf(r, sh[w]) : r + sh[w];
  return r;
}

// The multi-block sampler's workspace layout (floats, caller-owned so the chain can be graph-captured)
constexpr int kSbBlocks = 64, kSbThreads = 256, kSbBins = 1024;
enum {
  SB_BMAX = 0,                          // [64] block max
  SB_BIDX = SB_BMAX + kSbBlocks,        // [64] first index of the block max (as int bits)
  SB_BZ = SB_BIDX + kSbBlocks,          // [64] block mass sum exp(l - M)
  SB_BPART = SB_BZ + kSbBlocks,         // [64] block kept mass (tempered)
  SB_SCAL = SB_BPART + kSbBlocks,       // [8]  M, Z, lo, w, above, cut
  SB_HIST = SB_SCAL + 8,                // [64][1024] per-block histograms
  SB_FLOATS = SB_HIST + kSbBlocks * kSbBins
};

__device__ __forceinline__ float sb_logit(const float* logits, const uint8_t* mask, int i) {
  return (mask && !mask[i]) ? -INFINITY : logits[i];
}

template <int NT>
__device__ float sb_reduce(float v, bool is_max) {
  __shared__ float sh[NT / 64];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  v = is_max ? wave_max(v) : wave_sum(v);
  __syncthreads();
  if (lane == 0) sh[wave] = v;
  __syncthreads();
  float r = sh[0];
  for (int w = 1; w < NT / 64; ++w) r = is_max ? fmaxf(r, sh[w]) : r + sh[w];
  return r;
}

}  // namespace
