// pa_cache_chunk.hpp — the cache write of a prefill CHUNK, split by (sequence, cache block, KV head) instead of by slot:
// float16 K / V rows into float16 pages (x = 8) or fp8-E4M3 pages (x = 16), block size 16, head size 64 / 128.
//
// The slot operator (reshape_and_cache) sees a flat list of slots: it cannot tell which rows are one block, and a prompt that
// starts at an odd packed row falls to its token-by-token path — 2-byte (fp16) or 1-byte (fp8) V stores at a 32- / 16-byte
// stride.  This operator takes what the prefill attention takes (block_tables, seq_lens, cu_q_lens): sequence s owns rows
// cu_q_lens[s] .. cu_q_lens[s+1]-1, row j sits at position pos = seq_lens[s] - q_len + j, i.e. offset pos % 16 of block
// block_tables[s][pos / 16].  The bytes are the slot operator's for slot = table[pos / 16] * 16 + pos % 16, bit for bit.
//
// Work split: ONE WAVE per item (sequence, block of the chunk's span, KV head); no LDS, no barrier, waves are independent.
//   item = ((s * nb) + b) * KV + h, four consecutive items per workgroup — neighbouring waves are the KV heads of one
//   (sequence, block): adjacent slices of the same 16 source rows, adjacent tiles [blk][h] of the pool.
//   The span of s is blocks (L - q_len) / 16 .. (L - 1) / 16; the host knows only bounds, so nb = (max_q_len + 30) / 16 (a
//   chunk of q rows that starts at offset 15 touches that many) and waves past a sequence's span leave at once.
// A whole block (all 16 offsets live):
//   K  needs no transposition: the 16-byte unit (chunk c, token t) of the tile is 8 consecutive dims of row t (fp16) or 16
//      dims quantised (fp8).  Lane l takes t = l & 15, c = (l >> 4) + 4 i: a store instruction covers 1 KiB of the tile
//      contiguously (fp8 x head size 64: the whole tile), a load instruction four 64-byte (fp8: 128-byte) row segments.
//   V  is the transposition, done by ADDRESSING: lane d loads element d of token t for t = 0 .. 15 — each of the 16 load
//      instructions is one contiguous 128-byte row segment — and owns tile row d: 32 contiguous bytes (fp16) or the 16
//      quantised bytes (fp8), so the wave's stores cover the tile contiguously.  Head size 128 takes two passes.
// A partial block (a chunk's first block when (L - q_len) % 16 != 0, its last when L % 16 != 0: at most two per sequence, on
// a wave-uniform branch): only offsets [a, e) are live.  K units are per token: predicated.  V rows hold other tokens' bytes
// that must survive: element-wise stores for the live tokens only.  Loads are predicated too — a row past the chunk belongs
// to another sequence or lies past num_tokens.
// Guards (leave or skip, never fault): the conditions of prefill::seq_span (q_len <= 0, L < q_len, rows outside
// [0, num_tokens], more blocks than the table holds) write nothing for s; a table entry < 0 or >= num_blocks skips that block.
#pragma once

#include <type_traits>

#include "pa_cache_fp8.hpp"

namespace vmi {
namespace chunkwrite {

constexpr int BS = 16;     // tokens per block
constexpr int WAVES = 4;   // items per workgroup
// Whole tiles go out with PLAIN stores: the attention launch behind this one reads exactly these lines, and they are whole
// lines — nothing partial is left dirty in L2 (measured against non-temporal: profiles/prefill_cache_write.md).  The
// element-wise V stores of partial blocks are non-temporal, like the slot kernels' (profiles/r02b_call_pair_aftermath.md).
constexpr bool NT_WHOLE = false;

struct Params {
  const h16* key;                  // [num_tokens, KV, D] float16, row strides key_stride / value_stride (halves)
  const h16* value;
  void* kc;                        // [num_blocks, KV, D / x, 16, x]
  void* vc;                        // [num_blocks, KV, D, 16]
  const int32_t* block_tables;     // [num_seqs, max_blocks_per_seq]
  const int32_t* seq_lens;         // [num_seqs]
  const int32_t* cu_q_lens;        // [num_seqs + 1]
  int64_t key_stride, value_stride;
  int64_t kv_block_stride, kv_head_stride;   // in cache elements (halves / bytes), applied to both caches
  int32_t num_tokens, num_kv_heads, num_seqs, max_blocks_per_seq, num_blocks;
  int32_t nb;                      // blocks per sequence the grid provides
  float kv_scale;
};

template <class T>
__device__ __forceinline__ void put_tile(T* dst, T v) {
  if constexpr (NT_WHOLE) __builtin_nontemporal_store(v, dst);
  else *dst = v;
}

// 16 float16 values -> their 16 E4M3 bytes, x[i] in byte i: reshape_and_cache_fp8_kernel's conversion (float(x) / kv_scale
// in fp32, skipped at kv_scale == 1; two values per v_cvt_pk_fp8_f32, each converted on its own)
template <bool S1>
__device__ __forceinline__ u32x4 quant16(const h16 (&x)[16], float kv_scale) {
  u32x4 q = {0u, 0u, 0u, 0u};
#pragma unroll
  for (int e = 0; e < 16; e += 2) {
    float f0 = (float)x[e], f1 = (float)x[e + 1];
    if constexpr (!S1) {
      f0 = f0 / kv_scale;
      f1 = f1 / kv_scale;
    }
    q[e >> 2] |= f32x2_to_fp8e4m3_satfinite_hw(f0, f1) << (8 * (e & 3));
  }
  return q;
}
__device__ __forceinline__ u32x4 quant16(const h16 (&x)[16], float kv_scale) {
  return kv_scale == 1.0f ? quant16<true>(x, kv_scale) : quant16<false>(x, kv_scale);
}

template <int D, bool FP8>
__global__ void __launch_bounds__(WAVES * 64) pa_cache_chunks_kernel(const Params p) {
  using CT = std::conditional_t<FP8, uint8_t, h16>;   // a cache element
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  // everything down to `whole` is wave-uniform: scalar loads and branches
  const int64_t item = (int64_t)blockIdx.x * WAVES + wave;
  const int h = (int)(item % p.num_kv_heads);
  const int64_t sb = item / p.num_kv_heads;
  const int b = (int)(sb % p.nb);
  const int64_t s = sb / p.nb;
  if (s >= p.num_seqs) return;
  const int row_lo = p.cu_q_lens[s], row_hi = p.cu_q_lens[s + 1];
  const int q_len = row_hi - row_lo;
  const int L = p.seq_lens[s];
  if (q_len <= 0 || L < q_len || row_lo < 0 || row_hi > p.num_tokens || (L - 1) / BS + 1 > p.max_blocks_per_seq) return;
  const int ctx = L - q_len;                       // cached positions in front of the chunk
  const int blk = ctx / BS + b;
  if (blk > (L - 1) / BS) return;                  // past the span
  const int phys = p.block_tables[s * p.max_blocks_per_seq + blk];
  if (phys < 0 || phys >= p.num_blocks) return;
  const int p0 = blk * BS;
  const int a = ctx > p0 ? ctx - p0 : 0;           // live offsets [a, e)
  const int e = L - p0 < BS ? L - p0 : BS;
  const int64_t row0 = (int64_t)row_lo + (p0 - ctx);   // the row at offset 0 (below row_lo where a > 0: never touched)
  const bool whole = a == 0 && e == BS;
  const int64_t tile = (int64_t)phys * p.kv_block_stride + (int64_t)h * p.kv_head_stride;
  CT* ktile = static_cast<CT*>(p.kc) + tile;
  CT* vtile = static_cast<CT*>(p.vc) + tile;

  // K: unit (chunk c, token t) = 16 bytes, at unit index c * 16 + t of the tile
  const int t = lane & 15;
  if (t >= a && t < e) {
    const h16* krow = p.key + (row0 + t) * p.key_stride + h * D;
    if constexpr (!FP8) {
#pragma unroll
      for (int i = 0; i < D / 32; ++i) {
        const int c = (lane >> 4) + 4 * i;
        const u32x4 v = *reinterpret_cast<const u32x4*>(krow + c * 8);
        put_tile(reinterpret_cast<u32x4*>(ktile + (c * BS + t) * 8), v);
      }
    } else {
#pragma unroll
      for (int i = 0; i < D / 64; ++i) {
        const int c = (lane >> 4) + 4 * i;
        const h16x8 lo = __builtin_bit_cast(h16x8, *reinterpret_cast<const u32x4*>(krow + c * 16));
        const h16x8 hi = __builtin_bit_cast(h16x8, *reinterpret_cast<const u32x4*>(krow + c * 16 + 8));
        h16 x[16];
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          x[j] = lo[j];
          x[8 + j] = hi[j];
        }
        put_tile(reinterpret_cast<u32x4*>(ktile + (c * BS + t) * 16), quant16(x, p.kv_scale));
      }
    }
  }

  // V: lane d owns tile row d = element d of the block's 16 tokens
  const h16* vsrc = p.value + h * D;
#pragma unroll
  for (int pass = 0; pass < D / 64; ++pass) {
    const int d = lane + 64 * pass;
    if (whole) {
      h16 x[16];
#pragma unroll
      for (int j = 0; j < BS; ++j) x[j] = vsrc[(row0 + j) * p.value_stride + d];
      if constexpr (FP8) {
        put_tile(reinterpret_cast<u32x4*>(vtile + d * BS), quant16(x, p.kv_scale));
      } else {
        h16x8 lo, hi;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          lo[j] = x[j];
          hi[j] = x[8 + j];
        }
        put_tile(reinterpret_cast<u32x4*>(vtile + d * BS), __builtin_bit_cast(u32x4, lo));
        put_tile(reinterpret_cast<u32x4*>(vtile + d * BS + 8), __builtin_bit_cast(u32x4, hi));
      }
    } else {
      for (int j = a; j < e; ++j) {                // live tokens only, one element each
        const h16 x = vsrc[(row0 + j) * p.value_stride + d];
        if constexpr (FP8) {
          float f = (float)x;
          if (p.kv_scale != 1.0f) f = f / p.kv_scale;
          __builtin_nontemporal_store((uint8_t)(f32x2_to_fp8e4m3_satfinite_hw(f, f) & 0xffu), vtile + d * BS + j);
        } else {
          __builtin_nontemporal_store(x, vtile + d * BS + j);
        }
      }
    }
  }
}

}  // namespace chunkwrite
}  // namespace vmi
