// pa_prefill_fp8.hpp — the tiled causal prefill attention of pa_prefill.hpp over fp8-E4M3 pages (kv_cache_dtype "fp8" /
// "fp8_e4m3": the x = 16 layout reshape_and_cache_fp8_kernel writes, an element means fp8 * kv_scale).  fp16 query / out,
// block size 16, head size 64 or 128.  Launcher and C-ABI entry: pa_prefill.hip.
//
// Same operator, work split, grid order, per-column online softmax and selecting masks as pa_prefill_kernel (read its header
// first); what differs is how the one-byte pages become MFMA operands.  Every E4M3 value is a float16 value, so the bytes are
// decoded in registers (v_cvt_scalef32_pk_f16_fp8 with scale 1.0: two bytes per instruction, lossless) and the products run
// on the same v_mfma_f32_16x16x32_f16; q and the probabilities stay float16.
//
//   K operand        a K block is [D/16][16 tokens][16 dims] = D * 16 contiguous bytes.  Lane l loads 16 bytes at
//                    1 KiB * g + 16 * l (g < D/64): chunk 4g + (l >> 4), token l & 15, dims 64g + 16kg .. + 15 — one contiguous
//                    KiB per instruction, half as many K loads as the fp16 kernel.  The low 8 bytes are the A operand of MFMA
//                    (g, 0), the high 8 of MFMA (g, 1): the MFMA's k index 8kg + e stands for dim 64g + 16kg + 8j + e.  Only A
//                    and B must agree on it, and B = Q^T is loaded once: lane (n, kg) holds q[row n][64g + 16kg + 8j .. +7] for
//                    MFMA (g, j) — 16 contiguous halves per g.  The C layout is the fp16 kernel's: lane (n, kg) holds tokens
//                    4kg .. 4kg+3 of query column n.
//   V operand        O^T += V^T . P^T in the x32 form over a pair of blocks.  For d-tile t lane (n, kg) needs tokens 4kg .. 4kg+3
//                    of each block: ONE dword at row 16t + n, byte 4kg of the V page [D][16] — sixteen rows = 256 contiguous
//                    bytes per instruction — decoded by two conversions.  Bytes of tokens past the tile's last position are
//                    cleared on the RAW dwords (0x00 is +0) before decoding: the E4M3 NaN code 0x7F never becomes a half.
//   kv_scale         no instruction per element: K's factor rides in the score scale (scale * kv_scale * log2 e on the fp32
//                    scores, folded on the host), V's in the final kv_scale / sum.  kv_scale == 1 multiplies by 1.0f: exact.
//   pipelining       the fp16 kernel's register double buffer, on raw bytes: the next pair's K and this pair's V (D/8 dwords
//                    each) are in flight during the MFMAs; decoding happens at use.  No LDS, no barrier — but for the
//                    COOP form's one meeting of a short tile's four waves (coop_merge, pa_prefill.hpp).
#pragma once

#include "pa_prefill.hpp"

namespace vmi {
namespace prefill {

struct ParamsFp8 {
  h16* out;                     // [num_tokens, num_heads, D]
  const h16* q;                 // rows of stride q_stride
  const uint8_t* kc;            // [blocks, kv_heads, D/16, 16, 16] E4M3
  const uint8_t* vc;            // [blocks, kv_heads, D, 16] E4M3
  const int32_t* block_tables;  // [num_seqs, max_blocks_per_seq]
  const int32_t* seq_lens;      // [num_seqs]
  const int32_t* cu_q_lens;     // [num_seqs + 1]
  int64_t q_stride, kv_block_stride, kv_head_stride;   // the cache strides in bytes
  int32_t num_tokens, num_heads, q_per_kv, num_seqs, max_blocks_per_seq;
  float scale_log2e;            // scale * kv_scale * log2(e)
  float kv_scale;               // V's factor: applied with the final 1 / sum
  int32_t max_seq_len;          // as Params: the guard's bound, and the partition form's fields
  float* ws;
  int32_t part_tokens, num_parts, groups;
  int32_t g_shift;              // the head-packed form only: log2 q_per_kv
  int32_t part0;                // the suffix launch of the shared-prefix form only: the grid's first partition (else 0)
};
struct RelParamsFp8 : ParamsFp8 {   // the REL kernels' argument, as RelParams
  const float* alibi_slopes;    // [num_heads] fp32, or NULL; the term is NOT scaled by kv_scale
  int32_t window;               // W of the sliding window, 0: none
};
struct TreeParamsFp8 : ParamsFp8 {  // the TREE kernels' argument, as TreeParams
  const uint64_t* tree_mask;    // [num_tokens]
};
template <> inline constexpr int max_chunk_rows<TreeParamsFp8> = TREE_ROWS;

// four E4M3 bytes -> four halves (two dwords of half pairs), element order kept
__device__ __forceinline__ u32x2 e4m3x4_to_h16x4(uint32_t w) {
  return u32x2{__builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_f16_fp8((int)w, 1.0f, false)),
               __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_f16_fp8((int)w, 1.0f, true))};
}
// eight bytes -> one MFMA operand
__device__ __forceinline__ h16x8 e4m3x8_to_h16x8(uint32_t w0, uint32_t w1) {
  const u32x2 a = e4m3x4_to_h16x4(w0), b = e4m3x4_to_h16x4(w1);
  return __builtin_bit_cast(h16x8, u32x4{a[0], a[1], b[0], b[1]});
}

// Grid: as pa_prefill_kernel — x = group_rev * (num_seqs * num_heads) + seq * num_heads + head; SPLIT: its partition form
// (partition outer, store_partial() instead of the normalised store; V partials leave WITHOUT kv_scale: the merge applies it);
// COOP: its cooperative form (a group of at most 16 live rows is walked by all four waves, pairs interleaved, merged in LDS
// on the still unscaled triples; the barrier rule is written there); PACK: its head-packed form (column n = row j0 + (n >> log2 G),
// query head kvh * G + (n & (G - 1)); one always-cooperative tile per workgroup, x = ((part * tiles + tile_rev) * num_seqs + seq) *
// num_kv_heads + kvh) — a block is then fetched and DECODED once per KV head, not once per query head.  The permuted k index
// is a matter of dims alone: it stays as it is.  PREFIX: its shared-prefix form (pa_prefill_prefix_fp8_kernel<D>, below: column n =
// row 16 * tile + n of the packed batch, one walk of the prefix through row 0 of block_tables, partition 0's partials WITHOUT
// kv_scale; the barrier rule and the skipped select are written there) — a prefix block is then decoded once per tile of sixteen
// rows, not once per (sequence, head).  REL: its ALiBi / sliding-window form (pa_prefill_rel_fp8_kernel, argument RelParamsFp8:
// walk bounds, edge-pair selects, relative partitions and the barrier rule are written there and shared through struct Rel); the
// V bytes below the tile's window are cleared on the RAW dwords, before decoding, and the ALiBi term joins the score after
// kv_scale: scale * kv_scale multiplies q . k alone.  TREE: its token-tree form (pa_prefill_tree_fp8_kernel, argument
// TreeParamsFp8: the per-column word, the unselected context pairs, the guarded select on the chunk's pairs and the empty-share
// rule are written there and shared through struct Tree); nothing about the bytes changes.
template <int D, bool SPLIT, bool COOP, bool PACK, bool PREFIX, bool REL = false, bool TREE = false, class P = ParamsFp8>
__device__ __forceinline__ void prefill_tile_fp8(const P& p) {
  static_assert(COOP || !PACK, "the head-packed form is cooperative by construction");
  static_assert(!PREFIX || (SPLIT && COOP && !PACK), "the shared-prefix form is a cooperative tile of partition 0, one query head");
  static_assert(!REL || !PREFIX, "ALiBi / sliding window over a shared prefix is not built");
  static_assert(!TREE || (!PREFIX && !REL), "a token tree with a shared prefix, ALiBi or a sliding window is not built");
  constexpr int KG = D / 64;    // 64-dim groups of a K block: one 16-byte load, two MFMAs each
  constexpr int VT = D / 16;    // 16-dim tiles of the output: one dword per block, one MFMA each
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int n = lane & 15, kg = lane >> 4;
  Column col;
  if constexpr (PREFIX) {
    if (!prefix_column(p, n, col)) return;                 // (workgroup-uniform)
  } else {
    if (!chunk_column<SPLIT, COOP, PACK>(p, wave, n, col)) return;
  }
  const int part = col.part, head = col.head, pos = col.pos, last_pos = col.last_pos;
  const bool coop = col.coop;
  const int nblk = last_pos / BS + 1, npair = (nblk + 1) >> 1;
  // the trips I walk: all of them, or my partition's (it starts on a pair boundary; a tile that ends below it leaves)
  int pp0 = 0, pp1 = npair;
  Rel rel;
  if constexpr (REL) {
    rel.init(p, col);
    if (!rel.template bounds<SPLIT>(p, part, last_pos, npair, pp0, pp1)) return;   // (wave-uniform; workgroup-uniform when cooperating)
  } else if constexpr (SPLIT && !PREFIX) {
    if (last_pos < part * p.part_tokens) return;           // (wave-uniform; workgroup-uniform when cooperating)
    pp0 = part * (p.part_tokens >> 5);
    pp1 = min(npair, pp0 + (p.part_tokens >> 5));
  }
  const int blk_lo = REL ? rel.lo / BS : 0;                // REL: the first block the tile may read
  Tree tree;
  if constexpr (TREE) tree.init(p, col);

  // Q^T in the permuted k order of the K operand: for MFMA (g, j) dims 64g + 16kg + 8j .. +7
  const h16* qp = p.q + (int64_t)col.q_row * p.q_stride + (int64_t)head * D + 16 * kg;
  h16x8 qB[KG][2];
#pragma unroll
  for (int g = 0; g < KG; ++g)
#pragma unroll
    for (int j = 0; j < 2; ++j) qB[g][j] = *reinterpret_cast<const h16x8*>(qp + 64 * g + 8 * j);

  const int64_t head_off = (int64_t)col.kv_head * p.kv_head_stride;
  const uint8_t* kbase = p.kc + head_off + 16 * lane;
  const uint8_t* vbase = p.vc + head_off + n * BS + 4 * kg;
  const int32_t* bt = p.block_tables + (int64_t)col.table_row * p.max_blocks_per_seq;

  // a pair's physical blocks; the absent second block of an odd count re-reads the first (its tokens are masked)
  // (REL: nor is a block wholly below the tile's window read — the first pair's lower half re-reads the upper)
  auto phys_of = [&](int pp, int i) -> int64_t {
    int b = min(2 * pp + i, nblk - 1);
    if constexpr (REL) b = max(b, blk_lo);
    return (int64_t)__builtin_amdgcn_readfirstlane(bt[b]) * p.kv_block_stride;
  };
  auto load_k = [&](u32x4(&k)[2][KG], int pp) {
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const uint8_t* blk = kbase + phys_of(pp, i);
#pragma unroll
      for (int g = 0; g < KG; ++g) k[i][g] = *reinterpret_cast<const u32x4*>(blk + 1024 * g);
    }
  };
  auto load_v = [&](uint32_t(&v)[2][VT], int pp) {
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const uint8_t* blk = vbase + phys_of(pp, i);
#pragma unroll
      for (int t = 0; t < VT; ++t) v[i][t] = *reinterpret_cast<const uint32_t*>(blk + 16 * BS * t);
    }
  };

  f32x4 o[VT];
#pragma unroll
  for (int t = 0; t < VT; ++t) o[t] = f32x4{0.f, 0.f, 0.f, 0.f};
  float m = -3.0e38f, lsum = 0.f;     // running max (log2 domain) and this lane's share of the running sum

  u32x4 kcur[2][KG], knext[2][KG];
  uint32_t v[2][VT];
  // my trips: every pair of [pp0, pp1), or — cooperating — every fourth from pp0 + wave (none at all: the loop is skipped)
  int step = 1, first = pp0, last = pp1 - 1;
  if constexpr (COOP) {
    if (coop) {
      step = WAVES;
      first = pp0 + wave;
      last = first + (pp1 - 1 - first) / WAVES * WAVES;   // my last pair (unused when I have none)
    }
  }
  load_k(kcur, first);
  for (int pp = first; pp < pp1; pp += step) {
    load_v(v, pp);
    load_k(knext, min(pp + step, last));   // (my last trip re-reads its own pair: no branch around the loads)

    // ---- S^T = K . Q^T, scaled in fp32 (kv_scale included), causal mask selected ----
    float s[2][4];
    float mx = -INFINITY;
    const bool on_edge = REL ? rel.edge(pp) : TREE && tree.edge(pp);                 // (wave-uniform)
    const float dist = REL ? (float)(2 * pp * BS + 4 * kg - pos) : 0.f;             // REL: my first token's distance to my row
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      f32x4 acc = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int g = 0; g < KG; ++g) {
        acc = __builtin_amdgcn_mfma_f32_16x16x32_f16(e4m3x8_to_h16x8(kcur[i][g][0], kcur[i][g][1]), qB[g][0], acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_16x16x32_f16(e4m3x8_to_h16x8(kcur[i][g][2], kcur[i][g][3]), qB[g][1], acc, 0, 0, 0);
      }
      const int tok0 = (2 * pp + i) * BS + 4 * kg;
      if constexpr (REL) {
        mx = fmaxf(mx, rel.scores(s[i], acc, p.scale_log2e, dist + (float)(i * BS), tok0, pos, on_edge));
        continue;
      }
      if constexpr (TREE) {
        mx = fmaxf(mx, tree.scores(s[i], acc, p.scale_log2e, tok0, on_edge));
        continue;
      }
      if (PREFIX && !col.select) {   // (wave-uniform: every column of the tile sees the whole prefix)
#pragma unroll
        for (int r = 0; r < 4; ++r) mx = fmaxf(mx, s[i][r] = acc[r] * p.scale_log2e);
        continue;
      }
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        s[i][r] = (tok0 + r <= pos) ? acc[r] * p.scale_log2e : -INFINITY;
        mx = fmaxf(mx, s[i][r]);
      }
    }
    mx = fmaxf(mx, __shfl_xor(mx, 16));
    mx = fmaxf(mx, __shfl_xor(mx, 32));
    const float m_new = fmaxf(m, mx);
    const float alpha = __builtin_amdgcn_exp2f(m - m_new);
    m = m_new;
    h16x8 pB;
    float psum = 0.f;
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const h16 ph = (h16)__builtin_amdgcn_exp2f(s[i][r] - m_new);
        pB[4 * i + r] = ph;
        psum += (float)ph;
      }
    lsum = lsum * alpha + psum;
    if (__any(alpha != 1.f)) {
#pragma unroll
      for (int t = 0; t < VT; ++t) o[t] *= alpha;
    }

    // ---- O^T += V^T . P^T ----
    if (pp == npair - 1) {   // the only trip that can hold tokens past the tile's last position: clear their raw bytes
#pragma unroll
      for (int i = 0; i < 2; ++i) {
        const int nv = last_pos + 1 - ((2 * pp + i) * BS + 4 * kg);   // valid tokens of my four
        const uint32_t keep = nv >= 4 ? 0xffffffffu : nv <= 0 ? 0u : (1u << (8 * nv)) - 1u;
#pragma unroll
        for (int t = 0; t < VT; ++t) v[i][t] &= keep;
      }
    }
    if constexpr (REL) {
      if (pp == rel.lo >> 5) {   // the only trip that can hold tokens below the tile's window: clear their raw bytes, from the low end
#pragma unroll
        for (int i = 0; i < 2; ++i) {
          const int nb = rel.below((2 * pp + i) * BS + 4 * kg);
          const uint32_t keep = nb >= 4 ? 0u : 0xffffffffu << (8 * nb);
#pragma unroll
          for (int t = 0; t < VT; ++t) v[i][t] &= keep;
        }
      }
    }
#pragma unroll
    for (int t = 0; t < VT; ++t)
      o[t] = __builtin_amdgcn_mfma_f32_16x16x32_f16(e4m3x8_to_h16x8(v[0][t], v[1][t]), pB, o[t], 0, 0, 0);
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int g = 0; g < KG; ++g) kcur[i][g] = knext[i][g];
  }

  lsum += __shfl_xor(lsum, 16);
  lsum += __shfl_xor(lsum, 32);
  if constexpr (COOP) {
    if (coop) {   // all four waves are here: none left through a per-wave exit
      __shared__ CoopLds<D> lds;
      if (!coop_merge<D>(lds, wave, lane, o, m, lsum)) return;
    }
  }
  const int r = PACK ? n >> p.g_shift : n;               // my column's row within the tile
  const bool live = PREFIX ? col.live : r < col.live_rows;
  const int out_row = PREFIX ? col.out_row : col.row0 + r;
  if constexpr (SPLIT) {
    // unnormalised partials of the columns that see a token of this partition (the others hold sum 0 and are never merged)
    if constexpr (REL) {   // ... which here is a range of partitions with a lower end
      if (live && rel.owns(p, part, pos))
        store_partial<D>(p.ws, p.num_tokens, p.num_heads, p.num_parts, part, out_row, head, kg, o, m, lsum);
      return;
    }
    if (live && pos >= part * p.part_tokens)
      store_partial<D>(p.ws, p.num_tokens, p.num_heads, p.num_parts, part, out_row, head, kg, o, m, lsum);
    return;
  }
  if (live) {
    const float inv = p.kv_scale / lsum;   // (a stored row attends at least to token 0: lsum >= 1)
    h16* op = p.out + ((int64_t)out_row * p.num_heads + head) * D + 4 * kg;
#pragma unroll
    for (int t = 0; t < VT; ++t) {
      const h16x4 h = {(h16)(o[t][0] * inv), (h16)(o[t][1] * inv), (h16)(o[t][2] * inv), (h16)(o[t][3] * inv)};
      *reinterpret_cast<h16x4*>(op + 16 * t) = h;
    }
  }
}

template <int D, bool SPLIT = false, bool COOP = false, bool PACK = false>
__global__ void __launch_bounds__(WAVES * 64) pa_prefill_fp8_kernel(const ParamsFp8 p) {
  prefill_tile_fp8<D, SPLIT, COOP, PACK, false>(p);
}
template <int D>
__global__ void __launch_bounds__(WAVES * 64) pa_prefill_prefix_fp8_kernel(const ParamsFp8 p) {
  prefill_tile_fp8<D, true, true, false, true>(p);
}
template <int D, bool SPLIT = false, bool COOP = false, bool PACK = false>
__global__ void __launch_bounds__(WAVES * 64) pa_prefill_rel_fp8_kernel(const RelParamsFp8 p) {
  prefill_tile_fp8<D, SPLIT, COOP, PACK, false, true>(p);
}
template <int D, bool SPLIT = false, bool COOP = false, bool PACK = false>
__global__ void __launch_bounds__(WAVES * 64) pa_prefill_tree_fp8_kernel(const TreeParamsFp8 p) {
  prefill_tile_fp8<D, SPLIT, COOP, PACK, false, false, true>(p);
}

}  // namespace prefill
}  // namespace vmi
