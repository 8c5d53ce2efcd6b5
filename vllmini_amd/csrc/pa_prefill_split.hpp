// pa_prefill_split.hpp — the second launch of the context-split tiled prefill: pa_prefill_merge_kernel folds the partition
// kernels' partials (pa_prefill_kernel<D, true> / pa_prefill_fp8_kernel<D, true>, pa_prefill.hpp: store_partial) into `out`.
// Launcher, plan and pick rule: pa_prefill.hip.
//
// Two launches on one stream and nothing else: no workgroup waits for another, no counter, no flag in the workspace.  Which
// partials exist is ARITHMETIC: the row at position pos has exactly the partitions 0 .. pos / part_tokens, each with at least
// one visible token (sum >= 1, maximum finite).  The merge reads those and no other word: a tile that straddles a partition
// boundary computes columns whose every score is masked (sum 0 — they are not even stored), and the caller's workspace holds
// anything elsewhere, NaN patterns included.
//
//   out = sum_p 2^(m_p - M) o_p / sum_p 2^(m_p - M) l_p,   M = max_p m_p,   p ascending, fp32, one rounding to fp16
//
// (times kv_scale for fp8 pages, in the same place as the unsplit kernel: out_scale / sum).  A row with one partition gets
// w = 2^0 and o * (out_scale / l): the unsplit kernel's own last two operations.  The order is fixed and nothing is atomic:
// run-to-run bit-identical.
//
// Work split: D / 4 lanes per (row, head), each owns four dims — one 16-byte load per partition, D * 4 contiguous bytes
// per (row, head, partition) across the lanes — and 1024 / D rows of one (sequence, head) per 256-thread workgroup.  The
// maxima are read first (8 bytes per partition, the same address across the D / 4 lanes), then the accumulators.
#pragma once

#include "pa_prefill.hpp"

namespace vmi {
namespace prefill {

struct MergeParams {
  h16* out;                     // [num_tokens, num_heads, D]
  const float* ws;              // acc[parts][num_tokens][num_heads][D], then ml[parts][num_tokens][num_heads][2]
  const int32_t* seq_lens;      // [num_seqs]
  const int32_t* cu_q_lens;     // [num_seqs + 1]
  int32_t num_tokens, num_heads, num_seqs, max_blocks_per_seq, max_seq_len;
  int32_t part_tokens, num_parts;
  float out_scale;              // 1, or kv_scale for fp8 pages
};
// The merge behind the TREE partition kernels (pa_prefill.hpp, TREE): the same fields and the same code — the type only gives the
// guard the TREE kernels' bound on a chunk (a sequence with more than 64 rows wrote no partial, and gets no row of `out`).  A
// partition of a row that holds none of its tokens carries (m = -3e38, l = 0, o = 0): weight exp2(-3e38 - M) = 0 below.
struct MergeTreeParams : MergeParams {};
template <> inline constexpr int max_chunk_rows<MergeTreeParams> = TREE_ROWS;

// Grid: x = chunk * (num_seqs * num_heads) + seq * num_heads + head; chunk = 1024 / D consecutive rows of the sequence.
template <int D, class P = MergeParams>
__global__ void __launch_bounds__(256) pa_prefill_merge_kernel(const P p) {
  constexpr int LPR = D / 4;          // lanes per (row, head)
  constexpr int RPB = 256 / LPR;      // rows per workgroup
  const int items = p.num_seqs * p.num_heads;
  const int chunk = blockIdx.x / items;
  const int rem = blockIdx.x - chunk * items;
  const int seq = rem / p.num_heads, head = rem - seq * p.num_heads;
  int row_lo, q_len, L;
  if (!seq_span(p, seq, row_lo, q_len, L)) return;
  const int j = chunk * RPB + (int)threadIdx.x / LPR;
  if (j >= q_len) return;
  const int c = (int)threadIdx.x % LPR;
  const int np = min((L - q_len + j) / p.part_tokens + 1, p.num_parts);   // (L <= max_seq_len: the min never bites)

  const int64_t item = (int64_t)(row_lo + j) * p.num_heads + head;
  const int64_t pstride = (int64_t)p.num_tokens * p.num_heads;          // items per partition
  const float* ml = p.ws + (int64_t)p.num_parts * pstride * D + item * 2;
  const float* acc = p.ws + item * D + 4 * c;

  float M = -INFINITY;
  for (int q = 0; q < np; ++q) M = fmaxf(M, ml[q * pstride * 2]);
  f32x4 o = f32x4{0.f, 0.f, 0.f, 0.f};
  float den = 0.f;
  for (int q = 0; q < np; ++q) {
    const float w = __builtin_amdgcn_exp2f(ml[q * pstride * 2] - M);
    o += *reinterpret_cast<const f32x4*>(acc + q * pstride * D) * w;
    den += ml[q * pstride * 2 + 1] * w;
  }
  const float inv = p.out_scale / den;   // (the partition holding M contributes l >= 1 at w = 1)
  const h16x4 h = {(h16)(o[0] * inv), (h16)(o[1] * inv), (h16)(o[2] * inv), (h16)(o[3] * inv)};
  *reinterpret_cast<h16x4*>(p.out + item * D + 4 * c) = h;
}

// The merge behind the REL partition kernels (pa_prefill.hpp, REL: ALiBi slopes / a sliding window) — a kernel of its own, so
// that the one above stays what it is.  Same grid, work split, arithmetic and order; what differs is WHICH partials a row has:
// partitions count from the sequence's base = (window start of its first row) & ~31, the last one is open-ended, and the row
// at pos has exactly those of max(0, pos - W + 1) .. of pos (Rel::owns stores by the same arithmetic).  No other word of the
// workspace is read.
struct MergeRelParams : MergeParams {
  int32_t window;               // W of the sliding window, 0: none
};

template <int D>
__global__ void __launch_bounds__(256) pa_prefill_merge_rel_kernel(const MergeRelParams p) {
  constexpr int LPR = D / 4, RPB = 256 / LPR;
  const int items = p.num_seqs * p.num_heads;
  const int chunk = blockIdx.x / items;
  const int rem = blockIdx.x - chunk * items;
  const int seq = rem / p.num_heads, head = rem - seq * p.num_heads;
  int row_lo, q_len, L;
  if (!seq_span(p, seq, row_lo, q_len, L)) return;
  const int j = chunk * RPB + (int)threadIdx.x / LPR;
  if (j >= q_len) return;
  const int c = (int)threadIdx.x % LPR;
  const int win = p.window > 0 ? p.window : 0x7fffffff, pos = L - q_len + j;
  const int base = max(0, L - q_len - win + 1) & ~31, top = p.num_parts - 1;
  const int q0 = min((max(0, pos - win + 1) - base) / p.part_tokens, top);
  const int np = min((pos - base) / p.part_tokens, top) + 1;

  const int64_t item = (int64_t)(row_lo + j) * p.num_heads + head;
  const int64_t pstride = (int64_t)p.num_tokens * p.num_heads;
  const float* ml = p.ws + (int64_t)p.num_parts * pstride * D + item * 2;
  const float* acc = p.ws + item * D + 4 * c;

  float M = -INFINITY;
  for (int q = q0; q < np; ++q) M = fmaxf(M, ml[q * pstride * 2]);
  f32x4 o = f32x4{0.f, 0.f, 0.f, 0.f};
  float den = 0.f;
  for (int q = q0; q < np; ++q) {
    const float w = __builtin_amdgcn_exp2f(ml[q * pstride * 2] - M);
    o += *reinterpret_cast<const f32x4*>(acc + q * pstride * D) * w;
    den += ml[q * pstride * 2 + 1] * w;
  }
  const float inv = p.out_scale / den;
  const h16x4 h = {(h16)(o[0] * inv), (h16)(o[1] * inv), (h16)(o[2] * inv), (h16)(o[3] * inv)};
  *reinterpret_cast<h16x4*>(p.out + item * D + 4 * c) = h;
}

}  // namespace prefill
}  // namespace vmi
