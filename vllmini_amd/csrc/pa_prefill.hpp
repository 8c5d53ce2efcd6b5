// pa_prefill.hpp — tiled causal attention of a CHUNK of query rows per sequence over the paged KV cache (prefill, chunked
// prefill, and — with one row — decode), on the matrix cores.  fp16 query / out, fp16 pages, block size 16, x = 8, head size
// 64 or 128.  Launcher and C-ABI entry: pa_prefill.hip.
//
// Operator: sequence s owns query rows cu_q_lens[s] .. cu_q_lens[s+1]-1 (q_len of them); row j sits at position
// p = seq_lens[s] - q_len + j and attends to cache positions 0..p of the blocks in block_tables[s].  All seq_lens[s] K / V
// rows are in the cache before the launch.
//
// Work split.  A wave owns a 16-row query tile of one (sequence, head); a workgroup is four waves = 64 consecutive rows.
// The four tiles start together and walk the same K / V blocks from block 0 upwards, two blocks per trip, each straight
// from global memory into MFMA operand registers — a block fetched by one wave is an L1 / L2 hit for the other three (no
// LDS, no barrier: the tiles' trip counts differ by at most two, and a wave past its diagonal simply leaves).  The COOP form
// (below) changes this for a group with ONE live tile only: its four waves share that tile's context and meet in LDS.
//
// Arithmetic per trip (a PAIR of 16-token blocks), everything transposed so that no operand ever changes lanes:
//   S^T = K . Q^T    v_mfma_f32_16x16x32_f16, A = the K block exactly as it lies in the page ([D/8][16][8] halves: lane
//                    l = 16*kg + token reads 16 bytes at 1 KiB * chunk + 16 * l — one contiguous KiB per instruction),
//                    B = Q^T held in registers for the whole kernel (lane: query row l & 15, dims 32*chunk + 8*kg ..+7).
//                    The C layout leaves lane (n = l & 15, kg = l >> 4) with tokens 4*kg .. 4*kg+3 of query column n.
//   online softmax   per query COLUMN: the column's values live in the four lanes {n, n+16, n+32, n+48}, so the block
//                    maximum is two cross-lane steps (xor 16, xor 32); running max / sum / rescale in fp32; `scale`
//                    (times log2 e) multiplies the fp32 scores; the causal mask SELECTS -inf.
//   O^T += V^T . P^T v_mfma_f32_16x16x32_f16 over the pair: k index 8*kg + j = token 4*kg + j of the first block (j < 4) or
//                    4*kg + j - 4 of the second — for B that is the lane's own eight probabilities (rounded to fp16, the
//                    sum is taken over the ROUNDED values), for A = V^T two 8-byte pieces of the V page [D][16] (row
//                    16*t + n, tokens 4*kg ..): sixteen rows = one contiguous 512 B per instruction.
//                    The accumulator's column is again query n: the column's rescale factor applies to the lane's own
//                    registers, and the final 1 / sum as well.
// V elements of tokens past the tile's last position (the tail of the last block, the absent second block of an odd pair)
// are cleared by a bit mask before they meet a zero probability: the bytes there may be NaN patterns.  Tokens between a
// row's position and the tile's last position are rows the caller wrote (positions < seq_len) and meet p = 0.
// Blocks wholly above the tile's diagonal are never loaded; block-table entries past them are never read.
#pragma once

#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

namespace vmi {
namespace prefill {

typedef _Float16 h16;
typedef _Float16 h16x4 __attribute__((ext_vector_type(4)));
typedef _Float16 h16x8 __attribute__((ext_vector_type(8)));
typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int BS = 16;          // tokens per block
constexpr int TILE = 16;        // query rows per wave
constexpr int WAVES = 4;        // tiles per workgroup
constexpr int ROWS = TILE * WAVES;

struct Params {
  h16* out;                     // [num_tokens, num_heads, D]
  const h16* q;                 // rows of stride q_stride
  const h16* kc;                // [blocks, kv_heads, D/8, 16, 8]
  const h16* vc;                // [blocks, kv_heads, D, 16]
  const int32_t* block_tables;  // [num_seqs, max_blocks_per_seq]
  const int32_t* seq_lens;      // [num_seqs]
  const int32_t* cu_q_lens;     // [num_seqs + 1]
  int64_t q_stride, kv_block_stride, kv_head_stride;
  int32_t num_tokens, num_heads, q_per_kv, num_seqs, max_blocks_per_seq;
  float scale_log2e;            // scale * log2(e): the softmax runs on exp2
  int32_t max_seq_len;          // host-known bound on seq_lens: a longer sequence writes nothing (INT32_MAX: no bound)
  // the partition form only (SPLIT, see below)
  float* ws;                    // partials: [parts][num_tokens][num_heads][D] fp32, then [parts][num_tokens][num_heads][2]
  int32_t part_tokens, num_parts, groups;   // tokens per context partition (a multiple of 32), partitions, the host's bound on 64-row groups
  // the head-packed form only (PACK, see below), where `groups` is the host's bound on R-row tiles
  int32_t g_shift;              // log2 G, G = q_per_kv in {2, 4, 8, 16}
  // the suffix launch behind the shared-prefix tiles only (PREFIX, see below); 0 in every other launch
  int32_t part0;                // the grid's first partition: its partition axis counts num_parts - part0 from here
};
// The REL kernels' argument (a type of its own: the other kernels' argument block stays what it is)
struct RelParams : Params {
  const float* alibi_slopes;    // [num_heads] fp32, or NULL
  int32_t window;               // W of the sliding window, 0: none
};
// The TREE kernels' argument (again a type of its own)
struct TreeParams : Params {
  const uint64_t* tree_mask;    // [num_tokens]: one word per packed query row — bit i: the row attends token i of its own chunk
};
constexpr int TREE_ROWS = 64;   // a chunk's rows under a tree mask: the bits of a word
// the longest chunk the kernels of argument type P serve (the TREE types: TREE_ROWS)
template <class P> inline constexpr int max_chunk_rows = 0x7fffffff;
template <> inline constexpr int max_chunk_rows<TreeParams> = TREE_ROWS;

// THE guard of every kernel of the operator (unsplit, partition form, merge): a sequence with nothing to do, or with
// lengths the tensors cannot hold or the host did not plan for, writes nothing.  -> false: leave.
template <class P>
__device__ __forceinline__ bool seq_span(const P& p, int seq, int& row_lo, int& q_len, int& L) {
  row_lo = p.cu_q_lens[seq];
  const int row_hi = p.cu_q_lens[seq + 1];
  q_len = row_hi - row_lo;
  L = p.seq_lens[seq];
  return !(q_len <= 0 || L <= 0 || L - q_len < 0 || row_lo < 0 || row_hi > p.num_tokens ||
           (L + BS - 1) / BS > p.max_blocks_per_seq || L > p.max_seq_len || q_len > max_chunk_rows<P>);
}

// The partition form's epilogue: lane (n, kg) stores its column's UNNORMALISED fp32 accumulator — dims 16t + 4kg .. + 3 of
// row `row`, in the natural dim order: four lanes fill 64 contiguous bytes per t — and lane kg == 0 the column's running
// maximum (log2 domain) and sum.  Layout: acc[part][row][head][D], then ml[part][row][head][2].
template <int D>
__device__ __forceinline__ void store_partial(float* ws, int num_tokens, int num_heads, int num_parts, int part, int row,
                                              int head, int kg, const f32x4 (&o)[D / 16], float m, float lsum) {
  const int64_t item = ((int64_t)part * num_tokens + row) * num_heads + head;
  float* ap = ws + item * D + 4 * kg;
#pragma unroll
  for (int t = 0; t < D / 16; ++t) *reinterpret_cast<f32x4*>(ap + 16 * t) = o[t];
  if (kg == 0) {
    typedef float f32x2 __attribute__((ext_vector_type(2)));
    *reinterpret_cast<f32x2*>(ws + (int64_t)num_parts * num_tokens * num_heads * D + item * 2) = f32x2{m, lsum};
  }
}

// The cooperative form's meeting point (COOP, below): the four waves of a workgroup hold partial triples (o, m, l) of ONE tile,
// each over its own pairs of the context, in the SAME lanes — lane (n, kg) of every wave owns dims 16t + 4kg .. + 3 of query
// column n, and m / l (after the cross-lane sum) are the column's in all four of its lanes.  So the merge needs no lane to
// read another's slot: waves 1 - 3 write theirs, one barrier, wave 0 reads them back at its own lane index.
// Layout, per writing wave: acc[t][lane] f32x4 — a ds_write_b128 / ds_read_b128 of 64 lanes covers 1 KiB contiguously, lane l
// the bytes 16 l .. 16 l + 15: consecutive lanes on consecutive 16-byte slots, the order in which a 128-bit LDS access is
// free of bank conflicts — then m[lane] and l[lane], consecutive dwords.  64 * (D / 4 + 2) * 4 bytes per wave: 13.5 KiB for
// the three at D 64, 25.5 KiB at D 128.  Static, and only in the COOP instantiations.
template <int D>
struct CoopLds {
  f32x4 acc[WAVES - 1][D / 16][64];
  float m[WAVES - 1][64], l[WAVES - 1][64];
};

// EVERY wave of the workgroup calls this (one __syncthreads inside).  -> true in wave 0, whose (o, m, lsum) are then the merged
// triple:  M = max_w m_w first, then  o = sum_w 2^(m_w - M) o_w,  l = sum_w 2^(m_w - M) l_w,  w ascending, fp32 — the
// arithmetic of pa_prefill_merge_kernel, fixed order, nothing atomic.  A wave that walked no pair brings m = -3e38, l = 0,
// o = 0: its weight is 2^(-huge) = 0 (or 2^0 on a column nobody saw, where every term is 0).
template <int D>
__device__ __forceinline__ bool coop_merge(CoopLds<D>& lds, int wave, int lane, f32x4 (&o)[D / 16], float& m, float& lsum) {
  if (wave > 0) {
#pragma unroll
    for (int t = 0; t < D / 16; ++t) lds.acc[wave - 1][t][lane] = o[t];
    lds.m[wave - 1][lane] = m;
    lds.l[wave - 1][lane] = lsum;
  }
  __syncthreads();
  if (wave > 0) return false;
  float mw[WAVES - 1], M = m;
#pragma unroll
  for (int w = 0; w < WAVES - 1; ++w) M = fmaxf(M, mw[w] = lds.m[w][lane]);
  float wgt = __builtin_amdgcn_exp2f(m - M);
#pragma unroll
  for (int t = 0; t < D / 16; ++t) o[t] *= wgt;
  lsum *= wgt;
#pragma unroll
  for (int w = 0; w < WAVES - 1; ++w) {
    wgt = __builtin_amdgcn_exp2f(mw[w] - M);
#pragma unroll
    for (int t = 0; t < D / 16; ++t) o[t] += lds.acc[w][t][lane] * wgt;
    lsum += lds.l[w][lane] * wgt;
  }
  m = M;
  return true;
}

// What lane (n, kg) knows about ITS query column before the walk, in every form and over both page formats; the forms differ in
// how blockIdx.x and n become one of these (chunk_column, prefix_column), not in the trip behind it.
struct Column {
  int part;          // my context partition (0 unless SPLIT)
  int head, kv_head; // the column's query head and the KV head whose pages the tile walks
  int table_row;     // the block_tables row the walk reads
  int q_row;         // the column's row of `query` (a dead column repeats a live one)
  int row0, live_rows;  // chunk forms: the tile's first row of `out` / the workspace (column n: + its row r within the tile), and
                     // how many of the tile's rows are stored — wave-uniform both, so nothing per lane waits through the walk
  int out_row;       // PREFIX: the column's row of `out` / the workspace ...
  int pos;           // the column attends to tokens 0 .. pos
  int last_pos;      // the tile's last visible position: bounds the walk, and V is cleared past it
  bool live;         // ... and whether it is stored
  bool coop;         // the workgroup's four waves share this tile (workgroup-uniform)
  bool select;       // PREFIX only — false: no column of the tile needs the causal select
};

// The column map of the chunk forms (plain, SPLIT, COOP, PACK: the kernels' comment below).  -> false: leave.  A return here is
// wave-uniform, and workgroup-uniform but for `j0 >= q_len`, which a cooperating workgroup never takes.
template <bool SPLIT, bool COOP, bool PACK, class P>
__device__ __forceinline__ bool chunk_column(const P& p, int wave, int n, Column& c) {
  const int nh = PACK ? p.num_heads >> p.g_shift : p.num_heads;   // x's innermost axis: query heads, or — packed — KV heads
  const int items = p.num_seqs * nh;
  const int slot = blockIdx.x / items;
  const int rem = blockIdx.x - slot * items;
  const int seq = rem / nh, hx = rem - seq * nh;
  const int pslot = SPLIT ? slot / p.groups : 0;
  c.part = pslot + (SPLIT ? p.part0 : 0);              // my context partition: tokens part * part_tokens .. + part_tokens - 1
  const int grev = SPLIT ? slot - pslot * p.groups : slot;
  int row_lo, q_len, L;
  if (!seq_span(p, seq, row_lo, q_len, L)) return false;
  const int ctx = L - q_len;    // cached positions in front of the chunk
  const int ngroups = PACK ? (q_len + (TILE >> p.g_shift) - 1) >> (4 - p.g_shift) : (q_len + ROWS - 1) / ROWS;   // packed: R-row tiles
  if (grev >= ngroups) return false;
  int j0 = PACK ? (ngroups - 1 - grev) << (4 - p.g_shift)
                : ((ngroups - 1 - grev) * WAVES + wave) * TILE;   // first row of my tile within the chunk
  c.coop = PACK;                                                  // (workgroup-uniform)
  if constexpr (COOP && !PACK) {
    c.coop = q_len - (ngroups - 1 - grev) * ROWS <= TILE;         // my group's live rows fit one tile: all four waves take it
    if (c.coop) j0 = (ngroups - 1 - grev) * ROWS;
  }
  if (!c.coop && j0 >= q_len) return false;                       // (wave-uniform; never taken by a cooperating workgroup)

  const int r = PACK ? n >> p.g_shift : n;               // my column's row within the tile, and its query head
  c.head = PACK ? (hx << p.g_shift) + (n & ((1 << p.g_shift) - 1)) : hx;
  c.kv_head = PACK ? hx : c.head / p.q_per_kv;
  c.table_row = seq;
  const int jr = min(j0 + r, q_len - 1);                 // rows past the chunk repeat its last row and are not stored
  c.q_row = row_lo + jr;
  c.row0 = row_lo + j0;
  c.live_rows = q_len - j0;
  c.pos = ctx + jr;                                      // my column's position: it attends to tokens 0..pos
  c.last_pos = ctx + min(j0 + (PACK ? TILE >> p.g_shift : TILE) - 1, q_len - 1);
  c.select = true;
  return true;
}

// The column map of the PREFIX form (the kernels' comment below): column n of tile blockIdx.x / num_heads is row t = 16 * tile + n
// of the PACKED query array, whatever sequence owns it.  The lane finds that sequence by binary search in cu_q_lens (the last s
// with cu_q_lens[s] <= t; every index it reads is inside the array, whatever the array holds), takes the guard's word on it,
// and gets pos = seq_lens[s] - q_len + (t - row_lo).  A column past num_tokens, of a sequence the guard rejects, or that the
// sequence found does not own is DEAD: it repeats row min(t, num_tokens - 1) of `query` at the tile's largest position and is
// not stored.  last_pos = min(largest live pos, P - 1), P = part_tokens; select = some live column ends inside the prefix.
// The four waves of the workgroup map the same sixteen columns, so the reductions over them — and the return on a tile
// with no live column — are workgroup-uniform.
template <class P>
__device__ __forceinline__ bool prefix_column(const P& p, int n, Column& c) {
  const int tile = blockIdx.x / p.num_heads;
  c.head = blockIdx.x - tile * p.num_heads;
  c.kv_head = c.head / p.q_per_kv;
  c.part = 0;
  c.table_row = 0;                                       // the prefix's blocks are read from row 0 of block_tables ONLY
  c.coop = true;
  c.out_row = tile * TILE + n;
  c.q_row = min(c.out_row, p.num_tokens - 1);
  int s = 0, hi = p.num_seqs - 1;
  while (s < hi) {
    const int mid = (s + hi + 1) >> 1;
    if (p.cu_q_lens[mid] <= c.q_row) s = mid; else hi = mid - 1;
  }
  int row_lo, q_len, L;
  c.live = seq_span(p, s, row_lo, q_len, L) && c.out_row >= row_lo && c.out_row < row_lo + q_len;
  c.pos = c.live ? L - q_len + (c.out_row - row_lo) : -1;
  int pos_hi = c.pos, pos_lo = c.live ? c.pos : 0x7fffffff;
#pragma unroll
  for (int d = 1; d < TILE; d <<= 1) {                   // over the sixteen columns (the four kg copies of a column agree)
    pos_hi = max(pos_hi, __shfl_xor(pos_hi, d));
    pos_lo = min(pos_lo, __shfl_xor(pos_lo, d));
  }
  pos_hi = __builtin_amdgcn_readfirstlane(pos_hi);
  pos_lo = __builtin_amdgcn_readfirstlane(pos_lo);
  if (pos_hi < 0) return false;
  if (!c.live) c.pos = pos_hi;
  c.last_pos = min(pos_hi, p.part_tokens - 1);
  c.select = pos_lo < p.part_tokens - 1;
  return true;
}

// What the REL form (the kernels' comment below) adds to a column's state, over both page formats.  Two terms, both functions of
// t - pos: the row at pos sees tokens wlo = max(0, pos - W + 1) .. pos, and token t scores slope * (t - pos) on top of scale * q . k.
// Per COLUMN: wlo, slope (log2 domain; packed tiles hold several heads).  Per TILE (wave-uniform): lo = the window start of its
// first row — nothing below it is loaded, V below it is cleared; hi_lo = the window start of its last row — pairs that begin
// at or above it hold no token below any column's window; first_pos — pairs that end at or below it hold none above any column's
// diagonal.  base = the pair-aligned window start of the SEQUENCE's first row: its partitions count from there.
struct Rel {
  int wlo, lo, hi_lo, first_pos, base;
  float slope;
  template <class P>
  __device__ __forceinline__ void init(const P& p, const Column& c) {
    const int win = p.window > 0 ? p.window : 0x7fffffff;   // (pos - win + 1 >= 2 - 2^31: no overflow)
    // the column map (chunk_column, which REL leaves as it is) holds both implicitly: a column is q_row - row0 rows past the
    // tile's first row, so pos - (q_row - row0) is the tile's first position in all 64 lanes; and the guard passed, so the
    // sequence's two lengths can be read again
    first_pos = __builtin_amdgcn_readfirstlane(c.pos - (c.q_row - c.row0));
    const int ctx = p.seq_lens[c.table_row] - (p.cu_q_lens[c.table_row + 1] - p.cu_q_lens[c.table_row]);
    wlo = max(0, c.pos - win + 1);
    lo = max(0, first_pos - win + 1);
    hi_lo = max(0, c.last_pos - win + 1);
    base = max(0, ctx - win + 1) & ~31;
    slope = p.alibi_slopes ? p.alibi_slopes[c.head] * 1.4426950408889634f : 0.f;
  }
  // The pairs [pp0, pp1) the tile walks (on entry: [0, npair)); -> false: leave.  SPLIT: partition `part` covers tokens
  // [base + part * PT, base + (part + 1) * PT) — the LAST one has no upper end: base is rounded down to a pair, so a sequence's
  // span can exceed the planned W + max_q_len - 1 tokens by up to 31.  Every form starts no lower than the pair of `lo`; a
  // partition wholly below it, or wholly above the tile, leaves.  All of it is wave-uniform, and workgroup-uniform when the
  // four waves share the tile.
  template <bool SPLIT, class P>
  __device__ __forceinline__ bool bounds(const P& p, int part, int last_pos, int npair, int& pp0, int& pp1) const {
    if constexpr (SPLIT) {
      const int start = base + part * p.part_tokens;
      if (last_pos < start) return false;
      pp0 = start >> 5;
      if (part < p.num_parts - 1) pp1 = min(npair, pp0 + (p.part_tokens >> 5));
    }
    pp0 = max(pp0, lo >> 5);
    return pp0 < pp1;
  }
  // SPLIT: does the column at `pos` own partition `part`, i.e. see one of its tokens?  Partitions of wlo .. of pos, by
  // arithmetic — the merge (pa_prefill_split.hpp) counts the same way.  (wlo >= base: pos >= ctx.)
  template <class P>
  __device__ __forceinline__ bool owns(const P& p, int part, int pos) const {
    const int top = p.num_parts - 1;
    return part >= min((wlo - base) / p.part_tokens, top) && part <= min((pos - base) / p.part_tokens, top);
  }
  // does pair pp hold a token outside some column's (window start, pos]?  (wave-uniform)
  __device__ __forceinline__ bool edge(int pp) const { return 32 * pp < hi_lo || 32 * pp + 31 > first_pos; }
  // the fp32 scores of tokens tok0 .. tok0 + 3 = pos + d0 .. : one FMA each on the exact distance; on an edge pair the
  // SELECTED -inf outside [wlo, pos] (a K row below the window may be NaN: nothing of it survives the select); -> their maximum
  __device__ __forceinline__ float scores(float (&s)[4], const f32x4& acc, float scale, float d0, int tok0, int pos, bool on_edge) const {
    float mx = -INFINITY;
    if (on_edge) {   // (wave-uniform)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const float x = __builtin_fmaf(slope, d0 + (float)r, acc[r] * scale);
        mx = fmaxf(mx, s[r] = (unsigned)(tok0 + r - wlo) <= (unsigned)(pos - wlo) ? x : -INFINITY);
      }
    } else {
#pragma unroll
      for (int r = 0; r < 4; ++r) mx = fmaxf(mx, s[r] = __builtin_fmaf(slope, d0 + (float)r, acc[r] * scale));
    }
    return mx;
  }
  // how many of the four tokens tok0 .. tok0 + 3 lie below the tile's window start
  __device__ __forceinline__ int below(int tok0) const { return min(max(lo - tok0, 0), 4); }
};

// What the TREE form (the kernels' comment below) adds to a column's state, over both page formats.  ctx = the cached tokens in
// front of the chunk — a tile's columns are rows of ONE sequence, so it is wave-uniform and sits in a scalar register; word =
// the row's 64 bits, bit i: chunk token ctx + i is attended — bits above the row's own index j = pos - ctx cleared, bit j set,
// once, here (the guard passed: q_len <= 64, j <= 63).  Columns of one row (PACK: its G heads) and dead columns (which repeat
// the chunk's last row) read the word at their q_row.
struct Tree {
  int ctx;
  uint64_t word;
  template <class P>
  __device__ __forceinline__ void init(const P& p, const Column& c) {
    ctx = __builtin_amdgcn_readfirstlane(p.seq_lens[c.table_row] - (p.cu_q_lens[c.table_row + 1] - p.cu_q_lens[c.table_row]));
    const int j = c.pos - ctx;
    word = (p.tree_mask[c.q_row] & ((2ull << j) - 1ull)) | (1ull << j);   // (j == 63: 2 << 63 wraps to 0, the mask is all ones)
  }
  // does pair pp hold a chunk token?  (wave-uniform; the at most three pairs that overlap [ctx, last_pos])
  __device__ __forceinline__ bool edge(int pp) const { return 32 * pp + 31 >= ctx; }
  // bit r: token tok0 + r is attended — it lies below ctx, or it is chunk token d + r, d = tok0 - ctx, and that bit of the
  // word is set.  d <= -4: all four are context; -4 < d < 0: the low -d are; d >= 64: past bit 63, none (bits past the row's own
  // are clear, so tokens above pos and past the tile's last position drop out with them).  No shift count leaves 0 .. 63.
  __device__ __forceinline__ uint32_t keep(int tok0) const {
    const int d = tok0 - ctx;
    const int up = min(max(-d, 0), 4);
    const uint64_t w = d >= 64 ? 0ull : d >= 0 ? word >> (d & 63) : (word << up) | ((1ull << up) - 1ull);
    return (uint32_t)w & 15u;
  }
  // the fp32 scores of tokens tok0 .. tok0 + 3: scaled; on an edge pair the SELECTED -inf where the bit is clear (a K row past
  // the tile's last position may be NaN: nothing of it survives the select); -> their maximum
  __device__ __forceinline__ float scores(float (&s)[4], const f32x4& acc, float scale, int tok0, bool on_edge) const {
    float mx = -INFINITY;
    if (on_edge) {   // (wave-uniform)
      const uint32_t k = keep(tok0);
#pragma unroll
      for (int r = 0; r < 4; ++r) mx = fmaxf(mx, s[r] = (k >> r & 1u) ? acc[r] * scale : -INFINITY);
    } else {
#pragma unroll
      for (int r = 0; r < 4; ++r) mx = fmaxf(mx, s[r] = acc[r] * scale);
    }
    return mx;
  }
};

// Grid: one workgroup per (64-row group, sequence, head), x = group_rev * (num_seqs * num_heads) + seq * num_heads + head.
// group_rev counts a sequence's groups from its LAST one, so the first num_seqs * num_heads workgroups of the launch are
// every sequence's longest causal range; a sequence with fewer groups than the host bound leaves the surplus at once.
//
// SPLIT (the partition form, for few rows over a deep context): the grid gains a partition axis, x = (part * groups +
// group_rev) * (num_seqs * num_heads) + seq * num_heads + head, and a tile walks only the pairs of its partition
// [part * part_tokens, min((part + 1) * part_tokens, last_pos + 1)) — the trip itself is the same code.  It does not
// normalise and writes nothing to `out`: store_partial(), merged by pa_prefill_merge_kernel (pa_prefill_split.hpp) in a
// second launch.  Partition is the OUTER index, ascending: every chain is at most part_tokens / 32 trips, the full ones are
// all alike, and the lower a partition the more tiles own all of it — so the launch starts with the workgroups that all
// work their full length, and those that leave at once (partitions past a sequence's end) come last.  Neighbours in x are
// the heads of one sequence in one partition: the query heads of a KV head read the same pages at the same time.
//
// COOP (the cooperative form, for a group of at most 16 live rows: a decode row, look-ahead rows, a chunk's tail, a 16-row
// chunk): waves 1 - 3 of such a workgroup have no tile of their own, so all four take the group's ONE tile — same j0, pos,
// last_pos and Q operand — and wave w walks the pairs pp0 + w, pp0 + w + 4, ... below pp1: interleaved, so that the four stay on
// neighbouring pages and share the work evenly whatever the length.  The trip is the same code; each wave's double buffer
// prefetches its OWN next pair, and the V clearing of pair npair - 1 happens in the wave that owns it.  They meet in
// coop_merge(); wave 0 stores (normalised to `out`, or store_partial in the SPLIT form — grid, Params, workspace and merge
// launch are the plain forms').  Whether a workgroup cooperates depends on (sequence, group) alone: it is workgroup-uniform,
// and so is every return in front of the barrier on that path (guard, surplus group, partition past the tile — the four
// waves share last_pos); the per-wave `j0 >= q_len` exit is not on it.  A group with more than 16 live rows runs exactly
// the plain code: step 1 from pp0, no LDS access, no barrier — bit-identical results.
//
// PACK (the head-packed form, for short chunks of grouped-query attention, G = q_per_kv in {2, 4, 8, 16}): the 16 columns of a
// tile are (row, query head of ONE KV head) pairs, head-minor — column n is row j0 + (n >> log2 G) of the chunk and query head
// kvh * G + (n & (G - 1)) — so a tile is R = 16 / G rows x the G heads that read the same pages: one walk of the context per KV
// head instead of one per query head, and full tiles from q_len * G = 16 on.  Softmax, causal selection (each column's own
// pos), rescale and 1 / sum are per column already; what changes is the column's (row, head) in the Q address, in jr / pos /
// last_pos, in the liveness test and in the two stores — columns of one row are adjacent heads, neighbours in `out` and in the
// workspace.  One tile per workgroup, ALWAYS cooperative (only instantiated with COOP): the four waves take the tile, walk
// interleaved pairs and meet in coop_merge; there is no per-wave exit, every return in front of the barrier is
// workgroup-uniform.  Grid: x = ((part * tiles + tile_rev) * num_seqs + seq) * num_kv_heads + kvh, tiles = ceil(max_q_len / R)
// from the host (Params::groups), tile_rev from the sequence's last tile; workspace and merge launch are the SPLIT form's.
// On a sequence with q_len <= R the tile is the cooperative form's (same last_pos, pairs per wave and merge; an MFMA column
// depends on its own operand column only): bit-identical results.
//
// PREFIX (the shared-prefix form — cascade attention — for a batch whose sequences all begin with the same P = part_tokens cached
// tokens in the same blocks; the kernel is pa_prefill_prefix_kernel<D>, below): the forms above walk those blocks once per (sequence,
// head).  Here the 16 columns of a tile are 16 CONSECUTIVE ROWS OF THE PACKED BATCH for one query head — a tile may span sequences
// (prefix_column) — and the tile walks ONE copy of the prefix, read through row 0 of block_tables: partition 0 of the SPLIT scheme
// with PT = P.  It writes that partition's partials; the chunk forms, launched with part0 = 1, write partitions 1 .. of every
// sequence's own suffix, and the untouched merge launch folds them — three launches, one stream.  One tile per workgroup, ALWAYS
// cooperative: wave w walks pairs w, w + 4, ... of the tile's npair <= P / 32, the four meet in coop_merge, wave 0 calls
// store_partial(part 0), unnormalised (fp8: without kv_scale — the merge applies it).  A wave with no pair keeps m = -3e38, l = 0,
// o = 0 and still reaches the barrier.  THE BARRIER RULE: there is one return in front of the barrier, a tile with no live column,
// and it is workgroup-uniform because the four waves compute the same column map; the loop holds no exit.  Masking: a column that
// ends inside the prefix (a sequence with fewer than P tokens in front of its chunk) gets -inf by selection past its pos; V is
// cleared past the tile's LARGEST pos on the last pair, as in the other forms; when the tile's smallest pos is >= P - 1 — the
// normal case — the select is skipped, wave-uniformly.  Grid: x = tile * num_heads + head, tiles = ceil(num_tokens / 16):
// neighbours in x are the heads of one tile, so the heads of a KV head read the same pages at the same time.  (Packing them
// into one tile, as PACK does, is the follow-up.)
//
// REL (ALiBi slopes and a sliding window — two terms in t - pos — on the plain, SPLIT, COOP and PACK forms; kernels
// pa_prefill_rel_kernel, argument RelParams; never with PREFIX): the row at pos sees tokens pos - W < t <= pos and token t scores
// scale * q . k + slope[head] * (t - pos).  The state is struct Rel, above.  WALK: a tile's first pair is the pair of lo, the
// window start of its first row, or its partition's first pair if that is higher; cooperating waves interleave from there.
// Block-table entries and K / V bytes of blocks wholly below lo are never read: the half of the first pair that lies below lo
// re-reads the other block, as the absent half of an odd last pair does, and its tokens are masked.  MASKS: only the first pairs of
// a walk can hold a token below some column's window (those that begin below hi_lo) and only the last ones a token above some
// column's pos (those that end above first_pos); Rel::edge() tells, wave-uniformly, and the pairs between run with no select at
// all.  On an edge pair one unsigned comparison SELECTS -inf outside [wlo, pos] per column.  V elements below lo are cleared on
// the raw bits in the tile's first pair — the last pair's clearing in reverse — so NaN bytes of a freed block never meet p = 0;
// tokens between lo and a column's wlo are rows of the live window of an earlier row: finite, and they meet p = 0.  ALIBI:
// fp32, log2 domain, on the relative distance — small where the weights are large: (float)(pair's first token - pos) once per
// trip, the lane's token offsets added exactly, one FMA per score onto the scaled q . k (fp8 pages: kv_scale is in that scale
// only).  SPLIT: partitions count from Rel::base, not from token 0 (Rel::bounds, Rel::owns); the host sizes their number from
// min(max_seq_len, W + max_q_len - 1).  THE BARRIER RULE holds as before: REL adds one return in front of the barrier — a
// partition wholly below the tile's window, in Rel::bounds — and it depends on (part, the tile's first and last position, W) alone,
// which the four waves of a cooperating workgroup share; the loop still holds no exit.  A stored column sees at least itself:
// its maximum contributes exp2(0), sum >= 1.
//
// TREE (a token tree as the chunk — the verification rows of a speculative decoder — on the plain, SPLIT, COOP and PACK forms; kernels
// pa_prefill_tree_kernel, argument TreeParams; never with PREFIX or REL): row j of a chunk attends every cached token t < ctx and
// chunk token ctx + i, i <= j, iff bit i of its 64-bit word is set; bit j counts as set, bits above j are ignored (nodes come in
// a topological order: ancestors first).  Chunks of at most 64 rows: the guard (seq_span) rejects a longer one, in the tile kernels
// and in the merge.  The state is struct Tree, above.  Since no row sees past its own position, last_pos, the walk bounds, the
// partitions a row owns (0 .. pos / PT), the grid, the workspace and the merge arithmetic are the causal forms'.  MASKS: a pair that
// ends below ctx holds context tokens only and runs with NO select (Tree::edge, wave-uniform — the causal kernels select on every
// trip); the at most three pairs that overlap [ctx, last_pos] SELECT -inf where the bit is clear, by one guarded shift per four
// tokens (Tree::keep).  The clearing of V past last_pos, the double buffer, both MFMAs and the merges are untouched: an
// unattended chunk token at or below last_pos is a row the caller wrote — finite — and meets p = 0.  EMPTY SHARES: a column may
// see NO token in a whole trip, wave share or partition (a node without ancestors over ctx = 0: the pairs below its own hold other
// branches only).  m starts at -3e38, not -inf, so a trip of all -inf keeps m (fmaxf), alpha = exp2(0) = 1, and every
// p = exp2(-inf - m) = 0: the triple stays (m = -3e38, l = 0, o = 0).  coop_merge and the merge kernel give it the weight
// exp2(-3e38 - M) = 0 against the share that holds the row itself (M finite, l >= 1) — or exp2(0) on terms that are all 0 — and
// never form -inf - (-inf).  A row's own partition and the unsplit tile always hold the row itself: sum >= 1.  THE BARRIER RULE is
// unchanged: TREE adds no return (the longer-chunk exit is the guard's, per sequence: workgroup-uniform).
template <int D, bool SPLIT, bool COOP, bool PACK, bool PREFIX, bool REL = false, bool TREE = false, class P = Params>
__device__ __forceinline__ void prefill_tile(const P& p) {
  static_assert(COOP || !PACK, "the head-packed form is cooperative by construction");
  static_assert(!PREFIX || (SPLIT && COOP && !PACK), "the shared-prefix form is a cooperative tile of partition 0, one query head");
  static_assert(!REL || !PREFIX, "ALiBi / sliding window over a shared prefix is not built");
  static_assert(!TREE || (!PREFIX && !REL), "a token tree with a shared prefix, ALiBi or a sliding window is not built");
  constexpr int KC = D / 32;    // 32-dim chunks of a K block: one MFMA each
  constexpr int VT = D / 16;    // 16-dim tiles of the output: one MFMA each
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

  const h16* qp = p.q + (int64_t)col.q_row * p.q_stride + (int64_t)head * D + 8 * kg;
  h16x8 qB[KC];
#pragma unroll
  for (int c = 0; c < KC; ++c) qB[c] = *reinterpret_cast<const h16x8*>(qp + 32 * c);

  const int64_t head_off = (int64_t)col.kv_head * p.kv_head_stride;
  const h16* kbase = p.kc + head_off + 8 * lane;
  const h16* vbase = p.vc + head_off + n * BS + 4 * kg;
  const int32_t* bt = p.block_tables + (int64_t)col.table_row * p.max_blocks_per_seq;

  // a pair's physical blocks; the absent second block of an odd count re-reads the first (its tokens are masked)
  // (REL: nor is a block wholly below the tile's window read — the first pair's lower half re-reads the upper)
  auto phys_of = [&](int pp, int i) -> int64_t {
    int b = min(2 * pp + i, nblk - 1);
    if constexpr (REL) b = max(b, blk_lo);
    return (int64_t)__builtin_amdgcn_readfirstlane(bt[b]) * p.kv_block_stride;
  };
  auto load_k = [&](h16x8(&k)[2][KC], int pp) {
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const h16* blk = kbase + phys_of(pp, i);
#pragma unroll
      for (int c = 0; c < KC; ++c) k[i][c] = *reinterpret_cast<const h16x8*>(blk + 512 * c);
    }
  };
  auto load_v = [&](u32x2(&v)[2][VT], int pp) {
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const h16* blk = vbase + phys_of(pp, i);
#pragma unroll
      for (int t = 0; t < VT; ++t) v[i][t] = *reinterpret_cast<const u32x2*>(blk + 16 * BS * t);
    }
  };

  f32x4 o[VT];
#pragma unroll
  for (int t = 0; t < VT; ++t) o[t] = f32x4{0.f, 0.f, 0.f, 0.f};
  float m = -3.0e38f, lsum = 0.f;     // running max (log2 domain) and this lane's share of the running sum

  h16x8 kcur[2][KC], knext[2][KC];
  u32x2 v[2][VT];
  // my trips: every pair of [pp0, pp1), or — cooperating — every fourth from pp0 + wave (none at all: the loop is skipped,
  // the load in front of it re-reads the tile's last block)
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

    // ---- S^T = K . Q^T, scaled in fp32, causal mask selected ----
    float s[2][4];
    float mx = -INFINITY;
    const bool on_edge = REL ? rel.edge(pp) : TREE && tree.edge(pp);                 // (wave-uniform)
    const float dist = REL ? (float)(2 * pp * BS + 4 * kg - pos) : 0.f;             // REL: my first token's distance to my row
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      f32x4 acc = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int c = 0; c < KC; ++c) acc = __builtin_amdgcn_mfma_f32_16x16x32_f16(kcur[i][c], qB[c], acc, 0, 0, 0);
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
    if (pp == npair - 1) {   // the only trip that can hold tokens past the tile's last position: clear them
#pragma unroll
      for (int i = 0; i < 2; ++i) {
        const int nv = last_pos + 1 - ((2 * pp + i) * BS + 4 * kg);   // valid tokens of my four
        const u32x2 keep = {nv >= 2 ? 0xffffffffu : nv == 1 ? 0xffffu : 0u, nv >= 4 ? 0xffffffffu : nv == 3 ? 0xffffu : 0u};
#pragma unroll
        for (int t = 0; t < VT; ++t) v[i][t] &= keep;
      }
    }
    if constexpr (REL) {
      if (pp == rel.lo >> 5) {   // the only trip that can hold tokens below the tile's window: clear them, from the low end
#pragma unroll
        for (int i = 0; i < 2; ++i) {
          const int nb = rel.below((2 * pp + i) * BS + 4 * kg);
          const u32x2 keep = {nb >= 2 ? 0u : nb == 1 ? 0xffff0000u : 0xffffffffu, nb >= 4 ? 0u : nb == 3 ? 0xffff0000u : 0xffffffffu};
#pragma unroll
          for (int t = 0; t < VT; ++t) v[i][t] &= keep;
        }
      }
    }
#pragma unroll
    for (int t = 0; t < VT; ++t) {
      const u32x4 va = {v[0][t][0], v[0][t][1], v[1][t][0], v[1][t][1]};
      o[t] = __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(h16x8, va), pB, o[t], 0, 0, 0);
    }
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int c = 0; c < KC; ++c) kcur[i][c] = knext[i][c];
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
    const float inv = 1.f / lsum;   // (a stored row attends at least one token — TREE: itself — and its maximum contributes exp2(0): lsum >= 1)
    h16* op = p.out + ((int64_t)out_row * p.num_heads + head) * D + 4 * kg;
#pragma unroll
    for (int t = 0; t < VT; ++t) {
      const h16x4 h = {(h16)(o[t][0] * inv), (h16)(o[t][1] * inv), (h16)(o[t][2] * inv), (h16)(o[t][3] * inv)};
      *reinterpret_cast<h16x4*>(op + 16 * t) = h;
    }
  }
}

template <int D, bool SPLIT = false, bool COOP = false, bool PACK = false>
__global__ void __launch_bounds__(WAVES * 64) pa_prefill_kernel(const Params p) {
  prefill_tile<D, SPLIT, COOP, PACK, false>(p);
}
template <int D>
__global__ void __launch_bounds__(WAVES * 64) pa_prefill_prefix_kernel(const Params p) {
  prefill_tile<D, true, true, false, true>(p);
}
template <int D, bool SPLIT = false, bool COOP = false, bool PACK = false>
__global__ void __launch_bounds__(WAVES * 64) pa_prefill_rel_kernel(const RelParams p) {
  prefill_tile<D, SPLIT, COOP, PACK, false, true>(p);
}
template <int D, bool SPLIT = false, bool COOP = false, bool PACK = false>
__global__ void __launch_bounds__(WAVES * 64) pa_prefill_tree_kernel(const TreeParams p) {
  prefill_tile<D, SPLIT, COOP, PACK, false, false, true>(p);
}

}  // namespace prefill
}  // namespace vmi
