// pa_prefill.hip — launcher and C-ABI entries of the tiled causal prefill attention (kernels: pa_prefill.hpp over fp16 pages,
// pa_prefill_fp8.hpp over fp8-E4M3 pages).
// One launch serves every sequence of the call: plain prefill (seq_len == q_len), a chunk over a cached context
// (seq_len > q_len) and single decode rows alike.  The lengths live on the device, so the grid is sized from the host's
// bounds (num_seqs, max_q_len, num_heads) and surplus workgroups leave at once.
#include "pa_prefill.hpp"
#include "pa_prefill_fp8.hpp"
#include "pa_prefill_split.hpp"
#include "pa_cache_chunk.hpp"   // the chunk form of the cache write: its launcher and entries are at the end of this file

#include <limits.h>

#include <type_traits>

#include "pa_host.hpp"
#include "vmi_paged_attention.h"

namespace vmi {

// When the launch is split over the context, and how finely (partition_tokens == 0 in the plan).  Every number is read off
// the tables of profiles/prefill_split.md section 1 (MI355X, 256 CUs); section 2 there walks through them.
struct SplitRules {
  int underfill_wgs_per_cu;   // split only when the unsplit grid has FEWER workgroups than this per CU: at 2 per CU (512) the
                              // split no longer wins consistently, below it wins in every cell measured
  int min_context;            // ... and max_seq_len is at least this: the shallowest context measured (nothing below it was)
  int target_wgs_per_cu;      // partitions = what brings the grid to this many workgroups per CU ...
  int max_partitions;         // ... but no more than this: past 32 the merge's reads outweigh the shorter chains
  int floor_tokens;           // a partition is never shorter than this: 256 loses to 512 everywhere but the smallest cell
  int ceil_tokens;            // ... nor longer: 2 048 is the best or within 8 % of the best forced size in every deep cell
};
static constexpr SplitRules kSplitRules = {2, 4096, 3, 32, 512, 2048};

// The head-packed form's ratio G = num_heads / num_kv_heads: -> log2 G for G in {2, 4, 8, 16}, -1 otherwise
static int pack_shift(int32_t num_heads, int32_t num_kv_heads) {
  if (num_kv_heads <= 0 || num_heads <= 0 || num_heads % num_kv_heads != 0) return -1;
  const int g = num_heads / num_kv_heads;
  return g == 2 ? 1 : g == 4 ? 2 : g == 8 ? 3 : g == 16 ? 4 : -1;
}
static int fail_pack_ratio(int32_t num_heads, int32_t num_kv_heads) {
  if (num_kv_heads > 0 && num_heads > 0 && num_heads % num_kv_heads == 0)
    return fail(VMI_E_KV_HEADS, "paged_attention_prefill: the head-packed form is built for num_heads / num_kv_heads in "
                "{2, 4, 8, 16}, got ratio %d (num_heads=%d num_kv_heads=%d)", num_heads / num_kv_heads, num_heads, num_kv_heads);
  return fail(VMI_E_KV_HEADS, "paged_attention_prefill: num_heads=%d not divisible by num_kv_heads=%d", num_heads, num_kv_heads);
}

// -> VMI_OK and (partition_tokens, num_partitions, workspace_bytes); num_partitions == 1: do not split, 0 bytes.
// g_shift >= 0: the head-packed grid — ceil(max_q_len / R) tiles of R = 16 >> g_shift rows per (sequence, KV head).
// window > 0 (the REL entries): no row sees more than `window` tokens, a sequence's rows together at most window + max_q_len - 1
// — the rule, the partitions and the workspace are sized on that depth where it is less than max_seq_len (the partitions then
// count from each sequence's own window start: pa_prefill.hpp, Rel).
static int split_plan(int32_t num_tokens, int32_t num_heads, int32_t head_size, int32_t num_seqs, int32_t max_q_len,
                      int32_t max_seq_len_in, int32_t num_cus, int32_t partition_tokens_in, int32_t* partition_tokens,
                      int32_t* num_partitions, int64_t* workspace_bytes, int g_shift = -1, int32_t window = 0) {
  int64_t max_seq_len = max_seq_len_in;
  if (window > 0 && (int64_t)window + max_q_len - 1 < max_seq_len && max_q_len > 0) max_seq_len = (int64_t)window + max_q_len - 1;
  if (num_tokens < 0 || num_heads <= 0 || num_seqs < 0 || max_q_len < 0 || max_seq_len < 0 || num_cus <= 0)
    return fail(VMI_E_SHAPE, "paged_attention_prefill_split_plan: negative size (num_tokens=%d num_heads=%d num_seqs=%d "
                "max_q_len=%d max_seq_len=%d num_cus=%d)", num_tokens, num_heads, num_seqs, max_q_len, max_seq_len_in, num_cus);
  if (head_size != 64 && head_size != 128)
    return fail(VMI_E_HEAD_SIZE, "Unsupported head size: %d (paged_attention_prefill is built for 64 and 128)", head_size);
  if (partition_tokens_in < 0 || (partition_tokens_in & 31))
    return fail(VMI_E_SHAPE, "paged_attention_prefill: partition_tokens must be a positive multiple of 32, got %d",
                partition_tokens_in);
  int64_t pt = partition_tokens_in;
  if (pt == 0) {
    const SplitRules& r = kSplitRules;
    const int64_t rows = g_shift < 0 ? prefill::ROWS : prefill::TILE >> g_shift;   // chunk rows per workgroup
    const int64_t wgs = (((int64_t)max_q_len + rows - 1) / rows) * num_seqs * (g_shift < 0 ? num_heads : num_heads >> g_shift);
    pt = max_seq_len > 32 ? ((int64_t)max_seq_len + 31) & ~31ll : 32;   // one partition
    if (wgs > 0 && wgs < (int64_t)r.underfill_wgs_per_cu * num_cus && max_seq_len >= r.min_context) {
      int64_t parts = ((int64_t)r.target_wgs_per_cu * num_cus + wgs - 1) / wgs;
      if (parts > r.max_partitions) parts = r.max_partitions;
      pt = ((max_seq_len + parts - 1) / parts + 31) & ~31ll;
      pt = pt < r.floor_tokens ? r.floor_tokens : pt > r.ceil_tokens ? r.ceil_tokens : pt;
    }
  }
  const int64_t parts = max_seq_len > 0 ? (max_seq_len + pt - 1) / pt : 1;
  *partition_tokens = (int32_t)pt;
  *num_partitions = (int32_t)parts;
  *workspace_bytes = parts > 1 ? parts * num_tokens * num_heads * (head_size + 2) * 4 : 0;
  return VMI_OK;
}

// The tile kernel of (page format by the Params type, head size, form): one place for the sixteen instantiations, and below
// it the eight of the head-packed form
template <bool SPLIT, bool COOP>
static void launch_tiles(const prefill::Params& p, int head_size, dim3 grid, dim3 block, hipStream_t st) {
  if (head_size == 64)
    hipLaunchKernelGGL((prefill::pa_prefill_kernel<64, SPLIT, COOP>), grid, block, 0, st, p);
  else
    hipLaunchKernelGGL((prefill::pa_prefill_kernel<128, SPLIT, COOP>), grid, block, 0, st, p);
}
template <bool SPLIT, bool COOP>
static void launch_tiles(const prefill::ParamsFp8& p, int head_size, dim3 grid, dim3 block, hipStream_t st) {
  if (head_size == 64)
    hipLaunchKernelGGL((prefill::pa_prefill_fp8_kernel<64, SPLIT, COOP>), grid, block, 0, st, p);
  else
    hipLaunchKernelGGL((prefill::pa_prefill_fp8_kernel<128, SPLIT, COOP>), grid, block, 0, st, p);
}
template <bool SPLIT>
static void launch_packed(const prefill::Params& p, int head_size, dim3 grid, dim3 block, hipStream_t st) {
  if (head_size == 64)
    hipLaunchKernelGGL((prefill::pa_prefill_kernel<64, SPLIT, true, true>), grid, block, 0, st, p);
  else
    hipLaunchKernelGGL((prefill::pa_prefill_kernel<128, SPLIT, true, true>), grid, block, 0, st, p);
}
template <bool SPLIT>
static void launch_packed(const prefill::ParamsFp8& p, int head_size, dim3 grid, dim3 block, hipStream_t st) {
  if (head_size == 64)
    hipLaunchKernelGGL((prefill::pa_prefill_fp8_kernel<64, SPLIT, true, true>), grid, block, 0, st, p);
  else
    hipLaunchKernelGGL((prefill::pa_prefill_fp8_kernel<128, SPLIT, true, true>), grid, block, 0, st, p);
}
// the shared-prefix tiles (PREFIX): partition 0 of every row of the packed batch, one tile of 16 rows x one head per workgroup
static void launch_prefix(const prefill::Params& p, int head_size, dim3 grid, dim3 block, hipStream_t st) {
  if (head_size == 64)
    hipLaunchKernelGGL(prefill::pa_prefill_prefix_kernel<64>, grid, block, 0, st, p);
  else
    hipLaunchKernelGGL(prefill::pa_prefill_prefix_kernel<128>, grid, block, 0, st, p);
}
static void launch_prefix(const prefill::ParamsFp8& p, int head_size, dim3 grid, dim3 block, hipStream_t st) {
  if (head_size == 64)
    hipLaunchKernelGGL(prefill::pa_prefill_prefix_fp8_kernel<64>, grid, block, 0, st, p);
  else
    hipLaunchKernelGGL(prefill::pa_prefill_prefix_fp8_kernel<128>, grid, block, 0, st, p);
}
// the REL kernels (ALiBi slopes / sliding window): twenty-four instantiations — two page formats x two head sizes x the plain,
// SPLIT, COOP, SPLIT + COOP, PACK and PACK + SPLIT forms
template <bool SPLIT, bool COOP, bool PACK>
static void launch_rel_form(const prefill::RelParams& p, int head_size, dim3 grid, dim3 block, hipStream_t st) {
  if (head_size == 64)
    hipLaunchKernelGGL((prefill::pa_prefill_rel_kernel<64, SPLIT, COOP, PACK>), grid, block, 0, st, p);
  else
    hipLaunchKernelGGL((prefill::pa_prefill_rel_kernel<128, SPLIT, COOP, PACK>), grid, block, 0, st, p);
}
template <bool SPLIT, bool COOP, bool PACK>
static void launch_rel_form(const prefill::RelParamsFp8& p, int head_size, dim3 grid, dim3 block, hipStream_t st) {
  if (head_size == 64)
    hipLaunchKernelGGL((prefill::pa_prefill_rel_fp8_kernel<64, SPLIT, COOP, PACK>), grid, block, 0, st, p);
  else
    hipLaunchKernelGGL((prefill::pa_prefill_rel_fp8_kernel<128, SPLIT, COOP, PACK>), grid, block, 0, st, p);
}
template <bool SPLIT, class P>
static void launch_rel(const P& p, int head_size, bool coop, dim3 grid, dim3 block, hipStream_t st) {
  if (p.g_shift >= 0)
    launch_rel_form<SPLIT, true, true>(p, head_size, grid, block, st);
  else if (coop)
    launch_rel_form<SPLIT, true, false>(p, head_size, grid, block, st);
  else
    launch_rel_form<SPLIT, false, false>(p, head_size, grid, block, st);
}
// the TREE kernels (a token tree as the chunk): twenty-four instantiations again — two page formats x two head sizes x the plain,
// SPLIT, COOP, SPLIT + COOP, PACK and PACK + SPLIT forms
template <bool SPLIT, bool COOP, bool PACK>
static void launch_tree_form(const prefill::TreeParams& p, int head_size, dim3 grid, dim3 block, hipStream_t st) {
  if (head_size == 64)
    hipLaunchKernelGGL((prefill::pa_prefill_tree_kernel<64, SPLIT, COOP, PACK>), grid, block, 0, st, p);
  else
    hipLaunchKernelGGL((prefill::pa_prefill_tree_kernel<128, SPLIT, COOP, PACK>), grid, block, 0, st, p);
}
template <bool SPLIT, bool COOP, bool PACK>
static void launch_tree_form(const prefill::TreeParamsFp8& p, int head_size, dim3 grid, dim3 block, hipStream_t st) {
  if (head_size == 64)
    hipLaunchKernelGGL((prefill::pa_prefill_tree_fp8_kernel<64, SPLIT, COOP, PACK>), grid, block, 0, st, p);
  else
    hipLaunchKernelGGL((prefill::pa_prefill_tree_fp8_kernel<128, SPLIT, COOP, PACK>), grid, block, 0, st, p);
}
template <bool SPLIT, class P>
static void launch_tree(const P& p, int head_size, bool coop, dim3 grid, dim3 block, hipStream_t st) {
  if (p.g_shift >= 0)
    launch_tree_form<SPLIT, true, true>(p, head_size, grid, block, st);
  else if (coop)
    launch_tree_form<SPLIT, true, false>(p, head_size, grid, block, st);
  else
    launch_tree_form<SPLIT, false, false>(p, head_size, grid, block, st);
}
template <bool SPLIT, class P>
static void launch_tiles(const P& p, int head_size, bool coop, dim3 grid, dim3 block, hipStream_t st) {
  if (p.g_shift >= 0)
    launch_packed<SPLIT>(p, head_size, grid, block, st);
  else if (coop)
    launch_tiles<SPLIT, true>(p, head_size, grid, block, st);
  else
    launch_tiles<SPLIT, false>(p, head_size, grid, block, st);
}

// max_seq_len < 0: the plain entries — never split, no bound on seq_lens.  coop: the cooperative form of the tile kernels
// (pa_prefill.hpp, COOP) — same grid, same Params, same merge launch.  pack: the head-packed form (PACK) — one tile of
// 16 / G rows x G heads per workgroup, a grid over KV heads; Params, workspace and merge launch are the same again.
// prefix > 0 (the shared-prefix entries, which checked it: a multiple of 32, == partition_tokens, < max_seq_len — so there are
// at least two partitions and a workspace): partition 0 comes from the PREFIX tiles, launched first; coop / pack then are the
// form of the SUFFIX launch, whose partition axis starts at part0 = 1; the merge launch is the same.
// rel (the REL entries, which checked window >= 0): the REL kernels of the same form with alibi_slopes (may be NULL) and window
// (0: none); the plan counts on min(max_seq_len, window + max_q_len - 1), and the merge is the REL one.
// tree_mask (the TREE entries, which checked it and max_q_len <= 64; never with prefix or rel): the TREE kernels of the same form
// on the same grid, plan and workspace; the merge is the same kernel under the TREE guard (MergeTreeParams).
static int launch_pa_prefill(void* out, const void* query, const void* key_cache, const void* value_cache,
                             int32_t num_tokens, int32_t num_heads, int32_t head_size, int32_t num_kv_heads, float scale,
                             const int32_t* block_tables, const int32_t* seq_lens, const int32_t* cu_q_lens,
                             int32_t num_seqs, int32_t max_q_len, int32_t block_size, int32_t max_num_blocks_per_seq,
                             int64_t q_stride, int64_t kv_block_stride, int64_t kv_head_stride, int32_t device,
                             void* stream, bool fp8, float kv_scale, int32_t max_seq_len = -1,
                             int32_t partition_tokens = 0, void* workspace = nullptr, int64_t workspace_bytes = 0,
                             bool coop = false, bool pack = false, int32_t prefix = 0, bool rel = false,
                             const float* alibi_slopes = nullptr, int32_t window = 0, const uint64_t* tree_mask = nullptr) {
  // one validation for both page formats; the cache strides are in cache elements: halves, or bytes when fp8
  const bool empty = num_tokens == 0 || num_seqs == 0;   // (torch hands out null data pointers for empty tensors)
  if (!key_cache || !value_cache || (!empty && (!out || !query || !block_tables || !seq_lens || !cu_q_lens)))
    return fail(VMI_E_NULL_POINTER, "paged_attention_prefill: NULL tensor pointer");
  if (head_size != 64 && head_size != 128)
    return fail(VMI_E_HEAD_SIZE, "Unsupported head size: %d (paged_attention_prefill is built for 64 and 128)", head_size);
  if (block_size != prefill::BS)
    return fail(VMI_E_BLOCK_SIZE, "Unsupported block size: %d (paged_attention_prefill is built for 16)", block_size);
  if (num_tokens < 0 || num_seqs < 0 || num_heads <= 0 || max_q_len < 0 || max_num_blocks_per_seq < 0)
    return fail(VMI_E_SHAPE, "paged_attention_prefill: negative size (num_tokens=%d num_seqs=%d num_heads=%d max_q_len=%d "
                "max_num_blocks_per_seq=%d)", num_tokens, num_seqs, num_heads, max_q_len, max_num_blocks_per_seq);
  if (fp8 && !(kv_scale > 0.f && kv_scale <= 3.4028234664e38f))   // (NaN fails the first comparison)
    return fail(VMI_E_SHAPE, "paged_attention_prefill: kv_scale must be finite and positive, got %g", (double)kv_scale);
  if (num_kv_heads <= 0 || num_heads % num_kv_heads != 0)
    return fail(VMI_E_KV_HEADS, "paged_attention_prefill: num_heads=%d not divisible by num_kv_heads=%d", num_heads,
                num_kv_heads);
  const int g_shift = pack ? pack_shift(num_heads, num_kv_heads) : -1;
  if (pack && g_shift < 0) return fail_pack_ratio(num_heads, num_kv_heads);
  const int64_t kv_mask = fp8 ? 15 : 7;   // 16 bytes in cache elements
  if (!aligned16(query) || !aligned16(key_cache) || !aligned16(value_cache) || (reinterpret_cast<uintptr_t>(out) & 7u) ||
      (q_stride & 7) || (kv_block_stride & kv_mask) || (kv_head_stride & kv_mask))
    return fail(VMI_E_ALIGNMENT, "paged_attention_prefill: query/key_cache/value_cache and their strides must be 16-byte "
                "aligned (q_stride=%lld kv_block_stride=%lld kv_head_stride=%lld)", (long long)q_stride,
                (long long)kv_block_stride, (long long)kv_head_stride);
  const bool bounded = max_seq_len >= 0;                  // the split entries
  int32_t parts = 1;
  if (bounded) {
    if (max_seq_len > (int64_t)prefill::BS * max_num_blocks_per_seq)
      return fail(VMI_E_SHAPE, "paged_attention_prefill: max_seq_len=%d exceeds the block table (%d blocks of 16)", max_seq_len,
                  max_num_blocks_per_seq);
    if (partition_tokens <= 0 || (partition_tokens & 31))
      return fail(VMI_E_SHAPE, "paged_attention_prefill: partition_tokens must be a positive multiple of 32, got %d",
                  partition_tokens);
    int64_t need = 0;
    const int rc = split_plan(num_tokens, num_heads, head_size, num_seqs, max_q_len, max_seq_len, 1, partition_tokens,
                              &partition_tokens, &parts, &need, -1, window);
    if (rc != VMI_OK) return rc;
    if (parts > 1 && !empty && (!workspace || !aligned16(workspace) || workspace_bytes < need))
      return fail(VMI_E_WORKSPACE, "paged_attention_prefill: %d partitions need a 16-byte aligned workspace of %lld bytes (got %p, %lld bytes)",
                  parts, (long long)need, workspace, (long long)workspace_bytes);
  }
  if (empty || max_q_len == 0 || max_seq_len == 0) return VMI_OK;
  const int64_t tile_rows = pack ? prefill::TILE >> g_shift : prefill::ROWS;   // chunk rows per workgroup
  const int64_t groups = ((int64_t)max_q_len + tile_rows - 1) / tile_rows;
  const int64_t wgs = groups * num_seqs * (pack ? num_kv_heads : num_heads) * (parts - (prefix > 0));
  const int64_t prefix_wgs = ((int64_t)num_tokens + prefill::TILE - 1) / prefill::TILE * num_heads;
  constexpr int MERGE_ROWS = 1024 / 128;                  // the merge's rows per workgroup at its smallest (D 128)
  if ((int64_t)num_seqs * num_heads >= (1ll << 31) || wgs >= (1ll << 31) || (prefix > 0 && prefix_wgs >= (1ll << 31)) ||
      (parts > 1 && ((int64_t)max_q_len + MERGE_ROWS - 1) / MERGE_ROWS * num_seqs * num_heads >= (1ll << 31)))
    return fail(VMI_E_SHAPE, "paged_attention_prefill: %lld workgroups exceed the grid", (long long)wgs);

  auto fill = [&](auto& p) {
    p.out = static_cast<prefill::h16*>(out);
    p.q = static_cast<const prefill::h16*>(query);
    p.kc = static_cast<decltype(p.kc)>(key_cache);
    p.vc = static_cast<decltype(p.vc)>(value_cache);
    p.block_tables = block_tables;
    p.seq_lens = seq_lens;
    p.cu_q_lens = cu_q_lens;
    p.q_stride = q_stride;
    p.kv_block_stride = kv_block_stride;
    p.kv_head_stride = kv_head_stride;
    p.num_tokens = num_tokens;
    p.num_heads = num_heads;
    p.q_per_kv = num_heads / num_kv_heads;
    p.num_seqs = num_seqs;
    p.max_blocks_per_seq = max_num_blocks_per_seq;
    p.max_seq_len = bounded ? max_seq_len : INT_MAX;
    p.ws = static_cast<float*>(workspace);
    p.part_tokens = partition_tokens;
    p.num_parts = parts;
    p.groups = (int32_t)groups;
    p.g_shift = g_shift;
    p.part0 = 0;
  };

  DeviceGuard guard(device);
  if (guard.err != hipSuccess) return hip_fail(guard.err, "paged_attention_prefill: hipSetDevice");
  const dim3 grid((unsigned)wgs), block(prefill::WAVES * 64);
  hipStream_t st = static_cast<hipStream_t>(stream);
  // the shared-prefix tiles in front of the suffix launch, which then starts at partition 1
  auto prefix_tiles = [&](auto& p) -> hipError_t {
    if (prefix <= 0) return hipSuccess;
    launch_prefix(p, head_size, dim3((unsigned)prefix_wgs), block, st);
    p.part0 = 1;
    return hipGetLastError();
  };
  // the REL kernels of either page format, split (std::true_type) or not: the same fields plus the two terms
  auto rel_tiles = [&](auto split) {
    auto go = [&](auto& p, float score_scale) {
      fill(p);
      p.scale_log2e = score_scale * 1.4426950408889634f;
      p.alibi_slopes = alibi_slopes;
      p.window = window;
      launch_rel<decltype(split)::value>(p, head_size, coop, grid, block, st);
    };
    if (fp8) {
      prefill::RelParamsFp8 p;
      p.kv_scale = kv_scale;
      go(p, scale * kv_scale);
    } else {
      prefill::RelParams p;
      go(p, scale);
    }
  };
  // the TREE kernels of either page format, split or not: the same fields plus the words
  auto tree_tiles = [&](auto split) {
    auto go = [&](auto& p, float score_scale) {
      fill(p);
      p.scale_log2e = score_scale * 1.4426950408889634f;
      p.tree_mask = tree_mask;
      launch_tree<decltype(split)::value>(p, head_size, coop, grid, block, st);
    };
    if (fp8) {
      prefill::TreeParamsFp8 p;
      p.kv_scale = kv_scale;
      go(p, scale * kv_scale);
    } else {
      prefill::TreeParams p;
      go(p, scale);
    }
  };
  if (parts > 1) {
    // partition kernels, then the merge, on the caller's stream: the second launch is the only synchronisation
    prefill::MergeParams mp;
    mp.out = static_cast<prefill::h16*>(out);
    mp.ws = static_cast<const float*>(workspace);
    mp.seq_lens = seq_lens;
    mp.cu_q_lens = cu_q_lens;
    mp.num_tokens = num_tokens;
    mp.num_heads = num_heads;
    mp.num_seqs = num_seqs;
    mp.max_blocks_per_seq = max_num_blocks_per_seq;
    mp.max_seq_len = max_seq_len;
    mp.part_tokens = partition_tokens;
    mp.num_parts = parts;
    mp.out_scale = fp8 ? kv_scale : 1.0f;
    if (rel) {
      rel_tiles(std::true_type());
    } else if (tree_mask) {
      tree_tiles(std::true_type());
    } else if (fp8) {
      prefill::ParamsFp8 p;
      fill(p);
      p.scale_log2e = (scale * kv_scale) * 1.4426950408889634f;
      p.kv_scale = kv_scale;
      if (const hipError_t pe = prefix_tiles(p)) return hip_fail(pe, "paged_attention_prefill shared-prefix launch");
      launch_tiles<true>(p, head_size, coop, grid, block, st);
    } else {
      prefill::Params p;
      fill(p);
      p.scale_log2e = scale * 1.4426950408889634f;
      if (const hipError_t pe = prefix_tiles(p)) return hip_fail(pe, "paged_attention_prefill shared-prefix launch");
      launch_tiles<true>(p, head_size, coop, grid, block, st);
    }
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return hip_fail(e, "paged_attention_prefill partition launch");
    const int rpb = 1024 / head_size;
    const dim3 mgrid((unsigned)(((int64_t)max_q_len + rpb - 1) / rpb * num_seqs * num_heads));
    if (rel) {
      prefill::MergeRelParams mrp;
      static_cast<prefill::MergeParams&>(mrp) = mp;
      mrp.window = window;
      if (head_size == 64)
        hipLaunchKernelGGL(prefill::pa_prefill_merge_rel_kernel<64>, mgrid, dim3(256), 0, st, mrp);
      else
        hipLaunchKernelGGL(prefill::pa_prefill_merge_rel_kernel<128>, mgrid, dim3(256), 0, st, mrp);
    } else if (tree_mask) {
      prefill::MergeTreeParams mtp;
      static_cast<prefill::MergeParams&>(mtp) = mp;
      if (head_size == 64)
        hipLaunchKernelGGL((prefill::pa_prefill_merge_kernel<64, prefill::MergeTreeParams>), mgrid, dim3(256), 0, st, mtp);
      else
        hipLaunchKernelGGL((prefill::pa_prefill_merge_kernel<128, prefill::MergeTreeParams>), mgrid, dim3(256), 0, st, mtp);
    } else if (head_size == 64)
      hipLaunchKernelGGL(prefill::pa_prefill_merge_kernel<64>, mgrid, dim3(256), 0, st, mp);
    else
      hipLaunchKernelGGL(prefill::pa_prefill_merge_kernel<128>, mgrid, dim3(256), 0, st, mp);
    e = hipGetLastError();
    if (e != hipSuccess) return hip_fail(e, "paged_attention_prefill merge launch");
    return VMI_OK;
  }
  if (rel) {
    rel_tiles(std::false_type());
  } else if (tree_mask) {
    tree_tiles(std::false_type());
  } else if (fp8) {
    prefill::ParamsFp8 p;
    fill(p);
    p.scale_log2e = (scale * kv_scale) * 1.4426950408889634f;   // K's kv_scale rides in the score scale (x 1.0f is exact)
    p.kv_scale = kv_scale;                                       // V's in the final kv_scale / sum
    launch_tiles<false>(p, head_size, coop, grid, block, st);
  } else {
    prefill::Params p;
    fill(p);
    p.scale_log2e = scale * 1.4426950408889634f;
    launch_tiles<false>(p, head_size, coop, grid, block, st);
  }
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) return hip_fail(e, "paged_attention_prefill launch");
  return VMI_OK;
}

}  // namespace vmi

extern "C" int vmi_paged_attention_prefill_f16(
    void* out, const void* query, const void* key_cache, const void* value_cache,
    int32_t num_tokens, int32_t num_heads, int32_t head_size, int32_t num_kv_heads, float scale,
    const int32_t* block_tables, const int32_t* seq_lens, const int32_t* cu_q_lens,
    int32_t num_seqs, int32_t max_q_len, int32_t block_size, int32_t max_num_blocks_per_seq,
    int64_t q_stride, int64_t kv_block_stride, int64_t kv_head_stride, int32_t device, void* stream) {
  return vmi::launch_pa_prefill(out, query, key_cache, value_cache, num_tokens, num_heads, head_size, num_kv_heads, scale,
                                block_tables, seq_lens, cu_q_lens, num_seqs, max_q_len, block_size, max_num_blocks_per_seq,
                                q_stride, kv_block_stride, kv_head_stride, device, stream, false, 1.0f);
}

extern "C" int vmi_paged_attention_prefill_fp8(
    void* out, const void* query, const void* key_cache, const void* value_cache,
    int32_t num_tokens, int32_t num_heads, int32_t head_size, int32_t num_kv_heads, float scale,
    const int32_t* block_tables, const int32_t* seq_lens, const int32_t* cu_q_lens,
    int32_t num_seqs, int32_t max_q_len, int32_t block_size, int32_t max_num_blocks_per_seq,
    int64_t q_stride, int64_t kv_block_stride, int64_t kv_head_stride, int32_t device, void* stream, float kv_scale) {
  return vmi::launch_pa_prefill(out, query, key_cache, value_cache, num_tokens, num_heads, head_size, num_kv_heads, scale,
                                block_tables, seq_lens, cu_q_lens, num_seqs, max_q_len, block_size, max_num_blocks_per_seq,
                                q_stride, kv_block_stride, kv_head_stride, device, stream, true, kv_scale);
}

extern "C" int vmi_paged_attention_prefill_split_plan(
    int32_t num_tokens, int32_t num_heads, int32_t head_size, int32_t num_seqs, int32_t max_q_len, int32_t max_seq_len,
    int32_t num_cus, int32_t partition_tokens_in, int32_t* partition_tokens, int32_t* num_partitions,
    int64_t* workspace_bytes) {
  if (!partition_tokens || !num_partitions || !workspace_bytes)
    return vmi::fail(VMI_E_NULL_POINTER, "paged_attention_prefill_split_plan: NULL result pointer");
  if (num_cus == 0) {   // ask the current device
    int dev = 0;
    hipDeviceProp_t prop;
    hipError_t e = hipGetDevice(&dev);
    if (e == hipSuccess) e = hipGetDeviceProperties(&prop, dev);
    if (e != hipSuccess) return vmi::hip_fail(e, "paged_attention_prefill_split_plan: device properties");
    num_cus = prop.multiProcessorCount;
  }
  return vmi::split_plan(num_tokens, num_heads, head_size, num_seqs, max_q_len, max_seq_len, num_cus, partition_tokens_in,
                         partition_tokens, num_partitions, workspace_bytes);
}

extern "C" int vmi_paged_attention_prefill_split_f16(
    void* out, const void* query, const void* key_cache, const void* value_cache,
    int32_t num_tokens, int32_t num_heads, int32_t head_size, int32_t num_kv_heads, float scale,
    const int32_t* block_tables, const int32_t* seq_lens, const int32_t* cu_q_lens,
    int32_t num_seqs, int32_t max_q_len, int32_t block_size, int32_t max_num_blocks_per_seq,
    int64_t q_stride, int64_t kv_block_stride, int64_t kv_head_stride, int32_t device, void* stream,
    int32_t max_seq_len, int32_t partition_tokens, void* workspace, int64_t workspace_bytes) {
  if (max_seq_len < 0) return vmi::fail(VMI_E_SHAPE, "paged_attention_prefill: negative max_seq_len=%d", max_seq_len);
  return vmi::launch_pa_prefill(out, query, key_cache, value_cache, num_tokens, num_heads, head_size, num_kv_heads, scale,
                                block_tables, seq_lens, cu_q_lens, num_seqs, max_q_len, block_size, max_num_blocks_per_seq,
                                q_stride, kv_block_stride, kv_head_stride, device, stream, false, 1.0f, max_seq_len,
                                partition_tokens, workspace, workspace_bytes);
}

extern "C" int vmi_paged_attention_prefill_split_fp8(
    void* out, const void* query, const void* key_cache, const void* value_cache,
    int32_t num_tokens, int32_t num_heads, int32_t head_size, int32_t num_kv_heads, float scale,
    const int32_t* block_tables, const int32_t* seq_lens, const int32_t* cu_q_lens,
    int32_t num_seqs, int32_t max_q_len, int32_t block_size, int32_t max_num_blocks_per_seq,
    int64_t q_stride, int64_t kv_block_stride, int64_t kv_head_stride, int32_t device, void* stream,
    int32_t max_seq_len, int32_t partition_tokens, void* workspace, int64_t workspace_bytes, float kv_scale) {
  if (max_seq_len < 0) return vmi::fail(VMI_E_SHAPE, "paged_attention_prefill: negative max_seq_len=%d", max_seq_len);
  return vmi::launch_pa_prefill(out, query, key_cache, value_cache, num_tokens, num_heads, head_size, num_kv_heads, scale,
                                block_tables, seq_lens, cu_q_lens, num_seqs, max_q_len, block_size, max_num_blocks_per_seq,
                                q_stride, kv_block_stride, kv_head_stride, device, stream, true, kv_scale, max_seq_len,
                                partition_tokens, workspace, workspace_bytes);
}

extern "C" int vmi_paged_attention_prefill_coop_f16(
    void* out, const void* query, const void* key_cache, const void* value_cache,
    int32_t num_tokens, int32_t num_heads, int32_t head_size, int32_t num_kv_heads, float scale,
    const int32_t* block_tables, const int32_t* seq_lens, const int32_t* cu_q_lens,
    int32_t num_seqs, int32_t max_q_len, int32_t block_size, int32_t max_num_blocks_per_seq,
    int64_t q_stride, int64_t kv_block_stride, int64_t kv_head_stride, int32_t device, void* stream,
    int32_t max_seq_len, int32_t partition_tokens, void* workspace, int64_t workspace_bytes) {
  if (max_seq_len < 0) return vmi::fail(VMI_E_SHAPE, "paged_attention_prefill: negative max_seq_len=%d", max_seq_len);
  return vmi::launch_pa_prefill(out, query, key_cache, value_cache, num_tokens, num_heads, head_size, num_kv_heads, scale,
                                block_tables, seq_lens, cu_q_lens, num_seqs, max_q_len, block_size, max_num_blocks_per_seq,
                                q_stride, kv_block_stride, kv_head_stride, device, stream, false, 1.0f, max_seq_len,
                                partition_tokens, workspace, workspace_bytes, true);
}

extern "C" int vmi_paged_attention_prefill_coop_fp8(
    void* out, const void* query, const void* key_cache, const void* value_cache,
    int32_t num_tokens, int32_t num_heads, int32_t head_size, int32_t num_kv_heads, float scale,
    const int32_t* block_tables, const int32_t* seq_lens, const int32_t* cu_q_lens,
    int32_t num_seqs, int32_t max_q_len, int32_t block_size, int32_t max_num_blocks_per_seq,
    int64_t q_stride, int64_t kv_block_stride, int64_t kv_head_stride, int32_t device, void* stream,
    int32_t max_seq_len, int32_t partition_tokens, void* workspace, int64_t workspace_bytes, float kv_scale) {
  if (max_seq_len < 0) return vmi::fail(VMI_E_SHAPE, "paged_attention_prefill: negative max_seq_len=%d", max_seq_len);
  return vmi::launch_pa_prefill(out, query, key_cache, value_cache, num_tokens, num_heads, head_size, num_kv_heads, scale,
                                block_tables, seq_lens, cu_q_lens, num_seqs, max_q_len, block_size, max_num_blocks_per_seq,
                                q_stride, kv_block_stride, kv_head_stride, device, stream, true, kv_scale, max_seq_len,
                                partition_tokens, workspace, workspace_bytes, true);
}

extern "C" int vmi_paged_attention_prefill_gqa_plan(
    int32_t num_tokens, int32_t num_heads, int32_t head_size, int32_t num_seqs, int32_t max_q_len, int32_t max_seq_len,
    int32_t num_cus, int32_t partition_tokens_in, int32_t* partition_tokens, int32_t* num_partitions,
    int64_t* workspace_bytes, int32_t num_kv_heads) {
  if (!partition_tokens || !num_partitions || !workspace_bytes)
    return vmi::fail(VMI_E_NULL_POINTER, "paged_attention_prefill_gqa_plan: NULL result pointer");
  const int g_shift = vmi::pack_shift(num_heads, num_kv_heads);
  if (g_shift < 0) return vmi::fail_pack_ratio(num_heads, num_kv_heads);
  if (num_cus == 0) {   // ask the current device
    int dev = 0;
    hipDeviceProp_t prop;
    hipError_t e = hipGetDevice(&dev);
    if (e == hipSuccess) e = hipGetDeviceProperties(&prop, dev);
    if (e != hipSuccess) return vmi::hip_fail(e, "paged_attention_prefill_gqa_plan: device properties");
    num_cus = prop.multiProcessorCount;
  }
  return vmi::split_plan(num_tokens, num_heads, head_size, num_seqs, max_q_len, max_seq_len, num_cus, partition_tokens_in,
                         partition_tokens, num_partitions, workspace_bytes, g_shift);
}

extern "C" int vmi_paged_attention_prefill_gqa_f16(
    void* out, const void* query, const void* key_cache, const void* value_cache,
    int32_t num_tokens, int32_t num_heads, int32_t head_size, int32_t num_kv_heads, float scale,
    const int32_t* block_tables, const int32_t* seq_lens, const int32_t* cu_q_lens,
    int32_t num_seqs, int32_t max_q_len, int32_t block_size, int32_t max_num_blocks_per_seq,
    int64_t q_stride, int64_t kv_block_stride, int64_t kv_head_stride, int32_t device, void* stream,
    int32_t max_seq_len, int32_t partition_tokens, void* workspace, int64_t workspace_bytes) {
  if (max_seq_len < 0) return vmi::fail(VMI_E_SHAPE, "paged_attention_prefill: negative max_seq_len=%d", max_seq_len);
  return vmi::launch_pa_prefill(out, query, key_cache, value_cache, num_tokens, num_heads, head_size, num_kv_heads, scale,
                                block_tables, seq_lens, cu_q_lens, num_seqs, max_q_len, block_size, max_num_blocks_per_seq,
                                q_stride, kv_block_stride, kv_head_stride, device, stream, false, 1.0f, max_seq_len,
                                partition_tokens, workspace, workspace_bytes, true, true);
}

extern "C" int vmi_paged_attention_prefill_gqa_fp8(
    void* out, const void* query, const void* key_cache, const void* value_cache,
    int32_t num_tokens, int32_t num_heads, int32_t head_size, int32_t num_kv_heads, float scale,
    const int32_t* block_tables, const int32_t* seq_lens, const int32_t* cu_q_lens,
    int32_t num_seqs, int32_t max_q_len, int32_t block_size, int32_t max_num_blocks_per_seq,
    int64_t q_stride, int64_t kv_block_stride, int64_t kv_head_stride, int32_t device, void* stream,
    int32_t max_seq_len, int32_t partition_tokens, void* workspace, int64_t workspace_bytes, float kv_scale) {
  if (max_seq_len < 0) return vmi::fail(VMI_E_SHAPE, "paged_attention_prefill: negative max_seq_len=%d", max_seq_len);
  return vmi::launch_pa_prefill(out, query, key_cache, value_cache, num_tokens, num_heads, head_size, num_kv_heads, scale,
                                block_tables, seq_lens, cu_q_lens, num_seqs, max_q_len, block_size, max_num_blocks_per_seq,
                                q_stride, kv_block_stride, kv_head_stride, device, stream, true, kv_scale, max_seq_len,
                                partition_tokens, workspace, workspace_bytes, true, true);
}

// the shared-prefix entries' own checks, in front of the common ones; -> VMI_OK and the suffix launch's form
static int check_prefix(int32_t max_seq_len, int32_t partition_tokens, int32_t shared_prefix_len, int32_t suffix_form) {
  if (max_seq_len < 0) return vmi::fail(VMI_E_SHAPE, "paged_attention_prefill: negative max_seq_len=%d", max_seq_len);
  if (shared_prefix_len <= 0 || (shared_prefix_len & 31))
    return vmi::fail(VMI_E_SHAPE, "paged_attention_prefill: shared_prefix_len must be a positive multiple of 32, got %d",
                     shared_prefix_len);
  if (shared_prefix_len >= max_seq_len)
    return vmi::fail(VMI_E_SHAPE, "paged_attention_prefill: shared_prefix_len=%d must be less than max_seq_len=%d",
                     shared_prefix_len, max_seq_len);
  if (partition_tokens != shared_prefix_len)
    return vmi::fail(VMI_E_SHAPE, "paged_attention_prefill: partition_tokens=%d must equal shared_prefix_len=%d (the prefix is "
                     "partition 0)", partition_tokens, shared_prefix_len);
  if (suffix_form < 0 || suffix_form > 2)
    return vmi::fail(VMI_E_SHAPE, "paged_attention_prefill: suffix_form must be 0 (plain), 1 (cooperative) or 2 (head-packed), "
                     "got %d", suffix_form);
  return VMI_OK;
}

extern "C" int vmi_paged_attention_prefill_prefix_f16(
    void* out, const void* query, const void* key_cache, const void* value_cache,
    int32_t num_tokens, int32_t num_heads, int32_t head_size, int32_t num_kv_heads, float scale,
    const int32_t* block_tables, const int32_t* seq_lens, const int32_t* cu_q_lens,
    int32_t num_seqs, int32_t max_q_len, int32_t block_size, int32_t max_num_blocks_per_seq,
    int64_t q_stride, int64_t kv_block_stride, int64_t kv_head_stride, int32_t device, void* stream,
    int32_t max_seq_len, int32_t partition_tokens, void* workspace, int64_t workspace_bytes,
    int32_t shared_prefix_len, int32_t suffix_form) {
  const int rc = check_prefix(max_seq_len, partition_tokens, shared_prefix_len, suffix_form);
  if (rc != VMI_OK) return rc;
  return vmi::launch_pa_prefill(out, query, key_cache, value_cache, num_tokens, num_heads, head_size, num_kv_heads, scale,
                                block_tables, seq_lens, cu_q_lens, num_seqs, max_q_len, block_size, max_num_blocks_per_seq,
                                q_stride, kv_block_stride, kv_head_stride, device, stream, false, 1.0f, max_seq_len,
                                partition_tokens, workspace, workspace_bytes, suffix_form >= 1, suffix_form == 2,
                                shared_prefix_len);
}

extern "C" int vmi_paged_attention_prefill_prefix_fp8(
    void* out, const void* query, const void* key_cache, const void* value_cache,
    int32_t num_tokens, int32_t num_heads, int32_t head_size, int32_t num_kv_heads, float scale,
    const int32_t* block_tables, const int32_t* seq_lens, const int32_t* cu_q_lens,
    int32_t num_seqs, int32_t max_q_len, int32_t block_size, int32_t max_num_blocks_per_seq,
    int64_t q_stride, int64_t kv_block_stride, int64_t kv_head_stride, int32_t device, void* stream,
    int32_t max_seq_len, int32_t partition_tokens, void* workspace, int64_t workspace_bytes, float kv_scale,
    int32_t shared_prefix_len, int32_t suffix_form) {
  const int rc = check_prefix(max_seq_len, partition_tokens, shared_prefix_len, suffix_form);
  if (rc != VMI_OK) return rc;
  return vmi::launch_pa_prefill(out, query, key_cache, value_cache, num_tokens, num_heads, head_size, num_kv_heads, scale,
                                block_tables, seq_lens, cu_q_lens, num_seqs, max_q_len, block_size, max_num_blocks_per_seq,
                                q_stride, kv_block_stride, kv_head_stride, device, stream, true, kv_scale, max_seq_len,
                                partition_tokens, workspace, workspace_bytes, suffix_form >= 1, suffix_form == 2,
                                shared_prefix_len);
}

// the REL entries' own checks, in front of the common ones
static int check_rel(int32_t max_seq_len, const float* alibi_slopes, int32_t sliding_window, int32_t form) {
  if (max_seq_len < 0) return vmi::fail(VMI_E_SHAPE, "paged_attention_prefill: negative max_seq_len=%d", max_seq_len);
  if (sliding_window < 0)
    return vmi::fail(VMI_E_SHAPE, "paged_attention_prefill: sliding_window must be positive (0: none), got %d", sliding_window);
  if (form < 0 || form > 2)
    return vmi::fail(VMI_E_SHAPE, "paged_attention_prefill: form must be 0 (plain), 1 (cooperative) or 2 (head-packed), got %d", form);
  if (reinterpret_cast<uintptr_t>(alibi_slopes) & 3u)
    return vmi::fail(VMI_E_ALIGNMENT, "paged_attention_prefill: alibi_slopes must be 4-byte aligned");
  return VMI_OK;
}

extern "C" int vmi_paged_attention_prefill_rel_f16(
    void* out, const void* query, const void* key_cache, const void* value_cache,
    int32_t num_tokens, int32_t num_heads, int32_t head_size, int32_t num_kv_heads, float scale,
    const int32_t* block_tables, const int32_t* seq_lens, const int32_t* cu_q_lens,
    int32_t num_seqs, int32_t max_q_len, int32_t block_size, int32_t max_num_blocks_per_seq,
    int64_t q_stride, int64_t kv_block_stride, int64_t kv_head_stride, int32_t device, void* stream,
    int32_t max_seq_len, int32_t partition_tokens, void* workspace, int64_t workspace_bytes,
    const float* alibi_slopes, int32_t sliding_window, int32_t form) {
  const int rc = check_rel(max_seq_len, alibi_slopes, sliding_window, form);
  if (rc != VMI_OK) return rc;
  return vmi::launch_pa_prefill(out, query, key_cache, value_cache, num_tokens, num_heads, head_size, num_kv_heads, scale,
                                block_tables, seq_lens, cu_q_lens, num_seqs, max_q_len, block_size, max_num_blocks_per_seq,
                                q_stride, kv_block_stride, kv_head_stride, device, stream, false, 1.0f, max_seq_len,
                                partition_tokens, workspace, workspace_bytes, form >= 1, form == 2, 0, true, alibi_slopes,
                                sliding_window);
}

extern "C" int vmi_paged_attention_prefill_rel_fp8(
    void* out, const void* query, const void* key_cache, const void* value_cache,
    int32_t num_tokens, int32_t num_heads, int32_t head_size, int32_t num_kv_heads, float scale,
    const int32_t* block_tables, const int32_t* seq_lens, const int32_t* cu_q_lens,
    int32_t num_seqs, int32_t max_q_len, int32_t block_size, int32_t max_num_blocks_per_seq,
    int64_t q_stride, int64_t kv_block_stride, int64_t kv_head_stride, int32_t device, void* stream,
    int32_t max_seq_len, int32_t partition_tokens, void* workspace, int64_t workspace_bytes, float kv_scale,
    const float* alibi_slopes, int32_t sliding_window, int32_t form) {
  const int rc = check_rel(max_seq_len, alibi_slopes, sliding_window, form);
  if (rc != VMI_OK) return rc;
  return vmi::launch_pa_prefill(out, query, key_cache, value_cache, num_tokens, num_heads, head_size, num_kv_heads, scale,
                                block_tables, seq_lens, cu_q_lens, num_seqs, max_q_len, block_size, max_num_blocks_per_seq,
                                q_stride, kv_block_stride, kv_head_stride, device, stream, true, kv_scale, max_seq_len,
                                partition_tokens, workspace, workspace_bytes, form >= 1, form == 2, 0, true, alibi_slopes,
                                sliding_window);
}

extern "C" int vmi_paged_attention_prefill_rel_plan(
    int32_t num_tokens, int32_t num_heads, int32_t head_size, int32_t num_seqs, int32_t max_q_len, int32_t max_seq_len,
    int32_t num_cus, int32_t partition_tokens_in, int32_t* partition_tokens, int32_t* num_partitions,
    int64_t* workspace_bytes, int32_t num_kv_heads, int32_t sliding_window, int32_t form) {
  if (!partition_tokens || !num_partitions || !workspace_bytes)
    return vmi::fail(VMI_E_NULL_POINTER, "paged_attention_prefill_rel_plan: NULL result pointer");
  const int rc = check_rel(0, nullptr, sliding_window, form);
  if (rc != VMI_OK) return rc;
  const int g_shift = form == 2 ? vmi::pack_shift(num_heads, num_kv_heads) : -1;
  if (form == 2 && g_shift < 0) return vmi::fail_pack_ratio(num_heads, num_kv_heads);
  if (num_cus == 0) {   // ask the current device
    int dev = 0;
    hipDeviceProp_t prop;
    hipError_t e = hipGetDevice(&dev);
    if (e == hipSuccess) e = hipGetDeviceProperties(&prop, dev);
    if (e != hipSuccess) return vmi::hip_fail(e, "paged_attention_prefill_rel_plan: device properties");
    num_cus = prop.multiProcessorCount;
  }
  return vmi::split_plan(num_tokens, num_heads, head_size, num_seqs, max_q_len, max_seq_len, num_cus, partition_tokens_in,
                         partition_tokens, num_partitions, workspace_bytes, g_shift, sliding_window);
}

// the TREE entries' own checks, in front of the common ones
static int check_tree(int32_t num_tokens, int32_t num_seqs, int32_t max_q_len, int32_t max_seq_len, const uint64_t* tree_mask,
                      int32_t form) {
  if (max_seq_len < 0) return vmi::fail(VMI_E_SHAPE, "paged_attention_prefill: negative max_seq_len=%d", max_seq_len);
  if (!tree_mask && num_tokens != 0 && num_seqs != 0)   // (torch hands out null data pointers for empty tensors)
    return vmi::fail(VMI_E_NULL_POINTER, "paged_attention_prefill: NULL tree_mask");
  if (reinterpret_cast<uintptr_t>(tree_mask) & 7u)
    return vmi::fail(VMI_E_ALIGNMENT, "paged_attention_prefill: tree_mask must be 8-byte aligned");
  if (max_q_len > vmi::prefill::TREE_ROWS)
    return vmi::fail(VMI_E_SHAPE, "paged_attention_prefill: tree_mask holds one 64-bit word per row: max_q_len must be at most "
                     "%d, got %d", vmi::prefill::TREE_ROWS, max_q_len);
  if (form < 0 || form > 2)
    return vmi::fail(VMI_E_SHAPE, "paged_attention_prefill: form must be 0 (plain), 1 (cooperative) or 2 (head-packed), got %d", form);
  return VMI_OK;
}

extern "C" int vmi_paged_attention_prefill_tree_f16(
    void* out, const void* query, const void* key_cache, const void* value_cache,
    int32_t num_tokens, int32_t num_heads, int32_t head_size, int32_t num_kv_heads, float scale,
    const int32_t* block_tables, const int32_t* seq_lens, const int32_t* cu_q_lens,
    int32_t num_seqs, int32_t max_q_len, int32_t block_size, int32_t max_num_blocks_per_seq,
    int64_t q_stride, int64_t kv_block_stride, int64_t kv_head_stride, int32_t device, void* stream,
    int32_t max_seq_len, int32_t partition_tokens, void* workspace, int64_t workspace_bytes,
    const uint64_t* tree_mask, int32_t form) {
  const int rc = check_tree(num_tokens, num_seqs, max_q_len, max_seq_len, tree_mask, form);
  if (rc != VMI_OK) return rc;
  return vmi::launch_pa_prefill(out, query, key_cache, value_cache, num_tokens, num_heads, head_size, num_kv_heads, scale,
                                block_tables, seq_lens, cu_q_lens, num_seqs, max_q_len, block_size, max_num_blocks_per_seq,
                                q_stride, kv_block_stride, kv_head_stride, device, stream, false, 1.0f, max_seq_len,
                                partition_tokens, workspace, workspace_bytes, form >= 1, form == 2, 0, false, nullptr, 0,
                                tree_mask);
}

extern "C" int vmi_paged_attention_prefill_tree_fp8(
    void* out, const void* query, const void* key_cache, const void* value_cache,
    int32_t num_tokens, int32_t num_heads, int32_t head_size, int32_t num_kv_heads, float scale,
    const int32_t* block_tables, const int32_t* seq_lens, const int32_t* cu_q_lens,
    int32_t num_seqs, int32_t max_q_len, int32_t block_size, int32_t max_num_blocks_per_seq,
    int64_t q_stride, int64_t kv_block_stride, int64_t kv_head_stride, int32_t device, void* stream,
    int32_t max_seq_len, int32_t partition_tokens, void* workspace, int64_t workspace_bytes, float kv_scale,
    const uint64_t* tree_mask, int32_t form) {
  const int rc = check_tree(num_tokens, num_seqs, max_q_len, max_seq_len, tree_mask, form);
  if (rc != VMI_OK) return rc;
  return vmi::launch_pa_prefill(out, query, key_cache, value_cache, num_tokens, num_heads, head_size, num_kv_heads, scale,
                                block_tables, seq_lens, cu_q_lens, num_seqs, max_q_len, block_size, max_num_blocks_per_seq,
                                q_stride, kv_block_stride, kv_head_stride, device, stream, true, kv_scale, max_seq_len,
                                partition_tokens, workspace, workspace_bytes, form >= 1, form == 2, 0, false, nullptr, 0,
                                tree_mask);
}

// ----------------------------------------------------------------------------------------
// The chunk form of the cache write (kernels: pa_cache_chunk.hpp): a prefill chunk's K / V rows into the pages, split by
// (sequence, cache block, KV head) from the arguments the attention above takes.  The grid is sized from the host's bounds;
// the lengths stay on the device.
// ----------------------------------------------------------------------------------------
namespace vmi {

static int launch_cache_chunks(const void* key, const void* value, void* key_cache, void* value_cache, int32_t num_tokens,
                               int32_t num_kv_heads, int32_t head_size, const int32_t* block_tables, const int32_t* seq_lens,
                               const int32_t* cu_q_lens, int32_t num_seqs, int32_t max_q_len, int32_t block_size, int32_t x,
                               int32_t max_num_blocks_per_seq, int32_t num_blocks, int64_t key_stride, int64_t value_stride,
                               int64_t kv_block_stride, int64_t kv_head_stride, int32_t device, void* stream, bool fp8,
                               float kv_scale) {
  const bool empty = num_tokens == 0 || num_seqs == 0;   // (torch hands out null data pointers for empty tensors)
  if (!key_cache || !value_cache || (!empty && (!key || !value || !block_tables || !seq_lens || !cu_q_lens)))
    return fail(VMI_E_NULL_POINTER, "reshape_and_cache_chunks: NULL tensor pointer");
  if (head_size != 64 && head_size != 128)
    return fail(VMI_E_HEAD_SIZE, "Unsupported head size: %d (reshape_and_cache_chunks is built for 64 and 128)", head_size);
  if (block_size != chunkwrite::BS)
    return fail(VMI_E_BLOCK_SIZE, "Unsupported block size: %d (reshape_and_cache_chunks is built for 16)", block_size);
  if (x != (fp8 ? 16 : 8))
    return fail(VMI_E_X, "reshape_and_cache_chunks: key_cache.size(4) must be %d, got %d", fp8 ? 16 : 8, x);
  if (num_tokens < 0 || num_seqs < 0 || num_kv_heads <= 0 || max_q_len < 0 || max_num_blocks_per_seq < 0 || num_blocks < 0 ||
      key_stride < 0 || value_stride < 0 || kv_block_stride < 0 || kv_head_stride < 0)
    return fail(VMI_E_SHAPE, "reshape_and_cache_chunks: negative size (num_tokens=%d num_seqs=%d num_kv_heads=%d max_q_len=%d "
                "max_num_blocks_per_seq=%d num_blocks=%d)", num_tokens, num_seqs, num_kv_heads, max_q_len,
                max_num_blocks_per_seq, num_blocks);
  if (fp8 && !(kv_scale > 0.f && kv_scale <= 3.4028234664e38f))   // (NaN fails the first comparison)
    return fail(VMI_E_SHAPE, "reshape_and_cache_chunks: kv_scale must be finite and positive, got %g", (double)kv_scale);
  const int64_t kv_mask = fp8 ? 15 : 7;   // 16 bytes in cache elements
  if (!aligned16(key) || !aligned16(value) || !aligned16(key_cache) || !aligned16(value_cache) || (key_stride & 7) ||
      (value_stride & 7) || (kv_block_stride & kv_mask) || (kv_head_stride & kv_mask) ||
      ((reinterpret_cast<uintptr_t>(block_tables) | reinterpret_cast<uintptr_t>(seq_lens) | reinterpret_cast<uintptr_t>(cu_q_lens)) & 3u))
    return fail(VMI_E_ALIGNMENT, "reshape_and_cache_chunks: key/value/key_cache/value_cache and their strides must be 16-byte "
                "aligned (key_stride=%lld value_stride=%lld kv_block_stride=%lld kv_head_stride=%lld)", (long long)key_stride,
                (long long)value_stride, (long long)kv_block_stride, (long long)kv_head_stride);
  if (empty || max_q_len == 0) return VMI_OK;
  // a chunk of q rows that starts at offset 15 of a block touches (q + 30) / 16 blocks; one wave per (sequence, block, KV head)
  const int64_t nb = ((int64_t)max_q_len + 2 * chunkwrite::BS - 2) / chunkwrite::BS;
  const int64_t wgs = (nb * num_seqs * num_kv_heads + chunkwrite::WAVES - 1) / chunkwrite::WAVES;
  if (wgs >= (1ll << 31)) return fail(VMI_E_SHAPE, "reshape_and_cache_chunks: %lld workgroups exceed the grid", (long long)wgs);

  chunkwrite::Params p;
  p.key = static_cast<const h16*>(key);
  p.value = static_cast<const h16*>(value);
  p.kc = key_cache;
  p.vc = value_cache;
  p.block_tables = block_tables;
  p.seq_lens = seq_lens;
  p.cu_q_lens = cu_q_lens;
  p.key_stride = key_stride;
  p.value_stride = value_stride;
  p.kv_block_stride = kv_block_stride;
  p.kv_head_stride = kv_head_stride;
  p.num_tokens = num_tokens;
  p.num_kv_heads = num_kv_heads;
  p.num_seqs = num_seqs;
  p.max_blocks_per_seq = max_num_blocks_per_seq;
  p.num_blocks = num_blocks;
  p.nb = (int32_t)nb;
  p.kv_scale = kv_scale;

  DeviceGuard guard(device);
  if (guard.err != hipSuccess) return hip_fail(guard.err, "reshape_and_cache_chunks: hipSetDevice");
  const dim3 grid((unsigned)wgs), block(chunkwrite::WAVES * 64);
  hipStream_t st = static_cast<hipStream_t>(stream);
  if (fp8) {
    if (head_size == 64)
      hipLaunchKernelGGL((chunkwrite::pa_cache_chunks_kernel<64, true>), grid, block, 0, st, p);
    else
      hipLaunchKernelGGL((chunkwrite::pa_cache_chunks_kernel<128, true>), grid, block, 0, st, p);
  } else if (head_size == 64) {
    hipLaunchKernelGGL((chunkwrite::pa_cache_chunks_kernel<64, false>), grid, block, 0, st, p);
  } else {
    hipLaunchKernelGGL((chunkwrite::pa_cache_chunks_kernel<128, false>), grid, block, 0, st, p);
  }
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) return hip_fail(e, "reshape_and_cache_chunks launch");
  return VMI_OK;
}

}  // namespace vmi

extern "C" int vmi_reshape_and_cache_chunks_f16(
    const void* key, const void* value, void* key_cache, void* value_cache,
    int32_t num_tokens, int32_t num_kv_heads, int32_t head_size,
    const int32_t* block_tables, const int32_t* seq_lens, const int32_t* cu_q_lens,
    int32_t num_seqs, int32_t max_q_len, int32_t block_size, int32_t x, int32_t max_num_blocks_per_seq, int32_t num_blocks,
    int64_t key_stride, int64_t value_stride, int64_t kv_block_stride, int64_t kv_head_stride, int32_t device, void* stream) {
  return vmi::launch_cache_chunks(key, value, key_cache, value_cache, num_tokens, num_kv_heads, head_size, block_tables, seq_lens,
                                  cu_q_lens, num_seqs, max_q_len, block_size, x, max_num_blocks_per_seq, num_blocks, key_stride,
                                  value_stride, kv_block_stride, kv_head_stride, device, stream, false, 1.0f);
}

extern "C" int vmi_reshape_and_cache_chunks_fp8(
    const void* key, const void* value, void* key_cache, void* value_cache,
    int32_t num_tokens, int32_t num_kv_heads, int32_t head_size,
    const int32_t* block_tables, const int32_t* seq_lens, const int32_t* cu_q_lens,
    int32_t num_seqs, int32_t max_q_len, int32_t block_size, int32_t x, int32_t max_num_blocks_per_seq, int32_t num_blocks,
    int64_t key_stride, int64_t value_stride, int64_t kv_block_stride, int64_t kv_head_stride, int32_t device, void* stream,
    float kv_scale) {
  return vmi::launch_cache_chunks(key, value, key_cache, value_cache, num_tokens, num_kv_heads, head_size, block_tables, seq_lens,
                                  cu_q_lens, num_seqs, max_q_len, block_size, x, max_num_blocks_per_seq, num_blocks, key_stride,
                                  value_stride, kv_block_stride, kv_head_stride, device, stream, true, kv_scale);
}
