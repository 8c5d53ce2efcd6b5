// pa_prefill.hip — launcher and C-ABI entries of the tiled causal prefill attention (kernels: pa_prefill.hpp over fp16 pages,
// pa_prefill_fp8.hpp over fp8-E4M3 pages).
// One launch serves every sequence of the call: plain prefill (seq_len == q_len), a chunk over a cached context
// (seq_len > q_len) and single decode rows alike.  The lengths live on the device, so the grid is sized from the host's
// bounds (num_seqs, max_q_len, num_heads) and surplus workgroups leave at once.
#include "pa_prefill.hpp"
#include "pa_prefill_fp8.hpp"

#include "pa_host.hpp"
#include "vmi_paged_attention.h"

namespace vmi {

static int launch_pa_prefill(void* out, const void* query, const void* key_cache, const void* value_cache,
                             int32_t num_tokens, int32_t num_heads, int32_t head_size, int32_t num_kv_heads, float scale,
                             const int32_t* block_tables, const int32_t* seq_lens, const int32_t* cu_q_lens,
                             int32_t num_seqs, int32_t max_q_len, int32_t block_size, int32_t max_num_blocks_per_seq,
                             int64_t q_stride, int64_t kv_block_stride, int64_t kv_head_stride, int32_t device,
                             void* stream, bool fp8, float kv_scale) {
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
  const int64_t kv_mask = fp8 ? 15 : 7;   // 16 bytes in cache elements
  if (!aligned16(query) || !aligned16(key_cache) || !aligned16(value_cache) || (reinterpret_cast<uintptr_t>(out) & 7u) ||
      (q_stride & 7) || (kv_block_stride & kv_mask) || (kv_head_stride & kv_mask))
    return fail(VMI_E_ALIGNMENT, "paged_attention_prefill: query/key_cache/value_cache and their strides must be 16-byte "
                "aligned (q_stride=%lld kv_block_stride=%lld kv_head_stride=%lld)", (long long)q_stride,
                (long long)kv_block_stride, (long long)kv_head_stride);
  if (empty || max_q_len == 0) return VMI_OK;
  const int64_t groups = ((int64_t)max_q_len + prefill::ROWS - 1) / prefill::ROWS;
  const int64_t wgs = groups * num_seqs * num_heads;
  if ((int64_t)num_seqs * num_heads >= (1ll << 31) || wgs >= (1ll << 31))
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
  };

  DeviceGuard guard(device);
  if (guard.err != hipSuccess) return hip_fail(guard.err, "paged_attention_prefill: hipSetDevice");
  const dim3 grid((unsigned)wgs), block(prefill::WAVES * 64);
  if (fp8) {
    prefill::ParamsFp8 p;
    fill(p);
    p.scale_log2e = (scale * kv_scale) * 1.4426950408889634f;   // K's kv_scale rides in the score scale (x 1.0f is exact)
    p.kv_scale = kv_scale;                                       // V's in the final kv_scale / sum
    if (head_size == 64)
      hipLaunchKernelGGL(prefill::pa_prefill_fp8_kernel<64>, grid, block, 0, static_cast<hipStream_t>(stream), p);
    else
      hipLaunchKernelGGL(prefill::pa_prefill_fp8_kernel<128>, grid, block, 0, static_cast<hipStream_t>(stream), p);
  } else {
    prefill::Params p;
    fill(p);
    p.scale_log2e = scale * 1.4426950408889634f;
    if (head_size == 64)
      hipLaunchKernelGGL(prefill::pa_prefill_kernel<64>, grid, block, 0, static_cast<hipStream_t>(stream), p);
    else
      hipLaunchKernelGGL(prefill::pa_prefill_kernel<128>, grid, block, 0, static_cast<hipStream_t>(stream), p);
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
