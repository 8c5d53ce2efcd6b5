"""Python operator surface of the MI355X paged-attention decode path.

Mirrors, name for name and argument for argument, what the reference's pybind module
`paged_attention_cuda` exports and its Python stack calls:

  paged_attention_v1(...18 positional args...)      paged_attention_cuda.cpp:7-25,:52 ;
                                                    call site vllmini/model/gpt2.py:94-113
  cache_ops.reshape_and_cache(...7 positional...)   cache_kernels.h:11-14 ; paged_attention_cuda.cpp:58 ;
                                                    call site vllmini/model/gpt2.py:81-89

Each function reads sizes and strides off the tensors at the same places the reference
launchers do (attention_kernels.cu:701-707, cache_kernels.cu:265-272) and forwards raw device
pointers to the C-ABI (include/vmi_paged_attention.h) on torch's CURRENT stream, without
synchronising — same async contract as the reference (attention_kernels.cu:736-737).

Error behaviour: the reference raises RuntimeError through TORCH_CHECK for an unsupported
head size / block size / dtype / kv-cache dtype (attention_kernels.cu:764, 801; quant_utils.cuh:538,
564) and validates nothing else.  Here the same cases raise RuntimeError with the same message
stem, and malformed shapes/dtypes/devices (undefined behaviour in the reference) raise too.

There is no CPU or torch fallback: tensors must live on a HIP device and the HIP library must
be loadable, otherwise these functions raise.
"""
from __future__ import annotations

from typing import Optional

import torch

from . import _lib

__all__ = [
    "paged_attention_v1",
    "paged_attention_v2",
    "paged_attention_prefill",
    "reshape_and_cache",
    "reshape_and_cache_chunks",
    "pick_variant",
    "workspace_for",
    "prefill_workspace_for",
    "reset_workspaces",
    "variant_fits",
    "variant_names",
    "is_split",
    "check_workspaces",
]

_SUPPORTED_KV_CACHE_DTYPES = ("auto",)
_FP8_KV_CACHE_DTYPES = ("fp8", "fp8_e4m3", "fp8_e5m2")


def _ptr(t: Optional[torch.Tensor]) -> Optional[int]:
    return None if t is None else t.data_ptr()




def _check_kv_cache_dtype(kv_cache_dtype: str) -> int:
    """-> 0 for 16-bit caches ("auto"), 1 when the caches hold fp8 E4M3 bytes, 2 for fp8 E5M2 bytes.  The reference maps
    "fp8" and "fp8_e4m3" to E4M3 and "fp8_e5m2" to E5M2 (quant_utils.cuh:529-566); both are built here (the reference's
    own build never defines ENABLE_FP8, so its fp8 path is assert(false) — paged_attention_ext/setup.py:30-45 — and its
    source is the spec)."""
    if kv_cache_dtype in _SUPPORTED_KV_CACHE_DTYPES:
        return 0
    if kv_cache_dtype in ("fp8", "fp8_e4m3"):
        return 1
    if kv_cache_dtype == "fp8_e5m2":
        return 2
    raise RuntimeError(f"Unsupported data type of kv cache: {kv_cache_dtype}")


def _check_fp8_cache_dtype(fp8: int, key_cache: torch.Tensor, value_cache: torch.Tensor, kv_cache_dtype: str) -> None:
    ok = (torch.uint8, torch.float8_e5m2 if fp8 == 2 else torch.float8_e4m3fn)
    if key_cache.dtype not in ok or value_cache.dtype not in ok:
        raise RuntimeError(f"key_cache/value_cache must be uint8 (or {ok[1]}) for kv_cache_dtype='{kv_cache_dtype}'")


def _check_device(name: str, t: torch.Tensor, device: torch.device) -> None:
    if not t.is_cuda:
        raise RuntimeError(
            f"{name} must be a HIP device tensor (got {t.device}); this operator has no CPU path")
    if t.device != device:
        raise RuntimeError(f"{name} is on {t.device}, expected {device}")


def _raise_native(code: int) -> None:
    raise RuntimeError(f"{_lib.last_error()} (vmi code {code})")


_extras = _lib.require_extras      # the active library if it holds the out-of-scope operators, else RuntimeError("<what>: not in this build ...")


_raw_stream = getattr(torch._C, "_cuda_getCurrentRawStream", None)


def _stream_of(index: int) -> int:
    """The current HIP stream of device `index` as an integer handle (what the C-ABI takes)."""
    if _raw_stream is not None:
        return _raw_stream(index)
    return torch.cuda.current_stream(index).cuda_stream


def _on(name: str, t: torch.Tensor, index: int, dev) -> None:
    """`t` lives on HIP device `index` (there is no CPU path)."""
    if t.get_device() != index:
        _check_device(name, t, dev)      # raises with the full message


def _pa_common(out, query, key_cache, value_cache, num_kv_heads, scale, block_tables, seq_lens,
               block_size, max_seq_len, alibi_slopes, kv_cache_dtype, kv_scale, tp_rank,
               blocksparse_local_blocks, blocksparse_vert_stride, blocksparse_block_size,
               blocksparse_head_sliding_step):
    """Validate and flatten the 18 reference arguments into the C-ABI argument tuple.

    Runs on every call (a decode loop hands in fresh views each step, so nothing about a tensor can be remembered
    safely); written to touch each tensor as few times as possible — shape and stride tuples are fetched once and
    compared as tuples: 11.7 -> about 5 us per call on the GPU box's host (profiles/r02_host_overhead.md)."""
    qs = query.shape
    if len(qs) != 3:
        raise RuntimeError(f"query must be [num_seqs, num_heads, head_size], got {tuple(qs)}")
    qdt = query.dtype
    if qdt not in (torch.float16, torch.bfloat16, torch.float32):
        # the reference dispatches float / half / bf16 (quant_utils.cuh:529-566); its callers only use half
        # (gpt2.py, scheduler.py:13)
        raise RuntimeError(f"Unsupported input type of paged attention: {qdt}")
    fp8 = _check_kv_cache_dtype(kv_cache_dtype)
    f32 = qdt == torch.float32          # x = 4 cache layout, plain kernels: v1 over float32 caches only
    sparse = int(blocksparse_vert_stride) > 1
    if f32 and (fp8 or sparse):
        raise RuntimeError("Unsupported input type of paged attention: torch.float32 is built for kv_cache_dtype='auto' "
                           "without block-sparse attention")
    if sparse:          # is_block_sparse, attention_kernels.cu:822 — kernels of their own
        if fp8:
            raise RuntimeError("block-sparse paged attention (blocksparse_vert_stride > 1) is built for "
                               "kv_cache_dtype='auto' (fp16 / bf16 caches) only")
        if int(blocksparse_block_size) <= 0:
            raise RuntimeError(f"blocksparse_block_size must be positive, got {blocksparse_block_size}")
    index = query.get_device()
    dev = query.device
    if index < 0:
        _check_device("query", query, dev)
    _on("out", out, index, dev)
    _on("key_cache", key_cache, index, dev)
    _on("value_cache", value_cache, index, dev)
    _on("block_tables", block_tables, index, dev)
    _on("seq_lens", seq_lens, index, dev)
    kdt, vdt = key_cache.dtype, value_cache.dtype
    if fp8:
        _check_fp8_cache_dtype(fp8, key_cache, value_cache, kv_cache_dtype)
    elif kdt != qdt or vdt != qdt:
        raise RuntimeError(f"key_cache/value_cache must be {qdt} for kv_cache_dtype='auto'")
    if out.dtype != qdt:
        raise RuntimeError(f"out must be {qdt}, got {out.dtype}")
    if block_tables.dtype != torch.int32 or seq_lens.dtype != torch.int32:
        raise RuntimeError("block_tables and seq_lens must be int32")

    num_seqs, num_heads, head_size = qs  # attention_kernels.cu:701-703
    ks, vs = key_cache.shape, value_cache.shape
    if len(ks) != 5 or len(vs) != 4:
        raise RuntimeError("key_cache must be [num_blocks, num_kv_heads, head_size/x, block_size, x] "
                           "and value_cache [num_blocks, num_kv_heads, head_size, block_size]")
    x = ks[4]
    want_x = 16 if fp8 else (4 if f32 else 8)                     # x = 16 / sizeof(cache_t), attention_kernels.cu:200
    if x != want_x:
        raise RuntimeError(f"key_cache innermost dimension must be {want_x} (16 bytes per chunk), got {x}")
    block_size = int(block_size)
    if ks[3] != block_size or vs[3] != block_size:
        raise RuntimeError(f"block_size={block_size} does not match the cache tensors "
                           f"({ks[3]}, {vs[3]})")
    if ks[2] * x != head_size or vs[2] != head_size:
        raise RuntimeError("cache head_size does not match query head_size")
    num_kv_heads = int(num_kv_heads)
    if ks[1] != num_kv_heads or vs[1] != num_kv_heads:
        raise RuntimeError("cache num_kv_heads does not match num_kv_heads argument")
    qst = query.stride()
    if qst[2] != 1 or qst[1] != head_size:
        raise RuntimeError("query must be contiguous in its last two dimensions")
    kst, vst = key_cache.stride(), value_cache.stride()
    tile = head_size * block_size
    # every (block, head) tile dense; blocks and heads may be strided (size-1 dimensions carry no layout)
    if (kst[4] != 1 and x != 1) or (kst[3] != x and block_size != 1) or (kst[2] != block_size * x and ks[2] != 1) or \
            (kst[1] != tile and ks[1] != 1) or (vst[3] != 1 and block_size != 1) or \
            (vst[2] != block_size and head_size != 1) or (vst[1] != tile and vs[1] != 1):
        raise RuntimeError("each cache block must be dense")
    if vst[0] != kst[0] or vst[1] != kst[1]:
        # the reference applies key_cache's strides to both tensors (attention_kernels.cu:706-707)
        raise RuntimeError("key_cache and value_cache must have identical block/head strides")
    if not out.is_contiguous() or out.numel() != num_seqs * num_heads * head_size:
        # reference tests pass out as [S, H, 1, D] (tests/kernels/paged_attention.py:114)
        raise RuntimeError("out must be contiguous with num_seqs*num_heads*head_size elements")
    ts, tst = block_tables.shape, block_tables.stride()
    if len(ts) != 2 or ts[0] != num_seqs or tst[1] != 1:
        raise RuntimeError("block_tables must be [num_seqs, max_num_blocks_per_seq] with unit inner stride")
    if tst[0] != ts[1] and num_seqs > 1:
        raise RuntimeError("block_tables must be row-contiguous")
    ls = seq_lens.shape
    if len(ls) != 1 or ls[0] != num_seqs or not seq_lens.is_contiguous():
        raise RuntimeError("seq_lens must be a contiguous [num_seqs] tensor")
    alibi_ptr = None
    if alibi_slopes is not None:
        _check_device("alibi_slopes", alibi_slopes, dev)
        if alibi_slopes.dtype != torch.float32 or alibi_slopes.numel() != num_heads or \
                not alibi_slopes.is_contiguous():
            raise RuntimeError("alibi_slopes must be a contiguous float32 [num_heads] tensor")
        alibi_ptr = alibi_slopes.data_ptr()

    return (
        out.data_ptr(), query.data_ptr(), key_cache.data_ptr(), value_cache.data_ptr(),
        num_seqs, num_heads, head_size, num_kv_heads, float(scale),
        block_tables.data_ptr(), seq_lens.data_ptr(),
        block_size, int(max_seq_len), ts[1],   # attention_kernels.cu:704
        alibi_ptr,
        qst[0], kst[0], kst[1],  # :705-707
        index, _stream_of(index),
    )


# ---- the wrapper-owned workspace of paged_attention_v1 (ownership row: "if a split-KV path needs
# scratch, the Python wrapper allocates it with torch on the same stream").  One tensor per (device, stream): launches on
# one stream are ordered, so they can share it; launches on different streams get one each.  The native library keeps
# nothing — the pointer travels with every call.  Under stream capture nothing is allocated (an allocation would belong
# to the graph's private pool): a stream that has no workspace yet captures today's kernels; call workspace_for() before
# capturing to let the graph hold the split kernels.
_WS: dict = {}
_WS_HEAD_SIZES = (64, 128)
_ws_enabled = True


def _capturing() -> bool:
    try:
        return torch.cuda.is_current_stream_capturing()
    except Exception:
        return False


def workspace_for(index: int, stream: Optional[int] = None, create: bool = True) -> Optional[torch.Tensor]:
    """The workspace the operators hand to the library for launches on (device `index`, its current stream) — allocated
    and zeroed on first use (never during stream capture)."""
    if stream is None:
        stream = _stream_of(index)
    ws = _WS.get((index, stream))
    if ws is None and create and not _capturing():
        lib = _lib.load()
        nbytes = max(int(lib.vmi_paged_attention_v1_workspace_bytes(1, 1, d, 16)) for d in _WS_HEAD_SIZES)
        ws = torch.zeros(nbytes, dtype=torch.uint8, device=torch.device("cuda", index))   # zeroed on the current stream
        _WS[(index, stream)] = ws
    return ws


def reset_workspaces(index: Optional[int] = None) -> None:
    """Zero the control words of every cached workspace (of device `index`): after a launch that died in flight."""
    lib = _lib.load()
    for (i, st), ws in list(_WS.items()):
        if index is None or i == index:
            rc = lib.vmi_paged_attention_v1_workspace_reset(ws.data_ptr(), ws.numel(), i, st)
            if rc != 0:
                _raise_native(rc)


def workspace_status(index: int, stream: Optional[int] = None) -> int:
    """Polls that gave up in launches on this workspace (0 on a healthy run).  Synchronises."""
    ws = workspace_for(index, stream, create=False)
    return 0 if ws is None else int(ws[:4].view(torch.int32).item())


def set_workspace_enabled(on: bool) -> bool:
    """Process-wide switch (default on): off = the operators pass no workspace, i.e. yesterday's kernels.  Returns the
    previous setting."""
    global _ws_enabled
    prev, _ws_enabled = _ws_enabled, bool(on)
    return prev


def paged_attention_v1(
    out: torch.Tensor,
    query: torch.Tensor,
    key_cache: torch.Tensor,
    value_cache: torch.Tensor,
    num_kv_heads: int,
    scale: float,
    block_tables: torch.Tensor,
    seq_lens: torch.Tensor,
    block_size: int,
    max_seq_len: int,
    alibi_slopes: Optional[torch.Tensor],
    kv_cache_dtype: str,
    kv_scale: float,
    tp_rank: int = 0,
    blocksparse_local_blocks: int = 0,
    blocksparse_vert_stride: int = 1,
    blocksparse_block_size: int = 1,
    blocksparse_head_sliding_step: int = 0,
    *,
    _variant: int = 0,
) -> None:
    """Decode attention over the paged KV cache; writes `out` in place, returns None.

    Reference: attention_kernels.cu:805-826 (host), :86-496 (kernel).  `_variant` (keyword only,
    not part of the reference surface) forces a work decomposition for tuning/tests.
    """
    args = _pa_common(out, query, key_cache, value_cache, num_kv_heads, scale, block_tables,
                      seq_lens, block_size, max_seq_len, alibi_slopes, kv_cache_dtype, kv_scale,
                      tp_rank, blocksparse_local_blocks, blocksparse_vert_stride,
                      blocksparse_block_size, blocksparse_head_sliding_step)
    lib = _lib.load()
    # (the first five branches are the out-of-scope corners of the reference's dispatch: they exist in the extras library
    #  only, include/vmi_paged_attention_extras.h — on the product library _extras raises before any entry is touched)
    if query.dtype == torch.float32:               # the (float, float) dispatch branch: plain kernels, no variants
        if _variant:
            raise RuntimeError("_variant does not apply to float32 tensors")
        rc = _extras("paged_attention_v1 over float32 tensors").vmi_paged_attention_v1_f32(*args)
    elif int(blocksparse_vert_stride) > 1:           # block-sparse attention: its own kernels, no tuning variants
        if _variant:
            raise RuntimeError("_variant does not apply to block-sparse attention")
        rc = _extras("paged_attention_v1 with block-sparse attention").vmi_paged_attention_v1_blocksparse(
            *args, int(query.dtype == torch.bfloat16), int(tp_rank), int(blocksparse_local_blocks),
            int(blocksparse_vert_stride), int(blocksparse_block_size), int(blocksparse_head_sliding_step))
    elif _check_kv_cache_dtype(kv_cache_dtype) == 2:   # fp8 E5M2 cache
        rc = _extras("paged_attention_v1 over fp8-E5M2 pages").vmi_paged_attention_v1_fp8_e5m2(
            *args, float(kv_scale), int(_variant), int(query.dtype == torch.bfloat16))
    elif _check_kv_cache_dtype(kv_cache_dtype):      # fp8 E4M3 cache, float16 or bfloat16 query
        ws = workspace_for(args[18], args[19]) if (_ws_enabled and query.dtype == torch.float16 and args[6] in _WS_HEAD_SIZES) else None
        if ws is not None:
            rc = lib.vmi_paged_attention_v1_fp8_ws(*args, float(kv_scale), ws.data_ptr(), ws.numel(), int(_variant))
        else:
            fn = _extras("paged_attention_v1 over bfloat16 tensors").vmi_paged_attention_v1_fp8_bf16 \
                if query.dtype == torch.bfloat16 else lib.vmi_paged_attention_v1_fp8
            rc = fn(*args, float(kv_scale), int(_variant))
    elif query.dtype == torch.bfloat16:
        rc = _extras("paged_attention_v1 over bfloat16 tensors").vmi_paged_attention_v1_bf16(*args, int(_variant))
    else:
        ws = workspace_for(args[18], args[19]) if (_ws_enabled and args[6] in _WS_HEAD_SIZES) else None
        if ws is not None:
            rc = lib.vmi_paged_attention_v1_f16_ws(*args, ws.data_ptr(), ws.numel(), int(_variant))
        elif _variant:
            rc = lib.vmi_paged_attention_v1_f16_variant(*args, int(_variant))
        else:
            rc = lib.vmi_paged_attention_v1_f16(*args)
    if rc != 0:
        _raise_native(rc)
    return None


def paged_attention_v1_append(
    out: torch.Tensor,
    query: torch.Tensor,
    key: torch.Tensor,
    value: torch.Tensor,
    key_cache: torch.Tensor,
    value_cache: torch.Tensor,
    num_kv_heads: int,
    scale: float,
    block_tables: torch.Tensor,
    seq_lens: torch.Tensor,
    block_size: int,
    max_seq_len: int,
    alibi_slopes: Optional[torch.Tensor] = None,
    kv_cache_dtype: str = "auto",
    kv_scale: float = 1.0,
    *,
    _variant: int = 0,
    write_cache: bool = True,
) -> None:
    """Fused decode step (extension, include/vmi_paged_attention.h: vmi_paged_attention_v1_append_*):

        cache_ops.reshape_and_cache(key, value, key_cache, value_cache, slot_of_position(seq_lens-1), ...)
        paged_attention_v1(out, query, key_cache, value_cache, ...)

    in one launch — the pair the reference issues per layer (gpt2.py:87-112).  `seq_lens` already counts this
    step's token (as in gpt2.py:99-104); its slot is derived from the block table, so no slot_mapping is passed.
    Caches and `out` are bit-identical to the two-op sequence (tests/test_parity_gpu.py).

    write_cache=False (vmi_paged_attention_v1_newest_f16): the same attention — the newest token is read from key / value —
    WITHOUT the cache write; the caller stores the rows later (one reshape_and_cache for all the layers of a token:
    GPT2PagedDecoder(deferred_scatter=True)).  `out` is unchanged by it, the caches are not touched.
    """
    if _check_kv_cache_dtype(kv_cache_dtype):
        raise RuntimeError("paged_attention_v1_append is not built for an fp8 KV cache")
    if query.dtype == torch.float32:
        raise RuntimeError("paged_attention_v1_append is not built for float32 tensors")
    args = _pa_common(out, query, key_cache, value_cache, num_kv_heads, scale, block_tables,
                      seq_lens, block_size, max_seq_len, alibi_slopes, kv_cache_dtype, kv_scale, 0, 0, 1, 1, 0)
    num_seqs, _, head_size = (int(s) for s in query.shape)
    for name, t in (("key", key), ("value", value)):
        _check_device(name, t, query.device)
        if t.dtype != query.dtype:
            raise RuntimeError(f"{name} must be {query.dtype}, got {t.dtype}")
        if t.dim() != 3 or tuple(int(x) for x in t.shape) != (num_seqs, int(num_kv_heads), head_size):
            raise RuntimeError(f"{name} must be [num_seqs, num_kv_heads, head_size], got {tuple(t.shape)}")
        if t.stride(2) != 1 or t.stride(1) != head_size:
            raise RuntimeError(f"{name} must be contiguous in its last two dimensions")
    if not write_cache and query.dtype != torch.float16:
        raise RuntimeError("paged_attention_v1_append(write_cache=False) is built for float16 tensors")
    fn = _extras("paged_attention_v1_append over bfloat16 tensors").vmi_paged_attention_v1_append_bf16 \
        if query.dtype == torch.bfloat16 else (_lib.load().vmi_paged_attention_v1_append_f16 if write_cache else
                                               _lib.load().vmi_paged_attention_v1_newest_f16)
    rc = fn(*args, key.data_ptr(), value.data_ptr(), int(key.stride(0)), int(value.stride(0)), int(_variant))
    if rc != 0:
        _raise_native(rc)
    return None


def paged_attention_v2(
    out: torch.Tensor,
    exp_sums: torch.Tensor,
    max_logits: torch.Tensor,
    tmp_out: torch.Tensor,
    query: torch.Tensor,
    key_cache: torch.Tensor,
    value_cache: torch.Tensor,
    num_kv_heads: int,
    scale: float,
    block_tables: torch.Tensor,
    seq_lens: torch.Tensor,
    block_size: int,
    max_seq_len: int,
    alibi_slopes: Optional[torch.Tensor],
    kv_cache_dtype: str,
    kv_scale: float,
    tp_rank: int = 0,
    blocksparse_local_blocks: int = 0,
    blocksparse_vert_stride: int = 1,
    blocksparse_block_size: int = 1,
    blocksparse_head_sliding_step: int = 0,
    *,
    _variant: int = 0,
) -> None:
    """Split-KV decode attention (512-token partitions + merge); writes out/exp_sums/max_logits/tmp_out.

    Reference: paged_attention_cuda.cpp:27-47 (signature), attention_kernels.cu:966-990 (host),
    :529-562 + :564-669 (kernels).  The reference exports it but no Python caller exists
    (SURVEY.md §2 #7); it is the right operator when num_seqs*num_heads is far below the CU count.
    """
    fp8 = _check_kv_cache_dtype(kv_cache_dtype)
    if query.dtype == torch.float32:
        raise RuntimeError("Unsupported input type of paged attention: torch.float32 is built for paged_attention_v1 only")
    args = _pa_common(out, query, key_cache, value_cache, num_kv_heads, scale, block_tables,
                      seq_lens, block_size, max_seq_len, alibi_slopes, kv_cache_dtype, kv_scale,
                      tp_rank, blocksparse_local_blocks, blocksparse_vert_stride,
                      blocksparse_block_size, blocksparse_head_sliding_step)
    num_seqs, num_heads, head_size = (int(x) for x in query.shape)
    parts = (int(max_seq_len) + 511) // 512                       # attention_kernels.cu:885
    dev = query.device
    for name, t, dt, shape in (("exp_sums", exp_sums, torch.float32, (num_seqs, num_heads, parts)),
                               ("max_logits", max_logits, torch.float32, (num_seqs, num_heads, parts)),
                               ("tmp_out", tmp_out, query.dtype, (num_seqs, num_heads, parts, head_size))):
        _check_device(name, t, dev)
        if t.dtype != dt or tuple(t.shape) != shape or not t.is_contiguous():
            raise RuntimeError(f"{name} must be a contiguous {dt} tensor of shape {shape} "
                               f"(max_num_partitions = ceil(max_seq_len/512) = {parts})")
    if int(blocksparse_vert_stride) > 1:
        if _variant:
            raise RuntimeError("_variant does not apply to block-sparse attention")
        rc = _extras("paged_attention_v2 with block-sparse attention").vmi_paged_attention_v2_blocksparse(
            args[0], exp_sums.data_ptr(), max_logits.data_ptr(), tmp_out.data_ptr(), *args[1:],
            int(query.dtype == torch.bfloat16), int(tp_rank), int(blocksparse_local_blocks),
            int(blocksparse_vert_stride), int(blocksparse_block_size), int(blocksparse_head_sliding_step))
    elif fp8 and query.dtype == torch.bfloat16:
        rc = _extras("paged_attention_v2 over bfloat16 tensors").vmi_paged_attention_v2_fp8_bf16(
            args[0], exp_sums.data_ptr(), max_logits.data_ptr(), tmp_out.data_ptr(), *args[1:], float(kv_scale), int(_variant),
            int(fp8 == 2))
    elif fp8:
        fn8 = _extras("paged_attention_v2 over fp8-E5M2 pages").vmi_paged_attention_v2_fp8_e5m2 if fp8 == 2 else \
            _lib.load().vmi_paged_attention_v2_fp8
        rc = fn8(args[0], exp_sums.data_ptr(), max_logits.data_ptr(), tmp_out.data_ptr(), *args[1:],
                 float(kv_scale), int(_variant))
    else:
        fn = _extras("paged_attention_v2 over bfloat16 tensors").vmi_paged_attention_v2_bf16 if query.dtype == torch.bfloat16 else \
            _lib.load().vmi_paged_attention_v2_f16
        rc = fn(args[0], exp_sums.data_ptr(), max_logits.data_ptr(), tmp_out.data_ptr(), *args[1:], int(_variant))
    if rc != 0:
        _raise_native(rc)
    return None


# ---- the wrapper-owned workspace of the context-split prefill: the partition kernels' fp32 partials.  Per (device, stream)
# like _WS, grown on demand to the plan's bytes, never zeroed (every word the merge reads was written by the same call) and
# never allocated during stream capture.
_PWS: dict = {}
_NUM_CUS: dict = {}


def prefill_workspace_for(index: int, nbytes: int, stream: Optional[int] = None) -> Optional[torch.Tensor]:
    """The uint8 tensor paged_attention_prefill hands to the split launch on (device `index`, its current stream), at least
    `nbytes` long — None when it would have to be allocated during stream capture."""
    if stream is None:
        stream = _stream_of(index)
    ws = _PWS.get((index, stream))
    if ws is None or ws.numel() < nbytes:
        if _capturing():
            return None
        ws = _PWS[(index, stream)] = torch.empty(int(nbytes), dtype=torch.uint8, device=torch.device("cuda", index))
    return ws


def prefill_split_plan(num_tokens: int, num_heads: int, head_size: int, num_seqs: int, max_q_len: int, max_seq_len: int,
                       num_cus: int = 0, partition_tokens: int = 0) -> tuple:
    """(partition_tokens, num_partitions, workspace_bytes) of the context-split prefill launch: the library's rule
    (partition_tokens=0) or a forced partition size.  num_cus=0 asks the current device.  One partition = do not split."""
    import ctypes

    pt, parts, nbytes = ctypes.c_int32(), ctypes.c_int32(), ctypes.c_int64()
    rc = _lib.load().vmi_paged_attention_prefill_split_plan(int(num_tokens), int(num_heads), int(head_size), int(num_seqs),
                                                            int(max_q_len), int(max_seq_len), int(num_cus), int(partition_tokens),
                                                            ctypes.byref(pt), ctypes.byref(parts), ctypes.byref(nbytes))
    if rc != 0:
        _raise_native(rc)
    return pt.value, parts.value, nbytes.value


# cooperative=None, read off profiles/prefill_coop.md section 2 (MI355X, 256 CUs): the cooperative launch is taken for chunks
# of at most 16 rows from this max_seq_len on (the smallest measured context from which it wins beyond the ranges' overlap,
# in both page formats) ...
PREFILL_COOP_MIN_CONTEXT = 512
# ... while the grid has at most this many workgroups per CU, as (numerator, denominator): the fullest measured grid on which it
# wins in both formats.  At 3 per CU the float16 launch is bound by memory bandwidth and the form gains nothing there.
PREFILL_COOP_MAX_WGS_PER_CU = (3, 2)


def _num_cus(index: int) -> int:
    cus = _NUM_CUS.get(index)
    if cus is None:
        cus = _NUM_CUS[index] = int(torch.cuda.get_device_properties(index).multi_processor_count)
    return cus


def prefill_cooperative_for(max_q_len: int, max_seq_len: Optional[int], num_seqs: int, num_heads: int, num_cus: int) -> bool:
    """What paged_attention_prefill(cooperative=None) resolves to, from host-known bounds alone: the cooperative launch when
    no sequence has more than 16 rows (every workgroup then holds one live tile), max_seq_len is given and at least
    PREFILL_COOP_MIN_CONTEXT, and the num_seqs * num_heads workgroups leave the chip's SIMDs underfilled
    (PREFILL_COOP_MAX_WGS_PER_CU).  Measurements: profiles/prefill_coop.md."""
    num, den = PREFILL_COOP_MAX_WGS_PER_CU
    return max_seq_len is not None and 0 < int(max_q_len) <= 16 and int(max_seq_len) >= PREFILL_COOP_MIN_CONTEXT and \
        den * int(num_seqs) * int(num_heads) <= num * int(num_cus)


def prefill_gqa_plan(num_tokens: int, num_heads: int, head_size: int, num_seqs: int, max_q_len: int, max_seq_len: int,
                     num_kv_heads: int, num_cus: int = 0, partition_tokens: int = 0) -> tuple:
    """prefill_split_plan for the head-packed launch: the same rule and workspace bytes, counted on the packed grid of
    ceil(max_q_len / (16 / G)) * num_seqs * num_kv_heads workgroups, G = num_heads / num_kv_heads."""
    import ctypes

    pt, parts, nbytes = ctypes.c_int32(), ctypes.c_int32(), ctypes.c_int64()
    rc = _lib.load().vmi_paged_attention_prefill_gqa_plan(int(num_tokens), int(num_heads), int(head_size), int(num_seqs),
                                                          int(max_q_len), int(max_seq_len), int(num_cus), int(partition_tokens),
                                                          ctypes.byref(pt), ctypes.byref(parts), ctypes.byref(nbytes),
                                                          int(num_kv_heads))
    if rc != 0:
        _raise_native(rc)
    return pt.value, parts.value, nbytes.value


def _prefill_rel_plan(num_tokens: int, num_heads: int, head_size: int, num_seqs: int, max_q_len: int, max_seq_len: int,
                      num_cus: int, partition_tokens: int, num_kv_heads: int, sliding_window: int, form: int) -> tuple:
    """The plan of the ALiBi / sliding-window launch: prefill_split_plan (form 2: prefill_gqa_plan) on a context of
    min(max_seq_len, sliding_window + max_q_len - 1) tokens — no row sees more.  sliding_window 0: no window."""
    import ctypes

    pt, parts, nbytes = ctypes.c_int32(), ctypes.c_int32(), ctypes.c_int64()
    rc = _lib.load().vmi_paged_attention_prefill_rel_plan(int(num_tokens), int(num_heads), int(head_size), int(num_seqs),
                                                          int(max_q_len), int(max_seq_len), int(num_cus), int(partition_tokens),
                                                          ctypes.byref(pt), ctypes.byref(parts), ctypes.byref(nbytes),
                                                          int(num_kv_heads), int(sliding_window), int(form))
    if rc != 0:
        _raise_native(rc)
    return pt.value, parts.value, nbytes.value


PREFILL_PACK_RATIOS = (2, 4, 8, 16)


def _pack_ratio(num_heads: int, num_kv_heads: int) -> int:
    """num_heads / num_kv_heads when the head-packed form is built for it, else 0."""
    num_heads, num_kv_heads = int(num_heads), int(num_kv_heads)
    g = num_heads // num_kv_heads if num_kv_heads > 0 and num_heads % num_kv_heads == 0 else 0
    return g if g in PREFILL_PACK_RATIOS else 0


# pack_heads=None, read off profiles/prefill_gqa.md (MI355X, 256 CUs; 32/8 and 64/8 heads x 128, both page formats).  Chunks of
# at most this many rows leave columns of a one-head tile empty, and the packed launch won in every such cell measured, from
# 8 to 4 096 workgroups a partition ...
PREFILL_PACK_MAX_ROWS = 4
# ... while a 16-row chunk fills a one-head tile: no trip is saved, and the packed launch won only where its grid of
# tiles * num_seqs * num_kv_heads workgroups was at most one per CU (128 and 256 workgroups; at 2 048 and 4 096 it lost).
# Chunks of 5 - 15 rows on fuller grids, and longer chunks, were not measured: they stay with the other launches.
PREFILL_PACK_MAX_ROWS_UNDERFILLED = 16


def prefill_pack_heads_for(max_q_len: int, num_heads: int, num_kv_heads: int, max_seq_len: Optional[int] = None,
                           num_seqs: int = 0, num_cus: int = 0) -> bool:
    """What paged_attention_prefill(pack_heads=None) resolves to, from host-known bounds alone: the head-packed launch when the
    ratio is one it is built for, max_seq_len is given (every measured launch had it), and the chunks are at most
    PREFILL_PACK_MAX_ROWS rows — or at most PREFILL_PACK_MAX_ROWS_UNDERFILLED with no more than one packed workgroup per CU.
    Measurements: profiles/prefill_gqa.md."""
    g, q = _pack_ratio(num_heads, num_kv_heads), int(max_q_len)
    if not g or max_seq_len is None or q <= 0:
        return False
    if q <= PREFILL_PACK_MAX_ROWS:
        return True
    tiles = -(-q * g // 16)
    return q <= PREFILL_PACK_MAX_ROWS_UNDERFILLED and 0 < tiles * int(num_seqs) * int(num_kv_heads) <= int(num_cus)


def paged_attention_prefill(
    out: torch.Tensor,
    query: torch.Tensor,
    key_cache: torch.Tensor,
    value_cache: torch.Tensor,
    num_kv_heads: int,
    scale: float,
    block_tables: torch.Tensor,
    seq_lens: torch.Tensor,
    cu_q_lens: torch.Tensor,
    max_q_len: int,
    block_size: int,
    kv_cache_dtype: str = "auto",
    kv_scale: float = 1.0,
    max_seq_len: Optional[int] = None,
    partition_tokens: Optional[int] = None,
    cooperative: Optional[bool] = False,
    pack_heads: Optional[bool] = False,
    shared_prefix_len: Optional[int] = None,
    alibi_slopes: Optional[torch.Tensor] = None,
    sliding_window: Optional[int] = None,
    tree_mask: Optional[torch.Tensor] = None,
) -> None:
    """Tiled causal attention of a chunk of query rows per sequence over the paged cache (extension: the reference runs its
    prefill as eager masked attention, gpt2.py:46-58); writes `out` in place, returns None.

    query / out [num_tokens, num_heads, head_size] float16 (query rows may be strided: the fused projection's views);
    sequence s owns rows cu_q_lens[s] .. cu_q_lens[s+1]-1, which sit at positions seq_lens[s] - q_len .. seq_lens[s] - 1 of the
    blocks in block_tables[s] — their K / V rows are in the cache already (reshape_and_cache first).  seq_lens[s] == q_len is
    a plain prefill, > q_len a chunk over a cached context.  `max_q_len` bounds the q_len of every sequence (host-known: it
    sizes the grid).  Head size 64 / 128, block size 16; pages float16 (kv_cache_dtype "auto", x = 8) or fp8-E4M3 bytes
    ("fp8" / "fp8_e4m3", x = 16, uint8 or float8_e4m3fn tensors whose elements mean fp8 * kv_scale — what reshape_and_cache
    writes); "fp8_e5m2" pages have no prefill kernel (include/vmi_paged_attention.h).

    `max_seq_len` (a host-known bound on seq_lens; None: today's single launch) lets the launch SPLIT OVER THE CONTEXT: few rows
    over a deep cache — a chunk of a long prompt, verification rows, one long sequence — are spread over partitions of the
    context that meet in a wrapper-owned workspace (prefill_workspace_for) and a merge launch.  The library's rule decides
    from the host-known bounds whether and how finely (prefill_split_plan; profiles/prefill_split.md); `partition_tokens` (a
    multiple of 32, needs max_seq_len) forces the size, for tests and tuning.  A sequence longer than max_seq_len writes
    nothing.  Under stream capture with no cached workspace large enough, the single launch is taken.

    `cooperative` picks the COOPERATIVE form of the tile kernels: in a 64-row group with at most 16 live rows (a decode row,
    look-ahead rows, a chunk's tail, a 16-row chunk) the workgroup's four waves share the one tile's context and merge in LDS,
    where the plain form leaves three of them idle; groups with more live rows compute bit for bit what the plain form does.
    False (default): the plain launches.  True: the cooperative ones, split or not as above (without max_seq_len the block
    table's capacity stands in as the bound).  None: the measured rule, prefill_cooperative_for — never without max_seq_len.

    `pack_heads` picks the HEAD-PACKED form for grouped-query attention (num_heads / num_kv_heads in 2, 4, 8, 16; any other
    ratio raises): a tile's 16 columns are (row, query head of one KV head) pairs, so a short chunk — a decode row, look-ahead
    rows — walks its context once per KV head with full tiles, where the other forms walk it once per query head.  False
    (default): the launches above.  True: the packed ones, split or not by max_seq_len / partition_tokens through
    prefill_gqa_plan (without max_seq_len the block table's capacity stands in as the bound); `cooperative` is not consulted,
    the form is cooperative by construction.  None: the measured rule, prefill_pack_heads_for — never without max_seq_len.

    `shared_prefix_len` = P attends a SHARED PROMPT PREFIX once per batch (cascade attention), for a batch whose sequences all
    begin with the same system prompt or few-shot header.  Contract: the first P cached positions of every sequence of the call
    are the same tokens in the same blocks; their block indices are read from ROW 0 of `block_tables` only — the first P / 16
    entries of every other row are never read.  P is a positive multiple of 32, needs `max_seq_len` > P, and `partition_tokens`
    must be None or P: the prefix is partition 0 of the split scheme.  Three launches: prefix tiles of 16 consecutive rows of the
    packed batch x one head walk one copy of the prefix and write partition 0's partials, the partition kernels write every
    sequence's own suffix from partition 1 on — in the form `cooperative` / `pack_heads` choose, as above — and the same merge
    launch folds them.  The result is the unshared call's (same bound); only the route changes.  None (default): every launch
    above, bit for bit.  There is no rule behind None: the library cannot see sharing, the caller says so.  Under stream
    capture with no cached workspace large enough the unshared launch is taken (the per-sequence tables are valid).
    Measured advice (profiles/prefill_prefix.md, MI355X, 256 one-row sequences): it pays for batches of one-row chunks from
    P = 512 on (fp8 pages -16 % there, fp16 from longer prefixes: -29 % / -49 % at P = 2 048); it LOSES 12 - 27 % on chunks of 16 rows
    and more, whose tiles are full already, and 9 - 71 % at P <= 128, where three launches stand against one.

    `alibi_slopes` (a contiguous float32 [num_heads] tensor on the query's device) and `sliding_window` = W (a positive int) add
    the two score terms that are functions of t - pos, in every form above but the shared prefix and over both page formats (the REL
    kernels, csrc/pa_prefill.hpp): the row at cached position pos of head h scores token t as scale * q . k + slopes[h] * (t - pos)
    and attends the tokens pos - W < t <= pos — W of them, itself included; W >= seq_len is plain causal attention.  For fp8 pages
    the ALiBi term is not scaled by kv_scale.  THE WINDOW CONTRACT: with lo = max(0, seq_len - q_len - W + 1), the window start of
    the chunk's first row, blocks that lie wholly below lo are never read — neither their block_tables entries nor their K / V
    bytes, which may hold anything: a caller may free them.  With a window the work is proportional to W: the walk starts at the
    window, the partitions count from lo & ~31, and the split, cooperative and pack rules, the grid and the workspace are taken
    on min(max_seq_len, W + max_q_len - 1) instead of max_seq_len.  Both None (default): every launch above, bit for bit, through
    the same entries and kernels.  Either one together with `shared_prefix_len` raises: that combination is not built.
    Measured (profiles/prefill_rel.md, MI355X): the ALiBi term costs +5 % on a float16 prefill of 64 prompts and nothing
    measurable on decode rows; a window turns 38 into 12 - 17 us at 1 x 16 x 32 768 x 12 x 64 (W = 256 - 4 096) and 713 into 197 us for
    256 decode rows over 4 096 tokens at W = 1 024; no measured cell lost.

    `tree_mask` (a contiguous int64 [num_tokens] tensor on the query's device: one 64-bit word per packed query row, read as
    unsigned) makes every chunk a TOKEN TREE — the verification rows of a speculative decoder whose candidates branch — in every
    form above but the shared prefix and over both page formats (the TREE kernels, csrc/pa_prefill.hpp).  With ctx = seq_lens[s] -
    q_len, row j of sequence s's chunk attends every cached token t < ctx and chunk token ctx + i, i <= j, iff bit i of its word is
    set.  Bit j (the row itself) always counts as set and bits above j are ignored: nodes come in a topological order, ancestors
    first, and a word of -1 is plain causal attention for its row.  Row j's K / V sit at cached position ctx + j: write all q_len
    rows (reshape_and_cache / reshape_and_cache_chunks) first.  Needs max_q_len <= 64; a sequence whose q_len on the device exceeds
    64 writes nothing.  Form selection, the plans and the workspace are untouched: `cooperative`, `pack_heads`, `max_seq_len` and
    `partition_tokens` mean what they mean above, and the tree kernels of the chosen form are launched.  None (default): every
    launch above, bit for bit, through the same entries and kernels.  Together with `alibi_slopes`, `sliding_window` or
    `shared_prefix_len` it raises: those combinations are not built.  Measurements: profiles/prefill_tree.md."""
    if sliding_window is not None and (isinstance(sliding_window, bool) or not isinstance(sliding_window, int) or sliding_window <= 0):
        raise RuntimeError(f"paged_attention_prefill: sliding_window must be a positive int, got {sliding_window!r}")
    rel = alibi_slopes is not None or sliding_window is not None
    if rel and shared_prefix_len is not None:
        raise RuntimeError("paged_attention_prefill: alibi_slopes / sliding_window together with shared_prefix_len is not built")
    if tree_mask is not None and (rel or shared_prefix_len is not None):
        raise RuntimeError("paged_attention_prefill: tree_mask together with alibi_slopes, sliding_window or shared_prefix_len "
                           "is not built")
    if cooperative is not None and not isinstance(cooperative, bool):
        raise RuntimeError(f"paged_attention_prefill: cooperative must be True, False or None, got {cooperative!r}")
    if pack_heads is not None and not isinstance(pack_heads, bool):
        raise RuntimeError(f"paged_attention_prefill: pack_heads must be True, False or None, got {pack_heads!r}")
    if max_seq_len is None and partition_tokens is not None:
        raise RuntimeError("paged_attention_prefill: partition_tokens needs max_seq_len (the host-known bound on seq_lens)")
    if shared_prefix_len is not None:
        if isinstance(shared_prefix_len, bool) or not isinstance(shared_prefix_len, int) or shared_prefix_len <= 0 or \
                shared_prefix_len % 32:
            raise RuntimeError(f"paged_attention_prefill: shared_prefix_len must be a positive multiple of 32, got {shared_prefix_len!r}")
        if max_seq_len is None:
            raise RuntimeError("paged_attention_prefill: shared_prefix_len needs max_seq_len (the host-known bound on seq_lens)")
        if shared_prefix_len >= int(max_seq_len):
            raise RuntimeError(f"paged_attention_prefill: shared_prefix_len={shared_prefix_len} must be less than "
                               f"max_seq_len={max_seq_len}")
        if partition_tokens is not None and int(partition_tokens) != shared_prefix_len:
            raise RuntimeError(f"paged_attention_prefill: partition_tokens={partition_tokens} must be None or equal "
                               f"shared_prefix_len={shared_prefix_len} (the prefix is partition 0)")
    fp8 = _check_kv_cache_dtype(kv_cache_dtype)     # first: an unknown or unbuilt dtype is reported whatever the tensors are
    if fp8 == 2:
        raise RuntimeError(f"paged_attention_prefill is not built for E5M2 pages (kv_cache_dtype='{kv_cache_dtype}'); "
                           "float16 ('auto') and fp8-E4M3 ('fp8', 'fp8_e4m3') pages are")
    x = 16 if fp8 else 8
    qs = query.shape
    if len(qs) != 3:
        raise RuntimeError(f"query must be [num_tokens, num_heads, head_size], got {tuple(qs)}")
    if query.dtype != torch.float16:
        raise RuntimeError(f"Unsupported input type of paged attention prefill: {query.dtype} (float16 is built)")
    if alibi_slopes is not None and (alibi_slopes.dtype != torch.float32 or alibi_slopes.numel() != qs[1] or
                                     not alibi_slopes.is_contiguous()):
        raise RuntimeError("alibi_slopes must be a contiguous float32 [num_heads] tensor")      # (_pa_common's check)
    if tree_mask is not None:
        if tree_mask.dtype != torch.int64 or tree_mask.dim() != 1 or tree_mask.shape[0] != qs[0] or not tree_mask.is_contiguous():
            raise RuntimeError("tree_mask must be a contiguous int64 [num_tokens] tensor (one 64-bit word per query row)")
        if int(max_q_len) > 64:
            raise RuntimeError(f"paged_attention_prefill: tree_mask holds one 64-bit word per row: max_q_len must be at most 64, "
                               f"got {max_q_len}")
    index = query.get_device()
    dev = query.device
    if index < 0:
        _check_device("query", query, dev)
    if alibi_slopes is not None:
        _check_device("alibi_slopes", alibi_slopes, dev)
    if tree_mask is not None:
        _check_device("tree_mask", tree_mask, dev)
    _on("out", out, index, dev)
    _on("key_cache", key_cache, index, dev)
    _on("value_cache", value_cache, index, dev)
    _on("block_tables", block_tables, index, dev)
    _on("seq_lens", seq_lens, index, dev)
    _on("cu_q_lens", cu_q_lens, index, dev)
    if fp8:
        _check_fp8_cache_dtype(fp8, key_cache, value_cache, kv_cache_dtype)
    elif key_cache.dtype != torch.float16 or value_cache.dtype != torch.float16:
        raise RuntimeError("key_cache/value_cache must be torch.float16 for kv_cache_dtype='auto' (fp8-E4M3 pages: kv_cache_dtype='fp8')")
    if out.dtype != torch.float16:
        raise RuntimeError(f"out must be torch.float16, got {out.dtype}")
    if block_tables.dtype != torch.int32 or seq_lens.dtype != torch.int32 or cu_q_lens.dtype != torch.int32:
        raise RuntimeError("block_tables, seq_lens and cu_q_lens must be int32")
    num_tokens, num_heads, head_size = qs
    ks, vs = key_cache.shape, value_cache.shape
    if len(ks) != 5 or len(vs) != 4:
        raise RuntimeError("key_cache must be [num_blocks, num_kv_heads, head_size/x, block_size, x] "
                           "and value_cache [num_blocks, num_kv_heads, head_size, block_size]")
    if ks[4] != x:
        raise RuntimeError(f"key_cache innermost dimension must be {x} (16 bytes per chunk), got {ks[4]}")
    block_size = int(block_size)
    if ks[3] != block_size or vs[3] != block_size:
        raise RuntimeError(f"block_size={block_size} does not match the cache tensors ({ks[3]}, {vs[3]})")
    if ks[2] * x != head_size or vs[2] != head_size:
        raise RuntimeError("cache head_size does not match query head_size")
    num_kv_heads = int(num_kv_heads)
    if ks[1] != num_kv_heads or vs[1] != num_kv_heads:
        raise RuntimeError("cache num_kv_heads does not match num_kv_heads argument")
    qst = query.stride()
    if qst[2] != 1 or qst[1] != head_size:
        raise RuntimeError("query must be contiguous in its last two dimensions")
    kst, vst = key_cache.stride(), value_cache.stride()
    tile = head_size * block_size
    if kst[4] != 1 or kst[3] != x or kst[2] != block_size * x or (kst[1] != tile and ks[1] != 1) or vst[3] != 1 or \
            vst[2] != block_size or (vst[1] != tile and vs[1] != 1):
        raise RuntimeError("each cache block must be dense")
    if vst[0] != kst[0] or vst[1] != kst[1]:
        raise RuntimeError("key_cache and value_cache must have identical block/head strides")
    if not out.is_contiguous() or out.numel() != num_tokens * num_heads * head_size:
        raise RuntimeError("out must be contiguous with num_tokens*num_heads*head_size elements")
    ts, tst = block_tables.shape, block_tables.stride()
    num_seqs = seq_lens.shape[0] if seq_lens.dim() == 1 else -1
    if num_seqs < 0 or not seq_lens.is_contiguous():
        raise RuntimeError("seq_lens must be a contiguous [num_seqs] tensor")
    if len(ts) != 2 or ts[0] != num_seqs or tst[1] != 1 or (tst[0] != ts[1] and num_seqs > 1):
        raise RuntimeError("block_tables must be a row-contiguous [num_seqs, max_num_blocks_per_seq] tensor")
    if cu_q_lens.dim() != 1 or cu_q_lens.shape[0] != num_seqs + 1 or not cu_q_lens.is_contiguous():
        raise RuntimeError("cu_q_lens must be a contiguous [num_seqs + 1] tensor")
    args = (out.data_ptr(), query.data_ptr(), key_cache.data_ptr(), value_cache.data_ptr(),
            num_tokens, num_heads, head_size, num_kv_heads, float(scale),
            block_tables.data_ptr(), seq_lens.data_ptr(), cu_q_lens.data_ptr(),
            num_seqs, int(max_q_len), block_size, ts[1], qst[0], kst[0], kst[1], index, _stream_of(index))
    lib = _lib.load()
    window = min(int(sliding_window or 0), 2 ** 31 - 1)
    rule_len = max_seq_len                              # what the rules behind None read: with a window, the depth a sequence's rows see
    if window and max_seq_len is not None:
        rule_len = min(int(max_seq_len), window + int(max_q_len) - 1)
    pack = pack_heads
    if pack is None:
        pack = prefill_pack_heads_for(max_q_len, num_heads, num_kv_heads, rule_len, num_seqs, _num_cus(index))
    if pack and not _pack_ratio(num_heads, num_kv_heads):
        raise RuntimeError(f"paged_attention_prefill: pack_heads is built for num_heads / num_kv_heads in {PREFILL_PACK_RATIOS}, "
                           f"got num_heads={num_heads} num_kv_heads={num_kv_heads}")
    coop = cooperative
    if coop is None and not pack:
        coop = max_seq_len is not None and prefill_cooperative_for(max_q_len, rule_len, num_seqs, num_heads, _num_cus(index))
    if rel:                                             # the REL kernels of the same form, planned on the windowed depth
        form = 2 if pack else 1 if coop else 0
        if max_seq_len is None:                         # one launch, bounded by what the block table can hold
            bound = min(16 * ts[1], 2 ** 31 - 32)
            tail = (bound, max(32, (bound + 31) // 32 * 32), None, 0)
        else:
            pt, parts, nbytes = _prefill_rel_plan(num_tokens, num_heads, head_size, num_seqs, max_q_len, max_seq_len,
                                                  _num_cus(index), int(partition_tokens or 0), num_kv_heads, window, form)
            ws = prefill_workspace_for(index, nbytes, args[-1]) if parts > 1 else None
            if ws is None:                              # one partition (or capturing without a workspace): the single launch
                tail = (int(max_seq_len), max(32, (int(max_seq_len) + 31) // 32 * 32), None, 0)
            else:
                tail = (int(max_seq_len), pt, ws.data_ptr(), ws.numel())
        slopes = (_ptr(alibi_slopes), window, form)
        rc = lib.vmi_paged_attention_prefill_rel_fp8(*args, *tail, float(kv_scale), *slopes) if fp8 else \
            lib.vmi_paged_attention_prefill_rel_f16(*args, *tail, *slopes)
        if rc != 0:
            _raise_native(rc)
        return None
    if tree_mask is not None:                           # the TREE kernels of the same form, on the same plan and workspace
        if max_seq_len is None:                         # one launch, bounded by what the block table can hold
            bound = min(16 * ts[1], 2 ** 31 - 32)
            tail = (bound, max(32, (bound + 31) // 32 * 32), None, 0)
        else:
            plan = prefill_gqa_plan(num_tokens, num_heads, head_size, num_seqs, max_q_len, max_seq_len, num_kv_heads,
                                    _num_cus(index), int(partition_tokens or 0)) if pack else \
                prefill_split_plan(num_tokens, num_heads, head_size, num_seqs, max_q_len, max_seq_len, _num_cus(index),
                                   int(partition_tokens or 0))
            ws = prefill_workspace_for(index, plan[2], args[-1]) if plan[1] > 1 else None
            if ws is None:                              # one partition (or capturing without a workspace): the single launch
                tail = (int(max_seq_len), max(32, (int(max_seq_len) + 31) // 32 * 32), None, 0)
            else:
                tail = (int(max_seq_len), plan[0], ws.data_ptr(), ws.numel())
        words = (tree_mask.data_ptr(), 2 if pack else 1 if coop else 0)
        rc = lib.vmi_paged_attention_prefill_tree_fp8(*args, *tail, float(kv_scale), *words) if fp8 else \
            lib.vmi_paged_attention_prefill_tree_f16(*args, *tail, *words)
        if rc != 0:
            _raise_native(rc)
        return None
    prefix_ws = None
    if shared_prefix_len is not None:                   # the prefix is partition 0: the split plan's workspace for PT = P
        nbytes = prefill_split_plan(num_tokens, num_heads, head_size, num_seqs, max_q_len, max_seq_len, _num_cus(index),
                                    shared_prefix_len)[2]
        prefix_ws = prefill_workspace_for(index, nbytes, args[-1])   # None: capturing without one — the unshared launch below
    if prefix_ws is not None:
        tail = (int(max_seq_len), shared_prefix_len, prefix_ws.data_ptr(), prefix_ws.numel())
        form = (shared_prefix_len, 2 if pack else 1 if coop else 0)
        rc = lib.vmi_paged_attention_prefill_prefix_fp8(*args, *tail, float(kv_scale), *form) if fp8 else \
            lib.vmi_paged_attention_prefill_prefix_f16(*args, *tail, *form)
    elif (coop or pack) and max_seq_len is None:        # one cooperative launch, bounded by what the block table can hold
        bound = min(16 * ts[1], 2 ** 31 - 32)
        tail = (bound, max(32, (bound + 31) // 32 * 32), None, 0)
        form = "gqa" if pack else "coop"
        rc = getattr(lib, f"vmi_paged_attention_prefill_{form}_fp8")(*args, *tail, float(kv_scale)) if fp8 else \
            getattr(lib, f"vmi_paged_attention_prefill_{form}_f16")(*args, *tail)
    elif max_seq_len is not None:
        if pack:
            pt, parts, nbytes = prefill_gqa_plan(num_tokens, num_heads, head_size, num_seqs, max_q_len, max_seq_len,
                                                 num_kv_heads, _num_cus(index), int(partition_tokens or 0))
        else:
            pt, parts, nbytes = prefill_split_plan(num_tokens, num_heads, head_size, num_seqs, max_q_len, max_seq_len,
                                                   _num_cus(index), int(partition_tokens or 0))
        ws = prefill_workspace_for(index, nbytes, args[-1]) if parts > 1 else None
        if ws is None:                                  # one partition (or capturing without a workspace): the single launch
            pt, ws_ptr, ws_len = max(32, (int(max_seq_len) + 31) // 32 * 32), None, 0
        else:
            ws_ptr, ws_len = ws.data_ptr(), ws.numel()
        tail = (int(max_seq_len), pt, ws_ptr, ws_len)
        form = "gqa" if pack else "coop" if coop else "split"
        rc = getattr(lib, f"vmi_paged_attention_prefill_{form}_fp8")(*args, *tail, float(kv_scale)) if fp8 else \
            getattr(lib, f"vmi_paged_attention_prefill_{form}_f16")(*args, *tail)
    elif fp8:
        rc = lib.vmi_paged_attention_prefill_fp8(*args, float(kv_scale))
    else:
        rc = lib.vmi_paged_attention_prefill_f16(*args)
    if rc != 0:
        _raise_native(rc)
    return None


def reshape_and_cache(
    key: torch.Tensor,
    value: torch.Tensor,
    key_cache: torch.Tensor,
    value_cache: torch.Tensor,
    slot_mapping: torch.Tensor,
    kv_cache_dtype: str,
    kv_scale: float,
) -> None:
    """Scatter new-token K/V rows into the paged caches at `slot_mapping`; in place, returns None.

    Reference: cache_kernels.cu:256-281 (host), :152-207 (kernel).
    """
    fp8 = _check_kv_cache_dtype(kv_cache_dtype)
    kshape = key.shape
    if len(kshape) != 3 or kshape != value.shape:
        raise RuntimeError("key and value must both be [num_tokens, num_heads, head_size]")
    kdt = key.dtype
    if kdt not in (torch.float16, torch.bfloat16, torch.float32) or value.dtype != kdt:
        raise RuntimeError(f"Unsupported input type of reshape_and_cache: {kdt}")
    if kdt == torch.float32 and fp8:
        raise RuntimeError("Unsupported input type of reshape_and_cache: torch.float32 rows with an fp8 cache are not built")
    index = key.get_device()
    dev = key.device
    if index < 0:
        _check_device("key", key, dev)
    _on("value", value, index, dev)
    _on("key_cache", key_cache, index, dev)
    _on("value_cache", value_cache, index, dev)
    _on("slot_mapping", slot_mapping, index, dev)
    if fp8:
        _check_fp8_cache_dtype(fp8, key_cache, value_cache, kv_cache_dtype)
    elif key_cache.dtype != kdt or value_cache.dtype != kdt:
        raise RuntimeError(f"key_cache/value_cache must be {kdt} for kv_cache_dtype='auto'")
    if slot_mapping.dtype != torch.int64:
        raise RuntimeError("slot_mapping must be int64")
    num_tokens, num_heads, head_size = kshape       # cache_kernels.cu:265-267
    ks, vs = key_cache.shape, value_cache.shape
    if len(ks) != 5 or len(vs) != 4:
        raise RuntimeError("key_cache must be [num_blocks, num_heads, head_size/x, block_size, x] "
                           "and value_cache [num_blocks, num_heads, head_size, block_size]")
    block_size = ks[3]                                  # cache_kernels.cu:268
    x = ks[4]                                           # cache_kernels.cu:269
    if not key_cache.is_contiguous() or not value_cache.is_contiguous():
        # the reference computes dense offsets (cache_kernels.cu:187-194)
        raise RuntimeError("key_cache and value_cache must be contiguous")
    if ks[1] != num_heads or ks[2] * x != head_size or tuple(vs[1:]) != (num_heads, head_size, block_size):
        raise RuntimeError("cache shapes do not match key/value shapes")
    kst, vst = key.stride(), value.stride()
    if kst[2] != 1 or kst[1] != head_size or vst[2] != 1 or vst[1] != head_size:
        raise RuntimeError("key/value must be contiguous in their last two dimensions")
    if slot_mapping.numel() != num_tokens or not slot_mapping.is_contiguous():
        raise RuntimeError("slot_mapping must be a contiguous [num_tokens] tensor")
    stream = _stream_of(index)
    if fp8:                                                               # cache_kernels.cu:200-205
        a8 = (key.data_ptr(), value.data_ptr(), key_cache.data_ptr(), value_cache.data_ptr(),
              slot_mapping.data_ptr(), num_tokens, num_heads, head_size, block_size, x,
              kst[0], vst[0], float(kv_scale), index, stream)
        if fp8 == 2:
            rc = _extras("reshape_and_cache over fp8-E5M2 pages").vmi_reshape_and_cache_fp8_e5m2(*a8, int(kdt == torch.bfloat16))
        else:
            fn = _extras("reshape_and_cache (fp8) over bfloat16 rows").vmi_reshape_and_cache_fp8_bf16 if kdt == torch.bfloat16 else \
                _lib.load().vmi_reshape_and_cache_fp8
            rc = fn(*a8)
        if rc != 0:
            _raise_native(rc)
        return None
    fn16 = _extras("reshape_and_cache over float32 tensors").vmi_reshape_and_cache_f32 if kdt == torch.float32 else \
        _lib.load().vmi_reshape_and_cache_f16
    rc = fn16(
        key.data_ptr(), value.data_ptr(), key_cache.data_ptr(), value_cache.data_ptr(),
        slot_mapping.data_ptr(), num_tokens, num_heads, head_size, block_size, x,
        kst[0], vst[0],                                                   # cache_kernels.cu:271-272
        index, stream)
    if rc != 0:
        _raise_native(rc)
    return None


def reshape_and_cache_chunks(
    key: torch.Tensor,
    value: torch.Tensor,
    key_cache: torch.Tensor,
    value_cache: torch.Tensor,
    block_tables: torch.Tensor,
    seq_lens: torch.Tensor,
    cu_q_lens: torch.Tensor,
    max_q_len: int,
    kv_cache_dtype: str = "auto",
    kv_scale: float = 1.0,
) -> None:
    """The cache write of a prefill chunk, addressed like paged_attention_prefill instead of by slot (extension); in place,
    returns None.

    key / value [num_tokens, num_kv_heads, head_size] float16 (rows may be strided: the fused projection's views); sequence s
    owns rows cu_q_lens[s] .. cu_q_lens[s+1]-1, which go to positions seq_lens[s] - q_len .. seq_lens[s] - 1 of the blocks in
    block_tables[s] — the bytes reshape_and_cache writes for the slots table[pos // 16] * 16 + pos % 16, bit for bit, and no
    other byte.  `max_q_len` bounds the q_len of every sequence (host-known: it sizes the grid).  One wave per (sequence, cache
    block, KV head) writes a whole block as contiguous tiles whatever packed row the sequence starts at (csrc/pa_cache_chunk.hpp;
    profiles/prefill_cache_write.md).  Built for float16 rows, head size 64 / 128, block size 16, pages float16 ("auto", x = 8)
    or fp8-E4M3 ("fp8" / "fp8_e4m3", x = 16); anything else raises RuntimeError — there is no fallback to the slot operator.
    A sequence whose lengths the tensors cannot hold writes nothing; a table entry outside the pool skips its block."""
    fp8 = _check_kv_cache_dtype(kv_cache_dtype)
    if fp8 == 2:
        raise RuntimeError(f"reshape_and_cache_chunks is not built for E5M2 pages (kv_cache_dtype='{kv_cache_dtype}'); "
                           "float16 ('auto') and fp8-E4M3 ('fp8', 'fp8_e4m3') pages are")
    x = 16 if fp8 else 8
    kshape = key.shape
    if len(kshape) != 3 or kshape != value.shape:
        raise RuntimeError("key and value must both be [num_tokens, num_kv_heads, head_size]")
    if key.dtype != torch.float16 or value.dtype != torch.float16:
        raise RuntimeError(f"Unsupported input type of reshape_and_cache_chunks: {key.dtype} (float16 is built)")
    num_tokens, num_kv_heads, head_size = kshape
    ks, vs = key_cache.shape, value_cache.shape
    if len(ks) != 5 or len(vs) != 4:
        raise RuntimeError("key_cache must be [num_blocks, num_kv_heads, head_size/x, block_size, x] "
                           "and value_cache [num_blocks, num_kv_heads, head_size, block_size]")
    if head_size not in (64, 128):
        raise RuntimeError(f"Unsupported head size: {head_size} (reshape_and_cache_chunks is built for 64 and 128)")
    if ks[3] != 16 or vs[3] != 16:
        raise RuntimeError(f"Unsupported block size: {ks[3]} (reshape_and_cache_chunks is built for 16)")
    if ks[4] != x:
        raise RuntimeError(f"key_cache innermost dimension must be {x} (16 bytes per chunk), got {ks[4]}")
    index = key.get_device()
    dev = key.device
    if index < 0:
        _check_device("key", key, dev)
    _on("value", value, index, dev)
    _on("key_cache", key_cache, index, dev)
    _on("value_cache", value_cache, index, dev)
    _on("block_tables", block_tables, index, dev)
    _on("seq_lens", seq_lens, index, dev)
    _on("cu_q_lens", cu_q_lens, index, dev)
    if fp8:
        _check_fp8_cache_dtype(fp8, key_cache, value_cache, kv_cache_dtype)
    elif key_cache.dtype != torch.float16 or value_cache.dtype != torch.float16:
        raise RuntimeError("key_cache/value_cache must be torch.float16 for kv_cache_dtype='auto' (fp8-E4M3 pages: kv_cache_dtype='fp8')")
    if block_tables.dtype != torch.int32 or seq_lens.dtype != torch.int32 or cu_q_lens.dtype != torch.int32:
        raise RuntimeError("block_tables, seq_lens and cu_q_lens must be int32")
    if ks[0] != vs[0] or ks[1] != num_kv_heads or vs[1] != num_kv_heads or ks[2] * x != head_size or vs[2] != head_size:
        raise RuntimeError("cache shapes do not match key/value shapes")
    kst, vst = key.stride(), value.stride()
    if kst[2] != 1 or kst[1] != head_size or vst[2] != 1 or vst[1] != head_size:
        raise RuntimeError("key/value must be contiguous in their last two dimensions")
    kcs, vcs = key_cache.stride(), value_cache.stride()
    tile = head_size * 16
    if kcs[4] != 1 or kcs[3] != x or kcs[2] != 16 * x or (kcs[1] != tile and ks[1] != 1) or vcs[3] != 1 or vcs[2] != 16 or \
            (vcs[1] != tile and vs[1] != 1):
        raise RuntimeError("each cache block must be dense")
    if vcs[0] != kcs[0] or vcs[1] != kcs[1]:
        raise RuntimeError("key_cache and value_cache must have identical block/head strides")
    ts, tst = block_tables.shape, block_tables.stride()
    num_seqs = seq_lens.shape[0] if seq_lens.dim() == 1 else -1
    if num_seqs < 0 or not seq_lens.is_contiguous():
        raise RuntimeError("seq_lens must be a contiguous [num_seqs] tensor")
    if len(ts) != 2 or ts[0] != num_seqs or tst[1] != 1 or (tst[0] != ts[1] and num_seqs > 1):
        raise RuntimeError("block_tables must be a row-contiguous [num_seqs, max_num_blocks_per_seq] tensor")
    if cu_q_lens.dim() != 1 or cu_q_lens.shape[0] != num_seqs + 1 or not cu_q_lens.is_contiguous():
        raise RuntimeError("cu_q_lens must be a contiguous [num_seqs + 1] tensor")
    args = (key.data_ptr(), value.data_ptr(), key_cache.data_ptr(), value_cache.data_ptr(), num_tokens, num_kv_heads, head_size,
            block_tables.data_ptr(), seq_lens.data_ptr(), cu_q_lens.data_ptr(), num_seqs, int(max_q_len), 16, x, ts[1], ks[0],
            kst[0], vst[0], kcs[0], kcs[1], index, _stream_of(index))
    lib = _lib.load()
    rc = lib.vmi_reshape_and_cache_chunks_fp8(*args, float(kv_scale)) if fp8 else lib.vmi_reshape_and_cache_chunks_f16(*args)
    if rc != 0:
        _raise_native(rc)
    return None


# ---- tuning helpers (not part of the reference surface) --------------------------------------

_NAMES: dict = {}     # per loaded library (product / extras / diag have different menus): its variant names, asked for once


def variant_names() -> list[str]:
    lib = _lib.load()
    names = _NAMES.get(id(lib))
    if names is None:   # (~300 ctypes calls: 170 us — a decode step asks every time)
        n = lib.vmi_paged_attention_v1_variant_count()
        names = _NAMES[id(lib)] = [lib.vmi_paged_attention_v1_variant_name(i + 1).decode() for i in range(n)]
    return list(names)


def is_split(variant: int) -> bool:
    """Is `variant` a split kernel (pa_split.hpp: a (sequence, head) spread over several workgroups that meet in a workspace)?"""
    lib = _lib.load()
    if id(lib) not in _NAMES:
        variant_names()
    names = _NAMES[id(lib)]
    return 1 <= variant <= len(names) and "_x" in names[variant - 1]


def check_workspaces(index: Optional[int] = None) -> None:
    """Raise if any launch on a cached workspace (of device `index`) gave up waiting for another workgroup (the kernel then
    wrote NaN rows and counted the event in the workspace's first word).  Synchronises; for sync points: the end of a decode
    loop, a bench, a test.  Concurrent split launches on ONE workspace — two streams replaying graphs captured on the same
    side stream — are not supported: the workspace is per (device, stream at call or capture time)."""
    for (i, st), ws in list(_WS.items()):
        if index is None or i == index:
            n = int(ws[:4].view(torch.int32).item())
            if n:
                raise RuntimeError(f"paged_attention_v1: {n} poll(s) of a split kernel gave up on the workspace of device {i}, "
                                   f"stream {st:#x}: its workgroups were not co-resident (another kernel on the CUs, or two "
                                   "launches sharing the workspace); the affected rows are NaN.  ops.reset_workspaces() clears it")


def variant_names_v2() -> list[str]:
    lib = _lib.load()
    n = lib.vmi_paged_attention_v2_variant_count()
    return [lib.vmi_paged_attention_v2_variant_name(i + 1).decode() for i in range(n)]


def set_pv_mfma(on: bool) -> bool:
    """Opt-in (PER HOST THREAD since C-ABI 17 — thread-local in the library: set it on the thread that issues the
    launches; a setting made on the main thread does not reach a worker thread — default off; returns the calling
    thread's previous setting): with grouped-query attention let the
    operators pick the "_pvm" kernels, which also run probabilities x V on the matrix cores.  Results then match
    the reference kernel to the north-star 1e-3 instead of 1-2 fp16 ulp (include/vmi_paged_attention.h,
    vmi_set_pv_mfma); 1.2x faster with 8 query heads per KV head."""
    return bool(_lib.load().vmi_set_pv_mfma(int(bool(on))))


def variant_fits(variant: int, max_seq_len: int, for_append=False) -> bool:
    """Can `variant` (from pick_variant) serve a launch with this max_seq_len — and the fused append, if asked
    (for_append=True; "read": its form without the cache write, paged_attention_v1_append(write_cache=False))?
    False -> pass `_variant=0` and let the library choose."""
    mode = 2 if for_append == "read" else int(bool(for_append))
    return bool(_lib.load().vmi_paged_attention_v1_variant_fits(int(variant), int(max_seq_len), mode))


def last_variant() -> int:
    """Id of the variant the calling thread's last paged_attention_v1 launch ran (0: none yet / block-sparse)."""
    return int(_lib.load().vmi_paged_attention_v1_last_variant())


def last_launch_label() -> str:
    """Name(s) of what the calling thread's last paged_attention_v1 launch ran: "a", or "a | b (gated double launch: one
    of the two, chosen on the device from seq_lens)" — for labelling measurements."""
    lib = _lib.load()
    a, b = int(lib.vmi_paged_attention_v1_last_variant()), int(lib.vmi_paged_attention_v1_last_partner())
    if not a:
        return ""
    names = variant_names()
    return names[a - 1] if not b else f"{names[a - 1]} | {names[b - 1]} (gated double launch: the device picks one from seq_lens)"


def pick_variant(num_seqs: int, num_heads: int, head_size: int, max_seq_len: int, block_size: int = 16,
                 mean_seq_len: int = 0, bf16: bool = False, fp8=False, num_kv_heads: int = 0,
                 workspace: bool = False) -> int:
    """The library's work-decomposition heuristic (what `_variant=0` runs).  A caller that knows the batch's
    lengths on the host may pass their mean: a ragged batch (mean well below max_seq_len) then gets the
    many-waves-per-head decomposition; pass the result as `_variant`.  fp8: False / True (E4M3) / "e5m2".
    workspace=True: what the operators run when they hand the library a workspace (fp16 pages; the default of
    paged_attention_v1 outside stream capture)."""
    lib = _lib.load()
    fp8 = 2 if fp8 in (2, "e5m2", "fp8_e5m2") else int(bool(fp8))
    if workspace and not (mean_seq_len or bf16 or fp8):
        return int(lib.vmi_paged_attention_v1_pick_variant_ws(num_seqs, num_heads, int(num_kv_heads or 0), head_size, block_size,
                                                              max_seq_len))
    if num_kv_heads and num_kv_heads != num_heads:      # grouped-query attention: what the operators pick themselves
        return int(lib.vmi_paged_attention_v1_pick_variant_gqa(num_seqs, num_heads, int(num_kv_heads), head_size,
                                                               block_size, max_seq_len, int(bool(bf16)), fp8))
    if (fp8 == 2 or (fp8 and bf16)) and not getattr(lib, "_vmi_has_extras", False):
        return 0                                        # (the product library has no such kernel: what its menus answer for bf16)
    if fp8 == 2:
        return int(lib.vmi_paged_attention_v1_pick_variant_fp8_e5m2(num_seqs, num_heads, head_size, block_size,
                                                                    max_seq_len, int(mean_seq_len), int(bool(bf16))))
    if fp8:
        fn = lib.vmi_paged_attention_v1_pick_variant_fp8_bf16 if bf16 else lib.vmi_paged_attention_v1_pick_variant_fp8
        return int(fn(num_seqs, num_heads, head_size, block_size, max_seq_len, int(mean_seq_len)))
    if mean_seq_len or bf16:
        return int(lib.vmi_paged_attention_v1_pick_variant_hint(num_seqs, num_heads, head_size, block_size,
                                                                max_seq_len, int(mean_seq_len), int(bool(bf16))))
    return int(lib.vmi_paged_attention_v1_pick_variant(num_seqs, num_heads, head_size, block_size, max_seq_len))
