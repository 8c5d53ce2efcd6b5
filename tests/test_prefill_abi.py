"""CPU checks of the tiled prefill attention's boundary: vmi_paged_attention_prefill_f16 validates before any HIP call, the
operator has no CPU path, and GPT2PagedDecoder refuses prefill_attention="tiled" on a pool the kernel cannot serve."""
from __future__ import annotations

import ctypes

import pytest
import torch


def test_prefill_entry_validation_codes_without_gpu():
    from vllmini_amd import _lib

    lib = _lib.load()
    buf = (ctypes.c_char * 4096)()
    p16 = (ctypes.addressof(buf) + 15) & ~15

    def call(out=p16, tokens=4, hs=64, nkv=4, bs=16, qs=256):
        return lib.vmi_paged_attention_prefill_f16(out, p16, p16, p16, tokens, 4, hs, nkv, 0.125, p16, p16, p16,
                                                   1, 4, bs, 1, qs, 4096, 1024, 0, None)

    assert call(out=None) == 1                                  # VMI_E_NULL_POINTER
    assert call(hs=80) == 2 and b"Unsupported head size: 80" in lib.vmi_last_error_string()
    assert call(bs=32) == 3 and b"Unsupported block size: 32" in lib.vmi_last_error_string()
    assert call(nkv=3) == 4                                     # VMI_E_KV_HEADS
    assert call(qs=257) == 5                                    # VMI_E_ALIGNMENT
    assert call(tokens=0) == 0                                  # nothing to do: no HIP call


def test_prefill_operator_has_no_cpu_path():
    from vllmini_amd import ops

    T, H, D = 4, 2, 64
    q = torch.zeros(T, H, D, dtype=torch.float16)
    kc, vc = torch.zeros(3, H, D // 8, 16, 8, dtype=torch.float16), torch.zeros(3, H, D, 16, dtype=torch.float16)
    i32 = lambda *v: torch.tensor(v, dtype=torch.int32)         # noqa: E731
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.paged_attention_prefill(torch.empty_like(q), q, kc, vc, H, 0.125, i32(0).view(1, 1), i32(4), i32(0, 4), 4, 16)


def test_decoder_refuses_tiled_prefill_over_fp8_pages():
    from vllmini_amd.gpt2_decode import GPT2Dims, GPT2PagedDecoder, random_state_dict
    from vllmini_amd.kv_pool import PagedKVPool

    dims = GPT2Dims(vocab_size=64, n_positions=32, n_embd=128, n_layer=1, n_head=2)
    sd = random_state_dict(dims, "cpu")
    pool = PagedKVPool(8, 2, 64, 16, 4, 1, device="cpu", allocate_tensors=False, kv_cache_dtype="fp8")
    with pytest.raises(ValueError, match="prefill_attention='tiled' is built for float16"):
        GPT2PagedDecoder(dims, sd, pool, prefill_attention="tiled")
    assert GPT2PagedDecoder(dims, sd, pool).prefill_attention == "positions"      # the default is today's path
