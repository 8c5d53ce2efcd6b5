"""CPU checks of the fp8-E4M3 tiled prefill's boundary: vmi_paged_attention_prefill_fp8 validates before any HIP call, the
operator names E5M2 pages as not built, and GPT2PagedDecoder(prefill_attention="auto") resolves to the path that serves the pool."""
import ctypes

import pytest
import torch


def test_prefill_fp8_entry_validation_codes_without_gpu():
    from vllmini_amd import _lib

    lib = _lib.load()
    buf = (ctypes.c_char * 4096)()
    p16 = (ctypes.addressof(buf) + 15) & ~15

    def call(out=p16, tokens=4, hs=64, nkv=4, bs=16, qs=256, hst=1024, kvs=1.0):
        return lib.vmi_paged_attention_prefill_fp8(out, p16, p16, p16, tokens, 4, hs, nkv, 0.125, p16, p16, p16,
                                                   1, 4, bs, 1, qs, 4096, hst, 0, None, kvs)

    assert call(out=None) == 1                                  # VMI_E_NULL_POINTER
    assert call(hs=80) == 2 and b"Unsupported head size: 80" in lib.vmi_last_error_string()
    assert call(bs=32) == 3 and b"Unsupported block size: 32" in lib.vmi_last_error_string()
    for bad in (0.0, -1.0, float("inf"), float("nan")):
        assert call(kvs=bad, nkv=3) == 6 and b"kv_scale" in lib.vmi_last_error_string()   # VMI_E_SHAPE, in front of KV_HEADS
    assert call(nkv=3) == 4                                     # VMI_E_KV_HEADS
    assert call(qs=257) == 5                                    # VMI_E_ALIGNMENT
    assert call(hst=1032) == 5                                  # cache strides are in bytes: a multiple of 8 is not enough
    assert call(tokens=0) == 0                                  # nothing to do: no HIP call


def test_prefill_operator_names_e5m2_pages_as_not_built():
    from vllmini_amd import ops

    q, kc, vc = torch.zeros(4, 2, 64, dtype=torch.float16), torch.zeros(3, 2, 4, 16, 16, dtype=torch.uint8), torch.zeros(3, 2, 64, 16, dtype=torch.uint8)
    i32 = lambda *v: torch.tensor(v, dtype=torch.int32)         # noqa: E731
    for dtype, message in (("fp8_e5m2", "not built for E5M2"), ("fp8", "no CPU path")):   # (E4M3 gets as far as the device check)
        with pytest.raises(RuntimeError, match=message):
            ops.paged_attention_prefill(torch.empty_like(q), q, kc, vc, 2, 0.125, i32(0).view(1, 1), i32(4), i32(0, 4), 4, 16,
                                        kv_cache_dtype=dtype, kv_scale=0.5)


@pytest.mark.parametrize("kv_cache_dtype,block_size,want", [("fp8", 16, "tiled"), ("auto", 16, "tiled"), ("fp8", 32, "positions")])
def test_decoder_auto_resolves_to_the_path_that_serves_the_pool(kv_cache_dtype, block_size, want):
    from vllmini_amd.gpt2_decode import GPT2Dims, GPT2PagedDecoder, random_state_dict
    from vllmini_amd.kv_pool import PagedKVPool

    dims = GPT2Dims(vocab_size=64, n_positions=32, n_embd=128, n_layer=1, n_head=2)
    pool = PagedKVPool(8, 2, 64, block_size, 4, 1, device="cpu", allocate_tensors=False, kv_cache_dtype=kv_cache_dtype)
    assert GPT2PagedDecoder(dims, random_state_dict(dims, "cpu"), pool, prefill_attention="auto").prefill_attention == want
