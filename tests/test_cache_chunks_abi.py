"""CPU checks of the chunk cache write's boundary: the two entries are declared, exported and typed; they validate before any
HIP call; the operator and the decoder keyword refuse what the kernels do not serve."""
import ctypes

import pytest
import torch


@pytest.mark.parametrize("fp8", [False, True])
def test_chunk_entries_are_exported_and_validate_without_gpu(fp8):
    from vllmini_amd import _lib

    lib = _lib.load()
    name = "vmi_reshape_and_cache_chunks_" + ("fp8" if fp8 else "f16")
    assert getattr(lib, name).argtypes == _lib.SIGNATURES[name][1] and len(_lib.SIGNATURES[name][1]) == 22 + fp8
    buf = (ctypes.c_char * 4096)()
    p16 = (ctypes.addressof(buf) + 15) & ~15

    def call(key=p16, tokens=4, hs=64, seqs=1, mq=4, bs=16, x=16 if fp8 else 8, ks=192, hst=1024, kvs=1.0):
        tail = (kvs,) if fp8 else ()
        return getattr(lib, name)(key, p16, p16, p16, tokens, 1, hs, p16, p16, p16, seqs, mq, bs, x, 1, 8, ks, 192, 4096, hst,
                                  0, None, *tail)

    assert call(key=None) == 1                                  # VMI_E_NULL_POINTER
    assert call(hs=80) == 2 and b"Unsupported head size: 80" in lib.vmi_last_error_string()
    assert call(bs=32) == 3 and b"Unsupported block size: 32" in lib.vmi_last_error_string()
    assert call(x=4) == 9 and call(x=8 if fp8 else 16) == 9      # VMI_E_X: the other format's chunk width too
    assert call(key=p16 + 2) == 5 and call(ks=196) == 5          # VMI_E_ALIGNMENT: pointer, row stride
    assert call(hst=1032 if fp8 else 1028) == 5                  # cache strides: 16 bytes in cache elements (fp8: bytes)
    assert call(tokens=-1) == 6 and call(mq=-1) == 6             # VMI_E_SHAPE
    if fp8:
        for bad in (0.0, -1.0, float("inf"), float("nan")):
            assert call(kvs=bad) == 6 and b"kv_scale" in lib.vmi_last_error_string()
    assert call(tokens=0) == 0 and call(seqs=0) == 0 and call(mq=0) == 0   # nothing to do: no HIP call


def _tensors(D=64, BS=16, fp8=False, dtype=torch.float16):
    x = 16 if fp8 else 8
    cdt = torch.uint8 if fp8 else torch.float16
    i32 = lambda *v: torch.tensor(v, dtype=torch.int32)         # noqa: E731
    return (torch.zeros(4, 2, D, dtype=dtype), torch.zeros(4, 2, D, dtype=dtype), torch.zeros(3, 2, D // x, BS, x, dtype=cdt),
            torch.zeros(3, 2, D, BS, dtype=cdt), i32(0).view(1, 1), i32(4), i32(0, 4), 4)


@pytest.mark.parametrize("kw,dtype,message", [
    (dict(dtype=torch.bfloat16), "auto", "Unsupported input type"), (dict(dtype=torch.float32), "auto", "Unsupported input type"),
    (dict(fp8=True), "fp8_e5m2", "not built for E5M2"), (dict(D=80), "auto", "Unsupported head size: 80"),
    (dict(BS=32), "auto", "Unsupported block size: 32"), (dict(), "int8", "Unsupported data type of kv cache"),
    (dict(), "auto", "no CPU path"), (dict(fp8=True), "fp8", "no CPU path")])     # (what is served gets as far as the device check)
def test_chunk_operator_refuses_what_the_kernels_do_not_serve(kw, dtype, message):
    from vllmini_amd import cache_ops, ops

    assert cache_ops.reshape_and_cache_chunks is ops.reshape_and_cache_chunks and "reshape_and_cache_chunks" in cache_ops.__all__
    with pytest.raises(RuntimeError, match=message):
        cache_ops.reshape_and_cache_chunks(*_tensors(**kw), kv_cache_dtype=dtype, kv_scale=0.5)


@pytest.mark.parametrize("kv_cache_dtype,block_size,attention,asked,want", [
    ("auto", 16, "positions", "slots", "slots"), ("auto", 16, "positions", "chunks", "chunks"), ("fp8", 16, "positions", "chunks", "chunks"),
    ("fp8", 16, "auto", "auto", "chunks"), ("auto", 16, "positions", "auto", "slots"), ("fp8", 32, "auto", "auto", "slots"),
    ("fp8", 32, "positions", "chunks", ValueError), ("auto", 16, "positions", "blocks", ValueError)])
def test_decoder_cache_write_keyword(kv_cache_dtype, block_size, attention, asked, want):
    from vllmini_amd.gpt2_decode import GPT2Dims, GPT2PagedDecoder, random_state_dict
    from vllmini_amd.kv_pool import PagedKVPool

    dims = GPT2Dims(vocab_size=64, n_positions=32, n_embd=128, n_layer=1, n_head=2)
    pool = PagedKVPool(8, 2, 64, block_size, 4, 1, device="cpu", allocate_tensors=False, kv_cache_dtype=kv_cache_dtype)
    make = lambda **kw: GPT2PagedDecoder(dims, random_state_dict(dims, "cpu"), pool, prefill_attention=attention, **kw)   # noqa: E731
    assert make().prefill_cache_write == "slots"                # the default: today's behaviour
    if want is ValueError:
        with pytest.raises(ValueError, match="prefill_cache_write"):
            make(prefill_cache_write=asked)
    else:
        assert make(prefill_cache_write=asked).prefill_cache_write == want
