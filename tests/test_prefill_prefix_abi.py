"""CPU checks of the shared-prefix prefill's boundary: the two entries are declared, exported and typed, answer their validation
codes in front of any HIP call, and the operator checks its keyword."""
import ctypes
import os

import pytest
import torch

NAMES = ("vmi_paged_attention_prefill_prefix_f16", "vmi_paged_attention_prefill_prefix_fp8")


def test_prefix_entries_are_exported_and_declared():
    from vllmini_amd import _lib, build

    header = open(os.path.join(build.INCLUDE, "vmi_paged_attention.h")).read()
    exported = ctypes.CDLL(build.build())
    assert all(f"int {n}(" in header and hasattr(exported, n) for n in NAMES)
    for n in NAMES:                                             # the split entries' arguments + shared_prefix_len, suffix_form
        res, args = _lib.SIGNATURES[n.replace("prefix", "split")]
        assert _lib.SIGNATURES[n] == (res, args + [ctypes.c_int32, ctypes.c_int32])


def test_prefix_entries_validate_in_front_of_any_hip_call():
    from vllmini_amd import _lib

    lib = _lib.load()
    buf = (ctypes.c_char * 4096)()
    p16 = (ctypes.addressof(buf) + 15) & ~15
    need = 2 * 4 * 2 * 66 * 4                                   # 2 partitions x 4 tokens x 2 heads x (64 + 2) floats

    def call(fp8=False, max_len=64, pt=32, ws=p16, ws_bytes=need, tokens=4, prefix=32, form=0, kv=1):
        fn = getattr(lib, NAMES[fp8])
        return fn(p16, p16, p16, p16, tokens, 2, 64, kv, 0.125, p16, p16, p16, 1, 4, 16, 4, 256, 4096, 1024, 0, None,
                  max_len, pt, ws, ws_bytes, *((0.5,) if fp8 else ()), prefix, form)

    for fp8 in (False, True):
        assert call(fp8, prefix=48, pt=48) == 6 and b"multiple of 32" in lib.vmi_last_error_string()    # VMI_E_SHAPE
        assert call(fp8, prefix=0, pt=0) == 6 and call(fp8, prefix=-32, pt=-32) == 6
        assert call(fp8, prefix=64, pt=64) == 6 and b"less than max_seq_len" in lib.vmi_last_error_string()
        assert call(fp8, pt=64) == 6 and b"partition_tokens" in lib.vmi_last_error_string()            # the prefix is partition 0
        assert call(fp8, form=3) == 6 and b"suffix_form" in lib.vmi_last_error_string() and call(fp8, form=-1) == 6
        assert call(fp8, form=2, kv=2) == 4                                                              # VMI_E_KV_HEADS: ratio 1
        assert call(fp8, ws_bytes=need - 1) == 11 and b"workspace" in lib.vmi_last_error_string()        # VMI_E_WORKSPACE
        assert call(fp8, ws=None) == 11 and call(fp8, max_len=65) == 6                                   # absent; past the table
        assert call(fp8, tokens=0) == 0                                                                  # nothing to do: no HIP call


@pytest.mark.parametrize("kw,match", [
    (dict(shared_prefix_len=48, max_seq_len=64), "positive multiple of 32"),
    (dict(shared_prefix_len=0, max_seq_len=64), "positive multiple of 32"),
    (dict(shared_prefix_len=64, max_seq_len=64), "less than max_seq_len"),
    (dict(shared_prefix_len=32), "needs max_seq_len"),
    (dict(shared_prefix_len=32, max_seq_len=64, partition_tokens=64), "partition_tokens=64 must be None or equal"),
])
def test_operator_checks_shared_prefix_len(kw, match):
    from vllmini_amd import ops

    q, kc, vc = torch.zeros(4, 2, 64, dtype=torch.float16), torch.zeros(5, 2, 8, 16, 8, dtype=torch.float16), torch.zeros(5, 2, 64, 16, dtype=torch.float16)
    i32 = lambda *v: torch.tensor(v, dtype=torch.int32)         # noqa: E731
    with pytest.raises(RuntimeError, match=match):
        ops.paged_attention_prefill(torch.empty_like(q), q, kc, vc, 2, 0.125, i32(0, 1, 2, 3).view(1, 4), i32(40), i32(0, 4), 4, 16, **kw)
