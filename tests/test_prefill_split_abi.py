"""CPU checks of the context-split prefill's boundary: the plan's arithmetic and rule (vmi_paged_attention_prefill_split_plan with
num_cus given: no HIP call), the split entries' validation codes in front of any HIP call, and the operator's keyword check."""
import ctypes

import pytest
import torch


def _plan(tokens, heads, d, seqs, max_q, max_len, pt_in=0, cus=256):
    from vllmini_amd import _lib

    pt, parts, nbytes = ctypes.c_int32(-1), ctypes.c_int32(-1), ctypes.c_int64(-1)
    rc = _lib.load().vmi_paged_attention_prefill_split_plan(tokens, heads, d, seqs, max_q, max_len, cus, pt_in, ctypes.byref(pt),
                                                            ctypes.byref(parts), ctypes.byref(nbytes))
    return rc, pt.value, parts.value, nbytes.value


def test_split_plan_arithmetic_and_rule():
    assert _plan(300, 2, 64, 14, 90, 1029, 32) == (0, 32, 33, 33 * 300 * 2 * 66 * 4)       # forced: ceil(1029 / 32) partitions
    assert _plan(300, 2, 128, 14, 90, 1029, 64) == (0, 64, 17, 17 * 300 * 2 * 130 * 4)
    assert _plan(300, 2, 64, 14, 90, 1029, 1056)[1:] == (1056, 1, 0)                      # one partition: do not split, 0 bytes
    assert _plan(300, 2, 64, 14, 90, 1029, 48)[0] == 6 and _plan(300, 2, 64, 14, 90, 1029, -32)[0] == 6   # VMI_E_SHAPE
    assert _plan(300, 2, 80, 14, 90, 1029, 32)[0] == 2                                    # VMI_E_HEAD_SIZE
    # the rule: 64 prompts U{4..512} on 12 x 64 fill the chip unsplit (profiles/prefill_tiled.md section 1)
    assert _plan(15113, 12, 64, 64, 512, 512)[2:] == (1, 0)
    # ... and one 256-row chunk over 32 768 tokens on 32 heads does not: 128 workgroups on 256 CUs
    rc, pt, parts, nbytes = _plan(256, 32, 128, 1, 256, 32768)
    assert rc == 0 and pt % 32 == 0 and parts == -(-32768 // pt) > 1 and nbytes == parts * 256 * 32 * 130 * 4
    assert _plan(256, 32, 128, 1, 256, 512)[2] == 1                                       # as few workgroups, a shallow context


def test_split_entries_validate_in_front_of_any_hip_call():
    from vllmini_amd import _lib

    lib = _lib.load()
    buf = (ctypes.c_char * 4096)()
    p16 = (ctypes.addressof(buf) + 15) & ~15
    need = 2 * 4 * 4 * 66 * 4                                   # 2 partitions x 4 tokens x 4 heads x (64 + 2) floats

    def call(fp8=False, max_len=64, pt=32, ws=p16, ws_bytes=need, mb=4, tokens=4):
        tail = (max_len, pt, ws, ws_bytes)
        fn = lib.vmi_paged_attention_prefill_split_fp8 if fp8 else lib.vmi_paged_attention_prefill_split_f16
        return fn(p16, p16, p16, p16, tokens, 4, 64, 4, 0.125, p16, p16, p16, 1, 4, 16, mb, 256, 4096, 1024, 0, None, *tail,
                  *((0.5,) if fp8 else ()))

    for fp8 in (False, True):
        assert call(fp8, ws_bytes=need - 1) == 11 and b"workspace" in lib.vmi_last_error_string()   # VMI_E_WORKSPACE: too small
        assert call(fp8, ws=p16 + 8) == 11 and call(fp8, ws=None) == 11                             # misaligned, absent
        assert call(fp8, max_len=65) == 6 and b"block table" in lib.vmi_last_error_string()         # VMI_E_SHAPE: 65 > 16 * 4
        assert call(fp8, pt=40) == 6 and call(fp8, pt=0) == 6 and call(fp8, max_len=-1) == 6
        assert call(fp8, tokens=0) == 0                                                             # nothing to do: no HIP call


def test_partition_tokens_needs_max_seq_len():
    from vllmini_amd import ops

    q, kc, vc = torch.zeros(4, 2, 64, dtype=torch.float16), torch.zeros(3, 2, 8, 16, 8, dtype=torch.float16), torch.zeros(3, 2, 64, 16, dtype=torch.float16)
    i32 = lambda *v: torch.tensor(v, dtype=torch.int32)         # noqa: E731
    with pytest.raises(RuntimeError, match="partition_tokens needs max_seq_len"):
        ops.paged_attention_prefill(torch.empty_like(q), q, kc, vc, 2, 0.125, i32(0).view(1, 1), i32(4), i32(0, 4), 4, 16, partition_tokens=32)
