"""CPU checks of the head-packed prefill's boundary: the three entries are declared, exported and typed, answer their validation
codes in front of any HIP call, the plan keeps the split plan's workspace arithmetic, and the operator checks its keyword."""
import ctypes
import os

import pytest
import torch

NAMES = ("vmi_paged_attention_prefill_gqa_f16", "vmi_paged_attention_prefill_gqa_fp8")
PLAN = "vmi_paged_attention_prefill_gqa_plan"


def _plan(lib, heads, kv, tokens=6, d=64, seqs=2, max_q=3, max_len=1000, cus=256, pt_in=0):
    pt, parts, nbytes = ctypes.c_int32(), ctypes.c_int32(), ctypes.c_int64()
    rc = getattr(lib, PLAN)(tokens, heads, d, seqs, max_q, max_len, cus, pt_in, ctypes.byref(pt), ctypes.byref(parts),
                            ctypes.byref(nbytes), kv)
    return rc, pt.value, parts.value, nbytes.value


def test_gqa_entries_are_exported_and_declared():
    from vllmini_amd import _lib, build

    header = open(os.path.join(build.INCLUDE, "vmi_paged_attention.h")).read()
    exported = ctypes.CDLL(build.build())
    assert all(f"int {n}(" in header and hasattr(exported, n) for n in (*NAMES, PLAN))
    assert [_lib.SIGNATURES[n] for n in NAMES] == [_lib.SIGNATURES[n.replace("gqa", "split")] for n in NAMES]
    res, args = _lib.SIGNATURES["vmi_paged_attention_prefill_split_plan"]
    assert _lib.SIGNATURES[PLAN] == (res, args + [ctypes.c_int32])     # ... plus num_kv_heads


def test_gqa_entries_validate_in_front_of_any_hip_call():
    from vllmini_amd import _lib

    lib = _lib.load()
    buf = (ctypes.c_char * 4096)()
    p16 = (ctypes.addressof(buf) + 15) & ~15
    need = 2 * 4 * 4 * 66 * 4                                   # 2 partitions x 4 tokens x 4 heads x (64 + 2) floats

    def call(fp8=False, heads=4, kv=2, max_len=64, pt=32, ws=p16, ws_bytes=need, tokens=4):
        fn = getattr(lib, NAMES[fp8])
        return fn(p16, p16, p16, p16, tokens, heads, 64, kv, 0.125, p16, p16, p16, 1, 4, 16, 4, 256, 4096, 1024, 0, None,
                  max_len, pt, ws, ws_bytes, *((0.5,) if fp8 else ()))

    for fp8 in (False, True):
        assert call(fp8, kv=4) == 4 and b"ratio 1" in lib.vmi_last_error_string()                   # VMI_E_KV_HEADS
        assert call(fp8, heads=6) == 4 and b"ratio 3" in lib.vmi_last_error_string()
        assert call(fp8, heads=64, kv=2) == 4 and call(fp8, heads=5) == 4                           # 32; not divisible
        assert call(fp8, ws_bytes=need - 1) == 11 and b"workspace" in lib.vmi_last_error_string()   # VMI_E_WORKSPACE: too small
        assert call(fp8, ws=p16 + 8) == 11 and call(fp8, ws=None) == 11                             # misaligned, absent
        assert call(fp8, max_len=65) == 6 and call(fp8, pt=40) == 6 and call(fp8, max_len=-1) == 6  # VMI_E_SHAPE, as split
        assert call(fp8, tokens=0) == 0 and call(fp8, tokens=0, pt=64, ws=None, ws_bytes=0) == 0    # nothing to do: no HIP call


def test_gqa_plan_counts_the_packed_grid_and_keeps_the_workspace_bytes():
    from vllmini_amd import _lib

    lib = _lib.load()
    assert _plan(lib, 4, 4)[0] == 4 and _plan(lib, 6, 2)[0] == 4 and _plan(lib, 4, 0)[0] == 4
    assert _plan(lib, 32, 8, pt_in=256) == (0, 256, 4, 4 * 6 * 32 * 66 * 4)                          # P T H (D + 2) 4, forced size
    assert _plan(lib, 32, 8, pt_in=1024) == (0, 1024, 1, 0) and _plan(lib, 32, 8, pt_in=48)[0] == 6
    # the rule on the packed grid, ceil(max_q_len / (16 / G)) * num_seqs * num_kv_heads workgroups against 2 per CU: 4 rows on
    # 32 / 8 heads are ONE tile — 64 sequences make 512 workgroups (no split), 63 make 504 (split); the plain grid would hold 2 048
    deep = dict(d=128, max_q=4, max_len=16384)
    assert _plan(lib, 32, 8, tokens=256, seqs=64, **deep)[2] == 1
    assert _plan(lib, 32, 8, tokens=252, seqs=63, **deep)[1:3] == (2048, 8)
    assert _plan(lib, 32, 8, tokens=315, seqs=63, d=128, max_q=5, max_len=16384)[2] == 1             # 5 rows: two tiles


@pytest.mark.parametrize("bad", [1, 0, "yes"])
def test_pack_heads_must_be_a_bool_or_none(bad):
    from vllmini_amd import ops

    q, kc, vc = torch.zeros(4, 2, 64, dtype=torch.float16), torch.zeros(3, 2, 8, 16, 8, dtype=torch.float16), torch.zeros(3, 2, 64, 16, dtype=torch.float16)
    i32 = lambda *v: torch.tensor(v, dtype=torch.int32)         # noqa: E731
    with pytest.raises(RuntimeError, match="pack_heads must be True, False or None"):
        ops.paged_attention_prefill(torch.empty_like(q), q, kc, vc, 2, 0.125, i32(0).view(1, 1), i32(4), i32(0, 4), 4, 16, pack_heads=bad)
