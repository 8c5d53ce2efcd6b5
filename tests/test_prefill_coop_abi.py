"""CPU checks of the cooperative prefill's boundary: the two entries are declared, exported and typed, answer the split entries'
validation codes in front of any HIP call, and the operator checks its keyword."""
import ctypes
import os

import pytest
import torch

NAMES = ("vmi_paged_attention_prefill_coop_f16", "vmi_paged_attention_prefill_coop_fp8")


def test_coop_entries_are_exported_and_declared():
    from vllmini_amd import _lib, build

    header = open(os.path.join(build.INCLUDE, "vmi_paged_attention.h")).read()
    exported = ctypes.CDLL(build.build())
    assert all(f"int {n}(" in header and hasattr(exported, n) for n in NAMES)
    split = [_lib.SIGNATURES[n.replace("coop", "split")] for n in NAMES]
    assert [_lib.SIGNATURES[n] for n in NAMES] == split                # the split entries' argument lists


def test_coop_entries_validate_in_front_of_any_hip_call():
    from vllmini_amd import _lib

    lib = _lib.load()
    buf = (ctypes.c_char * 4096)()
    p16 = (ctypes.addressof(buf) + 15) & ~15
    need = 2 * 4 * 4 * 66 * 4                                   # 2 partitions x 4 tokens x 4 heads x (64 + 2) floats

    def call(fp8=False, max_len=64, pt=32, ws=p16, ws_bytes=need, mb=4, tokens=4):
        fn = getattr(lib, NAMES[fp8])
        return fn(p16, p16, p16, p16, tokens, 4, 64, 4, 0.125, p16, p16, p16, 1, 4, 16, mb, 256, 4096, 1024, 0, None,
                  max_len, pt, ws, ws_bytes, *((0.5,) if fp8 else ()))

    for fp8 in (False, True):
        assert call(fp8, ws_bytes=need - 1) == 11 and b"workspace" in lib.vmi_last_error_string()   # VMI_E_WORKSPACE: too small
        assert call(fp8, ws=p16 + 8) == 11 and call(fp8, ws=None) == 11                             # misaligned, absent
        assert call(fp8, max_len=65) == 6 and b"block table" in lib.vmi_last_error_string()         # VMI_E_SHAPE: 65 > 16 * 4
        assert call(fp8, pt=40) == 6 and call(fp8, pt=0) == 6 and call(fp8, max_len=-1) == 6
        assert call(fp8, tokens=0) == 0 and call(fp8, tokens=0, pt=64, ws=None, ws_bytes=0) == 0    # nothing to do: no HIP call


@pytest.mark.parametrize("bad", [1, 0, "yes"])
def test_cooperative_must_be_a_bool_or_none(bad):
    from vllmini_amd import ops

    q, kc, vc = torch.zeros(4, 2, 64, dtype=torch.float16), torch.zeros(3, 2, 8, 16, 8, dtype=torch.float16), torch.zeros(3, 2, 64, 16, dtype=torch.float16)
    i32 = lambda *v: torch.tensor(v, dtype=torch.int32)         # noqa: E731
    with pytest.raises(RuntimeError, match="cooperative must be True, False or None"):
        ops.paged_attention_prefill(torch.empty_like(q), q, kc, vc, 2, 0.125, i32(0).view(1, 1), i32(4), i32(0, 4), 4, 16, cooperative=bad)
