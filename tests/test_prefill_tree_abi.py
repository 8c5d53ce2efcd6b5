"""CPU checks of the token-tree prefill's boundary: entries declared, exported and typed; validation codes in front of any HIP call."""
import ctypes
import os

import pytest
import torch

NAMES = ("vmi_paged_attention_prefill_tree_f16", "vmi_paged_attention_prefill_tree_fp8")


def test_tree_entries_are_exported_and_declared():
    from vllmini_amd import _lib, build

    header = open(os.path.join(build.INCLUDE, "vmi_paged_attention.h")).read()
    exported = ctypes.CDLL(build.build())
    for n in NAMES:                                             # the split entries' arguments + tree_mask, form
        assert f"int {n}(" in header and hasattr(exported, n)
        res, args = _lib.SIGNATURES[n.replace("tree", "split")]
        assert _lib.SIGNATURES[n] == (res, args + [ctypes.c_void_p, ctypes.c_int32])


def test_tree_entries_validate_in_front_of_any_hip_call():
    from vllmini_amd import _lib

    lib = _lib.load()
    buf = (ctypes.c_char * 4096)()
    p16 = (ctypes.addressof(buf) + 15) & ~15

    def call(fp8=False, q=p16, tokens=4, heads=2, kv=1, max_q=4, form=0, mask=p16):
        fn = getattr(lib, NAMES[fp8])
        return fn(p16, q, p16, p16, tokens, heads, 64, kv, 0.125, p16, p16, p16, 1, max_q, 16, 4, 256, 4096, 1024, 0, None,
                  64, 64, None, 0, *((0.5,) if fp8 else ()), mask, form)

    for fp8 in (False, True):
        assert call(fp8, mask=None) == 1 and b"tree_mask" in lib.vmi_last_error_string() and call(fp8, q=None) == 1
        assert call(fp8, mask=p16 + 4) == 5 and b"tree_mask" in lib.vmi_last_error_string()         # VMI_E_ALIGNMENT
        assert call(fp8, max_q=65) == 6 and b"max_q_len" in lib.vmi_last_error_string()              # VMI_E_SHAPE
        assert call(fp8, form=3) == 6 and b"form" in lib.vmi_last_error_string() and call(fp8, form=-1) == 6
        assert call(fp8, form=2, heads=3) == 4 and call(fp8, form=2, kv=2) == 4                      # VMI_E_KV_HEADS: ratios 3 and 1
        assert call(fp8, tokens=0) == 0 and call(fp8, tokens=0, mask=None) == 0                      # nothing to do: no HIP call


@pytest.mark.parametrize("kw,match", [
    (dict(alibi_slopes=torch.zeros(2)), "tree_mask together with .* is not built"),
    (dict(sliding_window=8), "tree_mask together with .* is not built"),
    (dict(shared_prefix_len=32, max_seq_len=64), "tree_mask together with .* is not built"),
    (dict(tree_mask=torch.zeros(4, dtype=torch.int32)), "contiguous int64 .num_tokens. tensor"),
    (dict(tree_mask=torch.zeros(5, dtype=torch.int64)), "contiguous int64 .num_tokens. tensor"),
    (dict(tree_mask=torch.zeros(8, dtype=torch.int64)[::2]), "contiguous int64 .num_tokens. tensor"),
    (dict(max_q_len=65), "max_q_len must be at most 64"),
    (dict(), "no CPU path"),
])
def test_operator_checks_tree_mask(kw, match):
    from vllmini_amd import ops

    q, kc, vc = torch.zeros(4, 2, 64, dtype=torch.float16), torch.zeros(5, 2, 8, 16, 8, dtype=torch.float16), torch.zeros(5, 2, 64, 16, dtype=torch.float16)
    i32 = lambda *v: torch.tensor(v, dtype=torch.int32)         # noqa: E731
    kw = {"tree_mask": torch.zeros(4, dtype=torch.int64), "max_q_len": 4, **kw}
    with pytest.raises(RuntimeError, match=match):
        ops.paged_attention_prefill(torch.empty_like(q), q, kc, vc, 2, 0.125, i32(0, 1, 2, 3).view(1, 4), i32(40), i32(0, 4), kw.pop("max_q_len"), 16, **kw)
