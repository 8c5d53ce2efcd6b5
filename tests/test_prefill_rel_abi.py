"""CPU checks of the ALiBi / sliding-window prefill's boundary: the three entries are declared, exported and typed, the two launch
entries answer their validation codes in front of any HIP call, the operator checks its two keywords, and the plan counts on
min(max_seq_len, W + max_q_len - 1)."""
import ctypes
import os

import pytest
import torch

NAMES = ("vmi_paged_attention_prefill_rel_f16", "vmi_paged_attention_prefill_rel_fp8")


def test_rel_entries_are_exported_and_declared():
    from vllmini_amd import _lib, build

    header = open(os.path.join(build.INCLUDE, "vmi_paged_attention.h")).read()
    exported = ctypes.CDLL(build.build())
    assert all(f"int {n}(" in header and hasattr(exported, n) for n in (*NAMES, "vmi_paged_attention_prefill_rel_plan"))
    for n in NAMES:                                             # the split entries' arguments + alibi_slopes, sliding_window, form
        res, args = _lib.SIGNATURES[n.replace("rel", "split")]
        assert _lib.SIGNATURES[n] == (res, args + [ctypes.c_void_p, ctypes.c_int32, ctypes.c_int32])


def test_rel_entries_validate_in_front_of_any_hip_call():
    from vllmini_amd import _lib

    lib = _lib.load()
    buf = (ctypes.c_char * 4096)()
    p16 = (ctypes.addressof(buf) + 15) & ~15

    def call(fp8=False, q=p16, tokens=4, head=64, kv=1, block=16, window=8, form=0, slopes=p16):
        fn = getattr(lib, NAMES[fp8])
        return fn(p16, q, p16, p16, tokens, 2, head, kv, 0.125, p16, p16, p16, 1, 4, block, 4, 256, 4096, 1024, 0, None,
                  64, 64, None, 0, *((0.5,) if fp8 else ()), slopes, window, form)

    for fp8 in (False, True):
        assert call(fp8, q=None) == 1 and call(fp8, head=80) == 2 and call(fp8, block=32) == 3      # NULL, head size, block size
        assert call(fp8, kv=3) == 4 and call(fp8, form=2, kv=2) == 4                                 # VMI_E_KV_HEADS (form 2: ratio 1)
        assert call(fp8, window=-1) == 6 and b"sliding_window" in lib.vmi_last_error_string()        # VMI_E_SHAPE
        assert call(fp8, form=3) == 6 and b"form" in lib.vmi_last_error_string() and call(fp8, form=-1) == 6
        assert call(fp8, tokens=0) == 0 and call(fp8, tokens=0, slopes=None, window=0) == 0          # nothing to do: no HIP call


@pytest.mark.parametrize("kw,match", [
    (dict(sliding_window=0), "positive int"), (dict(sliding_window=-1), "positive int"),
    (dict(sliding_window=True), "positive int"), (dict(sliding_window=2.5), "positive int"),
    (dict(alibi_slopes=torch.zeros(2, dtype=torch.float16)), "contiguous float32 .num_heads. tensor"),
    (dict(alibi_slopes=torch.zeros(3)), "contiguous float32 .num_heads. tensor"),
    (dict(alibi_slopes=torch.zeros(2), shared_prefix_len=32, max_seq_len=64), "shared_prefix_len is not built"),
    (dict(sliding_window=8, shared_prefix_len=32, max_seq_len=64), "shared_prefix_len is not built"),
])
def test_operator_checks_alibi_slopes_and_sliding_window(kw, match):
    from vllmini_amd import ops

    q, kc, vc = torch.zeros(4, 2, 64, dtype=torch.float16), torch.zeros(5, 2, 8, 16, 8, dtype=torch.float16), torch.zeros(5, 2, 64, 16, dtype=torch.float16)
    i32 = lambda *v: torch.tensor(v, dtype=torch.int32)         # noqa: E731
    with pytest.raises(RuntimeError, match=match):
        ops.paged_attention_prefill(torch.empty_like(q), q, kc, vc, 2, 0.125, i32(0, 1, 2, 3).view(1, 4), i32(40), i32(0, 4), 4, 16, **kw)


def test_plan_counts_on_the_windowed_depth():
    """One 16-row chunk x 12 heads x 64 over a 32 768-token bound on 256 CUs splits today.  W = 256 is a 271-token context, under the
    split rule's 4 096: one partition, no workspace.  W = 4 096 plans like a 4 111-token context.  No window: the split plan."""
    from vllmini_amd import ops

    shape, deep = (16, 12, 64, 1, 16), 32768
    split = lambda max_len, pt=0: ops.prefill_split_plan(*shape, max_len, 256, pt)                  # noqa: E731
    rel = lambda w, pt=0, form=0, kv=12: ops._prefill_rel_plan(*shape, deep, 256, pt, kv, w, form)  # noqa: E731
    assert split(deep)[1] > 1 and rel(0) == split(deep) and rel(deep) == split(deep)
    assert rel(256)[1:] == (1, 0)
    assert rel(4096) == split(4096 + 16 - 1) and rel(4096)[1] > 1 and rel(4096)[2] == rel(4096)[1] * 16 * 12 * 66 * 4
    assert rel(4096, 512) == split(4111, 512) == (512, 9, 9 * 16 * 12 * 66 * 4)
    assert rel(4096, form=2, kv=3) == ops.prefill_gqa_plan(*shape, 4111, 3, 256)
