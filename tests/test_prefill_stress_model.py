"""What tests/test_prefill_stress_gpu.py can and cannot see, shown without a GPU on helpers.prefill_kernel_model (the arithmetic
of csrc/pa_prefill.hpp: pairs of blocks, fp16-rounded P, fp32 running sum): the kernel's arithmetic stays inside TOL(L) on
all five score profiles, and matrix cores that read fp16-subnormal P as zero — while the sum keeps them — would break the
sink profile's bound more than tenfold at the shapes the GPU test uses."""
import numpy as np
import pytest

from helpers import (PROFILES, pack_pages, prefill_kernel_model, prefill_reference, prefill_tol, read_pages, score_profile_case,
                     store_rows)

SEQS = ((1, 512), (17, 517), (65, 512))          # (q_len, seq_len): the GPU test's (q_len, ctx) = (1, 511), (17, 500), (65, 447)


def _model_errors(profile, fmt, kv_scale, H, KV, D, flush):
    """max |model - fp64 reference| / (TOL(L) * vmax) over the batch, through the same pages as the GPU test."""
    rng = np.random.default_rng(D + len(profile))
    q, rows = score_profile_case(rng, profile, SEQS, H, KV, D)
    kc, vc, tables = pack_pages(rng, [(store_rows(k, fmt, kv_scale), store_rows(v, fmt, kv_scale)) for k, v in rows], KV, D, fmt)
    lens = np.array([L for _, L in SEQS])
    cu = np.concatenate([[0], np.cumsum([ql for ql, _ in SEQS])])
    ref, row_len, vmax = prefill_reference(q, kc, vc, tables, lens, cu, D ** -0.5, fmt, kv_scale)
    got = np.empty_like(ref)
    for s, L in enumerate(lens):
        k, v = read_pages(kc, vc, tables[s], L, fmt)            # decoded, kv_scale folded like the launcher folds it
        got[cu[s]: cu[s + 1]] = prefill_kernel_model(q[cu[s]: cu[s + 1]], k, v, D ** -0.5 * kv_scale, kv_scale, flush)
    return (np.abs(got - ref).max(axis=(1, 2)) / (prefill_tol(row_len) * vmax)).max()


@pytest.mark.parametrize("fmt,kv_scale", [("f16", 1.0), ("fp8", 0.37)])
@pytest.mark.parametrize("profile", PROFILES)
def test_kernel_arithmetic_stays_inside_tol_on_every_profile(profile, fmt, kv_scale):
    worst = _model_errors(profile, fmt, kv_scale, 2, 1, 64, flush=False)
    print(f"model, {profile}, {fmt} kv_scale={kv_scale}: max err / bound = {worst:.3f}")
    assert worst <= 1.0


@pytest.mark.parametrize("fmt,kv_scale,H,KV,D", [("f16", 1.0, 2, 1, 64), ("f16", 1.0, 2, 2, 128), ("fp8", 0.37, 2, 1, 64)])
def test_sink_profile_catches_a_one_sided_subnormal_flush(fmt, kv_scale, H, KV, D):
    kept, flushed = (_model_errors("sink", fmt, kv_scale, H, KV, D, flush) for flush in (False, True))
    print(f"model, sink, {fmt} D={D}: err / bound = {kept:.3f} with subnormal P kept, {flushed:.1f} with the MFMA side flushed")
    assert kept <= 1.0 and flushed > 10.0
