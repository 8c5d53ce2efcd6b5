"""ops.paged_attention_prefill(pack_heads=True): the PACK form of csrc/pa_prefill.hpp / pa_prefill_fp8.hpp — a tile's 16 columns are
(row, query head of one KV head) pairs, one always-cooperative tile of 16 / G rows per workgroup — against
helpers.prefill_reference, fp64 causal attention over the same NaN-padded, shuffled pages.  Bound per row: helpers.prefill_tol(L) *
vmax, as for the plain kernels; the LDS merge's six fp32 roundings are inside it (tests/test_prefill_coop_gpu.py derives that)."""
import functools

import numpy as np
import pytest
import torch

import helpers

pytestmark = pytest.mark.gpu

SENTINEL = 77.0
MAX_SEQ_LEN = 1029
# (q_len, seq_len): waves with no pair, one pair each, a fifth pair back on wave 0; a chunk equal to R = 16 / G for one of the ratios
# each; a last tile with dead columns and the diagonal inside the last pair; many tiles; the guards; a deep row.
SEQS = [(1, 1), (1, 31), (1, 33), (1, 129), (2, 34), (4, 68), (8, 40), (16, 16), (5, 133), (9, 71), (37, 90), (0, 7), (3, 0),
        (3, 1029)]
CU = np.concatenate([[0], np.cumsum([q for q, _ in SEQS])]).astype(np.int32)


@functools.lru_cache(maxsize=None)
def _case(fmt, H, KV, D, kv_scale):
    rng = np.random.default_rng(H + D + (fmt == "fp8"))
    rows = [tuple(helpers.store_rows(rng.uniform(-1, 1, (L, KV, D)), fmt, kv_scale) for _ in range(2)) for _, L in SEQS]
    kc, vc, tables = helpers.pack_pages(rng, rows, KV, D, fmt)
    lens = np.array([L for _, L in SEQS], np.int32)
    q = rng.uniform(-1, 1, (CU[-1], H, D)).astype(np.float16)
    ref, row_len, vmax = helpers.prefill_reference(q, kc, vc, tables, lens, CU, D ** -0.5, fmt, kv_scale, None, SENTINEL)
    assert np.isfinite(ref).all()
    return q, kc, vc, tables, lens, ref, row_len, vmax


def _run(case, fmt, H, KV, D, kv_scale, nseq=len(SEQS), **kw):
    """The first nseq sequences of the batch."""
    from vllmini_amd import ops

    dev = torch.device("cuda:0")
    cu, (q, kc, vc, tables, lens) = CU[: nseq + 1], case[:5]
    q, tables, lens, max_q = q[: cu[-1]], tables[:nseq], lens[:nseq], int(np.diff(cu).max())
    if kw.get("partition_tokens"):                             # a caller's workspace holds anything: hand it over full of NaN
        nbytes = ops.prefill_gqa_plan(len(q), H, D, nseq, max_q, kw["max_seq_len"], KV, 256, kw["partition_tokens"])[2]
        ops.prefill_workspace_for(0, nbytes).view(torch.float32).fill_(float("nan"))
    out = torch.full(q.shape, SENTINEL, dtype=torch.float16, device=dev)
    pages = [torch.from_numpy(a.view(np.float16) if fmt == "f16" else a).to(dev) for a in (kc, vc)]
    ops.paged_attention_prefill(out, torch.from_numpy(q).to(dev), *pages, KV, D ** -0.5, torch.from_numpy(tables).to(dev),
                                torch.from_numpy(lens).to(dev), torch.from_numpy(cu).to(dev), max_q, 16,
                                kv_cache_dtype="auto" if fmt == "f16" else "fp8", kv_scale=kv_scale, **kw)
    return out.cpu()


@pytest.mark.parametrize("partition_tokens", [None, 32, 160])     # 160: five pairs a partition, pp0 > 0 in the walk
@pytest.mark.parametrize("H,KV,D", [(4, 2, 64), (8, 2, 128), (8, 1, 64), (16, 1, 128)])   # G = 2, 4, 8, 16
@pytest.mark.parametrize("fmt,kv_scale", [("f16", 1.0), ("fp8", 0.37)])
def test_head_packed_prefill_matches_fp64_attention(fmt, kv_scale, H, KV, D, partition_tokens):
    case = _case(fmt, H, KV, D, kv_scale)
    ref, row_len, vmax = case[5:]
    kw = dict(max_seq_len=MAX_SEQ_LEN, partition_tokens=partition_tokens)
    out = _run(case, fmt, H, KV, D, kv_scale, pack_heads=True, **kw)
    got = out.numpy().astype(np.float64)
    kept = row_len == 0                                        # rows of the guarded sequences
    assert kept.sum() == 3 and (got[kept] == SENTINEL).all()
    err = np.abs(got - ref).max(axis=(1, 2))                   # (NaN if any output of the row is: the comparison below then fails)
    bound = helpers.prefill_tol(row_len) * vmax
    print(f"packed prefill {fmt} H={H} KV={KV} D={D} PT={partition_tokens}: max |got - ref| = {err[~kept].max():.3e} "
          f"(bounds {bound[~kept].min():.3e} .. {bound[~kept].max():.3e}); rows over 1029 tokens {err[-3:].max():.3e}")
    assert (err[~kept] <= bound[~kept]).all(), (err[~kept].max(), np.flatnonzero(~(err <= bound) & ~kept))
    assert torch.equal(out, _run(case, fmt, H, KV, D, kv_scale, pack_heads=True, **kw))   # fixed merge order, no atomics
    # a chunk of at most R = 16 / G rows is ONE tile in both forms — same last_pos, pairs per wave and merge: bit for bit
    short = np.concatenate([np.arange(CU[s], CU[s + 1]) for s, (n, _) in enumerate(SEQS) if n <= 16 // (H // KV)])
    coop = _run(case, fmt, H, KV, D, kv_scale, cooperative=True, **kw)
    assert len(short) >= 4 and torch.equal(out[short], coop[short])


def test_pack_heads_none_resolves_by_the_rule_and_false_is_the_default():
    """None = the rule on the host-known bounds: True on the first six sequences (chunks of at most 4 rows), False on the whole batch
    (37 rows) and without max_seq_len; True without max_seq_len is the one packed launch bounded by the block table."""
    from vllmini_amd import ops

    rule = ops.prefill_pack_heads_for
    assert rule(4, 8, 2, 1029, 6, 256) and rule(4, 64, 8, 1024, 256, 256) and not rule(4, 8, 2, None, 6, 256)
    assert not rule(4, 8, 8, 1029, 6, 256) and not rule(4, 6, 2, 1029, 6, 256) and not rule(37, 8, 2, 1029, 14, 256)
    assert rule(16, 32, 8, 16384, 4, 256) and rule(16, 64, 8, 16384, 4, 256) and not rule(16, 32, 8, 4096, 64, 256)   # 128, 256, 2 048
    assert not rule(5, 32, 8, 1029, 17, 256) and not rule(17, 32, 8, 1029, 1, 256)                    # 2 * 17 * 8 = 272 workgroups
    a = ("f16", 8, 2, 128, 1.0)
    case = _case(*a)
    kw = dict(max_seq_len=MAX_SEQ_LEN)
    for nseq in (6, len(SEQS)):
        plain, packed = _run(case, *a, nseq, **kw), _run(case, *a, nseq, pack_heads=True, **kw)
        assert torch.equal(_run(case, *a, nseq, pack_heads=False, **kw), plain)
        assert not torch.equal(packed, plain)                                 # (else the comparisons below say nothing)
        assert torch.equal(_run(case, *a, nseq, pack_heads=None, **kw), packed if nseq == 6 else plain)
    assert torch.equal(_run(case, *a, 6, pack_heads=None), _run(case, *a, 6))
    assert torch.equal(_run(case, *a, pack_heads=True), _run(case, *a, pack_heads=True, max_seq_len=16 * 66))   # the table's capacity
