"""ops.paged_attention_prefill(cooperative=True): the COOP form of csrc/pa_prefill.hpp / pa_prefill_fp8.hpp — a 64-row group with
at most 16 live rows is walked by all four waves of its workgroup, pairs interleaved, merged through LDS — against
helpers.prefill_reference, fp64 causal attention over the same NaN-padded, shuffled pages.  Bound per row: helpers.prefill_tol(L) *
vmax, as for the plain kernels: the LDS merge adds at most six fp32 roundings of 2^-24 per output (four weights, three sums),
inside the bound's 2 L 2^-25 term from L = 2 on and inside its 2^-12 term for L = 1.  Measured maxima: profiles/prefill_coop.md."""
import functools

import numpy as np
import pytest
import torch

import helpers

pytestmark = pytest.mark.gpu

SENTINEL = 77.0
MAX_SEQ_LEN = 1029
# (q_len, seq_len): one or two pairs (waves with no work); four pairs, one per wave; a fifth pair, back on wave 0; a full tile and
# the diagonal inside the last pair; the guards; groups of more than 16 live rows beside a last group of 1 (17 = 16 + 1 is ONE
# group of 17), 16 and 6 rows; a deep row.
SEQS = [(1, 1), (1, 31), (1, 32), (1, 33), (1, 97), (1, 129), (5, 133), (16, 16), (16, 160), (7, 71), (0, 7), (3, 0), (17, 40),
        (80, 80), (70, 200), (5, 1029)]
CU = np.concatenate([[0], np.cumsum([q for q, _ in SEQS])]).astype(np.int32)
# rows of groups with more than 16 live rows: all of (17, 40), rows 0 - 63 of (80, 80) and (70, 200)
PLAIN_ROWS = np.concatenate([np.arange(CU[s], CU[s] + n) for s, n in ((12, 17), (13, 64), (14, 64))])


@functools.lru_cache(maxsize=None)
def _case(fmt, H, KV, D, kv_scale):
    rng = np.random.default_rng(D + (fmt == "fp8"))
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
    q, max_q = q[: cu[-1]], int(np.diff(cu).max())
    if kw.get("partition_tokens"):                             # a caller's workspace holds anything: hand it over full of NaN
        nbytes = ops.prefill_split_plan(len(q), H, D, nseq, max_q, kw["max_seq_len"], 256, kw["partition_tokens"])[2]
        ops.prefill_workspace_for(0, nbytes).view(torch.float32).fill_(float("nan"))
    out = torch.full(q.shape, SENTINEL, dtype=torch.float16, device=dev)
    pages = [torch.from_numpy(a.view(np.float16) if fmt == "f16" else a).to(dev) for a in (kc, vc)]
    ops.paged_attention_prefill(out, torch.from_numpy(q).to(dev), *pages, KV, D ** -0.5, torch.from_numpy(tables[:nseq]).to(dev),
                                torch.from_numpy(lens[:nseq]).to(dev), torch.from_numpy(cu).to(dev), max_q, 16,
                                kv_cache_dtype="auto" if fmt == "f16" else "fp8", kv_scale=kv_scale, **kw)
    return out.cpu()


@pytest.mark.parametrize("partition_tokens", [None, 32, 160])     # 160: five pairs a partition, pp0 > 0 in the walk
@pytest.mark.parametrize("H,KV,D", [(2, 1, 64), (2, 2, 128)])
@pytest.mark.parametrize("fmt,kv_scale", [("f16", 1.0), ("fp8", 0.37)])
def test_cooperative_prefill_matches_fp64_attention(fmt, kv_scale, H, KV, D, partition_tokens):
    case = _case(fmt, H, KV, D, kv_scale)
    ref, row_len, vmax = case[5:]
    kw = dict(max_seq_len=MAX_SEQ_LEN, partition_tokens=partition_tokens)
    out = _run(case, fmt, H, KV, D, kv_scale, cooperative=True, **kw)
    got = out.numpy().astype(np.float64)
    kept = row_len == 0                                        # rows of the guarded sequences
    assert kept.sum() == 3 and (got[kept] == SENTINEL).all()
    err = np.abs(got - ref).max(axis=(1, 2))                   # (NaN if any output of the row is: the comparison below then fails)
    bound = helpers.prefill_tol(row_len) * vmax
    print(f"coop prefill {fmt} H={H} KV={KV} D={D} PT={partition_tokens}: max |got - ref| = {err[~kept].max():.3e} "
          f"(bounds {bound[~kept].min():.3e} .. {bound[~kept].max():.3e}); row over 1029 tokens {err[-1]:.3e}")
    assert (err[~kept] <= bound[~kept]).all(), (err[~kept].max(), np.flatnonzero(~(err <= bound) & ~kept))
    assert torch.equal(out, _run(case, fmt, H, KV, D, kv_scale, cooperative=True, **kw))   # fixed merge order, no atomics
    plain = _run(case, fmt, H, KV, D, kv_scale, cooperative=False, **kw)
    assert torch.equal(out[PLAIN_ROWS], plain[PLAIN_ROWS])     # more than 16 live rows: the plain code, bit for bit


def test_cooperative_none_resolves_by_the_rule():
    """The short sequences alone (max_q_len 16, 24 workgroups): None = the rule on the host-known bounds, False without max_seq_len;
    True without max_seq_len is the one cooperative launch bounded by the block table."""
    from vllmini_amd import ops

    T, rule = ops.PREFILL_COOP_MIN_CONTEXT, ops.prefill_cooperative_for
    assert T == 512 and rule(16, T, 12, 2, 256) and not rule(16, T - 1, 12, 2, 256) and not rule(17, T, 12, 2, 256)
    assert not rule(16, None, 12, 2, 256) and rule(16, T, 32, 12, 256) and not rule(16, T, 64, 12, 256)   # 1.5 and 3 workgroups a CU
    case, a = _case("f16", 2, 1, 64, 1.0), ("f16", 2, 1, 64, 1.0, 12)   # through (3, 0): no chunk over 16 rows, none over 160 tokens
    plain = _run(case, *a, cooperative=False)
    assert not torch.equal(_run(case, *a, cooperative=True), plain)          # (else the comparisons below say nothing)
    assert torch.equal(_run(case, *a, cooperative=True, max_seq_len=T), _run(case, *a, cooperative=True))
    assert torch.equal(_run(case, *a, cooperative=None, max_seq_len=T), _run(case, *a, cooperative=True))
    assert torch.equal(_run(case, *a, cooperative=None), plain)
    assert torch.equal(_run(case, *a, cooperative=None, max_seq_len=T - 1), plain)
