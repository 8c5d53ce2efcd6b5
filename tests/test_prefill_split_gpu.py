"""ops.paged_attention_prefill split over the context (max_seq_len / partition_tokens: the partition kernels of csrc/pa_prefill.hpp
and pa_prefill_fp8.hpp, the merge of pa_prefill_split.hpp) against helpers.prefill_reference, fp64 causal attention over the same
NaN-padded, shuffled pages.  Bound per row: helpers.prefill_tol(L) * vmax, as for the unsplit kernels — the merge adds at most
P + 2 fp32 roundings of 2^-24 per output for a row with P <= L / 32 partitions, inside the bound's 2 L 2^-25 term.
Measured maxima: profiles/prefill_split.md section 5."""
import functools

import numpy as np
import pytest
import torch

import helpers

pytestmark = pytest.mark.gpu

SENTINEL = 77.0
MAX_SEQ_LEN = 1029
# (q_len, seq_len): decode rows with one partition / ending on a boundary / one token into the second / several partitions;
# (20, 40): a tile whose rows own one or two partitions at 32 (the all-masked partial); prefills straddling boundaries; chunks
# starting before, on and off a boundary; 33 partitions with a last one of 5 tokens; between them the guards (no rows, no tokens,
# longer than max_seq_len).
SEQS = [(1, 1), (0, 7), (1, 32), (1, 33), (1, 97), (3, 0), (20, 40), (40, 40), (90, 90), (3, MAX_SEQ_LEN + 1), (33, 64), (16, 64),
        (65, 165), (5, 1029)]
HEALTHY = [q > 0 and 0 < L <= MAX_SEQ_LEN for q, L in SEQS]


@functools.lru_cache(maxsize=None)
def _case(fmt, H, KV, D, kv_scale, healthy=tuple(HEALTHY)):
    rng = np.random.default_rng(D + (fmt == "fp8"))
    rows = [tuple(helpers.store_rows(rng.uniform(-1, 1, (L, KV, D)), fmt, kv_scale) for _ in range(2)) for _, L in SEQS]
    kc, vc, tables = helpers.pack_pages(rng, rows, KV, D, fmt)
    lens = np.array([L for _, L in SEQS], np.int32)
    cu = np.concatenate([[0], np.cumsum([q for q, _ in SEQS])]).astype(np.int32)
    q = rng.uniform(-1, 1, (cu[-1], H, D)).astype(np.float16)
    ref, row_len, vmax = helpers.prefill_reference(q, kc, vc, tables, lens, cu, D ** -0.5, fmt, kv_scale, list(healthy), SENTINEL)
    assert 16 * tables.shape[1] >= MAX_SEQ_LEN + 1 and np.isfinite(ref).all()
    return q, kc, vc, tables, lens, cu, ref, row_len, vmax


def _run(case, fmt, H, KV, D, kv_scale, strided=False, nan_workspace=None, **kw):
    from vllmini_amd import ops

    dev = torch.device("cuda:0")
    q, kc, vc, tables, lens, cu = case[:6]
    T, qd = q.shape[0], torch.from_numpy(q).to(dev)
    if strided:                                                # the fused projection's strided view
        buf = torch.zeros((T, 3 * H * D), dtype=torch.float16, device=dev)
        buf[:, : H * D] = qd.view(T, H * D)
        qd = buf[:, : H * D].view(T, H, D)
    if nan_workspace:                                          # a caller's workspace holds anything: hand it over full of NaN
        ops.prefill_workspace_for(0, nan_workspace).view(torch.float32).fill_(float("nan"))
    out = torch.full((T, H, D), SENTINEL, dtype=torch.float16, device=dev)
    pages = [torch.from_numpy(a.view(np.float16) if fmt == "f16" else a).to(dev) for a in (kc, vc)]
    ops.paged_attention_prefill(out, qd, *pages, KV, D ** -0.5, torch.from_numpy(tables).to(dev), torch.from_numpy(lens).to(dev),
                                torch.from_numpy(cu).to(dev), max(q for q, _ in SEQS), 16,
                                kv_cache_dtype="auto" if fmt == "f16" else "fp8", kv_scale=kv_scale, **kw)
    return out.cpu()


@pytest.mark.parametrize("partition_tokens", [32, 64])
@pytest.mark.parametrize("H,KV,D", [(2, 1, 64), (2, 2, 128)])
@pytest.mark.parametrize("fmt,kv_scale", [("f16", 1.0), ("fp8", 0.37)])
def test_split_prefill_matches_fp64_attention(fmt, kv_scale, H, KV, D, partition_tokens):
    from vllmini_amd import ops

    case = _case(fmt, H, KV, D, kv_scale)
    ref, row_len, vmax = case[6:]
    pt, parts, nbytes = ops.prefill_split_plan(len(ref), H, D, len(SEQS), 90, MAX_SEQ_LEN, 256, partition_tokens)
    assert (pt, parts) == (partition_tokens, -(-MAX_SEQ_LEN // partition_tokens)) and nbytes == parts * len(ref) * H * (D + 2) * 4
    kw = dict(strided=D == 64, nan_workspace=nbytes, max_seq_len=MAX_SEQ_LEN, partition_tokens=partition_tokens)
    out = _run(case, fmt, H, KV, D, kv_scale, **kw)
    got = out.numpy().astype(np.float64)
    kept = row_len == 0                                        # rows of the guarded sequences
    assert kept.sum() == 6 and (got[kept] == SENTINEL).all()
    err = np.abs(got - ref).max(axis=(1, 2))                   # (NaN if any output of the row is: the comparison below then fails)
    bound = helpers.prefill_tol(row_len) * vmax
    print(f"split prefill {fmt} H={H} KV={KV} D={D} PT={partition_tokens}: max |got - ref| = {err[~kept].max():.3e} "
          f"(bounds {bound[~kept].min():.3e} .. {bound[~kept].max():.3e}); row over 1029 tokens {err[-1]:.3e}")
    assert (err[~kept] <= bound[~kept]).all(), (err[~kept].max(), np.flatnonzero(~(err <= bound) & ~kept))
    assert torch.equal(out, _run(case, fmt, H, KV, D, kv_scale, **kw))          # fixed merge order, no atomics


@pytest.mark.parametrize("fmt,kv_scale", [("f16", 1.0), ("fp8", 0.37)])
def test_one_partition_is_the_unsplit_launch_bit_for_bit(fmt, kv_scale):
    healthy = tuple(q > 0 and L > 0 for q, L in SEQS)          # (the reference is not used here: every sequence within the bound)
    case = _case(fmt, 2, 1, 64, kv_scale, healthy)
    plain = _run(case, fmt, 2, 1, 64, kv_scale)
    one = _run(case, fmt, 2, 1, 64, kv_scale, max_seq_len=MAX_SEQ_LEN + 1, partition_tokens=1056)
    assert torch.equal(plain, one) and not (plain[-1] == SENTINEL).any()
