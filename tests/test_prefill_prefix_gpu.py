"""ops.paged_attention_prefill(shared_prefix_len=P): the PREFIX form of csrc/pa_prefill.hpp / pa_prefill_fp8.hpp — tiles of 16 consecutive
rows of the packed batch walk ONE copy of the prefix (partition 0), the chunk forms every sequence's own suffix from partition 1 on,
the merge launch folds them — against helpers.prefill_reference, fp64 causal attention over the same NaN-padded, shuffled pages.
Bound per row: helpers.prefill_tol(L) * vmax, as for the unshared launches (the LDS merge and the merge launch are inside it:
tests/test_prefill_coop_gpu.py, tests/test_prefill_split_gpu.py).

Every call here is a POISON case: only row 0 of the block tables names the prefix's blocks; the other rows hold, in their first
P / 16 entries, a block full of NaN (0x7F bytes for fp8 pages).  A finite result inside the bound says the prefix was read through
row 0 — that the new path ran."""
import functools

import numpy as np
import pytest
import torch

import helpers

pytestmark = pytest.mark.gpu

SENTINEL = 77.0
Q_LENS = [1, 3, 17, 1, 16]        # 38 rows: tiles cross sequence boundaries, the last tile has 6 live columns
CU = np.concatenate([[0], np.cumsum(Q_LENS)]).astype(np.int32)
FORMS = {"plain": {}, "coop": dict(cooperative=True), "pack": dict(pack_heads=True)}


def _lens(P):
    """Exactly P tokens in front of the chunk; ends on a partition boundary; reaches into partition 2; an ordinary decode row; fewer
    than P tokens in front of the chunk (rows inside the prefix: the per-column select)."""
    return np.array([P + 1, 2 * P, 2 * P + 9, P + 6, P + 6], np.int32)


@functools.lru_cache(maxsize=None)
def _case(fmt, H, KV, D, kv_scale, P):
    rng = np.random.default_rng(H + D + P + (fmt == "fp8"))
    lens = _lens(P)
    rows = [tuple(helpers.store_rows(rng.uniform(-1, 1, (L, KV, D)), fmt, kv_scale) for _ in range(2)) for L in [P, *(lens - P)]]
    kc, vc, own = helpers.pack_pages(rng, rows, KV, D, fmt)     # row 0: the prefix's blocks, row 1 + s: sequence s's own
    tables = np.concatenate([np.repeat(own[:1, : P // 16], len(lens), 0), own[1:]], axis=1)
    q = rng.uniform(-1, 1, (CU[-1], H, D)).astype(np.float16)
    poisoned = tables.copy()
    poisoned[1:, : P // 16] = np.setdiff1d(np.arange(len(kc)), own)[0]      # a block nobody owns: pack_pages left it full of NaN
    return q, kc, vc, tables, poisoned, lens


def _run(case, fmt, H, KV, D, kv_scale, P, lens, max_seq_len, **kw):
    from vllmini_amd import ops

    dev = torch.device("cuda:0")
    q, kc, vc, _, poisoned = case[:5]
    nbytes = ops.prefill_split_plan(len(q), H, D, len(lens), max(Q_LENS), max_seq_len, 256, P)[2]
    ops.prefill_workspace_for(0, nbytes).view(torch.float32).fill_(float("nan"))      # a caller's workspace holds anything
    out = torch.full(q.shape, SENTINEL, dtype=torch.float16, device=dev)
    pages = [torch.from_numpy(a.view(np.float16) if fmt == "f16" else a).to(dev) for a in (kc, vc)]
    ops.paged_attention_prefill(out, torch.from_numpy(q).to(dev), *pages, KV, D ** -0.5, torch.from_numpy(poisoned).to(dev),
                                torch.from_numpy(lens).to(dev), torch.from_numpy(CU).to(dev), max(Q_LENS), 16,
                                kv_cache_dtype="auto" if fmt == "f16" else "fp8", kv_scale=kv_scale, max_seq_len=max_seq_len,
                                shared_prefix_len=P, **kw)
    return out.cpu().numpy().astype(np.float64)


def _check(got, case, fmt, D, kv_scale, lens, healthy, label):
    q, kc, vc, tables = case[:4]
    ref, row_len, vmax = helpers.prefill_reference(q, kc, vc, tables, lens, CU, D ** -0.5, fmt, kv_scale, healthy, SENTINEL)
    kept = row_len == 0
    assert (got[kept] == SENTINEL).all()                       # rows of the guarded sequences
    err = np.abs(got - ref).max(axis=(1, 2))                   # (NaN if any output of the row is: the comparison below then fails)
    bound = helpers.prefill_tol(row_len) * vmax
    print(f"shared-prefix prefill {label}: max |got - ref| = {err[~kept].max():.3e} (bounds {bound[~kept].min():.3e} .. "
          f"{bound[~kept].max():.3e})")
    assert (err[~kept] <= bound[~kept]).all(), (err[~kept].max(), np.flatnonzero(~(err <= bound) & ~kept))


@pytest.mark.parametrize("P", [32, 96, 160])                  # pairs: one (waves 1 - 3 empty), three (uneven), five (wave 0 takes two)
@pytest.mark.parametrize("H,KV,D,form", [(2, 1, 64, "plain"), (2, 1, 64, "coop"), (2, 1, 64, "pack"), (2, 2, 128, "plain"),
                                         (2, 2, 128, "coop")])
@pytest.mark.parametrize("fmt,kv_scale", [("f16", 1.0), ("fp8", 0.37)])
def test_shared_prefix_prefill_matches_fp64_attention(fmt, kv_scale, H, KV, D, form, P):
    case = _case(fmt, H, KV, D, kv_scale, P)
    lens = case[5]
    got = _run(case, fmt, H, KV, D, kv_scale, P, lens, int(lens.max()), **FORMS[form])
    _check(got, case, fmt, D, kv_scale, lens, None, f"{fmt} H={H} KV={KV} D={D} {form} P={P}")


@pytest.mark.parametrize("fmt,kv_scale", [("f16", 1.0), ("fp8", 0.37)])
def test_malformed_sequences_write_nothing_between_healthy_ones(fmt, kv_scale):
    P = 96
    case = _case(fmt, 2, 1, 64, kv_scale, P)
    lens, max_seq_len = case[5].copy(), int(case[5].max())
    lens[1], lens[3] = 2, max_seq_len + 1                      # q_len 3 > seq_len 2; seq_len > max_seq_len
    got = _run(case, fmt, 2, 1, 64, kv_scale, P, lens, max_seq_len)
    _check(got, case, fmt, 64, kv_scale, lens, [True, False, True, False, True], f"{fmt} guards")
