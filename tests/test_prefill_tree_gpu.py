"""ops.paged_attention_prefill(tree_mask=): the TREE form of csrc/pa_prefill.hpp / pa_prefill_fp8.hpp — row j of a chunk attends the
cached context and chunk token i <= j iff bit i of its 64-bit word is set — in the plain, cooperative and head-packed launches, split
or not, against fp64 attention with the same boolean mask over the same NaN-padded, shuffled pages.  Bound per row: helpers.prefill_tol(n)
* vmax, n = the tokens the row attends (selection adds no arithmetic to the kept scores).  Measured maxima: profiles/prefill_tree.md."""
import functools

import numpy as np
import pytest
import torch

import helpers

pytestmark = pytest.mark.gpu

SENTINEL = 77.0
MAX_SEQ_LEN = 1029
# (q_len, seq_len): decode rows; a tree with no context; the tree region inside one pair, across the pair boundary at 32 and over
# three pairs; a 64-row group with more than 16 live rows; bit 63 over ctx = 0; a deep context; the guards
SEQS = [(1, 1), (1, 33), (5, 5), (7, 40), (16, 45), (17, 81), (64, 64), (64, 157), (12, 1029), (0, 7), (3, 0)]
CU = np.concatenate([[0], np.cumsum([q for q, _ in SEQS])]).astype(np.int32)
LENS = np.array([L for _, L in SEQS], np.int32)
FORMS = {"plain": {}, "coop": dict(cooperative=True), "pack": dict(pack_heads=True)}
CONFIGS = [("f16", 1.0, 2, 1, 64), ("fp8", 0.37, 4, 2, 128)]
ONE = np.uint64(1)


@functools.lru_cache(maxsize=None)
def _words(kind):
    """One uint64 per packed row.  "tree": the parent of node j is drawn from {context, 0 .. j - 1}, the word is the ancestor closure;
    "star": the self bit only; "chain": all ones; "dirty": the tree words with random bits above j (and so >= q_len) set."""
    rng, w = np.random.default_rng(7), np.zeros(CU[-1], np.uint64)
    for s, (ql, _) in enumerate(SEQS):
        for j in range(ql):
            parent = int(rng.integers(-1, j))
            w[CU[s] + j] = (w[CU[s] + parent] if parent >= 0 and kind != "star" else np.uint64(0)) | (ONE << np.uint64(j))
    if kind == "dirty":
        j = np.concatenate([np.arange(ql) for ql, _ in SEQS]).astype(np.uint64)
        w |= np.random.default_rng(8).integers(0, 2 ** 64, len(w), dtype=np.uint64) & (~np.uint64(0) << j << ONE)
    return np.full_like(w, ~np.uint64(0)) if kind == "chain" else w


@functools.lru_cache(maxsize=None)
def _case(fmt, kv_scale, H, KV, D):
    rng = np.random.default_rng(D + (fmt == "fp8"))
    rows = [tuple(helpers.store_rows(rng.uniform(-1, 1, (L, KV, D)), fmt, kv_scale) for _ in range(2)) for L in LENS]
    kc, vc, tables = helpers.pack_pages(rng, rows, KV, D, fmt)
    return rng.uniform(-1, 1, (CU[-1], H, D)).astype(np.float16), kc, vc, tables


@functools.lru_cache(maxsize=None)
def _reference(cfg, kind):
    """fp64: -inf where the row does not attend, softmax, . v -> (ref, tokens attended per row, vmax)."""
    fmt, kv_scale, H, KV, D = cfg
    q, kc, vc, tables = _case(*cfg)
    ref, n, vmax, words = np.full(q.shape, SENTINEL, np.float64), np.zeros(len(q), np.int64), 0.0, _words(kind)
    for s, (ql, L) in enumerate(SEQS):
        if ql == 0 or L == 0:
            continue
        k, v = helpers.read_pages(kc, vc, tables[s], L, fmt, kv_scale)
        i, j = np.arange(L)[None, :] - (L - ql), np.arange(ql)[:, None]               # chunk index of a token, of a row
        bit = (words[CU[s]: CU[s + 1], None] >> np.clip(i, 0, 63).astype(np.uint64)) & ONE
        seen = (i < 0) | (i == j) | ((i < j) & (bit == 1))
        vmax, n[CU[s]: CU[s + 1]] = max(vmax, float(np.abs(v).max())), seen.sum(1)
        for h in range(H):
            sc = np.where(seen, q[CU[s]: CU[s + 1], h].astype(np.float64) @ k[:, h // (H // KV)].T * D ** -0.5, -np.inf)
            p = np.exp(sc - sc.max(-1, keepdims=True))
            ref[CU[s]: CU[s + 1], h] = (p / p.sum(-1, keepdims=True)) @ v[:, h // (H // KV)]
    return ref, n, vmax


def _run(cfg, form, partition_tokens, kind):
    from vllmini_amd import ops

    fmt, kv_scale, H, KV, D = cfg
    dev = torch.device("cuda:0")
    q, kc, vc, tables = _case(*cfg)
    if partition_tokens:                                       # a caller's workspace holds anything: hand it over full of NaN
        nbytes = ops.prefill_split_plan(len(q), H, D, len(SEQS), 64, MAX_SEQ_LEN, 256, partition_tokens)[2]
        ops.prefill_workspace_for(0, nbytes).view(torch.float32).fill_(float("nan"))
    kw = {} if kind is None else dict(tree_mask=torch.from_numpy(_words(kind).view(np.int64)).to(dev))
    out = torch.full(q.shape, SENTINEL, dtype=torch.float16, device=dev)
    kc, vc = (torch.from_numpy(a.view(np.float16) if fmt == "f16" else a).to(dev) for a in (kc, vc))
    ops.paged_attention_prefill(out, torch.from_numpy(q).to(dev), kc, vc, KV, D ** -0.5, torch.from_numpy(tables).to(dev),
                                torch.from_numpy(LENS).to(dev), torch.from_numpy(CU).to(dev), 64, 16,
                                kv_cache_dtype="auto" if fmt == "f16" else "fp8", kv_scale=kv_scale, max_seq_len=MAX_SEQ_LEN,
                                partition_tokens=partition_tokens, **FORMS[form], **kw)
    return out.cpu()


@pytest.mark.parametrize("kind", ["tree", "star", "chain"])
@pytest.mark.parametrize("partition_tokens", [None, 32, 64])
@pytest.mark.parametrize("cfg", CONFIGS, ids=lambda c: c[0])
@pytest.mark.parametrize("form", FORMS)
def test_tree_masks_match_fp64_attention(form, cfg, partition_tokens, kind):
    """("star" on (64, 64) at partition_tokens 32: rows 32 .. 63 own a lower partition that holds none of their tokens.)"""
    ref, n, vmax = _reference(cfg, kind)
    bound, kept = helpers.prefill_tol(n) * vmax, n == 0          # kept: rows of the guarded sequences
    if kind != "chain":                                          # the inputs can catch an ignored mask: every tree differs from a chain
        apart = np.abs(ref - _reference(cfg, "chain")[0]).max(axis=(1, 2)) > 4 * bound
        assert all(apart[CU[s]: CU[s + 1]].any() for s, (ql, L) in enumerate(SEQS) if ql >= 5 and L)
    out = _run(cfg, form, partition_tokens, kind)
    got = out.numpy().astype(np.float64)
    assert kept.sum() == 3 and (got[kept] == SENTINEL).all()
    err = np.abs(got - ref).max(axis=(1, 2))                   # (NaN if any output of the row is: the comparison below then fails)
    print(f"tree prefill {cfg[0]} {form} PT={partition_tokens} {kind}: max |got - ref| = {err[~kept].max():.3e} (bounds {bound[~kept].min():.3e} .. {bound[~kept].max():.3e})")
    assert (err[~kept] <= bound[~kept]).all(), (err[~kept].max(), np.flatnonzero(~(err <= bound) & ~kept))
    if kind == "chain":                                          # the same arithmetic on the same values as the causal kernels
        assert torch.equal(out, _run(cfg, form, partition_tokens, None))


@pytest.mark.parametrize("partition_tokens", [None, 32])
@pytest.mark.parametrize("cfg", CONFIGS, ids=lambda c: c[0])
@pytest.mark.parametrize("form", FORMS)
def test_bits_above_a_row_are_ignored(form, cfg, partition_tokens):
    assert (_words("dirty") != _words("tree")).sum() >= 150
    assert torch.equal(_run(cfg, form, partition_tokens, "dirty"), _run(cfg, form, partition_tokens, "tree"))
