"""ops.paged_attention_prefill(alibi_slopes=, sliding_window=): the REL form of csrc/pa_prefill.hpp / pa_prefill_fp8.hpp — the row at
pos attends tokens pos - W < t <= pos and scores them scale * q . k + slope[h] * (t - pos) — in the plain, cooperative and head-packed
launches, split or not, against fp64 attention with the same two terms over the same NaN-padded, shuffled pages.  Bound per row:
helpers.prefill_tol(n) * vmax, n = the tokens the row attends.  The ALiBi term adds one fp32 rounding of x = |bias| to a weight
~ e^-x: at most 2^-24 x e^-x <= 2^-24 / e relative per probability, inside the bound's 2 n 2^-25 term.  Measured maxima:
profiles/prefill_rel.md."""
import functools

import numpy as np
import pytest
import torch

import helpers

pytestmark = pytest.mark.gpu

SENTINEL = 77.0
MAX_SEQ_LEN = 1029
# (q_len, seq_len): a window inside one pair, across pairs and across partitions; partitions wholly below a window; W larger than a
# context; groups of more (17, 80, 70) and of fewer than 16 live rows; a deep row; the guards
SEQS = [(1, 1), (1, 33), (1, 129), (5, 133), (16, 160), (17, 40), (80, 80), (70, 200), (5, 1029), (0, 7), (3, 0)]
CU = np.concatenate([[0], np.cumsum([q for q, _ in SEQS])]).astype(np.int32)
LENS = np.array([L for _, L in SEQS], np.int32)
FORMS = {"plain": {}, "coop": dict(cooperative=True), "pack": dict(pack_heads=True)}
CONFIGS = [("f16", 1.0, 2, 1, 64), ("fp8", 0.37, 4, 2, 128)]
SLOPES = {None: lambda H: None, "alibi": lambda H: 2.0 ** (-8.0 * np.arange(1, H + 1) / H), "ones": np.ones, "zeros": np.zeros}


@functools.lru_cache(maxsize=None)
def _case(fmt, kv_scale, H, KV, D):
    rng = np.random.default_rng(D + (fmt == "fp8"))
    rows = [tuple(helpers.store_rows(rng.uniform(-1, 1, (L, KV, D)), fmt, kv_scale) for _ in range(2)) for L in LENS]
    kc, vc, tables = helpers.pack_pages(rng, rows, KV, D, fmt)
    return rng.uniform(-1, 1, (CU[-1], H, D)).astype(np.float16), kc, vc, tables


@functools.lru_cache(maxsize=None)
def _reference(cfg, W, slopes):
    """fp64: scores + slope * (t - pos), -inf outside (pos - W, pos], softmax, . v -> (ref, tokens attended per row, vmax)."""
    fmt, kv_scale, H, KV, D = cfg
    q, kc, vc, tables = _case(*cfg)
    ref, n, vmax = np.full(q.shape, SENTINEL, np.float64), np.zeros(len(q), np.int64), 0.0
    sl = np.zeros(H) if slopes is None else SLOPES[slopes](H)
    for s, (ql, L) in enumerate(SEQS):
        if ql == 0 or L == 0:
            continue
        k, v = helpers.read_pages(kc, vc, tables[s], L, fmt, kv_scale)
        dist = np.arange(L)[None, :] - (L - ql + np.arange(ql))[:, None]           # t - pos
        seen = (dist <= 0) & (dist > -(W or L + 1))
        vmax, n[CU[s]: CU[s + 1]] = max(vmax, float(np.abs(v).max())), seen.sum(1)
        for h in range(H):
            sc = np.where(seen, q[CU[s]: CU[s + 1], h].astype(np.float64) @ k[:, h // (H // KV)].T * D ** -0.5 + sl[h] * dist, -np.inf)
            p = np.exp(sc - sc.max(-1, keepdims=True))
            ref[CU[s]: CU[s + 1], h] = (p / p.sum(-1, keepdims=True)) @ v[:, h // (H // KV)]
    return ref, n, vmax


def _run(cfg, form, partition_tokens=None, W=None, slopes=None, pages=None, **kw):
    from vllmini_amd import ops

    fmt, kv_scale, H, KV, D = cfg
    dev = torch.device("cuda:0")
    q, kc, vc, tables = (*_case(*cfg)[:1], *pages) if pages else _case(*cfg)
    if partition_tokens:                                       # a caller's workspace holds anything: hand it over full of NaN
        nbytes = ops.prefill_split_plan(len(q), H, D, len(SEQS), 80, MAX_SEQ_LEN, 256, partition_tokens)[2]   # (a window needs less)
        ops.prefill_workspace_for(0, nbytes).view(torch.float32).fill_(float("nan"))
    if slopes is not None:
        kw["alibi_slopes"] = torch.from_numpy(SLOPES[slopes](H).astype(np.float32)).to(dev)
    if W is not None:
        kw["sliding_window"] = W
    out = torch.full(q.shape, SENTINEL, dtype=torch.float16, device=dev)
    kc, vc = (torch.from_numpy(a.view(np.float16) if fmt == "f16" else a).to(dev) for a in (kc, vc))
    ops.paged_attention_prefill(out, torch.from_numpy(q).to(dev), kc, vc, KV, D ** -0.5, torch.from_numpy(tables).to(dev),
                                torch.from_numpy(LENS).to(dev), torch.from_numpy(CU).to(dev), 80, 16,
                                kv_cache_dtype="auto" if fmt == "f16" else "fp8", kv_scale=kv_scale, max_seq_len=MAX_SEQ_LEN,
                                partition_tokens=partition_tokens, **FORMS[form], **kw)
    return out.cpu()


def _check(out, ref, n, vmax, label):
    got, kept = out.numpy().astype(np.float64), n == 0           # kept: rows of the guarded sequences
    assert kept.sum() == 3 and (got[kept] == SENTINEL).all()
    err = np.abs(got - ref).max(axis=(1, 2))                   # (NaN if any output of the row is: the comparison below then fails)
    bound = helpers.prefill_tol(n) * vmax
    print(f"rel prefill {label}: max |got - ref| = {err[~kept].max():.3e} (bounds {bound[~kept].min():.3e} .. {bound[~kept].max():.3e})")
    assert (err[~kept] <= bound[~kept]).all(), (err[~kept].max(), np.flatnonzero(~(err <= bound) & ~kept))


@pytest.mark.parametrize("W,slopes", [(None, "alibi"), (33, None), (100, "alibi"), (1, "ones")])
@pytest.mark.parametrize("partition_tokens", [None, 32, 160])
@pytest.mark.parametrize("cfg", CONFIGS, ids=lambda c: c[0])
@pytest.mark.parametrize("form", FORMS)
def test_alibi_and_window_match_fp64_attention(form, cfg, partition_tokens, W, slopes):
    out = _run(cfg, form, partition_tokens, W, slopes)
    _check(out, *_reference(cfg, W, slopes), f"{cfg[0]} {form} PT={partition_tokens} W={W} slopes={slopes}")
    assert torch.equal(out, _run(cfg, form, partition_tokens, W, slopes))      # fixed merge orders, no atomics


@pytest.mark.parametrize("W", [33, 100])
@pytest.mark.parametrize("partition_tokens", [None, 32])
@pytest.mark.parametrize("cfg", CONFIGS, ids=lambda c: c[0])
@pytest.mark.parametrize("form", FORMS)
def test_blocks_below_the_window_are_never_read(form, cfg, partition_tokens, W):
    """THE WINDOW CONTRACT: every block wholly below lo = max(0, seq_len - q_len - W + 1) is overwritten with NaN in the pool and
    its table entry pointed at one in-range block full of NaN; the result is the untouched run's, bit for bit."""
    _, kc, vc, tables = _case(*cfg)
    kc, vc, poisoned = kc.copy(), vc.copy(), tables.copy()
    nan_block = np.setdiff1d(np.arange(len(kc)), tables)[0]      # a block nobody owns: pack_pages left it full of NaN
    for s, (ql, L) in enumerate(SEQS):
        freed = max(0, L - ql - W + 1) // 16
        kc[tables[s, :freed]], vc[tables[s, :freed]] = kc[nan_block], vc[nan_block]
        poisoned[s, :freed] = nan_block
    assert (poisoned != tables).sum() >= 60                      # (5, 1029) alone frees 58 blocks at W = 100
    out = _run(cfg, form, partition_tokens, W, "alibi", pages=(kc, vc, poisoned))
    assert torch.equal(out, _run(cfg, form, partition_tokens, W, "alibi"))


@pytest.mark.parametrize("cfg", CONFIGS, ids=lambda c: c[0])
@pytest.mark.parametrize("form", FORMS)
def test_a_wide_window_and_zero_slopes_are_plain_causal_attention(form, cfg):
    plain = _reference(cfg, None, None)
    _check(_run(cfg, form, W=MAX_SEQ_LEN), *plain, f"{cfg[0]} {form} W >= seq_len")
    _check(_run(cfg, form, 160, slopes="zeros"), *plain, f"{cfg[0]} {form} zero slopes")
    assert torch.equal(_run(cfg, form, 32, alibi_slopes=None, sliding_window=None), _run(cfg, form, 32))
