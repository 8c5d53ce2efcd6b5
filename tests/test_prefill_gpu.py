"""ops.paged_attention_prefill (csrc/pa_prefill.hpp: 16-row query tiles on the matrix cores, online softmax) against an fp64
causal attention over the same pages, and GPT2PagedDecoder(prefill_attention="tiled") against the "positions" path."""
from __future__ import annotations

import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

Q_LENS = (1, 15, 16, 17, 33, 65, 90)
CONTEXTS = (0, 5, 16, 37)
SENTINEL = 77.0
# 2^-12 (fp16 out, |out| <= 1: a convex combination of v) + 2 * 2^-11 (P rounded to fp16: numerator, and the sum of rounded P)
TOL = 1.25e-3


@functools.lru_cache(maxsize=None)
def _case(H, KV, D):
    """Every q_len x context as one batch, plus a sequence without rows and one without tokens; pages scattered over a shuffled
    pool whose unowned slots hold the fp16 NaN pattern.  Returns host tensors and the fp64 reference (computed once)."""
    rng = np.random.default_rng(H * 1000 + D)
    seqs = [(q, c + q) for q in Q_LENS for c in CONTEXTS] + [(0, 7), (3, 0)]          # (q_len, seq_len)
    order = rng.permutation(len(seqs))
    seqs = [seqs[i] for i in order]
    nblk = [-(-L // 16) for _, L in seqs]
    NB, MB = 2 * sum(nblk) + 3, max(nblk) + 1
    phys = rng.permutation(NB)[: sum(nblk)]
    kc = np.full((NB, KV, D // 8, 16, 8), 0x7E00, np.uint16).view(np.float16)
    vc = np.full((NB, KV, D, 16), 0x7E00, np.uint16).view(np.float16)
    tables = np.full((len(seqs), MB), -1, np.int32)
    cu = np.concatenate([[0], np.cumsum([q for q, _ in seqs])]).astype(np.int32)
    q = rng.uniform(-1, 1, (cu[-1], H, D)).astype(np.float16)
    ref = np.full((cu[-1], H, D), SENTINEL, np.float64)
    at = 0
    for s, (ql, L) in enumerate(seqs):
        tables[s, : nblk[s]] = phys[at: at + nblk[s]]
        at += nblk[s]
        k, v = (rng.uniform(-1, 1, (L, KV, D)).astype(np.float16) for _ in range(2))
        for t in range(L):
            b, o = tables[s, t // 16], t % 16
            kc[b, :, :, o, :] = k[t].reshape(KV, D // 8, 8)
            vc[b, :, :, o] = v[t]
        if ql == 0 or L == 0:
            continue
        # the reference reads the pages through the table, like the kernel
        pk = kc[tables[s, : nblk[s]]].transpose(0, 3, 1, 2, 4).reshape(-1, KV, D)[:L].astype(np.float64)
        pv = vc[tables[s, : nblk[s]]].transpose(0, 3, 1, 2).reshape(-1, KV, D)[:L].astype(np.float64)
        for h in range(H):
            sc = q[cu[s]: cu[s + 1], h].astype(np.float64) @ pk[:, h // (H // KV)].T * D ** -0.5          # [ql, L]
            sc[np.arange(L)[None, :] > (L - ql + np.arange(ql))[:, None]] = -np.inf
            p = np.exp(sc - sc.max(-1, keepdims=True))
            ref[cu[s]: cu[s + 1], h] = (p / p.sum(-1, keepdims=True)) @ pv[:, h // (H // KV)]
    lens = np.array([L for _, L in seqs], np.int32)
    return q, kc, vc, tables, lens, cu, ref


@pytest.mark.parametrize("strided", [False, True], ids=["contiguous", "fused_view"])
@pytest.mark.parametrize("H,KV,D", [(3, 3, 64), (4, 2, 64), (2, 2, 128)])
def test_prefill_matches_fp64_attention_over_the_same_pages(H, KV, D, strided):
    from vllmini_amd import ops

    dev = torch.device("cuda:0")
    q, kc, vc, tables, lens, cu, ref = _case(H, KV, D)
    T = q.shape[0]
    qd = torch.from_numpy(q).to(dev)
    if strided:
        buf = torch.zeros((T, 3 * H * D), dtype=torch.float16, device=dev)
        buf[:, : H * D] = qd.view(T, H * D)
        qd = buf[:, : H * D].view(T, H, D)
        assert qd.stride(0) == 3 * H * D
    out = torch.full((T, H, D), SENTINEL, dtype=torch.float16, device=dev)
    ops.paged_attention_prefill(out, qd, torch.from_numpy(kc).to(dev), torch.from_numpy(vc).to(dev), KV, D ** -0.5,
                                torch.from_numpy(tables).to(dev), torch.from_numpy(lens).to(dev), torch.from_numpy(cu).to(dev),
                                max(Q_LENS), 16)
    got = out.cpu().numpy().astype(np.float64)
    kept = (ref == SENTINEL).all(axis=(1, 2))                  # rows of the sequence without tokens
    assert kept.sum() == 3 and (got[kept] == SENTINEL).all()
    assert not (got[~kept] == SENTINEL).any()
    err = np.abs(got[~kept] - ref[~kept]).max()                # (NaN if any output is: the comparison below then fails)
    print(f"paged_attention_prefill H={H} KV={KV} D={D} strided={strided}: max |got - ref| = {err:.3e}")
    assert err <= TOL, err


def _model(num_blocks, n_layer, **dec_kw):
    from vllmini_amd.gpt2_decode import GPT2Dims, GPT2PagedDecoder, random_state_dict
    from vllmini_amd.kv_pool import PagedKVPool

    dev = torch.device("cuda:0")
    dims = GPT2Dims(vocab_size=512, n_positions=256, n_embd=128, n_layer=n_layer, n_head=2)
    pool = PagedKVPool(num_blocks, dims.n_head, dims.head_size, 16, 10, dims.n_layer, device=dev, max_seqs=16)
    g = torch.Generator(device=dev).manual_seed(99)            # stale bytes in unowned blocks must never matter
    pool.key_cache.uniform_(-4, 4, generator=g)
    pool.value_cache.uniform_(-4, 4, generator=g)
    sd = random_state_dict(dims, dev, seed=0)
    for k in sd:
        if k.endswith("weight") and "ln_" not in k:
            sd[k] = sd[k] * 4
    sd["lm_head.weight"] = sd["transformer.wte.weight"]
    return GPT2PagedDecoder(dims, sd, pool, **dec_kw)


@pytest.mark.parametrize("n_layer", [1, 3])
def test_prefill_batch_tiled_against_positions(n_layer):
    """Same tables and blocks; logits within test_serve_gpu's bound.  The cache is written by the same reshape_and_cache from the
    same rows wherever the rows do not depend on an attention output — every layer of the one-layer model, layer 0 of the
    three-layer one: bit-identical there.  Deeper layers' K / V inherit the two attentions' different rounding (fp16-GEMM noise)."""
    rng = np.random.default_rng(5)
    prompts = [rng.integers(0, 500, n).tolist() for n in (1, 16, 17, 3, 90, 33, 64)]
    ids = list(range(len(prompts)))
    pos, tiled = _model(400, n_layer, prefill_attention="positions"), _model(400, n_layer, prefill_attention="tiled")
    ref, got = pos.prefill_batch(ids, prompts), tiled.prefill_batch(ids, prompts)
    torch.cuda.synchronize()
    err = float((got.float() - ref.float()).abs().max())
    print(f"tiled vs positions, {n_layer} layer(s): max |dlogit| = {err:.3e} (max |logit| {float(ref.float().abs().max()):.2f})")
    assert got.shape == ref.shape and err <= 2e-2 + 2e-2 * float(ref.float().abs().max()), err
    for i in ids:
        assert np.array_equal(pos.pool.table(i), tiled.pool.table(i))
        assert pos.pool.allocated_blocks[i] == tiled.pool.allocated_blocks[i]
    first = sorted(int(b) for i in ids for b in pos.pool.table(i)[0] if b >= 0)           # layer 0's blocks
    owned = sorted(b for i in ids for b in pos.pool.allocated_blocks[i])
    for a, b in ((pos.pool.key_cache, tiled.pool.key_cache), (pos.pool.value_cache, tiled.pool.value_cache)):
        assert torch.equal(a[first].view(torch.int16), b[first].view(torch.int16))
        if n_layer == 1:
            assert first == owned and torch.equal(a.view(torch.int16), b.view(torch.int16))
        else:
            assert float((a[owned].float() - b[owned].float()).abs().max()) < 5e-2
