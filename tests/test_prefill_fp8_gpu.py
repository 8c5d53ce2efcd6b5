"""ops.paged_attention_prefill over fp8-E4M3 pages (csrc/pa_prefill_fp8.hpp) against an fp64 causal attention over the DECODED
pages, and GPT2PagedDecoder(prefill_attention="auto") over an fp8 pool against the "positions" path."""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

Q_LENS = (1, 15, 16, 17, 33, 65, 90)
CONTEXTS = (0, 5, 16, 37)
SENTINEL = 77.0
TOL = 1.25e-3   # (2^-12: fp16 out, + 2 * 2^-11: P rounded to fp16) x kv_scale * max |decoded v|, the largest value an output takes


@functools.lru_cache(maxsize=None)
def _case(H, KV, D, kv_scale):
    """One batch of every q_len x context + two empty sequences; shuffled pool, unowned bytes 0x7F (NaN).  Reference: fp64, decoded bytes."""
    rng = np.random.default_rng(H * 1000 + D)
    seqs = [(q, c + q) for q in Q_LENS for c in CONTEXTS] + [(0, 7), (3, 0)]          # (q_len, seq_len)
    seqs = [seqs[i] for i in rng.permutation(len(seqs))]
    nblk = [-(-L // 16) for _, L in seqs]
    NB, MB = 2 * sum(nblk) + 3, max(nblk) + 1
    phys = rng.permutation(NB)[: sum(nblk)]
    kc, vc = torch.full((NB, KV, D // 16, 16, 16), 0x7F, dtype=torch.uint8), torch.full((NB, KV, D, 16), 0x7F, dtype=torch.uint8)
    tables = np.full((len(seqs), MB), -1, np.int32)
    cu = np.concatenate([[0], np.cumsum([q for q, _ in seqs])]).astype(np.int32)
    q = rng.uniform(-1, 1, (cu[-1], H, D)).astype(np.float16)
    ref, vmax, at = np.full((cu[-1], H, D), SENTINEL, np.float64), 0.0, 0
    for s, (ql, L) in enumerate(seqs):
        tables[s, : nblk[s]] = phys[at: at + nblk[s]]
        at += nblk[s]
        k8, v8 = (torch.from_numpy(rng.uniform(-1, 1, (L, KV, D)).astype(np.float32)).to(torch.float8_e4m3fn).view(torch.uint8)
                  for _ in range(2))
        blk, off = torch.from_numpy(tables[s, np.arange(L) // 16].astype(np.int64)), torch.arange(L) % 16
        kc[blk, :, :, off, :], vc[blk, :, :, off] = k8.view(L, KV, D // 16, 16), v8
        if ql == 0 or L == 0:
            continue
        own = torch.from_numpy(tables[s, : nblk[s]].astype(np.int64))              # the reference reads the pages through the table
        pk = kc[own].view(torch.float8_e4m3fn).double().permute(0, 3, 1, 2, 4).reshape(-1, KV, D)[:L].numpy() * kv_scale
        pv = vc[own].view(torch.float8_e4m3fn).double().permute(0, 3, 1, 2).reshape(-1, KV, D)[:L].numpy() * kv_scale
        vmax = max(vmax, float(np.abs(pv).max()))
        for h in range(H):
            sc = q[cu[s]: cu[s + 1], h].astype(np.float64) @ pk[:, h // (H // KV)].T * D ** -0.5          # [ql, L]
            sc[np.arange(L)[None, :] > (L - ql + np.arange(ql))[:, None]] = -np.inf
            p = np.exp(sc - sc.max(-1, keepdims=True))
            ref[cu[s]: cu[s + 1], h] = (p / p.sum(-1, keepdims=True)) @ pv[:, h // (H // KV)]
    assert np.isfinite(ref).all() and vmax > 0
    return q, kc, vc, tables, np.array([L for _, L in seqs], np.int32), cu, ref, vmax


@pytest.mark.parametrize("kv_scale", [1.0, 0.37])
@pytest.mark.parametrize("H,KV,D", [(3, 3, 64), (4, 2, 64), (2, 2, 128)])
def test_prefill_fp8_matches_fp64_attention_over_the_decoded_pages(H, KV, D, kv_scale):
    from vllmini_amd import ops

    dev = torch.device("cuda:0")
    q, kc, vc, tables, lens, cu, ref, vmax = _case(H, KV, D, kv_scale)
    T, qd = q.shape[0], torch.from_numpy(q).to(dev)
    if H == 4:                                                 # the fused projection's strided view
        buf = torch.zeros((T, 3 * H * D), dtype=torch.float16, device=dev)
        buf[:, : H * D] = qd.view(T, H * D)
        qd = buf[:, : H * D].view(T, H, D)
    out = torch.full((T, H, D), SENTINEL, dtype=torch.float16, device=dev)
    cdt = torch.float8_e4m3fn if D == 128 else torch.uint8     # both accepted element types
    ops.paged_attention_prefill(out, qd, kc.to(dev).view(cdt), vc.to(dev).view(cdt), KV, D ** -0.5, torch.from_numpy(tables).to(dev),
                                torch.from_numpy(lens).to(dev), torch.from_numpy(cu).to(dev), max(Q_LENS), 16,
                                kv_cache_dtype="fp8", kv_scale=kv_scale)
    got = out.cpu().numpy().astype(np.float64)
    kept = (ref == SENTINEL).all(axis=(1, 2))                  # rows of the sequence without tokens
    assert kept.sum() == 3 and (got[kept] == SENTINEL).all() and not (got[~kept] == SENTINEL).any()
    err = np.abs(got[~kept] - ref[~kept]).max()                # (NaN if any output is: the comparison below then fails)
    print(f"paged_attention_prefill fp8 H={H} KV={KV} D={D} kv_scale={kv_scale}: max |got - ref| = {err:.3e} (bound {TOL * vmax:.3e})")
    assert err <= TOL * vmax, (err, TOL * vmax)


def _model(n_layer, **dec_kw):
    from vllmini_amd.gpt2_decode import GPT2Dims, GPT2PagedDecoder, random_state_dict
    from vllmini_amd.kv_pool import PagedKVPool

    dev = torch.device("cuda:0")
    dims = GPT2Dims(vocab_size=512, n_positions=256, n_embd=128, n_layer=n_layer, n_head=2)
    pool = PagedKVPool(400, 2, 64, 16, 10, n_layer, device=dev, max_seqs=16, kv_cache_dtype="fp8", kv_scale=0.5)
    g = torch.Generator(device=dev).manual_seed(99)            # stale bytes (NaN codes among them) must never matter
    pool.key_cache.random_(0, 256, generator=g)
    pool.value_cache.random_(0, 256, generator=g)
    sd = {k: v * 4 if k.endswith("weight") and "ln_" not in k else v for k, v in random_state_dict(dims, dev, seed=0).items()}
    sd["lm_head.weight"] = sd["transformer.wte.weight"]
    return GPT2PagedDecoder(dims, sd, pool, **dec_kw)


@pytest.mark.parametrize("n_layer", [1, 3])
def test_prefill_batch_auto_against_positions_over_an_fp8_pool(n_layer):
    """Cache bit-identical where rows do not depend on an attention output (one layer: all; three: layer 0).  One layer: logits
    within test_serve_gpu's bound.  Three: deeper K / V re-quantise differently rounded rows (an fp8 step can flip), so both paths
    are one sample of the same noise around the eager path: auto may be at most twice as far from it as positions."""
    rng = np.random.default_rng(5)
    prompts = [rng.integers(0, 500, n).tolist() for n in (1, 16, 17, 3, 90, 33, 64)]
    ids = list(range(len(prompts)))
    pos, auto = _model(n_layer, prefill_attention="positions"), _model(n_layer, prefill_attention="auto")
    assert auto.prefill_attention == "tiled"
    ref, got = pos.prefill_batch(ids, prompts).float(), auto.prefill_batch(ids, prompts).float()
    assert got.shape == ref.shape and all(np.array_equal(pos.pool.table(i), auto.pool.table(i)) for i in ids)
    first = sorted(int(b) for i in ids for b in pos.pool.table(i)[0] if b >= 0)            # layer 0's blocks
    for a, b in ((pos.pool.key_cache, auto.pool.key_cache), (pos.pool.value_cache, auto.pool.value_cache)):
        assert torch.equal(a[first], b[first]) and (n_layer > 1 or torch.equal(a, b))
    if n_layer == 1:
        err, top = float((got - ref).abs().max()), float(ref.abs().max())
        print(f"fp8 pool, auto vs positions, 1 layer: max |dlogit| = {err:.3e} (max |logit| {top:.2f})")
        assert err <= 2e-2 + 2e-2 * top, err
    else:
        eager = _model(n_layer, paged_prefill=False).prefill_batch(ids, prompts).float()
        e_auto, e_pos = float((got - eager).abs().max()), float((ref - eager).abs().max())
        print(f"fp8 pool, {n_layer} layers, against eager: max |auto - eager| = {e_auto:.3e}, max |positions - eager| = {e_pos:.3e}")
        assert e_auto <= 2 * e_pos, (e_auto, e_pos)
