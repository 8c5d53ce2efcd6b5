"""The chunk cache write (ops.reshape_and_cache_chunks, csrc/pa_cache_chunk.hpp) on the GPU: ONE batch that holds every boundary
case, over pools pre-filled with random bytes — the whole pools must equal the pre-fill with the live positions replaced, bit for
bit, against plain numpy indexing and against the slot operator, which is the definition of the bytes."""
import functools

import numpy as np
import pytest
import torch

from helpers import BS, store_rows

pytestmark = pytest.mark.gpu

MB = 5                                   # table width: 80 tokens
# (q_len, seq_len): one-token and exact blocks, one short / one over, an aligned start with three whole blocks, a start at offset 7
# that ends at offset 8, both ends inside one block, decode rows that complete / open a block, q_len 0, seq_len < q_len, a
# sequence longer than its table (81 tokens), and a healthy one whose middle table entry is -1
SEQS = [(1, 1), (16, 16), (15, 15), (17, 17), (48, 64), (33, 40), (3, 10), (1, 16), (1, 17), (0, 5), (4, 2), (5, 16 * MB + 1), (40, 48)]
HOLE = (len(SEQS) - 1, 1)                # (sequence, table column) of the -1 entry
MAX_Q_LEN = 64                           # above every real q_len
SPECIAL = [np.inf, -np.inf, np.nan, 460, -460, 500, -500, 6e-8, -6e-8, 3e-5]   # saturation, NaN, fp16 subnormals


@functools.lru_cache(maxsize=None)
def batch(KV, D):
    """Tables over a permuted pool, cu_q_lens, and per packed row its slot (-1: not written) — shared by every case."""
    rng = np.random.default_rng(KV * 1000 + D)
    need = len(SEQS) * MB
    perm = rng.permutation(need + 7).astype(np.int32)
    tables = perm[:need].reshape(len(SEQS), MB).copy()
    tables[HOLE] = -1
    cu = np.concatenate([[0], np.cumsum([q for q, _ in SEQS])]).astype(np.int32)
    slots = np.full(cu[-1], -1, np.int64)
    for s, (q, L) in enumerate(SEQS):
        if q <= 0 or L < q or -(-L // BS) > MB:
            continue
        pos = L - q + np.arange(q)
        blk = tables[s, pos // BS].astype(np.int64)
        slots[cu[s]: cu[s + 1]] = np.where(blk >= 0, blk * BS + pos % BS, -1)
    return need + 7, tables, cu, slots


@pytest.mark.parametrize("fmt,kv_scale,special", [("f16", 1.0, False), ("fp8", 1.0, False), ("fp8", 0.5, False),
                                                  ("f16", 1.0, True), ("fp8", 0.37, True)])
@pytest.mark.parametrize("KV,D", [(1, 64), (3, 128)])
def test_chunks_write_exactly_the_slot_operators_bytes(KV, D, fmt, kv_scale, special):
    from vllmini_amd import cache_ops

    NB, tables, cu, slots = batch(KV, D)
    T = int(cu[-1])
    x, dt = (8, np.uint16) if fmt == "f16" else (16, np.uint8)
    rng = np.random.default_rng(7)
    buf = rng.uniform(-3, 3, (T + 3, 3 * KV * D)).astype(np.float16)          # q | k | v: rows past cu[-1] exist
    if special:
        at = rng.integers(0, buf.size, 4000)
        buf.reshape(-1)[at] = np.asarray(SPECIAL, np.float16)[rng.integers(0, len(SPECIAL), at.size)]
    kc0, vc0 = rng.integers(0, 256, (NB, KV, D // x, BS, x * dt().itemsize), np.uint8), rng.integers(0, 256, (NB, KV, D, BS * dt().itemsize), np.uint8)
    dev = torch.device("cuda:0")
    t_buf = torch.from_numpy(buf).to(dev)
    k, v = (t_buf[:T, i * KV * D: (i + 1) * KV * D].view(T, KV, D) for i in (1, 2))
    cdt = torch.float16 if fmt == "f16" else torch.uint8
    pools = lambda: (torch.from_numpy(kc0).to(dev).view(cdt), torch.from_numpy(vc0).to(dev).view(cdt))   # noqa: E731
    name = "auto" if fmt == "f16" else "fp8"
    kc, vc = pools()
    cache_ops.reshape_and_cache_chunks(k, v, kc, vc, torch.from_numpy(tables).to(dev), torch.tensor([L for _, L in SEQS], dtype=torch.int32, device=dev),
                                       torch.from_numpy(cu).to(dev), MAX_Q_LEN, name, kv_scale)
    kc_s, vc_s = pools()
    cache_ops.reshape_and_cache(k, v, kc_s, vc_s, torch.from_numpy(slots).to(dev), name, kv_scale)
    torch.cuda.synchronize()
    got_k, got_v = kc.cpu().numpy().view(dt), vc.cpu().numpy().view(dt)
    assert np.array_equal(got_k, kc_s.cpu().numpy().view(dt)) and np.array_equal(got_v, vc_s.cpu().numpy().view(dt))
    assert not np.array_equal(got_k, kc0.view(dt))               # (something was written)
    if not special:                                              # the same pools by plain indexing: 1.0 and 0.5 divide exactly
        live = slots >= 0
        blk, off = slots[live] // BS, slots[live] % BS
        want_k, want_v = kc0.view(dt).copy(), vc0.view(dt).copy()
        rows_k, rows_v = (store_rows(buf[:T, i * KV * D: (i + 1) * KV * D].reshape(T, KV, D)[live], fmt, kv_scale).view(dt) for i in (1, 2))
        want_k[blk, :, :, off, :] = rows_k.reshape(-1, KV, D // x, x)
        want_v[blk, :, :, off] = rows_v
        assert np.array_equal(got_k, want_k) and np.array_equal(got_v, want_v)


@pytest.mark.parametrize("kv_cache_dtype", ["auto", "fp8"])
def test_decoder_chunks_equals_slots(kv_cache_dtype):
    from vllmini_amd.gpt2_decode import GPT2Dims, GPT2PagedDecoder, random_state_dict
    from vllmini_amd.kv_pool import PagedKVPool

    dims = GPT2Dims(vocab_size=64, n_positions=64, n_embd=128, n_layer=2, n_head=2)
    rng = np.random.default_rng(3)
    prompts = [rng.integers(0, 64, T).tolist() for T in (1, 16, 17, 33, 40)]
    got = {}
    for how in ("slots", "chunks"):
        pool = PagedKVPool(64, 2, 64, 16, 4, 2, device="cuda:0", kv_cache_dtype=kv_cache_dtype, kv_scale=0.5 if kv_cache_dtype == "fp8" else 1.0)
        dec = GPT2PagedDecoder(dims, random_state_dict(dims, "cuda:0"), pool, prefill_attention="auto", prefill_cache_write=how)
        assert dec.prefill_attention == "tiled" and dec.prefill_cache_write == how
        got[how] = (dec.prefill_batch(list(range(5)), prompts), pool.key_cache, pool.value_cache)
    assert all(torch.equal(a, b) for a, b in zip(got["slots"], got["chunks"])) and got["chunks"][1].any()
