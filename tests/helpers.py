"""Shared builders for the parity tests (numpy side; the GPU tests upload these)."""
from __future__ import annotations

import numpy as np

BS = 16


def make_case(rng, num_seqs, num_heads, head_size, lens, num_blocks=None, max_blocks=None,
              num_kv_heads=None, kv="uniform", poison_tail=False, q_row_pad=0, block_size=BS):
    """Random paged-KV decode case in the reference layout.

    lens: list of per-sequence context lengths.  Every sequence gets distinct physical blocks in a
    shuffled order; table tails are -1.  With poison_tail the cache slots past each context length
    (and all unowned blocks) hold NaN, which must never leak into the output
    (attention_kernels.cu:302-303, 420-430).  q_row_pad > 0 makes `query` a strided view
    (row stride = (1+q_row_pad)*H*D, like the fused-qkv view at gpt2.py:35-39).
    """
    BS = block_size  # noqa: N806 (shadows the module default on purpose)
    lens = np.asarray(lens, dtype=np.int32)
    assert lens.shape == (num_seqs,)
    num_kv_heads = num_kv_heads or num_heads
    nblk = (lens + BS - 1) // BS
    need = int(nblk.sum())
    num_blocks = num_blocks or max(need + 3, 8)
    max_blocks = max_blocks or max(int(nblk.max()), 1)
    if kv == "uniform":
        kc = rng.uniform(-1, 1, (num_blocks, num_kv_heads, head_size // 8, BS, 8)).astype(np.float16)
        vc = rng.uniform(-1, 1, (num_blocks, num_kv_heads, head_size, BS)).astype(np.float16)
    else:
        kc = rng.standard_normal((num_blocks, num_kv_heads, head_size // 8, BS, 8)).astype(np.float16)
        vc = rng.standard_normal((num_blocks, num_kv_heads, head_size, BS)).astype(np.float16)
    perm = rng.permutation(num_blocks)[:need].astype(np.int32)
    tables = np.full((num_seqs, max_blocks), -1, dtype=np.int32)
    pos = 0
    owned = np.zeros(num_blocks, dtype=bool)
    for s in range(num_seqs):
        n = int(nblk[s])
        tables[s, :n] = perm[pos:pos + n]
        owned[perm[pos:pos + n]] = True
        pos += n
    if poison_tail:
        kc[~owned] = np.nan
        vc[~owned] = np.nan
        for s in range(num_seqs):
            L = int(lens[s])
            if L % BS:
                last = tables[s, nblk[s] - 1]
                kc[last, :, :, L % BS:, :] = np.nan
                vc[last, :, :, L % BS:] = np.nan
    width = (1 + q_row_pad) * num_heads * head_size
    qbuf = rng.standard_normal((num_seqs, width)).astype(np.float16)
    q = qbuf[:, : num_heads * head_size].reshape(num_seqs, num_heads, head_size)  # strided view if padded
    return dict(q=q, qbuf=qbuf, kc=kc, vc=vc, tables=tables, lens=lens, num_kv_heads=num_kv_heads,
                scale=float(head_size) ** -0.5, num_heads=num_heads, head_size=head_size, bs=BS)


def ulp16(x):
    """fp16 unit in the last place at |x| (float64 array)."""
    ax = np.maximum(np.abs(np.asarray(x, dtype=np.float64)), 2.0 ** -14)
    return 2.0 ** (np.floor(np.log2(ax)) - 10)


# ---- tiled prefill attention (ops.paged_attention_prefill): pages, fp64 reference, arithmetic model, score profiles ----

def _e4m3_table():
    c = np.arange(256)
    e, m = (c >> 3) & 15, (c & 7).astype(np.float64)
    val = np.where(e == 0, m / 8 * 2.0 ** -6, (1 + m / 8) * 2.0 ** (e.astype(np.float64) - 7))
    val = np.where(c & 0x80, -val, val)
    val[[0x7F, 0xFF]] = np.nan
    return val


E4M3 = _e4m3_table()          # float64 value of every OCP E4M3 code (0x7F / 0xFF: NaN)
PROFILES = ("sink", "ascending", "diagonal", "wide", "flat")


def prefill_tol(L):
    """Bound on |out - fp64 attention| / vmax for a row over L tokens (derivation: tests/test_prefill_stress_gpu.py)."""
    return 2.0 ** -12 + 2 * 2.0 ** -11 + 2 * np.asarray(L, np.float64) * 2.0 ** -25


def store_rows(x, fmt, kv_scale=1.0):
    """Real-valued K / V rows -> what the cache holds: float16 ("f16"), or E4M3 codes of x / kv_scale ("fp8", saturating)."""
    if fmt == "f16":
        return np.asarray(x).astype(np.float16)
    import torch

    y = np.clip(np.asarray(x, np.float64) / kv_scale, -448, 448).astype(np.float32)
    return torch.from_numpy(y).to(torch.float8_e4m3fn).view(torch.uint8).numpy()


def pack_pages(rng, rows, KV, D, fmt, spare=None):
    """rows: per sequence (k, v), each [L, KV, D] as stored (float16, or uint8 E4M3 codes).  Pages scattered over a shuffled
    pool; unowned slots and the tails of last blocks hold the NaN pattern (0x7E00 / 0x7F).  Returns the raw pool arrays
    (uint16 for "f16": view as float16) and the block tables (-1 past a sequence's blocks, one spare column)."""
    x, nan, dt = (8, 0x7E00, np.uint16) if fmt == "f16" else (16, 0x7F, np.uint8)
    nblk = [-(-len(k) // BS) for k, _ in rows]
    need = sum(nblk)
    NB = need + (need // 4 + 3 if spare is None else spare)
    phys = rng.permutation(NB)[:need]
    kc, vc = np.full((NB, KV, D // x, BS, x), nan, dt), np.full((NB, KV, D, BS), nan, dt)
    tables = np.full((len(rows), max(nblk) + 1), -1, np.int32)
    at = 0
    for s, (k, v) in enumerate(rows):
        n, L = nblk[s], len(k)
        own = phys[at: at + n]
        at += n
        tables[s, :n] = own
        if n == 0:
            continue
        assert k.shape == v.shape == (L, KV, D) and k.dtype.itemsize == v.dtype.itemsize == dt().itemsize
        pk, pv = np.full((n * BS, KV, D), nan, dt), np.full((n * BS, KV, D), nan, dt)
        pk[:L], pv[:L] = k.view(dt), v.view(dt)
        kc[own] = pk.reshape(n, BS, KV, D // x, x).transpose(0, 2, 3, 1, 4)
        vc[own] = pv.reshape(n, BS, KV, D).transpose(0, 2, 3, 1)
    return kc, vc, tables


def read_pages(kc, vc, table_row, L, fmt, kv_scale=1.0):
    """The first L K / V rows of a sequence, read through its block table and decoded to float64: [L, KV, D] each."""
    own = np.asarray(table_row[: -(-L // BS)], np.int64)
    KV, D = vc.shape[1], vc.shape[2]
    k = kc[own].transpose(0, 3, 1, 2, 4).reshape(-1, KV, D)[:L]
    v = vc[own].transpose(0, 3, 1, 2).reshape(-1, KV, D)[:L]
    if fmt == "f16":
        return k.view(np.float16).astype(np.float64), v.view(np.float16).astype(np.float64)
    return E4M3[k] * kv_scale, E4M3[v] * kv_scale


def causal_scores(q_rows, k, h, H, scale):
    """fp64 scores in nats of head h's query rows (the LAST len(q_rows) positions of the sequence); -inf above the diagonal."""
    ql, L = len(q_rows), len(k)
    sc = q_rows[:, h].astype(np.float64) @ k[:, h // (H // k.shape[1])].T * scale
    sc[np.arange(L)[None, :] > (L - ql + np.arange(ql))[:, None]] = -np.inf
    return sc


def prefill_reference(q, kc, vc, tables, lens, cu, scale, fmt, kv_scale=1.0, healthy=None, sentinel=77.0):
    """fp64 causal attention over the same pages, read through the block table (fp8: decoded bytes x kv_scale).  Sequences
    not marked healthy (default: q_len > 0 and seq_len > 0) are left out: their rows hold `sentinel`.  Returns
    (ref [T, H, D], per-row seq_len [T] (0 on left-out rows), vmax = max |decoded v| over the sequences compared)."""
    T, H, _ = q.shape
    ref, row_len, vmax = np.full(q.shape, sentinel, np.float64), np.zeros(T, np.int64), 0.0
    for s, L in enumerate(lens):
        lo, hi = int(cu[s]), int(cu[s + 1])
        if not (hi > lo and L > 0 if healthy is None else healthy[s]):
            continue
        k, v = read_pages(kc, vc, tables[s], int(L), fmt, kv_scale)
        vmax, row_len[lo:hi] = max(vmax, float(np.abs(v).max())), L
        for h in range(H):
            sc = causal_scores(q[lo:hi], k, h, H, scale)
            p = np.exp(sc - sc.max(-1, keepdims=True))
            ref[lo:hi, h] = (p / p.sum(-1, keepdims=True)) @ v[:, h // (H // k.shape[1])]
    return ref, row_len, vmax


def prefill_kernel_model(q_rows, k, v, scale, out_scale=1.0, flush_mfma_subnormals=False):
    """The arithmetic of csrc/pa_prefill.hpp for one sequence on the CPU: a trip per PAIR of blocks, fp32 scores in the
    log2 domain, running max / sum in fp32, P rounded to fp16, the sum taken over the rounded P, fp32 accumulator, fp16
    out.  k / v are the decoded rows WITHOUT kv_scale for fp8 pages (scale = scale * kv_scale, out_scale = kv_scale, as
    the launcher folds them).  flush_mfma_subnormals models matrix cores that read fp16-subnormal P as zero while the sum
    on the VALU keeps them."""
    ql, H, D = q_rows.shape
    L = len(k)
    out = np.empty((ql, H, D), np.float64)
    with np.errstate(under="ignore", over="ignore"):
        for h in range(H):
            g = h // (H // k.shape[1])
            s = (causal_scores(q_rows, k, h, H, 1.0).astype(np.float32) * np.float32(scale * 1.4426950408889634))
            m, lsum, o = np.full(ql, -3.0e38, np.float32), np.zeros(ql, np.float32), np.zeros((ql, D), np.float32)
            for t0 in range(0, L, 2 * BS):
                st = s[:, t0: t0 + 2 * BS]
                m_new = np.maximum(m, st.max(1))
                alpha = np.exp2(m - m_new).astype(np.float32)
                p = np.exp2(st - m_new[:, None]).astype(np.float32).astype(np.float16)
                lsum = lsum * alpha + p.astype(np.float32).sum(1, dtype=np.float32)
                if flush_mfma_subnormals:
                    p = np.where(np.abs(p) < 2.0 ** -14, np.float16(0), p)
                o = o * alpha[:, None] + (p.astype(np.float64) @ v[t0: t0 + 2 * BS, g]).astype(np.float32)
                m = m_new
            out[:, h] = (o * (np.float32(out_scale) / lsum)[:, None]).astype(np.float16)
    return out


def score_profile_case(rng, profile, seqs, H, KV, D):
    """Query rows and REAL-valued K / V rows whose scores follow `profile` along the context (tests/test_prefill_stress_gpu.py).
    seqs: (q_len, seq_len) per sequence.  Returns q [T, H, D] float16 and per sequence (k, v) float64 [L, KV, D], |v| <= 1."""
    scale, g = D ** -0.5, 4.0
    u = rng.uniform(0.5, 1, (KV, D)) * rng.choice([-1.0, 1.0], (KV, D))       # the score direction per kv head
    w = rng.uniform(0.5, 1, (KV, D)) * rng.choice([-1.0, 1.0], (KV, D))       # the sink profile's common V row
    unit = g * (u * u).sum(1) * scale                                           # nats per unit of c_t, per kv head
    gd = (30 / scale) ** 0.5                                                    # diagonal: gd^2 * scale = 30
    qs, rows = [], []
    for ql, L in seqs:
        pos, t = L - ql + np.arange(ql), np.arange(L)
        q, k = np.zeros((ql, H, D)), np.zeros((L, KV, D))
        v = rng.uniform(-1, 1, (L, KV, D))
        if profile == "sink":                    # token 0 at 0 nats, the others 10 +- 0.2 below: P in [2^-24, 2^-14)
            c = -(10 + rng.uniform(-0.2, 0.2, (L, KV))) / unit
            c[0] = 0
            k = c[:, :, None] * u
            v = rng.uniform(0.8, 1, (L, KV, 1)) * w
            v[0] = -w
            q[:] = g * u[np.arange(H) // (H // KV)]
        elif profile in ("ascending", "wide"):   # 40 nats of rise with 2 nats of noise / N(0, 8^2) nats
            target = 40 * t / max(L - 1, 1) + rng.normal(0, 2, L) if profile == "ascending" else rng.normal(0, 8, L)
            k = (target[:, None] / unit)[:, :, None] * u + rng.uniform(-0.02, 0.02, (L, KV, D))
            q = g * u[np.arange(H) // (H // KV)] * np.array([1, 0.9] * H)[:H, None] + rng.uniform(-0.05, 0.05, (ql, H, D))
        elif profile == "diagonal":              # one-hot rows: a row peaks at its own position and every D tokens before
            for h in range(H):
                q[np.arange(ql), h, (pos + 7 * h) % D] = gd
            for kv in range(KV):
                k[t, kv, (t + 7 * kv * (H // KV)) % D] = gd
        else:                                    # flat: K = 0, a uniform average
            assert profile == "flat"
            q = rng.uniform(-1, 1, (ql, H, D))
        qs.append(q.astype(np.float16))
        rows.append((k, v))
    return np.concatenate(qs), rows
