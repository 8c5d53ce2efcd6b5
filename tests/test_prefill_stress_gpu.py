"""ops.paged_attention_prefill (csrc/pa_prefill.hpp over fp16 pages, csrc/pa_prefill_fp8.hpp over fp8-E4M3 pages) where U(-1, 1)
inputs of at most 127 tokens cannot reach: peaked and drifting softmaxes, probabilities that are fp16-subnormal, contexts
of thousands of tokens, blocks beyond 2^32 elements, every E4M3 code through the kernel's own decode, and the guard clauses.

Reference: fp64 causal attention over the same pages, read through the block table (fp8: decoded bytes x kv_scale;
helpers.prefill_reference).  Unowned pool slots and the tails of last blocks hold NaN patterns (0x7E00 / 0x7F); pages are
scattered over a shuffled pool.

Bound.  |got - ref| <= TOL(L) * vmax per row, L the row's seq_len, vmax = 1 for fp16 pages (|v| <= 1 in every case here) and
kv_scale * max |decoded v| for fp8 pages — the largest value an output, a convex combination of V rows, can take.

    TOL(L) = 2^-12 + 2 * 2^-11 + 2 * L * 2^-25

  2^-12      the fp16 output: half an ulp of a value below 1 (x vmax).
  2 * 2^-11  P is rounded to fp16 before the matrix cores, a relative 2^-11 per probability >= 2^-14: once in the numerator
             sum(p v), once in the denominator, which sums the same rounded values.  (The first two terms are the bound of
             tests/test_prefill_gpu.py and tests/test_prefill_fp8_gpu.py.)
  2*L*2^-25  below 2^-14 fp16 is subnormal and the rounding is ABSOLUTE, at most half of 2^-24 per token: at most L * 2^-25
             in the numerator (|v| <= vmax) and L * 2^-25 in the denominator, which is >= 1.
The fp32 accumulations (relative 2^-24 per step) and the fp32 scores are far below these.  helpers.prefill_kernel_model, the
kernel's arithmetic on the CPU, stays below 0.25 * TOL on every profile (tests/test_prefill_stress_model.py); matrix cores
that flushed subnormal P on their side only would exceed TOL 16-fold on the sink profile at these shapes (same file)."""
import numpy as np
import pytest
import torch

from helpers import (E4M3, PROFILES, causal_scores, pack_pages, prefill_reference, prefill_tol, read_pages, score_profile_case,
                     store_rows)

pytestmark = pytest.mark.gpu

SENTINEL = 77.0
SHAPES = [(2, 1, 64), (2, 2, 128)]                                   # (H, KV, D)
FORMATS = [("f16", 1.0), ("fp8", 1.0), ("fp8", 0.37)]                # (pages, kv_scale)
FINITE = np.array([c for c in range(256) if c & 0x7F != 0x7F], np.uint8)        # the 254 E4M3 codes that are not NaN


def _on_device(a):
    a = a.view(np.float16) if a.dtype == np.uint16 else a
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")


def _launch(q, kc, vc, tables, lens, cu, KV, fmt, kv_scale, max_q_len):
    """kc / vc: pool arrays from helpers.pack_pages, or device tensors.  Returns the output on the host, float64."""
    from vllmini_amd import ops

    T, H, D = q.shape
    out = torch.full((T, H, D), SENTINEL, dtype=torch.float16, device="cuda:0")
    kc, vc = (t if torch.is_tensor(t) else _on_device(t) for t in (kc, vc))
    kw = dict(kv_cache_dtype="fp8", kv_scale=kv_scale) if fmt == "fp8" else {}
    ops.paged_attention_prefill(out, _on_device(q), kc, vc, KV, D ** -0.5, _on_device(np.asarray(tables, np.int32)),
                                _on_device(np.asarray(lens, np.int32)), _on_device(np.asarray(cu, np.int32)), max_q_len, 16, **kw)
    torch.cuda.synchronize()
    return out.cpu().numpy().astype(np.float64)


def _check(got, ref, row_len, vmax, what):
    """Rows left out of the reference keep the sentinel; every other row is written, finite and within TOL(L) * vmax."""
    kept = row_len == 0
    assert (got[kept] == SENTINEL).all(), f"{what}: a sequence that must write nothing wrote"
    assert np.isfinite(got[~kept]).all() and not (got[~kept] == SENTINEL).any(), what
    err, bound = np.abs(got[~kept] - ref[~kept]).max(axis=(1, 2)), prefill_tol(row_len[~kept]) * vmax
    worst = int(np.argmax(err / bound))
    print(f"{what}: max |got - ref| = {err.max():.3e} (bound {bound[worst]:.3e} at L = {row_len[~kept][worst]}, "
          f"worst err / bound = {err[worst] / bound[worst]:.3f})")
    assert (err <= bound).all(), (what, err[worst], bound[worst])
    return err.max()


def _batch(rng, q, rows, seqs, KV, D, fmt, kv_scale):
    kc, vc, tables = pack_pages(rng, [(store_rows(k, fmt, kv_scale), store_rows(v, fmt, kv_scale)) for k, v in rows], KV, D, fmt)
    lens = np.array([L for _, L in seqs], np.int32)
    cu = np.concatenate([[0], np.cumsum([ql for ql, _ in seqs])]).astype(np.int32)
    return kc, vc, tables, lens, cu


# ---- 1. adversarial score distributions ----

PROFILE_SEQS = ((1, 512), (17, 517), (65, 512))           # (q_len, seq_len) for (q_len, ctx) = (1, 511), (17, 500), (65, 447)


@pytest.mark.parametrize("fmt,kv_scale", FORMATS)
@pytest.mark.parametrize("H,KV,D", SHAPES)
@pytest.mark.parametrize("profile", PROFILES)
def test_prefill_under_adversarial_score_profiles(profile, H, KV, D, fmt, kv_scale):
    """(a) sink: token 0 is the maximum, every other probability is fp16-subnormal and the V rows are coherent, so that
    mass moves the output; (b) ascending: the running maximum moves in almost every trip; (c) diagonal: every row peaks at
    its own position, each column of the last trip rescales differently; (d) wide: N(0, 8^2) nats; (e) flat: K = 0."""
    rng = np.random.default_rng(D + len(profile))
    q, rows = score_profile_case(rng, profile, PROFILE_SEQS, H, KV, D)
    kc, vc, tables, lens, cu = _batch(rng, q, rows, PROFILE_SEQS, KV, D, fmt, kv_scale)
    ref, row_len, vmax = prefill_reference(q, kc, vc, tables, lens, cu, D ** -0.5, fmt, kv_scale)
    if fmt == "f16":
        vmax = 1.0
    # the profile holds for the rounded (and, for fp8, quantised) rows the kernel reads
    for s, (ql, L) in enumerate(PROFILE_SEQS):
        k, _ = read_pages(kc, vc, tables[s], L, fmt, kv_scale)
        sc = np.stack([causal_scores(q[cu[s]: cu[s + 1]], k, h, H, D ** -0.5) for h in range(H)])       # [H, ql, L]
        seen, top = np.isfinite(sc), sc.max(-1)
        if profile == "sink":               # 9.705 nats = 2^-14: every probability but token 0's is an fp16 subnormal
            assert (sc[..., 0] == 0).all() and (sc[..., 1:][seen[..., 1:]] < -9.71).all() and (sc[seen] > -10.5).all()
        elif profile == "ascending":
            assert 25 < np.median(top) < 50 and (sc[..., 0] < 8).all()
        elif profile == "diagonal":
            assert (np.abs(top - 30) < 3).all() and ((sc > 25).sum(-1) >= L // D - 1).all() and (sc[seen] >= 0).all()
        elif profile == "wide":
            assert 6 < sc[seen].std() < 10
        else:
            assert (sc[seen] == 0).all()
    got = _launch(q, kc, vc, tables, lens, cu, KV, fmt, kv_scale, 65)
    _check(got, ref, row_len, vmax, f"profile {profile} H={H} KV={KV} D={D} {fmt} kv_scale={kv_scale}")


# ---- 2. deep contexts and far blocks ----

DEEP_SEQS = ((1, 2048), (5, 5), (1, 4096), (17, 2057), (16, 53), (90, 2080), (64, 4096))      # two short ones in between


@pytest.mark.parametrize("fmt,kv_scale", FORMATS)
@pytest.mark.parametrize("H,KV,D", SHAPES)
def test_prefill_over_deep_contexts(H, KV, D, fmt, kv_scale):
    """Up to 128 trips of the double-buffered loop: decode through the prefill kernel over 2047 / 4095 cached tokens, chunks
    over long contexts (odd and even block counts: the `min(2*pp+i, nblk-1)` clamp and the last trip's re-read)."""
    rng = np.random.default_rng(7 * D + KV)
    q = (4 * rng.uniform(-1, 1, (sum(ql for ql, _ in DEEP_SEQS), H, D))).astype(np.float16)       # scores: sigma 1.3 nats
    rows = [(rng.uniform(-1, 1, (L, KV, D)), rng.uniform(-1, 1, (L, KV, D))) for _, L in DEEP_SEQS]
    kc, vc, tables, lens, cu = _batch(rng, q, rows, DEEP_SEQS, KV, D, fmt, kv_scale)
    ref, row_len, vmax = prefill_reference(q, kc, vc, tables, lens, cu, D ** -0.5, fmt, kv_scale)
    got = _launch(q, kc, vc, tables, lens, cu, KV, fmt, kv_scale, 90)
    _check(got, ref, row_len, 1.0 if fmt == "f16" else vmax, f"deep contexts H={H} KV={KV} D={D} {fmt} kv_scale={kv_scale}")


@pytest.mark.parametrize("fmt,kv_scale", [("f16", 1.0), ("fp8", 0.37)])
def test_prefill_reads_blocks_beyond_2_to_the_32_elements(fmt, kv_scale):
    """K and V interleaved per block in ONE uninitialised pool of 2^32 elements and a little more (block stride 2 * D * 16):
    one sequence's blocks sit above element offset 2^32, one's above 2^31, one's at the bottom.  Only the owned blocks are
    written (tails NaN), and only they come back to the host: the reference reads what the device holds."""
    H, KV, D, seqs = 2, 1, 128, ((17, 57), (17, 57), (17, 57))
    rng = np.random.default_rng(11)
    q = rng.uniform(-1, 1, (51, H, D)).astype(np.float16)
    rows = [(rng.uniform(-1, 1, (L, KV, D)), rng.uniform(-1, 1, (L, KV, D))) for _, L in seqs]
    kc, vc, tables, lens, cu = _batch(rng, q, rows, seqs, KV, D, fmt, kv_scale)
    stride = 2 * KV * D * 16                                            # elements per block of the interleaved pool
    NB = 2 ** 32 // stride + 24
    far = np.full_like(tables, -1)
    for s, lo in enumerate((2 ** 32 // stride + 1, 2 ** 31 // stride + 1, 0)):        # 4 shuffled blocks out of 20 each
        far[s, :4] = lo + rng.permutation(20)[:4]
    assert (far[0, :4].astype(np.int64) * stride > 2 ** 32).all() and (far[1, :4].astype(np.int64) * stride > 2 ** 31).all()
    assert far.max() < NB and (tables[:, :4] >= 0).all() and (tables[:, 4:] < 0).all()
    small, idx = _on_device(tables[:, :4].reshape(-1).astype(np.int64)), _on_device(far[:, :4].reshape(-1).astype(np.int64))
    pool = torch.empty((NB, 2, *vc.shape[1:]), dtype=torch.float16 if fmt == "f16" else torch.uint8, device="cuda:0")
    kf, vf = pool[:, 0].view(NB, *kc.shape[1:]), pool[:, 1]
    try:
        kf[idx], vf[idx] = _on_device(kc)[small], _on_device(vc)[small]
        got = _launch(q, kf, vf, far, lens, cu, KV, fmt, kv_scale, 17)
        back = [t[idx].cpu().numpy() for t in (kf, vf)]                 # the owned blocks only, gathered on the device
    finally:
        del pool, kf, vf                                                # 8 GiB (fp16) / 4 GiB (fp8): back to the driver now
        torch.cuda.empty_cache()
    local = np.full_like(tables, -1)
    local[:, :4] = np.arange(12).reshape(3, 4)
    kb, vb = (b.view(np.uint16) if fmt == "f16" else b for b in back)
    assert np.array_equal(kb, kc[tables[:, :4].reshape(-1)]) and np.array_equal(vb, vc[tables[:, :4].reshape(-1)])
    ref, row_len, vmax = prefill_reference(q, kb, vb, local, lens, cu, D ** -0.5, fmt, kv_scale)
    _check(got, ref, row_len, 1.0 if fmt == "f16" else vmax, f"far blocks {fmt} kv_scale={kv_scale}")


# ---- 3. every E4M3 code through the fp8 prefill kernel ----

@pytest.mark.parametrize("H,KV,D", SHAPES)
def test_prefill_fp8_v_decode_is_exact_for_every_code(H, KV, D):
    """One-hot q and K (q 32 e_i, K 16 e_t: the selected token is >= 45 nats above the others, whose probabilities round
    to 0 in fp16, its own is exp2(0) = 1, the sum 1): out[j] is the decoded V row of the token row j selects, bit for bit —
    every E4M3 value is an fp16 value.  V rows hold every finite code at every `token % 4` byte of the kernel's V dword."""
    L = D
    seqs = ((L, L), (17, L))                                           # a whole prompt, and a chunk over a cached context
    t, d = np.arange(L)[:, None, None], np.arange(D)[None, None, :]
    v8 = FINITE[(d + D * (t // 4) + 101 * np.arange(KV)[None, :, None]) % 254]                     # [L, KV, D]
    k8 = np.zeros((L, KV, D), np.uint8)
    k8[np.arange(L), :, np.arange(L)] = 0x58                            # 16.0
    assert E4M3[0x58] == 16
    for kv in range(KV):                                                # the coverage this test is about
        for r in range(4):
            assert set(v8[r::4, kv].reshape(-1).tolist()) == set(FINITE.tolist()), (kv, r)
    rng = np.random.default_rng(D)
    kc, vc, tables = pack_pages(rng, [(k8, v8)] * len(seqs), KV, D, "fp8")
    lens = np.array([L for _, L in seqs], np.int32)
    cu = np.concatenate([[0], np.cumsum([ql for ql, _ in seqs])]).astype(np.int32)
    sel = np.concatenate([L - ql + np.arange(ql) for ql, L in seqs])    # the token each row selects: its own position
    q = np.zeros((len(sel), H, D), np.float16)
    q[np.arange(len(sel)), :, sel] = 32
    got = _launch(q, kc, vc, tables, lens, cu, KV, "fp8", 1.0, L)
    want = E4M3[v8][sel][:, np.arange(H) // (H // KV)]                  # [T, H, D]
    assert np.isfinite(want).all() and np.array_equal(want.astype(np.float16).astype(np.float64), want)
    bad = np.argwhere(got != want)                                      # (+-0 compare equal as values; NaN would not)
    assert len(bad) == 0, f"{len(bad)} elements differ, first (row, head, dim) {bad[0]}: got {got[tuple(bad[0])]}, want {want[tuple(bad[0])]}"


def _k_decode_case(H, KV, D):
    """256 sequences of 8 tokens and 8 rows, one per (sign, exponent) bucket x pair of byte positions; head h of sequence s
    probes one dim of K with a one-hot row of magnitude g: score(j, t) = g * K[t][dim] * scale.  Token t holds the bucket's
    mantissa t (the top bucket has 7 finite codes: token 7 repeats the last), so row j sees mantissas 0..j with its own on
    top, and g puts 0.7 nats between neighbouring codes.  Every other K byte is a random finite code (it meets q = 0)."""
    rng = np.random.default_rng(3 * D)
    S, L, scale = 256, 8, D ** -0.5
    k8 = FINITE[rng.integers(0, 254, (S, L, KV, D))]
    v8 = store_rows(rng.uniform(-1, 1, (S, L, KV, D)), "fp8")
    bucket = np.arange(S) // 8                                          # sign * 16 + exponent
    base = ((bucket // 16) << 7 | (bucket % 16) << 3).astype(np.uint8)
    codes = base[:, None] + np.minimum(np.arange(L)[None, :], np.where(bucket % 16 == 15, 6, 7)[:, None]).astype(np.uint8)   # [S, L]
    dim = np.stack([2 * (np.arange(S) % 8) + h + 16 * ((5 * np.arange(S) + h) % (D // 16)) for h in range(H)], 1)      # [S, H]
    step = 2.0 ** (np.maximum(bucket % 16, 1) - 10.0)                   # value of one mantissa step in the bucket
    g = (np.where(bucket // 16, -1.0, 1.0) * 0.7 / (step * scale)).astype(np.float16)                     # [S]
    q = np.zeros((S, L, H, D), np.float16)
    for h in range(H):
        k8[np.arange(S)[:, None], np.arange(L)[None, :], h // (H // KV), dim[:, h, None]] = codes
        q[np.arange(S)[:, None], np.arange(L)[None, :], h, dim[:, h, None]] = g[:, None]
    return k8, v8, q.reshape(S * L, H, D), codes, dim, g


@pytest.mark.parametrize("H,KV,D", SHAPES)
def test_prefill_fp8_k_decode_of_every_code_moves_the_output(H, KV, D):
    """The K operand's decode (both half selects of all four dwords of the 16-byte chunk): the scores ARE the decoded codes,
    0.7 nats apart, and a decode that took any code for its neighbour would move the output by more than 100 x the bound (asserted: > 4 x)."""
    k8, v8, q, codes, dim, g = _k_decode_case(H, KV, D)
    S, L, scale = len(k8), 8, D ** -0.5
    # coverage: every finite code at every byte of the kernel's 16-byte K chunk, among the bytes a query row reads
    covered = {(int(c), int(r)) for h in range(H) for c, r in zip(codes.reshape(-1), np.repeat(dim[:, h] % 16, L))}
    assert covered == {(int(c), r) for c in FINITE for r in range(16)}
    rng = np.random.default_rng(D + 1)
    kc, vc, tables = pack_pages(rng, list(zip(k8, v8)), KV, D, "fp8")
    lens, cu = np.full(S, L, np.int32), (L * np.arange(S + 1)).astype(np.int32)
    ref, row_len, vmax = prefill_reference(q, kc, vc, tables, lens, cu, scale, "fp8")
    tol = prefill_tol(L) * vmax

    # The mutation check, on the CPU, before the GPU result is looked at: decode code c as the NEXT code of its sign (past
    # the last finite one: 480, the value that pattern would have) and the reference of every (sequence, head) that reads
    # c must move by more than 4 * TOL * vmax.  Only the probed bytes matter (the rest meet q = 0), so the attention is
    # recomputed in its compact form: [S, H, rows, tokens] scores from the probed codes alone.
    v = E4M3[v8].transpose(0, 2, 1, 3)[:, np.arange(H) // (H // KV)]                                     # [S, H, L, D]
    mask = np.where(np.tril(np.ones((L, L), bool)), 0.0, -np.inf)

    def compact(values, ss):                                            # values: [..., 8, L] decoded probed codes of sequences ss
        sc = g[ss].astype(np.float64)[:, None, None, None] * values[..., None, None, :] * scale + mask   # [..., 8, 1, L, L]
        p = np.exp(sc - sc.max(-1, keepdims=True))
        return (p / p.sum(-1, keepdims=True)) @ v[ss]                   # [..., 8, H, L, D]

    c256 = np.arange(256)
    nxt = np.where(c256 & 0x7F == 0x7E, np.where(c256 & 0x80, -480.0, 480.0), E4M3[(c256 + 1) % 256])
    ref_c, mutations, least = ref.reshape(S, L, H, D).transpose(0, 2, 1, 3), set(), np.inf
    for b in range(32):                                                 # a (sign, exponent) bucket: 8 sequences, 8 (7) codes
        ss = slice(8 * b, 8 * b + 8)
        plain = compact(E4M3[codes[ss]], ss)
        assert np.abs(plain - ref_c[ss]).max() < 1e-12                  # the compact form IS the reference
        cs = np.unique(codes[ss])
        mutated = np.where(codes[None, ss] == cs[:, None, None], nxt[codes[ss]][None], E4M3[codes[ss]][None])   # [codes, 8, L]
        moved = np.abs(compact(mutated, ss) - plain[None]).max(axis=(-1, -2))                          # [codes, 8, H]
        assert (moved > 4 * tol).all(), (b, moved.min(), 4 * tol)      # at every byte position the code is read from
        mutations |= set(cs.tolist())
        least = min(least, moved.min())
    assert mutations == set(FINITE.tolist())
    print(f"K decode D={D}: the least a mutated code moves the reference is {least:.3e} (4 * TOL * vmax = {4 * tol:.3e})")

    got = _launch(q, kc, vc, tables, lens, cu, KV, "fp8", 1.0, L)
    _check(got, ref, row_len, vmax, f"K decode of every code H={H} KV={KV} D={D}")


# ---- 4. the guards ----

@pytest.mark.parametrize("fmt,kv_scale", FORMATS)
@pytest.mark.parametrize("H,KV,D", SHAPES)
def test_prefill_guards_leave_malformed_sequences_alone(H, KV, D, fmt, kv_scale):
    """The kernel reads cu_q_lens[s], cu_q_lens[s + 1] and seq_lens[s] (all inside their tensors here) and returns on
    `q_len <= 0 || L <= 0 || ctx < 0 || row_lo < 0 || row_hi > num_tokens || blocks > max_blocks_per_seq` before it forms
    any address from them.  Malformed sequences between healthy ones write nothing; the healthy ones are unaffected.

      rows   0..20  healthy (20, 37)
      rows  20..40  seq_len 5 < q_len 20                                   (ctx < 0)
      step  40->30  a negative cu_q_lens step                              (q_len <= 0)
      rows  30..40  healthy (10, 10)   — the rows the sequence above it declined
      rows  40..57  seq_len 200: 13 blocks > the table's 12 columns        (blocks > max_blocks_per_seq)
      step  57->-4  a cu_q_lens entry below zero                           (q_len <= 0)
      rows  -4..60  starts below zero                                      (row_lo < 0)
      rows  60..93  healthy (33, 180)
      rows  93..105 ends at 105 > num_tokens = 100                         (row_hi > num_tokens)"""
    cu = np.array([0, 20, 40, 30, 40, 57, -4, 60, 93, 105], np.int32)
    lens = np.array([37, 5, 9, 10, 200, 9, 70, 180, 30], np.int32)
    healthy = np.array([1, 0, 0, 1, 0, 0, 0, 1, 0], bool)
    T = 100
    rng = np.random.default_rng(D + 13)
    q = rng.uniform(-1, 1, (T, H, D)).astype(np.float16)
    # every sequence owns real blocks for min(seq_len, 180) tokens: a guard that let one through would still read owned memory
    rows = [(rng.uniform(-1, 1, (min(L, 180), KV, D)), rng.uniform(-1, 1, (min(L, 180), KV, D))) for L in lens]
    kc, vc, tables = pack_pages(rng, [(store_rows(k, fmt, kv_scale), store_rows(v, fmt, kv_scale)) for k, v in rows], KV, D, fmt)
    assert tables.shape[1] == 13
    tables = np.ascontiguousarray(tables[:, :12])                      # 180 tokens fill the table's width; 200 do not fit
    ref, row_len, vmax = prefill_reference(q, kc, vc, tables, lens, cu, D ** -0.5, fmt, kv_scale, healthy=healthy)
    assert (row_len > 0).sum() == 63
    got = _launch(q, kc, vc, tables, lens, cu, KV, fmt, kv_scale, 64)
    _check(got, ref, row_len, 1.0 if fmt == "f16" else vmax, f"guards H={H} KV={KV} D={D} {fmt} kv_scale={kv_scale}")
