#!/usr/bin/env python3
"""The prefill attention launch alone with a token-tree mask (ops.paged_attention_prefill(tree_mask=): the TREE kernels) against the
same call without the keyword on the SAME tensors — max_seq_len given, cooperative=None, pack_heads=None, so every candidate takes
the launch the rules pick, which the keyword does not change.  Record: profiles/prefill_tree.md.

  --mode tree     the cost of the mask: `chain` (all-ones words: the causal result) and `tree` (random-tree words: the parent of
                  node j drawn from {context, 0 .. j - 1}, the word its ancestor closure) against `none`
  --mode base     `none` alone: the launches that existed before the keyword.  --repo DIR imports the package from another
                  checkout (the parent commit, built there), to time both libraries on the same seeded tensors in one job

Per cell (sequences x rows x context x heads x kv heads x head size, and page format) the candidates are alternated inside one
process: warm-up of each, then --pairs rounds of every candidate in turn.  A sample is HIP events on the launch stream around ONE
call, recorded behind a ~1 ms matmul so that the host runs ahead of the device (the events then time the kernels, not the wrapper).
Medians with min - max.  Accuracy: the first sequence against fp64 attention with the same mask over the same (decoded) pages.

  prefill_tree_probe.py --mode tree|base [--out FILE.json] [--pairs 50] [--cells 256x16x1024x32x8x128,...] [--fmts f16,fp8] [--repo DIR]"""
import argparse, json, os, sys
import numpy as np, torch

ap = argparse.ArgumentParser()
ap.add_argument("--mode", required=True, choices=("tree", "base"))
ap.add_argument("--out", default="")
ap.add_argument("--pairs", type=int, default=50)
ap.add_argument("--cells", required=True)
ap.add_argument("--fmts", default="f16,fp8")
ap.add_argument("--repo", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
args = ap.parse_args()
sys.path.insert(0, args.repo)
from vllmini_amd import ops

dev = torch.device("cuda:0")
CUS = torch.cuda.get_device_properties(0).multi_processor_count
blocker = torch.randn(4096, 4096, device=dev)
g = torch.Generator(device=dev).manual_seed(0)


def tree_words(S, Q):
    """[S * Q] int64: every sequence its own random tree of Q nodes"""
    rng, w = np.random.default_rng(2), np.zeros((S, Q), np.uint64)
    for j in range(Q):
        parent = rng.integers(-1, j, S)
        w[:, j] = np.where(parent >= 0, w[np.arange(S), np.maximum(parent, 0)], np.uint64(0)) | (np.uint64(1) << np.uint64(j))
    return torch.from_numpy(w.reshape(-1).view(np.int64)).to(dev)


def make_cell(S, Q, L, H, KV, D, fmt):
    nb = -(-L // 16)
    NB = S * nb + 7
    x = 8 if fmt == "f16" else 16
    kc = torch.randn((NB, KV, D // x, 16, x), device=dev, generator=g)
    vc = torch.randn((NB, KV, D, 16), device=dev, generator=g)
    kc, vc = (kc.half(), vc.half()) if fmt == "f16" else (t.to(torch.float8_e4m3fn).view(torch.uint8) for t in (kc, vc))
    q = torch.randn((S * Q, H, D), device=dev, generator=g).half()
    tables = torch.randperm(NB, device=dev, generator=g)[: S * nb].view(S, nb).to(torch.int32)
    cu = (torch.arange(S + 1, dtype=torch.int32) * Q).to(dev)
    lens = torch.full((S,), L, dtype=torch.int32, device=dev)

    def call(**kw):
        out = torch.empty_like(q)
        ops.paged_attention_prefill(out, q, kc, vc, KV, D ** -0.5, tables, lens, cu, Q, 16, kv_cache_dtype="auto" if fmt == "f16" else "fp8",
                                    kv_scale=1.0, max_seq_len=L, cooperative=None, pack_heads=None, **kw)
        return out

    def reference(words):
        """fp64 attention of the first sequence's rows over its pages under the words' mask (None: causal): [Q, H, D]"""
        dec = (lambda t: t.double()) if fmt == "f16" else (lambda t: t.view(torch.float8_e4m3fn).double())
        own = tables[0].long()
        k = dec(kc[own]).permute(0, 3, 1, 2, 4).reshape(nb * 16, KV, D)[:L].repeat_interleave(H // KV, dim=1)
        v = dec(vc[own]).permute(0, 3, 1, 2).reshape(nb * 16, KV, D)[:L].repeat_interleave(H // KV, dim=1)
        i, j = torch.arange(L, device=dev)[None, :] - (L - Q), torch.arange(Q, device=dev)[:, None]
        seen = i <= j
        if words is not None:
            seen = (i < 0) | (i == j) | ((i < j) & ((words[:Q, None] >> i.clamp(0, 62)) & 1).bool())   # (i < j <= 63: never bit 63)
        s = torch.einsum("qhd,lhd->hql", q[:Q].double(), k) * D ** -0.5
        return torch.einsum("hql,lhd->qhd", torch.softmax(s.masked_fill(~seen[None], float("-inf")), -1), v)
    return call, reference


records = []
for fmt in args.fmts.split(","):
    for cell in args.cells.split(","):
        S, Q, L, H, KV, D = (int(x) for x in cell.split("x"))
        call, reference = make_cell(S, Q, L, H, KV, D, fmt)
        cands = {"none": (lambda: call(), None)}
        if args.mode == "tree":
            chain, tree = torch.full((S * Q,), -1, dtype=torch.int64, device=dev), tree_words(S, Q)
            cands["chain"] = (lambda: call(tree_mask=chain), chain)
            cands["tree"] = (lambda: call(tree_mask=tree), tree)
        pack = ops.prefill_pack_heads_for(Q, H, KV, L, S, CUS)
        coop = not pack and ops.prefill_cooperative_for(Q, L, S, H, CUS)
        plan = ops.prefill_gqa_plan(S * Q, H, D, S, Q, L, KV, CUS) if pack else ops.prefill_split_plan(S * Q, H, D, S, Q, L, CUS)
        launch = {"form": "pack" if pack else "coop" if coop else "plain", "partition_tokens": plan[0], "partitions": plan[1]}
        err = {}
        for name, (fn, words) in cands.items():             # warm-up, and the accuracy of each
            for _ in range(3):
                out = fn()
            err[name] = float((out[:Q].double() - reference(words)).abs().max())
        ev = {name: [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(args.pairs)] for name in cands}
        for r in range(args.pairs):
            for name, (fn, _) in cands.items():             # alternated: a drift of the machine hits every candidate
                torch.mm(blocker, blocker)
                ev[name][r][0].record()
                fn()
                ev[name][r][1].record()
        torch.cuda.synchronize()
        us = {name: np.array([a.elapsed_time(b) * 1e3 for a, b in v]) for name, v in ev.items()}
        records.append({"fmt": fmt, "cell": cell, "launch": launch, "median_us": {k: float(np.median(v)) for k, v in us.items()},
                        "min_max_us": {k: [float(v.min()), float(v.max())] for k, v in us.items()}, "max_abs_err": err})
        print(f"{fmt:3s} {cell:24s} [{launch['form']} x{launch['partitions']}] | " + "  ".join(
            f"{k} {np.median(v):7.1f} ({v.min():.1f}-{v.max():.1f})" for k, v in us.items()) + " | err " + " ".join(f"{k} {e:.1e}" for k, e in err.items()), flush=True)
        if args.out:
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "w") as f:
                json.dump(records, f, indent=1)
        del call, reference, cands
        torch.cuda.empty_cache()
