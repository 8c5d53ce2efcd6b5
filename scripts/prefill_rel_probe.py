#!/usr/bin/env python3
"""The prefill attention launch alone with ALiBi slopes and a sliding window (ops.paged_attention_prefill(alibi_slopes=,
sliding_window=): the REL kernels) against the same call without the keywords on the SAME tensors — max_seq_len given,
cooperative=None, pack_heads=None, so each call takes the launch its rules pick (with a window: on min(max_seq_len, W + rows - 1)).
Record: profiles/prefill_rel.md.

  --mode alibi    the cost of the term: `alibi` against `none`
  --mode window   what the window buys: `w<W>` for every --windows W against `none`; the plan of each is recorded
  --mode base     `none` alone: the launches that existed before the keywords.  --repo DIR imports the package from another
                  checkout (the parent commit, built there), to time both libraries on the same seeded tensors in one job

Per cell (sequences x rows x context x heads x kv heads x head size, and page format; rows 0: prompts of U{4..context} tokens, a plain
prefill) the candidates are alternated inside one process: warm-up of each, then --pairs rounds of every candidate in turn.  A sample is
HIP events on the launch stream around ONE call, recorded behind a ~1 ms matmul so that the host runs ahead of the device (the events
then time the kernels, not the wrapper).  Medians with min - max.  Accuracy: the first sequence against fp64 attention with the same
two terms over the same (decoded) pages.

  prefill_rel_probe.py --mode alibi|window|base [--out FILE.json] [--pairs 50] [--cells 256x1x1024x32x8x128,...] [--fmts f16,fp8]
                       [--windows 256,1024,4096] [--repo DIR]"""
import argparse, json, os, sys
import numpy as np, torch

ap = argparse.ArgumentParser()
ap.add_argument("--mode", required=True, choices=("alibi", "window", "base"))
ap.add_argument("--out", default="")
ap.add_argument("--pairs", type=int, default=50)
ap.add_argument("--cells", required=True)
ap.add_argument("--fmts", default="f16,fp8")
ap.add_argument("--windows", default="256,1024,4096")
ap.add_argument("--repo", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
args = ap.parse_args()
sys.path.insert(0, args.repo)
from vllmini_amd import ops

dev = torch.device("cuda:0")
CUS = torch.cuda.get_device_properties(0).multi_processor_count
blocker = torch.randn(4096, 4096, device=dev)
g = torch.Generator(device=dev).manual_seed(0)


def make_cell(S, Q, L, H, KV, D, fmt):
    lens = torch.full((S,), L, dtype=torch.int32) if Q else torch.randint(4, L + 1, (S,), generator=torch.Generator().manual_seed(1)).int()
    qlens = torch.full((S,), Q, dtype=torch.int32) if Q else lens
    nb = -(-L // 16)
    NB = S * nb + 7
    x = 8 if fmt == "f16" else 16
    kc = torch.randn((NB, KV, D // x, 16, x), device=dev, generator=g)
    vc = torch.randn((NB, KV, D, 16), device=dev, generator=g)
    kc, vc = (kc.half(), vc.half()) if fmt == "f16" else (t.to(torch.float8_e4m3fn).view(torch.uint8) for t in (kc, vc))
    q = torch.randn((int(qlens.sum()), H, D), device=dev, generator=g).half()
    tables = torch.randperm(NB, device=dev, generator=g)[: S * nb].view(S, nb).to(torch.int32)
    cu = torch.cat([torch.zeros(1, dtype=torch.int32), qlens.cumsum(0).int()]).to(dev)
    slopes = (2.0 ** (-8.0 * torch.arange(1, H + 1) / H)).float().to(dev)
    lens_d, max_q = lens.to(dev), int(qlens.max())

    def call(**kw):
        out = torch.empty_like(q)
        ops.paged_attention_prefill(out, q, kc, vc, KV, D ** -0.5, tables, lens_d, cu, max_q, 16, kv_cache_dtype="auto" if fmt == "f16" else "fp8",
                                    kv_scale=1.0, max_seq_len=L, cooperative=None, pack_heads=None, **kw)
        return out

    def reference(alibi, W):
        """fp64 attention of the first sequence's rows over its pages, with the two terms: [q_len, H, D]"""
        n, ql = int(lens[0]), int(qlens[0])
        dec = (lambda t: t.double()) if fmt == "f16" else (lambda t: t.view(torch.float8_e4m3fn).double())
        own = tables[0].long()
        k = dec(kc[own]).permute(0, 3, 1, 2, 4).reshape(nb * 16, KV, D)[:n].repeat_interleave(H // KV, dim=1)
        v = dec(vc[own]).permute(0, 3, 1, 2).reshape(nb * 16, KV, D)[:n].repeat_interleave(H // KV, dim=1)
        dist = torch.arange(n, device=dev)[None, :] - (n - ql + torch.arange(ql, device=dev))[:, None]        # t - pos
        s = torch.einsum("qhd,lhd->hql", q[:ql].double(), k) * D ** -0.5
        if alibi:
            s += slopes.double()[:, None, None] * dist[None]
        s.masked_fill_(((dist > 0) | (dist <= -(W or n + 1)))[None], float("-inf"))
        return torch.einsum("hql,lhd->qhd", torch.softmax(s, -1), v)
    return call, reference, slopes, max_q, int(qlens.sum())


records = []
for fmt in args.fmts.split(","):
    for cell in args.cells.split(","):
        S, Q, L, H, KV, D = (int(x) for x in cell.split("x"))
        call, reference, slopes, max_q, T = make_cell(S, Q, L, H, KV, D, fmt)
        cands = {"none": (lambda: call(), False, 0)}
        if args.mode == "alibi":
            cands["alibi"] = (lambda: call(alibi_slopes=slopes), True, 0)
        if args.mode == "window":
            for W in (int(w) for w in args.windows.split(",")):
                cands[f"w{W}"] = (lambda W=W: call(sliding_window=W), False, W)
        plans, err = {}, {}
        for name, (fn, alibi, W) in cands.items():          # the launch each takes, warm-up, and the accuracy of each
            depth = min(L, W + max_q - 1) if W else L
            pack = ops.prefill_pack_heads_for(max_q, H, KV, depth, S, CUS)
            coop = not pack and ops.prefill_cooperative_for(max_q, depth, S, H, CUS)
            plan = ops.prefill_gqa_plan(T, H, D, S, max_q, depth, KV, CUS) if pack else ops.prefill_split_plan(T, H, D, S, max_q, depth, CUS)
            plans[name] = {"form": "pack" if pack else "coop" if coop else "plain", "partition_tokens": plan[0], "partitions": plan[1]}
            for _ in range(3):
                out = fn()
            err[name] = float((out[: reference(alibi, W).shape[0]].double() - reference(alibi, W)).abs().max())
        ev = {name: [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(args.pairs)] for name in cands}
        for r in range(args.pairs):
            for name, (fn, _, _) in cands.items():          # alternated: a drift of the machine hits every candidate
                torch.mm(blocker, blocker)
                ev[name][r][0].record()
                fn()
                ev[name][r][1].record()
        torch.cuda.synchronize()
        us = {name: np.array([a.elapsed_time(b) * 1e3 for a, b in v]) for name, v in ev.items()}
        records.append({"fmt": fmt, "cell": cell, "plans": plans, "median_us": {k: float(np.median(v)) for k, v in us.items()},
                        "min_max_us": {k: [float(v.min()), float(v.max())] for k, v in us.items()}, "max_abs_err": err})
        print(f"{fmt:3s} {cell:24s} | " + "  ".join(f"{k} {np.median(v):7.1f} ({v.min():.1f}-{v.max():.1f}) [{plans[k]['form']} x{plans[k]['partitions']}]"
                                                   for k, v in us.items()) + " | err " + " ".join(f"{k} {e:.1e}" for k, e in err.items()), flush=True)
        if args.out:
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "w") as f:
                json.dump(records, f, indent=1)
        del call, reference, cands
        torch.cuda.empty_cache()
