#!/usr/bin/env python3
"""The prefill attention launch alone for short chunks of grouped-query attention: the head-packed form
(ops.paged_attention_prefill(pack_heads=True): a tile's columns are (row, query head of one KV head) pairs, one walk of the context
per KV head) against the launch the operator picks without it (cooperative=None: plain or cooperative by the measured rule), both
with max_seq_len given, so each is split over the context by its own plan.  For one-row cells paged_attention_v1 is timed too, for
the record.  Record: profiles/prefill_gqa.md.

Per cell (sequences x rows x context x heads x kv heads x head size x page format) the candidates are alternated inside one process:
warm-up of each, then --pairs rounds of every candidate in turn.  A sample is HIP events on the launch stream around ONE call,
recorded behind a ~1 ms matmul so that the host runs ahead of the device (the events then time the kernels, not the wrapper).
Medians with min - max.  Accuracy: the first sequence of each cell against fp64 attention over the same (decoded) pages.

  prefill_gqa_probe.py [--out FILE.json] [--pairs 50] [--cells 1x4x32768x32x8x128,...] [--fmts f16,fp8]"""
import argparse, json, os, sys
import numpy as np, torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from vllmini_amd import ops

SHAPES = ("1x4x32768", "4x4x16384", "4x16x16384", "256x1x1024", "256x4x1024", "64x16x4096")
ap = argparse.ArgumentParser()
ap.add_argument("--out", default="")
ap.add_argument("--pairs", type=int, default=50)
ap.add_argument("--cells", default=",".join(f"{s}x{h}x8x128" for h in (32, 64) for s in SHAPES))
ap.add_argument("--fmts", default="f16,fp8")
args = ap.parse_args()

dev = torch.device("cuda:0")
CUS = torch.cuda.get_device_properties(0).multi_processor_count
blocker = torch.randn(4096, 4096, device=dev)
g = torch.Generator(device=dev).manual_seed(0)


def make_cell(S, Q, L, H, KV, D, fmt):
    nb = -(-L // 16)
    NB = S * nb + 7
    x = 8 if fmt == "f16" else 16
    kc = torch.randn((NB, KV, D // x, 16, x), device=dev, generator=g)
    vc = torch.randn((NB, KV, D, 16), device=dev, generator=g)
    if fmt == "f16":
        kc, vc = kc.half(), vc.half()
    else:
        kc, vc = (t.to(torch.float8_e4m3fn).view(torch.uint8) for t in (kc, vc))
    q = torch.randn((S * Q, H, D), device=dev, generator=g).half()
    tables = torch.randperm(NB, device=dev, generator=g)[: S * nb].view(S, nb).to(torch.int32)
    lens = torch.full((S,), L, dtype=torch.int32, device=dev)
    cu = (torch.arange(S + 1, device=dev) * Q).to(torch.int32)
    out = torch.empty_like(q)
    dtype = "auto" if fmt == "f16" else "fp8"

    def call(**kw):
        ops.paged_attention_prefill(out, q, kc, vc, KV, D ** -0.5, tables, lens, cu, Q, 16, kv_cache_dtype=dtype, kv_scale=1.0,
                                    max_seq_len=L, **kw)
        return out

    def decode():
        ops.paged_attention_v1(out, q, kc, vc, KV, D ** -0.5, tables, lens, 16, L, None, dtype, 1.0)
        return out

    def reference():
        """fp64 attention of the first sequence's rows over its pages: [Q, H, D]"""
        dec = (lambda t: t.double()) if fmt == "f16" else (lambda t: t.view(torch.float8_e4m3fn).double())
        own = tables[0].long()
        k = dec(kc[own]).permute(0, 3, 1, 2, 4).reshape(nb * 16, KV, D)[:L]          # [blocks, 16, KV, D/x, x]
        v = dec(vc[own]).permute(0, 3, 1, 2).reshape(nb * 16, KV, D)[:L]
        k, v = (t.repeat_interleave(H // KV, dim=1) for t in (k, v))                  # [L, H, D]
        s = torch.einsum("qhd,lhd->hql", q[:Q].double(), k) * D ** -0.5
        pos = L - Q + torch.arange(Q, device=dev)
        s.masked_fill_(torch.arange(L, device=dev)[None, None, :] > pos[None, :, None], float("-inf"))
        return torch.einsum("hql,lhd->qhd", torch.softmax(s, -1), v)
    return call, decode, reference, Q


records = []
for fmt in args.fmts.split(","):
    for cell in args.cells.split(","):
        S, Q, L, H, KV, D = (int(x) for x in cell.split("x"))
        call, decode, reference, _ = make_cell(S, Q, L, H, KV, D, fmt)
        plans = {"parent": ops.prefill_split_plan(S * Q, H, D, S, Q, L, CUS)[:2],
                 "packed": ops.prefill_gqa_plan(S * Q, H, D, S, Q, L, KV, CUS)[:2]}
        cands = {"parent": lambda: call(cooperative=None), "packed": lambda: call(pack_heads=True)}
        if Q == 1:
            cands["v1"] = decode
        ref = reference()
        err = {}
        for name, fn in cands.items():                       # warm-up, and the accuracy of each
            for _ in range(3):
                o = fn()
            err[name] = float((o[:Q].double() - ref).abs().max())
        ev = {name: [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(args.pairs)]
              for name in cands}
        for r in range(args.pairs):
            for name, fn in cands.items():                   # alternated: a drift of the machine hits every candidate
                torch.mm(blocker, blocker)
                ev[name][r][0].record()
                fn()
                ev[name][r][1].record()
        torch.cuda.synchronize()
        us = {name: np.array([a.elapsed_time(b) * 1e3 for a, b in v]) for name, v in ev.items()}
        records.append({"fmt": fmt, "cell": cell, "plans_pt_parts": plans,
                        "parent_cooperative": ops.prefill_cooperative_for(Q, L, S, H, CUS),
                        "median_us": {k: float(np.median(v)) for k, v in us.items()},
                        "min_max_us": {k: [float(v.min()), float(v.max())] for k, v in us.items()},
                        "max_abs_err_vs_fp64": err})
        print(f"{fmt:3s} {cell:24s} parent pt,parts={plans['parent']} coop={records[-1]['parent_cooperative']} packed "
              f"{plans['packed']} | " + "  ".join(f"{k} {np.median(v):7.1f} ({v.min():.1f}-{v.max():.1f})" for k, v in us.items()) +
              " | err " + " ".join(f"{k} {e:.1e}" for k, e in err.items()), flush=True)
        if args.out:
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "w") as f:
                json.dump(records, f, indent=1)
        del call, decode, reference, cands
        torch.cuda.empty_cache()
