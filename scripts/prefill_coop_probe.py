#!/usr/bin/env python3
"""The prefill attention launch alone for chunks of at most 16 rows: the plain tile kernels (one wave of four walks the context)
against the cooperative form (ops.paged_attention_prefill(cooperative=True): the four waves share it and merge in LDS).  Record:
profiles/prefill_coop.md.

Per cell (sequences x rows x context x heads x page format) four candidates — plain unsplit, plain under the split rule,
cooperative unsplit, cooperative under the split rule (each side's best of its two is what the note compares) — are alternated
inside one process: warm-up of each, then --pairs rounds of every candidate in turn.  A sample is HIP events on the launch stream
around ONE call, recorded behind a ~1 ms matmul so that the host runs ahead of the device (the events then time the kernels, not
the wrapper).  Medians with min - max; every candidate's output is compared with the plain unsplit launch's on the same inputs.
--forced adds both forms at forced partition sizes (does the best partition count move once a workgroup is faster?).

  prefill_coop_probe.py [--out FILE.json] [--pairs 50] [--cells 1x16x32768x12x12x64,...] [--fmts f16,fp8] [--forced 512,2048]
  cell = sequences x rows x context x heads x kv_heads x head_size"""
import argparse, json, os, sys
import numpy as np, torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from vllmini_amd import ops

SWEEP = ",".join(f"64x16x{L}x12x12x64" for L in (64, 128, 256, 512, 1024, 2048, 4096))
ap = argparse.ArgumentParser()
ap.add_argument("--out", default="")
ap.add_argument("--pairs", type=int, default=50)
ap.add_argument("--cells", default="1x16x32768x12x12x64,4x16x16384x32x8x128,256x4x1024x12x12x64," + SWEEP)
ap.add_argument("--fmts", default="f16,fp8")
ap.add_argument("--forced", type=lambda s: [int(x) for x in s.split(",") if x], default=[])
args = ap.parse_args()

dev = torch.device("cuda:0")
CUS = torch.cuda.get_device_properties(0).multi_processor_count
blocker = torch.randn(4096, 4096, device=dev)
g = torch.Generator(device=dev).manual_seed(0)


def make_cell(S, Q, L, H, KV, D, fmt):
    nb = -(-L // 16)
    NB = S * nb + 7
    if fmt == "f16":
        kc = torch.randn((NB, KV, D // 8, 16, 8), device=dev, generator=g).half()
        vc = torch.randn((NB, KV, D, 16), device=dev, generator=g).half()
    else:
        kc = torch.randn((NB, KV, D // 16, 16, 16), device=dev, generator=g).to(torch.float8_e4m3fn).view(torch.uint8)
        vc = torch.randn((NB, KV, D, 16), device=dev, generator=g).to(torch.float8_e4m3fn).view(torch.uint8)
    q = torch.randn((S * Q, H, D), device=dev, generator=g).half()
    tables = torch.randperm(NB, device=dev, generator=g)[: S * nb].view(S, nb).to(torch.int32)
    lens = torch.full((S,), L, dtype=torch.int32, device=dev)
    cu = (torch.arange(S + 1, device=dev) * Q).to(torch.int32)
    out = torch.empty_like(q)

    def call(**kw):
        ops.paged_attention_prefill(out, q, kc, vc, KV, D ** -0.5, tables, lens, cu, Q, 16,
                                    kv_cache_dtype="auto" if fmt == "f16" else "fp8", kv_scale=1.0, **kw)
        return out
    return call


records = []
for fmt in args.fmts.split(","):
    for cell in args.cells.split(","):
        S, Q, L, H, KV, D = (int(x) for x in cell.split("x"))
        call = make_cell(S, Q, L, H, KV, D, fmt)
        plan = ops.prefill_split_plan(S * Q, H, D, S, Q, L, CUS)
        cands = {"plain": {}, "plain_rule": dict(max_seq_len=L), "coop": dict(cooperative=True),
                 "coop_rule": dict(cooperative=True, max_seq_len=L)}
        for pt in args.forced:
            if pt < L:
                cands[f"plain_pt{pt}"] = dict(max_seq_len=L, partition_tokens=pt)
                cands[f"coop_pt{pt}"] = dict(cooperative=True, max_seq_len=L, partition_tokens=pt)
        base = call().clone()
        diff = {}
        for name, kw in cands.items():                       # warm-up, and the outputs side by side
            for _ in range(3):
                o = call(**kw)
            diff[name] = float((o.float() - base.float()).abs().max())
        ev = {name: [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(args.pairs)]
              for name in cands}
        for r in range(args.pairs):
            for name, kw in cands.items():                   # alternated: a drift of the machine hits every candidate
                torch.mm(blocker, blocker)
                ev[name][r][0].record()
                call(**kw)
                ev[name][r][1].record()
        torch.cuda.synchronize()
        us = {name: np.array([a.elapsed_time(b) * 1e3 for a, b in v]) for name, v in ev.items()}
        records.append({"fmt": fmt, "cell": cell, "rule_plan": plan,
                        "median_us": {k: float(np.median(v)) for k, v in us.items()},
                        "min_max_us": {k: [float(v.min()), float(v.max())] for k, v in us.items()},
                        "max_abs_diff_vs_plain": diff})
        print(f"{fmt:3s} {cell:24s} rule pt={plan[0]} parts={plan[1]} | " +
              "  ".join(f"{k} {np.median(v):7.1f} ({v.min():.1f}-{v.max():.1f})" for k, v in us.items()) +
              f" | max|d| {max(diff.values()):.1e}", flush=True)
        if args.out:
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "w") as f:
                json.dump(records, f, indent=1)
        del call
        torch.cuda.empty_cache()
