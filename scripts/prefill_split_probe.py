#!/usr/bin/env python3
"""The prefill attention launch alone, unsplit against split over the context (ops.paged_attention_prefill with max_seq_len /
partition_tokens), for few rows over a deep cache.  Record: profiles/prefill_split.md.

Per cell (sequences x chunk rows x context x heads x page format) the candidates — the unsplit launch, the split at forced
partition sizes, the library's rule — are alternated inside one process: warm-up of each, then --pairs rounds of every candidate
in turn.  A sample is HIP events on the launch stream around ONE call, recorded behind a ~1 ms matmul so that the host runs ahead
of the device (the events then time the kernels, not the wrapper).  Medians with min - max; every candidate's output is compared
with the unsplit launch's on the same inputs.

  prefill_split_probe.py [--out FILE.json] [--pairs 50] [--seqs 1,4] [--chunks 16,256,1024] [--contexts 4096,16384,32768]
                         [--heads 12x12x64,32x8x128] [--fmts f16,fp8] [--forced 256,512,1024,2048]
  prefill_split_probe.py --trace PT ...     warm-up + 20 calls of ONE candidate (PT = 0: the rule, -1: unsplit) of the first cell:
                                            run under `rocprofv3 --kernel-trace --stats -- python scripts/prefill_split_probe.py
                                            --trace 0 ...` and read the partition and merge kernels' times."""
import argparse, json, os, sys
import numpy as np, torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from vllmini_amd import ops

ints = lambda s: [int(x) for x in s.split(",") if x]          # noqa: E731
ap = argparse.ArgumentParser()
ap.add_argument("--out", default="")
ap.add_argument("--pairs", type=int, default=50)
ap.add_argument("--seqs", type=ints, default=[1, 4])
ap.add_argument("--chunks", type=ints, default=[16, 256, 1024])
ap.add_argument("--contexts", type=ints, default=[4096, 16384, 32768])
ap.add_argument("--heads", default="12x12x64,32x8x128")
ap.add_argument("--fmts", default="f16,fp8")
ap.add_argument("--forced", type=ints, default=[256, 512, 1024, 2048])
ap.add_argument("--trace", type=int, default=None)
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


def candidates(L):
    c = {"unsplit": {}}
    for pt in args.forced:
        if pt < L:
            c[f"pt{pt}"] = dict(max_seq_len=L, partition_tokens=pt)
    c["rule"] = dict(max_seq_len=L)
    return c


records = []
for fmt in args.fmts.split(","):
    for hs in args.heads.split(","):
        H, KV, D = (int(x) for x in hs.split("x"))
        for S in args.seqs:
            for Q in args.chunks:
                for L in args.contexts:
                    call = make_cell(S, Q, L, H, KV, D, fmt)
                    cands = candidates(L)
                    plan = ops.prefill_split_plan(S * Q, H, D, S, Q, L, CUS)
                    if args.trace is not None:
                        kw = {} if args.trace < 0 else dict(max_seq_len=L, **({"partition_tokens": args.trace} if args.trace else {}))
                        for _ in range(24):
                            call(**kw)
                        torch.cuda.synchronize()
                        print(f"trace {fmt} {hs} S={S} Q={Q} L={L} {kw} (rule's plan: {plan})", flush=True)
                        sys.exit(0)
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
                    rec = {"fmt": fmt, "heads": hs, "seqs": S, "chunk": Q, "context": L, "rule_plan": plan,
                           "unsplit_workgroups": -(-Q // 64) * S * H,
                           "median_us": {k: float(np.median(v)) for k, v in us.items()},
                           "min_max_us": {k: [float(v.min()), float(v.max())] for k, v in us.items()},
                           "max_abs_diff_vs_unsplit": diff}
                    records.append(rec)
                    print(f"{fmt:3s} {hs:9s} S={S} Q={Q:4d} L={L:5d} rule pt={plan[0]} parts={plan[1]} | " +
                          "  ".join(f"{k} {np.median(v):8.1f} ({v.min():.1f}-{v.max():.1f})" for k, v in us.items()) +
                          f" | max|d| {max(diff.values()):.1e}", flush=True)
                    if args.out:
                        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
                        with open(args.out, "w") as f:
                            json.dump(records, f, indent=1)
                    del call
                    torch.cuda.empty_cache()
