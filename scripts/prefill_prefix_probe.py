#!/usr/bin/env python3
"""The prefill attention launch alone on a batch whose sequences share a prompt prefix: ops.paged_attention_prefill(shared_prefix_len=P)
— prefix tiles over the packed batch, the suffix launch from partition 1 on, the merge launch — against the launch the operator picks
without the keyword on the SAME tensors (max_seq_len given, cooperative=None, pack_heads=None: one launch, or split by the library's
rule).  The block tables are valid per sequence (every row names the shared blocks), so both routes compute the same operator.
Record: profiles/prefill_prefix.md.

Per cell (sequences x rows x prefix x seq_len x heads x kv heads x head size, and page format) the two candidates are alternated inside
one process: warm-up of each, then --pairs rounds of both in turn.  A sample is HIP events on the launch stream around ONE call,
recorded behind a ~1 ms matmul so that the host runs ahead of the device (the events then time the kernels, not the wrapper).
Medians with min - max.  Accuracy: the first sequence of each cell against fp64 attention over the same (decoded) pages, and the largest
difference between the two routes over all rows.

  prefill_prefix_probe.py [--out FILE.json] [--pairs 50] [--cells 256x1x512x1024x12x12x64,...] [--fmts f16,fp8]"""
import argparse, json, os, sys
import numpy as np, torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from vllmini_amd import ops

CELLS = ("256x1x512x1024x12x12x64", "256x1x2048x2304x32x8x128", "64x16x1024x1536x32x8x128", "8x256x2048x2304x32x8x128",
         "256x1x32x544x12x12x64", "256x1x64x576x12x12x64", "256x1x128x640x12x12x64", "256x1x256x768x12x12x64",
         "256x1x512x1024x32x8x128")
ap = argparse.ArgumentParser()
ap.add_argument("--out", default="")
ap.add_argument("--pairs", type=int, default=50)
ap.add_argument("--cells", default=",".join(CELLS))
ap.add_argument("--fmts", default="f16,fp8")
args = ap.parse_args()

dev = torch.device("cuda:0")
CUS = torch.cuda.get_device_properties(0).multi_processor_count
blocker = torch.randn(4096, 4096, device=dev)
g = torch.Generator(device=dev).manual_seed(0)


def make_cell(S, Q, P, L, H, KV, D, fmt):
    nb, npre = -(-L // 16), P // 16
    NB = npre + S * (nb - npre) + 7
    x = 8 if fmt == "f16" else 16
    kc = torch.randn((NB, KV, D // x, 16, x), device=dev, generator=g)
    vc = torch.randn((NB, KV, D, 16), device=dev, generator=g)
    if fmt == "f16":
        kc, vc = kc.half(), vc.half()
    else:
        kc, vc = (t.to(torch.float8_e4m3fn).view(torch.uint8) for t in (kc, vc))
    q = torch.randn((S * Q, H, D), device=dev, generator=g).half()
    perm = torch.randperm(NB, device=dev, generator=g).to(torch.int32)
    tables = torch.cat([perm[:npre].expand(S, npre), perm[npre: npre + S * (nb - npre)].view(S, nb - npre)], dim=1).contiguous()
    lens = torch.full((S,), L, dtype=torch.int32, device=dev)
    cu = (torch.arange(S + 1, device=dev) * Q).to(torch.int32)
    dtype = "auto" if fmt == "f16" else "fp8"

    def call(**kw):
        out = torch.empty_like(q)
        ops.paged_attention_prefill(out, q, kc, vc, KV, D ** -0.5, tables, lens, cu, Q, 16, kv_cache_dtype=dtype, kv_scale=1.0,
                                    max_seq_len=L, cooperative=None, pack_heads=None, **kw)
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
    return call, reference


records = []
for fmt in args.fmts.split(","):
    for cell in args.cells.split(","):
        S, Q, P, L, H, KV, D = (int(x) for x in cell.split("x"))
        call, reference = make_cell(S, Q, P, L, H, KV, D, fmt)
        plan = ops.prefill_split_plan(S * Q, H, D, S, Q, L, CUS)[:2]
        cands = {"parent": lambda: call(), "shared": lambda: call(shared_prefix_len=P)}
        ref = reference()
        err, outs = {}, {}
        for name, fn in cands.items():                       # warm-up, and the accuracy of each
            for _ in range(3):
                outs[name] = fn()
            err[name] = float((outs[name][:Q].double() - ref).abs().max())
        err["shared_vs_parent"] = float((outs["shared"].double() - outs["parent"].double()).abs().max())
        ev = {name: [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(args.pairs)]
              for name in cands}
        for r in range(args.pairs):
            for name, fn in cands.items():                   # alternated: a drift of the machine hits both candidates
                torch.mm(blocker, blocker)
                ev[name][r][0].record()
                fn()
                ev[name][r][1].record()
        torch.cuda.synchronize()
        us = {name: np.array([a.elapsed_time(b) * 1e3 for a, b in v]) for name, v in ev.items()}
        records.append({"fmt": fmt, "cell": cell, "parent_plan_pt_parts": plan,
                        "coop_rule": ops.prefill_cooperative_for(Q, L, S, H, CUS),
                        "pack_rule": ops.prefill_pack_heads_for(Q, H, KV, L, S, CUS),
                        "median_us": {k: float(np.median(v)) for k, v in us.items()},
                        "min_max_us": {k: [float(v.min()), float(v.max())] for k, v in us.items()},
                        "max_abs_err": err})
        print(f"{fmt:3s} {cell:28s} parent pt,parts={plan} coop={records[-1]['coop_rule']} pack={records[-1]['pack_rule']} | " +
              "  ".join(f"{k} {np.median(v):7.1f} ({v.min():.1f}-{v.max():.1f})" for k, v in us.items()) +
              " | err " + " ".join(f"{k} {e:.1e}" for k, e in err.items()), flush=True)
        if args.out:
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "w") as f:
                json.dump(records, f, indent=1)
        del call, reference, cands, outs
        torch.cuda.empty_cache()
