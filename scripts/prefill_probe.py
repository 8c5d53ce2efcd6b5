#!/usr/bin/env python3
"""prefill_batch three ways on one build, alternated inside one process: the eager masked attention, the causal attention
through paged_attention_v1 ("positions": paged_prefill) and the tiled MFMA kernel (prefill_attention="tiled"; over an fp8 pool,
--kv-cache-dtype fp8, the third path is prefill_attention="auto", which resolves to the fp8 tiled kernel).
GPT-2 small, prompts U{4..512}; warm-up, then a host clock around a synchronise per call, medians; the paths' logits side by side.

  prefill_probe.py [--reps R] [--out FILE.json]      the three-way timing for n in {1, 8, 32, 64}
  prefill_probe.py --trace PATH [--n 64]             warm-up + 3 calls of ONE path (positions | tiled | auto, printed as what it
                                                     resolved to): run it under
                                                     `rocprofv3 --kernel-trace --stats -- python scripts/prefill_probe.py --trace tiled`
                                                     and read the attention kernel's time; prints the launch's operations
                                                     (4 D sum(p + 1) per head) and unique K / V bytes per layer beside it.
  prefill_probe.py --cache-write ab                  the tiled path with the cache write by slots (reshape_and_cache) against by
                                                     chunks (reshape_and_cache_chunks), alternated the same way; with --trace,
                                                     --cache-write slots | chunks picks the traced call's cache write."""
import argparse, json, os, sys, time
import numpy as np, torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from vllmini_amd.gpt2_decode import GPT2Dims, GPT2PagedDecoder, random_state_dict
from vllmini_amd.kv_pool import PagedKVPool

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=7)
ap.add_argument("--out", default="")
ap.add_argument("--trace", choices=["positions", "tiled", "auto"], default="")
ap.add_argument("--n", type=int, default=64)
ap.add_argument("--kv-cache-dtype", choices=["auto", "fp8"], default="auto")
ap.add_argument("--cache-write", choices=["slots", "chunks", "ab"], default="slots")
args = ap.parse_args()

dev = torch.device("cuda:0")
dims = GPT2Dims()
sd = random_state_dict(dims, dev)
FP8 = args.kv_cache_dtype == "fp8"
TILED = "auto" if FP8 else "tiled"              # the third path's name: "tiled" refuses fp8 pools, "auto" resolves to their kernel
PATHS = {"eager": dict(paged_prefill=False), "positions": dict(), TILED: dict(prefill_attention=TILED)}
if args.trace:
    PATHS.setdefault(args.trace, dict(prefill_attention=args.trace))
    PATHS[args.trace] = dict(PATHS[args.trace], prefill_cache_write=args.cache_write)
AB = args.cache_write == "ab"
if AB:
    PATHS = {how: dict(prefill_attention=TILED, prefill_cache_write=how) for how in ("slots", "chunks")}


def make(n, kw):
    pool = PagedKVPool(12 * 40 * n + 64, 12, 64, 16, 65, 12, device=dev, max_seqs=n, kv_cache_dtype=args.kv_cache_dtype)
    return GPT2PagedDecoder(dims, sd, pool, **kw)


def call(dec, n, prompts):
    for s in range(n):
        dec.pool.free(s)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    lg = dec.prefill_batch(list(range(n)), prompts)
    torch.cuda.synchronize()
    return time.perf_counter() - t0, lg


def shape_counts(prompts):
    """Per layer, all heads: multiply-adds x 2 of QK^T and PV over the causal ranges, and the K / V bytes a launch must read once."""
    H, D = dims.n_head, dims.head_size
    pairs = sum(T * (T + 1) // 2 for T in map(len, prompts))          # sum over positions of (p + 1)
    return 4 * D * pairs * H, 2 * sum(map(len, prompts)) * H * D * (1 if FP8 else 2)


rng = np.random.default_rng(0)
records = []
for n in ((args.n,) if args.trace else (1, 8, 32, 64)):
    prompts = [rng.integers(0, dims.vocab_size, int(rng.integers(4, 513))).tolist() for _ in range(n)]
    tok = sum(len(p) for p in prompts)
    flops, kv_bytes = shape_counts(prompts)
    if args.trace:
        dec = make(n, PATHS[args.trace])
        for _ in range(4):
            call(dec, n, prompts)
        print(f"trace {args.trace} -> {dec.prefill_attention}, cache write {dec.prefill_cache_write} (kv_cache_dtype={args.kv_cache_dtype}): n={n} tokens={tok} layers={dims.n_layer}; per attention launch {flops/1e9:.3f} GFLOP, "
              f"unique K/V {kv_bytes/1e6:.2f} MB", flush=True)
        continue
    decs = {name: make(n, kw) for name, kw in PATHS.items()}
    ts, logits = {name: [] for name in decs}, {}
    for rep in range(args.reps + 1):                                    # rep 0 is the warm-up
        for name, dec in decs.items():                                  # alternated: a drift of the machine hits all three
            t, lg = call(dec, n, prompts)
            if rep:
                ts[name].append(t)
            logits[name] = lg.float().cpu()
    med = {name: float(np.median(v)) for name, v in ts.items()}
    spread = {name: (float(np.min(v)), float(np.max(v))) for name, v in ts.items()}
    if AB:
        same = bool(torch.equal(logits["slots"], logits["chunks"]))
        records.append({"n": n, "tokens": tok, "kv_cache_dtype": args.kv_cache_dtype, "median_ms": {k: v * 1e3 for k, v in med.items()},
                        "min_max_ms": {k: [a * 1e3, b * 1e3] for k, (a, b) in spread.items()}, "logits_equal": same})
        print(f"n={n:3d} tokens={tok:6d}  " + "  ".join(f"{k} {med[k]*1e3:8.3f} ms ({spread[k][0]*1e3:.3f} - {spread[k][1]*1e3:.3f})" for k in med) +
              f"  chunks / slots {med['chunks'] / med['slots']:.3f}  logits equal {same}", flush=True)
        del decs
        torch.cuda.empty_cache()
        continue
    d = {name: (logits[name] - logits["eager"]).abs().max().item() for name in ("positions", TILED)}
    same = (logits[TILED].argmax(-1) == logits["positions"].argmax(-1)).float().mean().item()
    records.append({"n": n, "tokens": tok, "kv_cache_dtype": args.kv_cache_dtype, "median_ms": {k: v * 1e3 for k, v in med.items()},
                    "min_max_ms": {k: [a * 1e3, b * 1e3] for k, (a, b) in spread.items()},
                    "max_dlogit_vs_eager": d, f"argmax_agree_{TILED}_positions": same,
                    "attention_gflop_per_layer": flops / 1e9, "unique_kv_mb_per_layer": kv_bytes / 1e6})
    print(f"n={n:3d} tokens={tok:6d}  " + "  ".join(f"{k} {med[k]*1e3:8.2f} ms ({tok/med[k]/1e3:7.1f} k tok/s)" for k in med) +
          f"  max|dlogit| vs eager: positions {d['positions']:.3e} {TILED} {d[TILED]:.3e}  argmax {TILED}==positions {same:.3f}", flush=True)
    del decs
    torch.cuda.empty_cache()
if args.out and records:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(records, f, indent=1)
