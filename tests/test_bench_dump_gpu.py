"""`bench.py --dump-outputs` on the GPU: a plain run times ONE region of exactly --steps steps, and what it writes is what the
last timed step left for its caller — checked against the CPU oracle on a small, odd-sized workload — and is the same, bit for
bit, in a second run with the same arguments."""
from __future__ import annotations

import dataclasses
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import oracle

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ARGS = ["--gpus", "1", "--steps", "4", "--warmup", "1", "--batch", "7", "--seq-len", "100"]
NAMES = ["key_cache_blocks", "key_cache_rows", "out", "value_cache_blocks", "value_cache_rows"]


@pytest.mark.gpu
def test_plain_run_dumps_the_last_timed_steps_outputs(tmp_path, capsys):
    import bench
    from vllmini_amd.workload import CONFIGS, make_workload

    r = subprocess.run([sys.executable, os.path.join(REPO, "bench.py"), *ARGS, "--dump-outputs", str(tmp_path / "a")],
                       capture_output=True, text=True, timeout=300, cwd=REPO)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1, r.stdout[:500]
    line = json.loads(lines[0])
    assert line["metric"] == "decode_tokens_per_sec_paged_attention_v1_per_layer" and line["unit"] == "tokens/s"
    assert line["higher_is_better"] is True and line["dtype"] == "f16" and line["full"] is False
    assert line["steps"] == 4 and line["warmup"] == 1 and line["timed_regions"] == 1 and len(line["ms_per_step_regions"]) == 1
    assert line["ms_per_step"] > 0 and line["value"] == pytest.approx(7 * 4 / (line["ms_per_step"] * 4 / 1e3), rel=1e-9)
    assert line["roofline"] is None and line["cpu_baseline"] is None           # both take passes of their own: --full
    assert not [k for k in line if k != "ms_per_step" and (k.endswith("_step") or k.startswith("paged_attention_v1_us"))], sorted(line)
    a = {n: np.load(tmp_path / "a" / f"{n}.npy") for n in NAMES}
    assert sorted(os.listdir(tmp_path / "a")) == [n + ".npy" for n in NAMES]
    assert all(x.dtype == np.float32 for x in a.values()) and sum(x.nbytes for x in a.values()) <= 64 << 20

    # the same arguments again (in this process): the same inputs, so the same files
    capsys.readouterr()
    bench.main([*ARGS, "--dump-outputs", str(tmp_path / "b")])
    assert json.loads(capsys.readouterr().out)["steps"] == 4
    for n in NAMES:
        assert np.array_equal(a[n], np.load(tmp_path / "b" / f"{n}.npy")), n

    # the workload bench.py builds for these arguments, and what the last of its 4 steps (table set 1) leaves: this step's
    # k / v rows at its slots, attention over table set 1 of the updated caches
    c = dataclasses.replace(CONFIGS["cfg3"], name="cfg3_b7_l100", batch=7, seq_len=100, num_blocks=2 * 7 * 7)
    wl = make_workload(c, torch.device("cuda", 0), seed=1234, table_sets=2)
    q, k, v = (np.ascontiguousarray(x.cpu().numpy()) for x in (wl.query, wl.key, wl.value))
    kc, vc = wl.key_cache.cpu().numpy(), wl.value_cache.cpu().numpy()
    for t in (0, 1):
        oracle.reshape_and_cache(k, v, kc, vc, wl.slots[t].cpu().numpy())
    assert np.array_equal(a["key_cache_rows"], k.astype(np.float32)) and np.array_equal(a["value_cache_rows"], v.astype(np.float32))
    blk = (wl.slots[1] // c.block_size).cpu().numpy()
    pick = np.sort(np.random.default_rng(0).permutation(c.batch)[:bench.DUMP_BLOCKS])
    assert np.array_equal(a["key_cache_blocks"], kc[blk[pick]].astype(np.float32))
    assert np.array_equal(a["value_cache_blocks"], vc[blk[pick]].astype(np.float32))
    ref = oracle.paged_attention_v1(q, kc, vc, c.kv_heads, wl.scale, wl.tables[1].cpu().numpy(), wl.seq_lens.cpu().numpy(),
                                    c.block_size)
    err = np.abs(a["out"].astype(np.float64) - ref.astype(np.float64)).max()
    print(f"out vs oracle: max|d| = {err:.3e}")
    assert np.isfinite(a["out"]).all() and err <= 1e-3, err                  # smoke()'s bound for the same comparison
