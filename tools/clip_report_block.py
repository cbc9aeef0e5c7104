#!/usr/bin/env python
"""One block of bench.py's cfg4_shard configuration (BASELINE configs[3] per-GPU shard: 256 agents, d = 18, H = 8, 16 seeds,
B = 3000, 10 epochs) with the clip report off and on: ms per block of each, their ratio, and what the report says after the timed
blocks.  bench.py itself never turns the switch on.  On the GPU:

    python tools/clip_report_block.py [--blocks 3] [--workload cfg4_shard]
"""
import argparse
import gc
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402
from rcmarl_amd import capi  # noqa: E402
from rcmarl_amd.engine import EngineConfig, RPBCACEngine  # noqa: E402


def make_engine(w, lib, clip_report):
    N, S = w["N"], w["S"]
    cfg = EngineConfig(N, w.get("labels", ["Cooperative"] * N), bench.build_graph(w["graph"], N, w["d"]), H=w["H"], gamma=0.9,
                       slow_lr=0.002, fast_lr=w.get("fast_lr", 0.01), max_ep_len=20, n_ep_fixed=50, n_epochs=10, buffer_size=2000,
                       nrow=w["nrow"], ncol=w["ncol"], n_seeds=S, rng_mode="device", critic_hid=w.get("critic_hid", 20),
                       clip_report=clip_report)
    seeds = list(range(1, S + 1))
    eng = RPBCACEngine(cfg, seeds=seeds, device="cuda", lib=lib)
    eng.init_glorot(base_seed=1)
    eng.set_goals(np.stack([np.random.RandomState(int(s)).randint(0, 5, size=(N, 2)) for s in seeds]))
    while eng.B + eng.n_last <= cfg.buffer_size:          # the steady state of the reference loop, as bench.py sets it up
        eng.rollout_block(cfg.n_ep_fixed)
    return eng


def run(w, lib, clip_report, blocks):
    eng = make_engine(w, lib, clip_report)
    eng.run_block()                                       # warm-up
    eng.sync()
    times = []
    for _ in range(blocks):
        t0 = time.perf_counter()
        eng.run_block()
        eng.sync()
        times.append((time.perf_counter() - t0) * 1e3)
    out = {"clip_report": clip_report, "ms_per_block": sorted(times)[len(times) // 2], "min_ms": min(times), "max_ms": max(times)}
    if clip_report:
        rep = eng.clip_report()
        for net, r in rep.items():
            tot = float(r["steps"]) * r["P_hid"] * eng.S * eng.N * eng.cfg.H
            out[net] = {"steps": r["steps"], "below_share_of_H_P_hid": float(r["below"].sum()) / tot,
                        "above_share_of_H_P_hid": float(r["above"].sum()) / tot,
                        "sender_rate_max": float(np.nanmax(r["sender_rate"])), "sender_rate_mean": float(np.nanmean(r["sender_rate"]))}
    del eng
    gc.collect()
    torch.cuda.empty_cache()
    return out


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=3)
    ap.add_argument("--workload", default="cfg4_shard", choices=sorted(bench.WORKLOADS))
    args = ap.parse_args()
    w = bench.WORKLOADS[args.workload]
    lib = capi.load()
    off = run(w, lib, False, args.blocks)
    on = run(w, lib, True, args.blocks)
    print("%s: %.1f ms per block with the clip report off, %.1f ms on (x%.3f; medians of %d blocks)"
          % (args.workload, off["ms_per_block"], on["ms_per_block"], on["ms_per_block"] / off["ms_per_block"], args.blocks))
    print(json.dumps({"tool": "clip_report_block", "workload": args.workload, "blocks": args.blocks, "off": off, "on": on,
                      "ratio": on["ms_per_block"] / off["ms_per_block"]}))
