#!/usr/bin/env python
"""One BASELINE configs[4]-shaped block (bench.py's cfg5_1gpu: 1024 agents, 512-unit critic, B = 3000, 10 epochs) with a wide
team-reward net, beside the same block with the 20-unit one: ms per block, split into rollout / local fits / consensus / actor
phase, and the peak device memory of each engine.  On the GPU:

    python tools/wide_tr_block.py [--tr_hid 512] [--blocks 1] [--agents 1024]
"""
import argparse
import gc
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402
from rcmarl_amd import capi  # noqa: E402
from rcmarl_amd.engine import EngineConfig, RPBCACEngine  # noqa: E402
import numpy as np  # noqa: E402


def make_engine(w, N, tr_hid, lib):
    cfg = EngineConfig(N, ["Cooperative"] * N, bench.build_graph(w["graph"], N, w["d"]), H=w["H"], gamma=0.9, slow_lr=0.002,
                       fast_lr=w["fast_lr"], max_ep_len=20, n_ep_fixed=50, n_epochs=10, buffer_size=2000, nrow=w["nrow"], ncol=w["ncol"],
                       n_seeds=1, rng_mode="device", critic_hid=w["critic_hid"], tr_hid=tr_hid)
    eng = RPBCACEngine(cfg, seeds=[1], device="cuda", lib=lib)
    eng.init_glorot(base_seed=1)
    eng.set_goals(np.stack([np.random.RandomState(1).randint(0, 5, size=(N, 2))]))
    while eng.B + eng.n_last <= cfg.buffer_size:          # the steady state of the reference loop, as bench.py sets it up
        eng.rollout_block(cfg.n_ep_fixed)
    return eng


def run(w, N, tr_hid, lib, blocks):
    torch.cuda.reset_peak_memory_stats()
    eng = make_engine(w, N, tr_hid, lib)
    eng.profile_phases = True
    eng.run_block()                                       # warm-up
    for k in eng.timers:
        eng.timers[k] = 0.0
    eng.sync()
    t0 = time.perf_counter()
    for _ in range(blocks):
        eng.run_block()
    eng.sync()
    total = (time.perf_counter() - t0) / blocks * 1e3
    t = {k: v / blocks * 1e3 for k, v in eng.timers.items() if k != "blocks"}
    finite = all(bool(torch.isfinite(eng.theta[k]).all().item()) for k in ("critic", "tr", "actor"))
    print("%d agents, critic %d, tr_hid %4d: %8.1f ms per block = rollout %7.1f + local fits %7.1f + consensus %7.1f + actor phase %7.1f;  "
          "peak device memory %.1f GiB (packed path: critic %s, team-reward net %s; weights finite: %s)"
          % (N, w["critic_hid"], tr_hid, total, t["rollout"], t["phase1"], t["phase2"], t["phase3"],
             torch.cuda.max_memory_allocated() / 2.0 ** 30, eng._pk_ok("critic", "s", eng.lat_B), eng._pk_ok("tr", "sa", eng.lat_B), finite),
          flush=True)
    del eng
    gc.collect()
    torch.cuda.empty_cache()


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--tr_hid", type=int, default=512)
    ap.add_argument("--blocks", type=int, default=1)
    ap.add_argument("--agents", type=int, default=0, help="agent count (default: the workload's 1024)")
    args = ap.parse_args()
    w = bench.WORKLOADS["cfg5_1gpu"]
    lib = capi.load()
    for hid in (20, args.tr_hid):
        run(w, args.agents or w["N"], hid, lib, args.blocks)
