#!/usr/bin/env python
"""One BASELINE configs[4]-shaped block (bench.py's cfg5_1gpu: 1024 agents, 512-unit critic, B = 3000, 10 epochs) with a wide actor,
beside the same block with the 20-unit actor: ms per block, split into rollout / epochs / actor phase, and the wide actor's Adam
step on its own (HIP events around its launches).  On the GPU:

    python tools/wide_actor_block.py [--actor_hid 512] [--blocks 2]
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


def make_engine(w, actor_hid, lib):
    N = w["N"]
    cfg = EngineConfig(N, ["Cooperative"] * N, bench.build_graph(w["graph"], N, w["d"]), H=w["H"], gamma=0.9, slow_lr=0.002,
                       fast_lr=w["fast_lr"], max_ep_len=20, n_ep_fixed=50, n_epochs=10, buffer_size=2000, nrow=w["nrow"], ncol=w["ncol"],
                       n_seeds=1, rng_mode="device", critic_hid=w["critic_hid"], actor_hid=actor_hid)
    eng = RPBCACEngine(cfg, seeds=[1], device="cuda", lib=lib)
    eng.init_glorot(base_seed=1)
    eng.set_goals(np.stack([np.random.RandomState(1).randint(0, 5, size=(N, 2))]))
    while eng.B + eng.n_last <= cfg.buffer_size:          # the steady state of the reference loop, as bench.py sets it up
        eng.rollout_block(cfg.n_ep_fixed)
    return eng


def run(w, actor_hid, lib, blocks):
    eng = make_engine(w, actor_hid, lib)
    step_ms = []
    if eng.actor_wide:
        inner = eng._actor_step_wide

        def timed(*a):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            inner(*a)
            e1.record()
            step_ms.append((e0, e1))
        eng._actor_step_wide = timed
    eng.profile_phases = True
    eng.run_block()                                       # warm-up
    for k in eng.timers:
        eng.timers[k] = 0.0
    step_ms.clear()
    eng.sync()
    t0 = time.perf_counter()
    for _ in range(blocks):
        eng.run_block()
    eng.sync()
    total = (time.perf_counter() - t0) / blocks * 1e3
    t = {k: v / blocks * 1e3 for k, v in eng.timers.items() if k != "blocks"}
    adam = sum(a.elapsed_time(b) for a, b in step_ms) / max(len(step_ms), 1)
    finite = bool(torch.isfinite(eng.theta["actor"]).all().item())
    print("actor_hid %4d: %8.1f ms per block = rollout %7.1f + local fits %7.1f + consensus %7.1f + actor phase %7.1f%s  (actor weights finite: %s)"
          % (actor_hid, total, t["rollout"], t["phase1"], t["phase2"], t["phase3"],
             " (of it the Adam step's nine launches: %.1f)" % adam if step_ms else "", finite))
    del eng
    gc.collect()
    torch.cuda.empty_cache()


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--actor_hid", type=int, default=512)
    ap.add_argument("--blocks", type=int, default=2)
    args = ap.parse_args()
    w = bench.WORKLOADS["cfg5_1gpu"]
    lib = capi.load()
    for hid in (20, args.actor_hid):
        run(w, hid, lib, args.blocks)
