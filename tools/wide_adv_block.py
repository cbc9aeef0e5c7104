#!/usr/bin/env python
"""One block of a resilience scenario beside wide nets: 4 cooperative agents + 1 Malicious one on a 5 x 5 grid (H = 1), 64-unit
critic and team-reward net, a full replay buffer of 2000 rows, 10 consensus epochs, S seeds batched -- the Malicious agent's three
mini-batch fits per epoch (private critic, compromised team-reward net, compromised critic: 630 SGD steps each) are what the block
is made of.  One warm-up block, one timed block: ms per block, split into rollout / phase I (local fits and the adversaries' message
generators) / consensus / actor phase.  Uses only the public EngineConfig surface, so the same file times any checkout.  On the GPU:

    python tools/wide_adv_block.py [--seeds 16] [--hid 64] [--blocks 1]
"""
import argparse
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from rcmarl_amd import capi  # noqa: E402
from rcmarl_amd.engine import EngineConfig, RPBCACEngine  # noqa: E402

LABELS = ["Cooperative"] * 4 + ["Malicious"]
IN_NODES = [[(i + k) % 5 for k in range(4)] for i in range(5)]


def make_engine(S, hid, lib):
    cfg = EngineConfig(5, LABELS, IN_NODES, H=1, gamma=0.9, slow_lr=0.002, fast_lr=0.01, max_ep_len=20, n_ep_fixed=50, n_epochs=10,
                       buffer_size=2000, nrow=5, ncol=5, n_seeds=S, rng_mode="device", lattice=False, critic_hid=hid, tr_hid=hid)
    eng = RPBCACEngine(cfg, seeds=list(range(1, S + 1)), device="cuda", lib=lib)
    eng.init_glorot(base_seed=1)
    eng.set_goals(np.stack([np.random.RandomState(s).randint(0, 5, size=(5, 2)) for s in range(1, S + 1)]))
    while eng.B + eng.n_last <= cfg.buffer_size:          # the steady state of the reference loop, as bench.py sets it up
        eng.rollout_block(cfg.n_ep_fixed)
    return eng


def run(S, hid, lib, blocks):
    eng = make_engine(S, hid, lib)
    eng.profile_phases = True
    t0 = time.perf_counter()
    eng.run_block()                                       # warm-up
    eng.sync()
    warm = time.perf_counter() - t0
    for k in eng.timers:
        eng.timers[k] = 0.0
    eng.sync()
    t0 = time.perf_counter()
    for _ in range(blocks):
        eng.run_block()
    eng.sync()
    total = (time.perf_counter() - t0) / blocks * 1e3
    t = {k: v / blocks * 1e3 for k, v in eng.timers.items() if k != "blocks"}
    finite = all(bool(torch.isfinite(eng.theta[k]).all().item()) for k in ("critic", "tr", "actor", "critic_local"))
    print("4 cooperative + 1 Malicious, critic %d, team-reward net %d, B %d, S %d: %10.1f ms per block = rollout %8.1f + phase I %10.1f + "
          "consensus %8.1f + actor phase %8.1f  (warm-up block %.1f ms; weights finite: %s)"
          % (hid, hid, eng.B, S, total, t["rollout"], t["phase1"], t["phase2"], t["phase3"], warm * 1e3, finite), flush=True)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--seeds", type=int, default=16)
    ap.add_argument("--hid", type=int, default=64)
    ap.add_argument("--blocks", type=int, default=1)
    args = ap.parse_args()
    run(args.seeds, args.hid, capi.load(), args.blocks)
