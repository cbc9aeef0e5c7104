#!/usr/bin/env python
"""One block of the reference's headline scenario with a wide actor: 4 cooperative agents + 1 Malicious one on a 5 x 5 grid (H = 1), a
full replay buffer of 2000 rows, 10 consensus epochs, S seeds batched, the actor phase on 1000 rows -- so the Malicious agents'
actor.fit(batch_size=200, epochs=1) is five shuffled mini-batches per (seed, adversary) chain.  Times the block with
EngineConfig(adv_actor="loop") (the nine-launch composition, chain after chain) against adv_actor="auto" (one launch from the measured
chain count on): one warm-up block, then `--blocks` timed ones, each timed on its own; reports the median per block, the actor phase's
share and the run-to-run spread (max - min over the timed blocks).  Two cases: a 64-unit actor beside 20-unit critics at 16 seeds, and
a 512-unit actor beside a 512-unit critic at 4 seeds.  Uses only the public EngineConfig surface.  On the GPU:

    python tools/wide_actor_adv_block.py [--blocks 3] [--case small|large|both]
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
CASES = {"small": (16, 64, 20), "large": (4, 512, 512)}       # seeds, actor width, critic width


def make_engine(S, actor_hid, critic_hid, adv_actor, lib):
    cfg = EngineConfig(5, LABELS, IN_NODES, H=1, gamma=0.9, slow_lr=0.002, fast_lr=0.01, max_ep_len=20, n_ep_fixed=50, n_epochs=10,
                       buffer_size=2000, nrow=5, ncol=5, n_seeds=S, rng_mode="device", lattice=False, actor_hid=actor_hid,
                       critic_hid=critic_hid, adv_actor=adv_actor)
    eng = RPBCACEngine(cfg, seeds=list(range(1, S + 1)), device="cuda", lib=lib)
    eng.init_glorot(base_seed=1)
    eng.set_goals(np.stack([np.random.RandomState(s).randint(0, 5, size=(5, 2)) for s in range(1, S + 1)]))
    while eng.B + eng.n_last <= cfg.buffer_size:          # the steady state of the reference loop, as bench.py sets it up
        eng.rollout_block(cfg.n_ep_fixed)
    return eng


def run(S, actor_hid, critic_hid, adv_actor, lib, blocks):
    eng = make_engine(S, actor_hid, critic_hid, adv_actor, lib)
    eng.profile_phases = True
    eng.run_block()                                       # warm-up
    eng.sync()
    route = eng.adv.actor_route() or "the loop"
    totals, phase3 = [], []
    for _ in range(blocks):
        for k in eng.timers:
            eng.timers[k] = 0.0
        eng.sync()
        t0 = time.perf_counter()
        eng.run_block()
        eng.sync()
        totals.append((time.perf_counter() - t0) * 1e3)
        phase3.append(eng.timers["phase3"] * 1e3)
    finite = all(bool(torch.isfinite(eng.theta[k]).all().item()) for k in ("critic", "tr", "actor", "critic_local"))
    print("4 cooperative + 1 Malicious, actor %d, critic %d, B %d, S %d (%d chains), adv_actor=%-6s -> %s: %9.1f ms per block (median of %d; "
          "spread %.1f ms), actor phase %8.1f ms (spread %.1f ms); adversaries' Adam steps %d; weights finite: %s"
          % (actor_hid, critic_hid, eng.B, S, S * len(eng.adv.adv), adv_actor, route, float(np.median(totals)), blocks,
             max(totals) - min(totals), float(np.median(phase3)), max(phase3) - min(phase3), eng.adv.adam_t, finite), flush=True)
    return float(np.median(totals)), max(totals) - min(totals)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=3)
    ap.add_argument("--case", choices=("small", "large", "both"), default="both")
    args = ap.parse_args()
    lib = capi.load()
    for name in (("small", "large") if args.case == "both" else (args.case,)):
        S, actor_hid, critic_hid = CASES[name]
        t_loop, s_loop = run(S, actor_hid, critic_hid, "loop", lib, args.blocks)
        t_auto, s_auto = run(S, actor_hid, critic_hid, "auto", lib, args.blocks)
        print("%s: auto - loop = %+.1f ms per block (run-to-run spread: loop %.1f ms, auto %.1f ms)" % (name, t_auto - t_loop, s_loop, s_auto),
              flush=True)
