#!/usr/bin/env python
"""Generate tests/golden/ragged_reference.npz by EXECUTING THE REFERENCE'S OWN SOURCES (build container only; see make_golden.py):

    python tests/golden/make_ragged_golden.py

ONE update block of the reference's train_RPBCAC on a 6-agent IRREGULAR instance with per-agent H: in-neighbourhoods of 3, 3, 4,
5, 5 and 6 agents, H = 1, 1, 1, 2, 2, 2.  Recorded: the initial weights, the block's replay rows (the reference appends them to
the caller's exp_buffer lists) and the end-of-block weights.  tests/test_ragged_oracle_golden.py holds oracle.update_block to it,
which pins the oracle's behaviour on irregular graphs to the reference rather than to itself.  Data only.
"""
import contextlib
import io
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))          # tests/
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))  # repo root
import make_golden as MG  # noqa: E402  (loads the reference under the shims: MG.REF)

REF, keras = MG.REF, MG.keras
N = 6
DEGREES, H = (3, 3, 4, 5, 5, 6), (1, 1, 1, 2, 2, 2)


def main():
    from oracle.rpbcac_oracle import ShuffleStream
    seed = 400
    args = {"n_agents": N, "agent_label": ["Cooperative"] * N,
            "in_nodes": [[(i + k) % N for k in range(d)] for i, d in enumerate(DEGREES)],
            "n_actions": 5, "n_states": 2, "n_episodes": 4, "max_ep_len": 5, "n_ep_fixed": 4, "n_epochs": 2,
            "slow_lr": 0.002, "fast_lr": 0.01, "batch_size": 200, "buffer_size": 400, "gamma": 0.9, "H": list(H),
            "common_reward": False, "summary_dir": "./", "pretrained_agents": False, "random_seed": seed}
    np.random.seed(seed)
    s_desired = np.random.randint(0, 5, size=(N, 2))
    s_initial = np.random.randint(0, 5, size=(N, 2))
    nets = MG.build_models(N, seed=seed)
    init = [[MG.flat_net(m.get_weights()) for m in trio] for trio in nets]
    agents = [REF.resilient.RPBCAC_agent(*nets[i], slow_lr=args["slow_lr"], fast_lr=args["fast_lr"], gamma=args["gamma"], H=H[i])
              for i in range(N)]
    env = REF.grid_world.Grid_World(nrow=5, ncol=5, n_agents=N, desired_state=s_desired, initial_state=s_initial,
                                    randomize_state=True, scaling=True)
    keras.set_shuffle_stream(ShuffleStream(seed))
    buf = ([], [], [], [])
    with contextlib.redirect_stdout(io.StringIO()):
        weights, sim = REF.train_agents.train_RPBCAC(env, agents, args, exp_buffer=buf)
    out = {"args": np.asarray(json.dumps(args)), "desired": s_desired}
    for key, lst in zip(("s", "ns", "a", "r"), buf):
        out["replay/" + key] = np.asarray(lst, dtype=np.float32)
    assert out["replay/s"].shape == (args["n_ep_fixed"] * args["max_ep_len"], N, 2)
    for i in range(N):
        for k, net in enumerate(("actor", "critic", "tr")):
            out["init/%d/%s" % (i, net)] = init[i][k]
            out["final/%d/%s" % (i, net)] = MG.flat_net(weights[i][k])
    path = os.path.join(HERE, "ragged_reference.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes,", len(out), "arrays")


if __name__ == "__main__":
    main()
