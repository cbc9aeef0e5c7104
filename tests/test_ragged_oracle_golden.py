"""oracle.update_block on an IRREGULAR graph with per-agent H against the reference's own train_RPBCAC (run verbatim under the Keras
shim by tests/golden/make_ragged_golden.py): one update block of a 6-agent instance with in-neighbourhoods of 3, 3, 4, 5, 5, 6 agents
and H = 1, 1, 1, 2, 2, 2.  Same bar as test_oracle_golden.py: the bits (the shim's Keras arithmetic is the oracle's own).  This pins
the oracle that the ragged kernel and engine tests compare against to the reference rather than to itself.  CPU-only."""
import json
import os

import numpy as np

from helpers import flatten, net_dims, unflatten
from oracle import rpbcac_oracle as O

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ragged_reference.npz")


def test_update_block_on_an_irregular_graph_matches_the_reference_fixture():
    g = np.load(GOLDEN, allow_pickle=False)
    args = json.loads(str(g["args"]))
    n, H = args["n_agents"], args["H"]
    assert sorted(set(len(r) for r in args["in_nodes"])) == [3, 4, 5, 6] and sorted(set(H)) == [1, 2]
    agents = []
    for i in range(n):
        w = [unflatten(g["init/%d/%s" % (i, k)], *net_dims(n, k)) for k in ("actor", "critic", "tr")]
        agents.append(O.make_agent("Cooperative", w[0], w[1], w[2], args["slow_lr"], args["fast_lr"], args["gamma"], H[i]))
    s, ns, r, a = (np.asarray(g["replay/" + k], np.float32) for k in ("s", "ns", "r", "a"))
    assert s.shape == (args["n_ep_fixed"] * args["max_ep_len"], n, 2) and r.shape == a.shape == (s.shape[0], n, 1)
    O.update_block(agents, args["agent_label"], args["in_nodes"], s, ns, r, a, args["n_epochs"], args["common_reward"],
                   args["max_ep_len"], args["n_ep_fixed"], O.ShuffleStream(args["random_seed"]))
    for i, ag in enumerate(agents):
        for k, net in enumerate(("actor", "critic", "tr")):
            np.testing.assert_array_equal(flatten(ag.parameters()[k]), g["final/%d/%s" % (i, net)], err_msg="agent %d %s" % (i, net))
