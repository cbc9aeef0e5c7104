"""C2 end to end (BASELINE configs[4] as ONE instance over several GPUs): RPBCACEngine.shard_agents
shards the wide critic of a single-seed instance by AGENTS (TD targets, local fits, estimate consensus, values) and by
parameter COLUMNS (hidden-layer consensus), with the exchanges of parallel.ShardedConsensus in between.  world_size 2
under gloo, kernels from the hipemu build: after two update blocks (and a trailing episode) every parameter of every network, the Adam slots,
the replay rows and the three logged curves equal the UNSHARDED engine's bit for bit, on both ranks.  CPU-only.

The last case leaves the packed-operand path on the way (RPBCACEngine._poll_pk_range): ONE agent of the LAST rank starts with a critic
operand beyond the f16 range of the packed form, so only that rank's kernels raise the flag.  The ranks must still decide together:
each records after every block whether it is off the packed path and whether it warned (equal to the unsharded engine's record, which
sees the flag too), and the sequence of its row all-gathers -- which buffer, which columns -- equal across the ranks: a rank that kept
the packed path alone would gather V(s) where its peer gathers V(s') in the actor phase (same shapes: nothing hangs, the TD errors
are wrong)."""
import os
import socket
import sys

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

_HERE = os.path.dirname(os.path.abspath(__file__))

# (agents, d, H, graph, critic width, lattice path, rng mode, update blocks, agent with an out-of-range critic operand or None)
CASES = [(4, 4, 1, "circ", 64, True, "device", 2, None),        # packed bf16x3 layer 1: 2 agents x 64 units = one 128-row tile per rank
         (6, 3, 1, "rand", 24, False, "numpy", 2, None),        # dense f32 path, general K1 kernel
         (4, 4, 1, "circ", 128, True, "device", 2, None),       # dense layers on pre-split packed operands (csrc/dense_pk.hip)
         (4, 4, 1, "circ", 128, True, "device", 3, 3)]          # ... left in block 0: agent 3 (rank 1) carries W2[k][j] = 70 > 63.48
RANK_ONLY = "rank_"                                             # keys of a rank's record the unsharded engine has no counterpart of


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _run(case, lib, shard):
    import engine_checks as EC
    import warnings
    n, d, H, graph, hid, lattice, rng_mode, n_blocks, planted = case
    rng = np.random.default_rng(n * 7 + d)
    if graph == "circ":
        nodes = [[(i + k) % n for k in range(d)] for i in range(n)]
    else:
        nodes = [[i] + [int(x) for x in rng.permutation([j for j in range(n) if j != i])[:d - 1]] for i in range(n)]
    n_epochs = 2 if hid % 128 == 0 else 1       # (two epochs: the second takes its TD target from the cached layer-2 activations)
    args = EC.make_args(["Cooperative"] * n, H=H, n_episodes=2 * n_blocks + 1, max_ep_len=3, n_ep_fixed=2, n_epochs=n_epochs, buffer_size=9, seed=17,
                        in_nodes=nodes)
    W, goals = EC.make_inputs(args, 5, (17,), critic_hid=hid)
    if planted is not None:
        assert planted >= n // 2                                  # among the LAST rank's agents only
        EC.plant_out_of_range_w2(W[0][planted]["critic"])
    calls = {"exchange": {}, "rows": []}
    record = {"pk_none": [], "warned": [], "gathers": []}
    caught = []

    def watch(eng):
        """after every block: is this engine off the packed path, has it warned so far; every row all-gather by buffer and columns"""
        run_block, gather = eng.run_block, eng._allgather_rows

        def run_block_recorded():
            out = run_block()
            record["pk_none"].append(eng.pk is None)
            record["warned"].append(len([w for w in caught if "packed-operand" in str(w.message)]))
            return out

        def gather_recorded(full, c0, c1):
            named = [("ybuf." + k, v) for k, v in eng.ybuf.items()] + [("w_v", getattr(eng, "w_v", None))]
            named += [("%s.%s" % (dname, k), v) for dname in ("theta", "msg", "loss") for k, v in getattr(eng, dname).items()]
            names = [k for k, v in named if v is not None and v.data_ptr() == full.data_ptr()]
            assert len(names) == 1, names
            record["gathers"].append("%s[%d:%d]" % (names[0], c0, c1))
            return gather(full, c0, c1)
        eng.run_block, eng._allgather_rows = run_block_recorded, gather_recorded

    def tweak(eng):
        watch(eng)
        eng.shard_agents()
        assert eng.shard.shard_tr == (not lattice)           # 2 agents x 20 units do not fill a 128-row tile of the packed operands
        fit = eng._local_fit_wide

        def count(net, exchange):
            def counted_exchange(msg_local):
                calls["exchange"][net] = calls["exchange"].get(net, 0) + 1
                assert msg_local.shape[1] == n // 2
                return exchange(msg_local)
            return counted_exchange
        for net, sc in eng.shard.sc.items():
            sc.exchange = count(net, sc.exchange)

        def counted_fit(net, xkey, y, B, mask):
            calls["rows"].append((eng.N, y.shape[1], eng.msg[net].shape[1]))      # inside the window: this rank's agents only
            return fit(net, xkey, y, B, mask)
        eng._local_fit_wide = counted_fit
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        eng, logs = EC.run_engine(args, 5, 5, rng_mode, "cpu", lib, (17,), W, goals, lattice=lattice, critic_hid=hid,
                                  tweak=tweak if shard else watch)
    assert eng.wide and eng.lat_active == lattice and (eng.shard is not None) == shard and not eng._windowed
    if shard:           # n_blocks update blocks x n_epochs: one transpose each way per epoch, fits on half of the agents
        ne = n_blocks * n_epochs
        assert calls["exchange"] == ({"critic": ne} if lattice else {"critic": ne, "tr": ne}), calls
        assert calls["rows"] == [(n // 2, n // 2, n // 2)] * ne, calls
    out = {"theta_" + k: v.numpy().copy() for k, v in eng.theta.items()}
    out.update({"adam_m": eng.adam_m.numpy().copy(), "adam_v": eng.adam_v.numpy().copy(),
                "loss_critic": eng.loss["critic"].numpy().copy(), "loss_tr": eng.loss["tr"].numpy().copy()})
    out.update({"rp_" + k: v[:, :eng.B].numpy().copy() for k, v in eng.rp.items()})
    out.update({"log_" + k: np.asarray(v) for k, v in logs.items()})
    out.update({"pk_none_after_block": np.asarray(record["pk_none"]), "range_warnings_after_block": np.asarray(record["warned"])})
    if shard:
        out[RANK_ONLY + "gathers"] = np.asarray(record["gathers"])
    return out


def _worker(rank, world, port, out_dir):
    sys.path.insert(0, os.path.dirname(_HERE))
    sys.path.insert(0, _HERE)
    os.environ["MASTER_ADDR"], os.environ["MASTER_PORT"] = "127.0.0.1", str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from emu_util import emu_lib
    lib = emu_lib()
    for ci, case in enumerate(CASES):
        got = _run(case, lib, shard=True)
        np.savez(os.path.join(out_dir, "c%d_r%d.npz" % (ci, rank)), **got)
        if rank == 0:
            np.savez(os.path.join(out_dir, "c%d_ref.npz" % ci), **_run(case, lib, shard=False))
    dist.destroy_process_group()


def test_agent_sharded_wide_critic_equals_unsharded_world2(tmp_path):
    world = 2
    mp.spawn(_worker, args=(world, _free_port(), str(tmp_path)), nprocs=world, join=True)
    for ci in range(len(CASES)):
        ref = np.load(os.path.join(str(tmp_path), "c%d_ref.npz" % ci))
        ranks = [np.load(os.path.join(str(tmp_path), "c%d_r%d.npz" % (ci, rank))) for rank in range(world)]
        n, hid, lattice, n_blocks, planted = CASES[ci][0], CASES[ci][4], CASES[ci][5], CASES[ci][7], CASES[ci][8]
        # the ranks decide together: the same collectives in the same order on the same buffers, the same path after every block
        for rank in range(1, world):
            assert list(ranks[rank][RANK_ONLY + "gathers"]) == list(ranks[0][RANK_ONLY + "gathers"]), \
                "case %d: rank %d and rank 0 all-gather different buffers:\n%s" % (ci, rank, "\n".join(
                    "  %3d  %-24s %s" % (q, a, b) for q, (a, b) in enumerate(zip(ranks[0][RANK_ONLY + "gathers"], ranks[rank][RANK_ONLY + "gathers"]))
                    if a != b))
            np.testing.assert_array_equal(ranks[rank]["pk_none_after_block"], ranks[0]["pk_none_after_block"])
            np.testing.assert_array_equal(ranks[rank]["range_warnings_after_block"], ranks[0]["range_warnings_after_block"])
        # ... and the case is what it says: on the packed path (or not) to begin with, off it from block 0 on with ONE warning
        packed = lattice and hid % 128 == 0
        assert list(ref["pk_none_after_block"]) == [not packed or planted is not None] * n_blocks
        assert list(ref["range_warnings_after_block"]) == [0 if planted is None else 1] * n_blocks
        for rank in range(world):
            got = ranks[rank]
            assert sorted(k for k in got.files if not k.startswith(RANK_ONLY)) == sorted(ref.files)
            for k in ref.files:
                np.testing.assert_array_equal(got[k], ref[k], err_msg="case %d rank %d %s" % (ci, rank, k))


def test_shard_agents_refuses_what_it_cannot_shard():
    sys.path.insert(0, _HERE)
    import engine_checks as EC
    from emu_util import emu_lib
    from rcmarl_amd.engine import EngineConfig, RPBCACEngine
    args = EC.make_args(["Cooperative"] * 5, H=1, n_episodes=2, max_ep_len=3, n_ep_fixed=2, n_epochs=1, buffer_size=9, seed=1)

    def engine(S, hid):
        cfg = EngineConfig(5, args["agent_label"], args["in_nodes"], H=1, max_ep_len=3, n_ep_fixed=2, n_epochs=1, buffer_size=9,
                           n_seeds=S, rng_mode="device", lattice=False, critic_hid=hid)
        return RPBCACEngine(cfg, seeds=list(range(S)), device="cpu", lib=emu_lib())
    assert engine(1, 24).shard_agents(rank=0, world=1).shard is None           # one rank: nothing to shard
    with pytest.raises(ValueError, match="ONE instance"):
        engine(2, 24).shard_agents(rank=0, world=2)                            # several seeds shard by seed instead
    with pytest.raises(ValueError, match="ONE instance"):
        engine(1, 20).shard_agents(rank=0, world=2)                            # the reference's 20-unit critic: nothing to gain
    with pytest.raises(ValueError, match="multiple of the number of ranks"):
        engine(1, 24).shard_agents(rank=0, world=2)                            # 5 agents over 2 ranks
