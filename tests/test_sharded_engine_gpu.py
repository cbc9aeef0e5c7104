"""The agent-sharded wide-critic instance (RPBCACEngine.shard_agents) on REAL kernels: two "ranks" as
two threads of this process, each with its own engine on cuda:0, the two collectives as plain device copies
(parallel.ThreadComm).  Checks what the gloo/hipemu test cannot: the gfx950 kernels (LDS-DMA, packed lattice operands,
MFMA GEMMs) running on agent-range views of every buffer.  Result: bit-identical to the unsharded engine.

The last two cases leave the packed-operand path in block 0 (an out-of-range critic operand in ONE agent of the LAST rank, see
tests/test_sharded_engine_gloo.py): both ranks are off it after every block, each warned once, and their row all-gathers name the
same buffers in the same order."""
import threading

import numpy as np
import pytest
import torch

import engine_checks as EC
from rcmarl_amd import capi
from rcmarl_amd.parallel import ThreadComm

pytestmark = pytest.mark.gpu

# (agents, d, H, graph, critic width, lattice path, agent with an out-of-range critic operand or None)
CASES = [(8, 4, 1, "circ", 64, True, None),          # packed bf16x3 layer 1: 4 agents x 64 units = two 128-row tiles per rank
         (8, 3, 1, "rand", 128, False, None),        # dense f32-MFMA path, general K1 kernel
         (16, 6, 2, "circ", 512, True, None),        # the cfg-5 critic width
         (64, 6, 2, "circ", 64, True, None),         # 32 agents per rank: the 20-unit team-reward net is sharded too (packed operands)
         (128, 66, 32, "circ", 512, True, None),     # BASELINE configs[4] at an eighth of the agents: d = 66, H = 32, 512-unit critic
         (8, 4, 1, "circ", 128, True, 6),            # the packed-operand path left in block 0: agent 6 (rank 1) has W2[k][j] = 70
         (8, 4, 1, "circ", 512, True, 6)]


def _setup(case):
    n, d, H, graph, hid, lattice, planted = case
    rng = np.random.default_rng(n * 7 + d)
    if graph == "circ":
        nodes = [[(i + k) % n for k in range(d)] for i in range(n)]
    else:
        nodes = [[i] + [int(x) for x in rng.permutation([j for j in range(n) if j != i])[:d - 1]] for i in range(n)]
    args = EC.make_args(["Cooperative"] * n, H=H, n_episodes=9 if planted is None else 13, max_ep_len=5, n_ep_fixed=4, n_epochs=2, buffer_size=30, seed=23,
                        in_nodes=nodes, fast_lr=0.002)
    W, goals = EC.make_inputs(args, 6, (23,), critic_hid=hid)
    if planted is not None:                            # three update blocks: the block after the fallback is inside the run
        assert planted >= n // 2
        EC.plant_out_of_range_w2(W[0][planted]["critic"])
    return args, W, goals, hid, lattice


def _snapshot(eng, logs):
    out = {"theta_" + k: v.cpu().numpy() for k, v in eng.theta.items()}
    out.update({"adam_m": eng.adam_m.cpu().numpy(), "loss_critic": eng.loss["critic"].cpu().numpy(),
                "loss_tr": eng.loss["tr"].cpu().numpy()})
    out.update({"rp_" + k: v[:, :eng.B].cpu().numpy() for k, v in eng.rp.items()})
    out.update({"log_" + k: np.asarray(v) for k, v in logs.items()})
    return out


def _watch(eng, record, caught):
    """after every block: is this engine off the packed path, how often has it warned; every row all-gather by buffer and columns"""
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


@pytest.mark.parametrize("case", CASES, ids=lambda c: "N%d-d%d-%s-hid%d-%s%s" % (c[0], c[1], c[3], c[4], "lattice" if c[5] else "dense",
                                                                                 "" if c[6] is None else "-range-fallback"))
def test_agent_sharded_wide_critic_two_ranks_on_one_gpu(case):
    import warnings
    lib = capi.load()
    args, W, goals, hid, lattice = _setup(case)
    planted, n_blocks = case[6], (2 if case[6] is None else 3)
    world = 2
    records = [{"pk_none": [], "warned": [], "gathers": []} for _ in range(world + 1)]
    # (one recorder for the whole process: the warnings module's state is not per thread)
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        _sharded_and_unsharded(case, lib, args, W, goals, hid, lattice, world, records, caught)
    ref_rec = records[world]
    packed = lattice and hid % 128 == 0
    assert ref_rec["pk_none"] == [not packed or planted is not None] * n_blocks, ref_rec
    assert ref_rec["warned"][-1] == (0 if planted is None else 1), ref_rec
    assert records[0]["gathers"] and records[1]["gathers"] == records[0]["gathers"], \
        [(q, a, b) for q, (a, b) in enumerate(zip(records[0]["gathers"], records[1]["gathers"])) if a != b]
    for r in range(world):
        assert records[r]["pk_none"] == ref_rec["pk_none"], (r, records[r]["pk_none"])
    # every engine of this process warns into the same list: the unsharded one first, then one warning per rank
    assert len([w for w in caught if "packed-operand" in str(w.message)]) == (0 if planted is None else 1 + world)


def _sharded_and_unsharded(case, lib, args, W, goals, hid, lattice, world, records, caught):
    ref_eng, ref_logs = EC.run_engine(args, 6, 6, "device", "cuda", lib, (23,), W, goals, lattice=lattice, critic_hid=hid,
                                      tweak=lambda e: _watch(e, records[world], caught))
    assert ref_eng.wide and ref_eng.lat_active == lattice
    assert all(bool(torch.isfinite(v).all()) for v in ref_eng.theta.values())
    ref = _snapshot(ref_eng, ref_logs)
    comms, results, errors = ThreadComm.make(world), [None] * world, []

    def rank_main(r):
        try:
            torch.cuda.set_device(0)
            eng, logs = EC.run_engine(args, 6, 6, "device", "cuda", lib, (23,), W, goals, lattice=lattice, critic_hid=hid,
                                      tweak=lambda e: (_watch(e, records[r], caught), e.shard_agents(comm=comms[r])))
            assert eng.shard is not None and eng.shard.n_loc == case[0] // world and not eng._windowed
            # the team-reward net joins whenever its packed operands split on 128-row tiles (or are not used)
            assert eng.shard.shard_tr == ((not lattice) or (eng.shard.n_loc * 20) % 128 == 0)
            assert sorted(eng.shard.sc) == (["critic", "tr"] if eng.shard.shard_tr else ["critic"])
            results[r] = _snapshot(eng, logs)
        except BaseException as e:            # noqa: BLE001 -- reported below; the peer's barrier breaks by timeout/abort
            errors.append((r, repr(e)))
            comms[r]._sh["barrier"].abort()
    threads = [threading.Thread(target=rank_main, args=(r,)) for r in range(world)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errors, errors
    for r in range(world):
        assert sorted(results[r]) == sorted(ref)
        for k in ref:
            np.testing.assert_array_equal(results[r][k], ref[k], err_msg="rank %d %s" % (r, k))
