"""Checks of the clip report (what the resilient aggregation trims, per recipient and in-neighbour slot), shared by the hipemu (CPU)
tests and the GPU tests.

Kernel checks take a *backend* as tests/kernel_checks.py does (bk.lib, bk.dev, bk.ptr, bk.host, bk.stream); engine checks take
(device, lib).  Every comparison is exact integer equality with a NumPy recount whose window comes from oracle.aggregation_bounds:
the counts are integers, so there is no tolerance anywhere in this file.
"""
import ctypes

import numpy as np

import engine_checks as EC
import kernel_checks as KC
import ragged_checks as RC
from oracle import rpbcac_oracle as O
from rcmarl_amd import capi
from rcmarl_amd.engine import EngineConfig, RPBCACEngine

HUGE = np.float32(3e38)


# ---- the recount ------------------------------------------------------------------------------------------------------------
def recount(msg, in_nodes, H, coop, P_hid, ldc):
    """(below, above) int64 [S][N][ldc] of ONE call: for cooperative i and slot k, the columns p < P_hid of neighbour k's row that lie
    strictly below / above the oracle's clip window of (i, p).  NumPy's < and > are the IEEE comparisons the contract names."""
    S, N = msg.shape[:2]
    below, above = np.zeros((S, N, ldc), np.int64), np.zeros((S, N, ldc), np.int64)
    for s in range(S):
        for i in range(N):
            if not coop[i]:
                continue
            vals = msg[s, in_nodes[i], :P_hid]
            lo, hi, _ = O.aggregation_bounds(vals, int(H[i]))
            below[s, i, :len(in_nodes[i])] = (vals < lo[None]).sum(axis=1)
            above[s, i, :len(in_nodes[i])] = (vals > hi[None]).sum(axis=1)
    return below, above


def prefill(rng, S, N, ldc):
    """accumulators that are not zero: the entry adds, and what it must not touch keeps these bits"""
    return (rng.integers(1, 2 ** 40, size=(S, N, ldc)).astype(np.int64), rng.integers(1, 2 ** 40, size=(S, N, ldc)).astype(np.int64))


def scratch_for(bk, S, N, ldc, P_hid, rng):
    n = bk.lib.rcmarl_consensus_clip_counts_scratch(S, N, ldc, P_hid)
    assert n >= 0
    return bk.dev(rng.integers(-2 ** 31, 2 ** 31 - 1, size=max(n, 1)).astype(np.int32))      # contents must not matter


def run_regular(bk, msg, nbr, coop, d, H, P_hid, ldc, below0, above0, calls=1, rng=None):
    S, N, ldp = msg.shape
    rng = np.random.default_rng(0) if rng is None else rng
    d_msg, d_nbr, d_coop = bk.dev(msg), bk.dev(np.asarray(nbr, np.int32)), bk.dev(np.asarray(coop, np.int32))
    d_b, d_a, d_s = bk.dev(below0), bk.dev(above0), scratch_for(bk, S, N, ldc, P_hid, rng)
    for _ in range(calls):
        bk.lib.rcmarl_consensus_clip_counts(bk.ptr(d_msg), bk.ptr(d_nbr), bk.ptr(d_coop), bk.ptr(d_b), bk.ptr(d_a), bk.ptr(d_s),
                                            S, N, ldp, P_hid, d, H, ldc, bk.stream)
    return bk.host(d_b).copy(), bk.host(d_a).copy()


def run_ragged(bk, msg, in_nodes, H, coop, P_hid, ldc, below0, above0, rng=None):
    S, N, ldp = msg.shape
    rng = np.random.default_rng(0) if rng is None else rng
    off, idx, order, classes, table = RC.csr_and_classes(in_nodes, H, coop)
    d_msg, d_off, d_idx, d_order = bk.dev(msg), bk.dev(off), bk.dev(idx), bk.dev(order)
    d_b, d_a, d_s = bk.dev(below0), bk.dev(above0), scratch_for(bk, S, N, ldc, P_hid, rng)
    bk.lib.rcmarl_consensus_clip_counts_ragged(bk.ptr(d_msg), bk.ptr(d_off), bk.ptr(d_idx), bk.ptr(d_order), table, len(classes),
                                               bk.ptr(d_b), bk.ptr(d_a), bk.ptr(d_s), S, N, ldp, P_hid, ldc, bk.stream)
    return bk.host(d_b).copy(), bk.host(d_a).copy(), classes, order


def check_invariant(db, da, H, P_hid):
    """a window trims at most H values on each side of every column"""
    Hn = np.asarray(H, np.int64)[None, :]
    assert (db.sum(axis=2) <= Hn * P_hid).all() and (da.sum(axis=2) <= Hn * P_hid).all()
    assert (db >= 0).all() and (da >= 0).all()


# ---- kernel: regular graphs ---------------------------------------------------------------------------------------------------
def check_regular(bk, N, d, H, graph, S, P, P_hid, seed=1, n_noncoop=1, extra_ldc=2):
    """rcmarl_consensus_clip_counts against the recount: non-zero accumulators, huge values planted in the output-layer columns
    and in the rows of the non-cooperative agents (their rows are never counted FOR, their values are counted when a cooperative
    agent lists them), two calls double what one call adds, and what must stay untouched keeps its bits."""
    rng = np.random.default_rng(seed)
    ldp, ldc = KC.pad64(P), d + extra_ldc
    nbr = KC.circulant(N, d) if graph == "circ" else KC.random_regular(N, d, rng)
    in_nodes = [[int(j) for j in row] for row in nbr]
    coop = np.ones(N, np.int32)
    coop[rng.permutation(N)[:n_noncoop]] = 0
    msg = RC.k1_messages(rng, S, N, ldp, in_nodes)
    msg[:, :, P_hid:] = HUGE * np.where(rng.random((S, N, ldp - P_hid)) < 0.5, 1, -1).astype(np.float32)
    msg[:, coop == 0, :P_hid] = HUGE
    b0, a0 = prefill(rng, S, N, ldc)
    wb, wa = recount(msg, in_nodes, [H] * N, coop, P_hid, ldc)
    check_invariant(wb, wa, [H] * N, P_hid)
    if H > 0 and n_noncoop:
        assert wa.sum() > 0 and wb.sum() > 0              # the case clips on both sides
    for calls in (1, 2):
        gb, ga = run_regular(bk, msg, nbr, coop, d, H, P_hid, ldc, b0, a0, calls=calls, rng=rng)
        np.testing.assert_array_equal(gb, b0 + calls * wb, err_msg="below, %d call(s)" % calls)
        np.testing.assert_array_equal(ga, a0 + calls * wa, err_msg="above, %d call(s)" % calls)
    # (the equalities above already say it; spelt out: slots >= d and rows of non-cooperative agents keep their bits)
    np.testing.assert_array_equal(gb[:, :, d:], b0[:, :, d:])
    np.testing.assert_array_equal(ga[:, coop == 0], a0[:, coop == 0])
    assert (gb[:, :, 0] == b0[:, :, 0]).all() and (ga[:, :, 0] == a0[:, :, 0]).all()     # the own value is never outside its window


def check_ties(bk, N=9, d=7, H=2, S=2, P=100, P_hid=70, seed=5):
    """A message matrix of five levels, +0 and -0 among them, so that ties decide every window; one agent whose own value is the
    extreme of every column: the window opens to it, so its slot 0 -- and every other agent's slot 0 -- counts nothing."""
    rng = np.random.default_rng(seed)
    ldp, ldc = KC.pad64(P), d
    levels = np.array([-1.0, -0.0, 0.0, 0.5, 2.0], np.float32)
    msg = levels[rng.integers(0, 5, size=(S, N, ldp))]
    msg[:, 3] = np.float32(7.0)                              # agent 3: the maximum of every column
    msg[0, 3, ::2] = np.float32(-7.0)                        # ... or the minimum
    nbr = KC.random_regular(N, d, rng)
    in_nodes = [[int(j) for j in row] for row in nbr]
    coop = np.ones(N, np.int32)
    z = np.zeros((S, N, ldc), np.int64)
    wb, wa = recount(msg, in_nodes, [H] * N, coop, P_hid, ldc)
    assert wb.sum() > 0 and wa.sum() > 0
    gb, ga = run_regular(bk, msg, nbr, coop, d, H, P_hid, ldc, z, z, rng=rng)
    np.testing.assert_array_equal(gb, wb)
    np.testing.assert_array_equal(ga, wa)
    assert not gb[:, :, 0].any() and not ga[:, :, 0].any()
    check_invariant(gb, ga, [H] * N, P_hid)
    # +0 and -0 alone: nothing is strictly below or above anything
    msg2 = np.where(rng.random((S, N, ldp)) < 0.5, np.float32(0.0), np.float32(-0.0)).astype(np.float32)
    gb, ga = run_regular(bk, msg2, nbr, coop, d, H, P_hid, ldc, z, z, rng=rng)
    assert not gb.any() and not ga.any()
    # a NaN is never counted (a column of NaNs; what the window is there does not matter)
    msg3 = msg.copy()
    msg3[:, :, 4] = np.float32(np.nan)
    msg3[:, :, 4 + 64] = np.float32(np.nan)
    keep = np.ones(P_hid, bool)
    keep[[4, 68]] = False
    wb3, wa3 = recount(msg3[:, :, :P_hid][:, :, keep], in_nodes, [H] * N, coop, P_hid - 2, ldc)
    gb, ga = run_regular(bk, msg3, nbr, coop, d, H, P_hid, ldc, z, z, rng=rng)
    np.testing.assert_array_equal(gb, wb3)
    np.testing.assert_array_equal(ga, wa3)


def check_H0(bk, N=5, d=4, S=2, P=215, P_hid=150, seed=3):
    """H = 0: the window is [min, max], nothing changes (regular entry; ragged entry with only H = 0 classes)"""
    rng = np.random.default_rng(seed)
    ldp = KC.pad64(P)
    nbr = KC.circulant(N, d)
    msg = rng.normal(size=(S, N, ldp)).astype(np.float32)
    coop = np.ones(N, np.int32)
    b0, a0 = prefill(rng, S, N, d)
    gb, ga = run_regular(bk, msg, nbr, coop, d, 0, P_hid, d, b0, a0, rng=rng)
    np.testing.assert_array_equal(gb, b0)
    np.testing.assert_array_equal(ga, a0)
    gb, ga, _, _ = run_ragged(bk, msg, [[int(j) for j in r] for r in nbr], [0] * N, coop, P_hid, d, b0, a0, rng=rng)
    np.testing.assert_array_equal(gb, b0)
    np.testing.assert_array_equal(ga, a0)


# ---- kernel: irregular graphs --------------------------------------------------------------------------------------------------
def check_ragged(bk, N=24, S=2, P=215, P_hid=150, seed=1):
    """rcmarl_consensus_clip_counts_ragged on ragged_checks.ragged_graph (degrees 1 .. 21, the last one beyond the generated
    networks of the ragged kernels; H from 0 up) against the recount and against the regular entry run class by class."""
    rng = np.random.default_rng(seed)
    ldp = KC.pad64(P)
    in_nodes, H, coop = RC.ragged_graph(N, rng)
    ldc = max(len(r) for r in in_nodes)
    msg = RC.k1_messages(rng, S, N, ldp, in_nodes)
    msg[:, :, P_hid:] = HUGE
    msg[:, coop == 0, :P_hid] = -HUGE
    b0, a0 = prefill(rng, S, N, ldc)
    gb, ga, classes, order = run_ragged(bk, msg, in_nodes, H, coop, P_hid, ldc, b0, a0, rng=rng)
    assert any(d > 20 and h > 0 for d, h, _, _ in classes) and any(h == 0 for _, h, _, _ in classes) and (coop == 0).any()
    wb, wa = recount(msg, in_nodes, H, coop, P_hid, ldc)
    check_invariant(wb, wa, H, P_hid)
    assert wb.sum() > 0 and wa.sum() > 0
    np.testing.assert_array_equal(gb, b0 + wb)
    np.testing.assert_array_equal(ga, a0 + wa)
    # class by class through the regular entry (coop masked to the class, a dense table of its rows), accumulating
    cb, ca = b0, a0
    for d, h, first, count in classes:
        nbr, mask = RC.dense_table_of_class(in_nodes, order[first:first + count], d)
        cb, ca = run_regular(bk, msg, nbr, mask, d, h, P_hid, ldc, cb, ca, rng=rng)
    np.testing.assert_array_equal(gb, cb)
    np.testing.assert_array_equal(ga, ca)


# ---- argument validation (no GPU) -------------------------------------------------------------------------------------------
def check_argument_validation(lib):
    import pytest
    one = ctypes.c_void_p(64)                     # non-null, never dereferenced: validation comes before any HIP call
    S, N, ldp, P_hid, d, H, ldc = 1, 5, 64, 40, 4, 1, 4
    assert lib.rcmarl_consensus_clip_counts_scratch(S, N, ldc, P_hid) > 0
    assert lib.rcmarl_consensus_clip_counts_scratch(0, N, ldc, P_hid) == 0
    good = [one, one, one, one, one, one, S, N, ldp, P_hid, d, H, ldc, None]
    bad = [{0: None}, {1: None}, {2: None}, {3: None}, {4: None}, {5: None}, {6: 0}, {7: 0}, {8: 65}, {8: 32}, {9: 0}, {9: 65},
           {10: 2}, {10: 6, 12: 6}, {12: 3}, {11: -1}, {11: 0, 5: None}]
    for change in bad:
        args = list(good)
        for k, v in change.items():
            args[k] = v
        with pytest.raises(capi.RcmarlError, match="RCMARL_ERR_ARG"):
            lib.rcmarl_consensus_clip_counts(*args)
    h0 = list(good)
    h0[11] = 0
    assert lib.rcmarl_consensus_clip_counts(*h0) == 0          # H = 0: RCMARL_OK without a launch (nothing here is a real pointer)
    big = list(good)
    big[7] = 5000                                             # the [N][4] tile image beyond the LDS, as K1
    with pytest.raises(capi.RcmarlError, match="RCMARL_ERR_UNSUPPORTED"):
        lib.rcmarl_consensus_clip_counts(*big)

    def cls(d_, h_, first, count):
        return (capi.RaggedClass * 1)(capi.RaggedClass(d_, h_, first, count))
    rgood = [one, one, one, one, cls(3, 1, 0, 2), 1, one, one, one, S, N, ldp, P_hid, ldc, None]
    rbad = [{0: None}, {1: None}, {2: None}, {3: None}, {4: None}, {5: 0}, {6: None}, {7: None}, {8: None}, {9: 0}, {10: 0}, {11: 65},
            {12: 0}, {12: 65}, {13: 2}, {4: cls(2, 1, 0, 2)}, {4: cls(0, 0, 0, 2)}, {4: cls(3, -1, 0, 2)}, {4: cls(3, 1, -1, 2)},
            {4: cls(3, 1, 0, 0)}, {4: cls(3, 1, 4, 2)}, {4: cls(6, 1, 0, 2), 13: 6}]
    for change in rbad:
        args = list(rgood)
        for k, v in change.items():
            args[k] = v
        with pytest.raises(capi.RcmarlError, match="RCMARL_ERR_ARG"):
            lib.rcmarl_consensus_clip_counts_ragged(*args)
    r0 = list(rgood)
    r0[4] = cls(3, 0, 0, 2)
    assert lib.rcmarl_consensus_clip_counts_ragged(*r0) == 0


# ---- engine -----------------------------------------------------------------------------------------------------------------
class RecountingLib:
    """The library with the two clip-count entries wrapped: every call is counted and, when an engine is attached, recounted in
    NumPy from the message matrix the engine holds at that moment (eng.msg[net]; the graph, H and roles come from its config)."""

    def __init__(self, lib):
        self._lib, self.calls, self.eng = lib, 0, None
        self.want = {}

    def __getattr__(self, name):
        fn = getattr(self._lib, name)
        if name not in ("rcmarl_consensus_clip_counts", "rcmarl_consensus_clip_counts_ragged"):
            return fn

        def counted(*a):
            self.calls += 1
            if self.eng is not None:
                self._recount(a[0])
            return fn(*a)
        return counted

    def _recount(self, msg_ptr):
        eng = self.eng
        net = [k for k in ("critic", "tr") if eng.msg[k].data_ptr() == msg_ptr]
        assert len(net) == 1, "the count entry must read eng.msg[net]"
        net = net[0]
        eng.sync()
        c = eng.cfg
        P_hid = eng.P[net] - (eng.hid[net] + 1)
        b, a = recount(eng.msg[net].cpu().numpy()[:, :, :], c.in_nodes, c.H_per_agent, eng.coop_np, P_hid, max(c.degrees))
        if net not in self.want:
            self.want[net] = [np.zeros_like(b), np.zeros_like(a), 0]
        self.want[net][0] += b
        self.want[net][1] += a
        self.want[net][2] += 1


def run_engine(args, device, lib, seeds, W, goals, clip_report, critic_hid=20, attach=None, n_episodes=None, eng=None):
    """engine_checks.run_engine (rng_mode 'device', a 5 x 5 grid) with the clip_report keyword"""
    n, S = args["n_agents"], len(seeds)
    if eng is None:
        cfg = EngineConfig(n, args["agent_label"], args["in_nodes"], H=args["H"], gamma=args["gamma"], slow_lr=args["slow_lr"],
                           fast_lr=args["fast_lr"], max_ep_len=args["max_ep_len"], n_ep_fixed=args["n_ep_fixed"],
                           n_epochs=args["n_epochs"], buffer_size=args["buffer_size"], common_reward=args["common_reward"],
                           nrow=5, ncol=5, n_seeds=S, rng_mode="device", lattice=False, critic_hid=critic_hid, clip_report=clip_report)
        eng = RPBCACEngine(cfg, seeds=list(seeds), device=device, lib=lib)
        for s in range(S):
            for i in range(n):
                for net in ("actor", "critic", "tr"):
                    eng.set_weights(s, i, net, W[s][i][net])
        eng.set_goals(np.stack(goals))
    if attach is not None:
        attach.eng = eng
    n_episodes = args["n_episodes"] if n_episodes is None else n_episodes
    return eng, (eng.train(n_episodes) if n_episodes else None)


def tiny_args(labels, H=1, in_nodes=None, seed=11):
    """two blocks of two epochs on a tiny grid, as the engine checks size them"""
    return EC.make_args(labels, H=H, n_episodes=4, max_ep_len=3, n_ep_fixed=2, n_epochs=2, buffer_size=9, seed=seed, in_nodes=in_nodes)


def assert_report_equals_recount(eng, proxy, n_blocks=2):
    rep = eng.clip_report()
    assert set(rep) == {"critic", "tr"}
    for net in ("critic", "tr"):
        wb, wa, n = proxy.want[net]
        r = rep[net]
        assert n == n_blocks * eng.cfg.n_epochs == r["steps"]
        assert r["below"].dtype == np.int64 and r["below"].shape == (eng.S, eng.N, max(eng.cfg.degrees))
        np.testing.assert_array_equal(r["below"], wb, err_msg=net)
        np.testing.assert_array_equal(r["above"], wa, err_msg=net)
        assert r["P_hid"] == eng.P[net] - (eng.hid[net] + 1) and r["in_nodes"] == eng.cfg.in_nodes
        # sender_rate from its definition, independently of the engine's loop
        c = eng.cfg
        for j in range(eng.N):
            slots = [(i, k) for i in range(eng.N) if eng.coop_np[i] for k in range(1, len(c.in_nodes[i])) if c.in_nodes[i][k] == j]
            if not slots:
                assert np.isnan(r["sender_rate"][:, j]).all()
                continue
            tot = sum(wb[:, i, k] + wa[:, i, k] for i, k in slots).astype(np.float64)
            np.testing.assert_array_equal(r["sender_rate"][:, j], tot / (float(n) * r["P_hid"] * len(slots)))
    return rep


def check_engine_recount(device, lib, scenario, monkeypatch):
    """clip_report() equals the summed NumPy recount of every clip-count call: 'malicious' = a regular team with one Malicious agent,
    'ragged' = the "malicious" irregular scenario of ragged_checks, 'wide' = critic_hid 32"""
    monkeypatch.setenv("RCMARL_GRAPH", "0")            # the recount reads the message matrix at every call: no captured epochs
    critic_hid = 20
    if scenario == "malicious":
        args = tiny_args(["Cooperative"] * 4 + ["Malicious"])
    elif scenario == "ragged":
        sc = RC.SCENARIOS["malicious"]
        args = tiny_args(sc["labels"], H=list(sc["H"]), in_nodes=[list(r) for r in sc["in_nodes"]])
    else:
        args, critic_hid = tiny_args(["Cooperative"] * 5), 32
    seeds = (11, 12) if scenario == "malicious" else (11,)      # two seeds once: the report is per seed
    W, goals = EC.make_inputs(args, 5, seeds, critic_hid=critic_hid)
    proxy = RecountingLib(lib)
    eng, _ = run_engine(args, device, proxy, seeds, W, goals, True, critic_hid=critic_hid, attach=proxy)
    assert eng.cfg.regular == (scenario != "ragged") and eng.wide == (scenario == "wide")
    assert proxy.calls == 2 * 2 * args["n_epochs"]          # nets x blocks x epochs
    rep = assert_report_equals_recount(eng, proxy)
    if scenario != "wide":
        assert rep["critic"]["below"].sum() + rep["critic"]["above"].sum() > 0
    return eng, rep


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def check_switch_changes_nothing(device, lib):
    """on against off: parameter matrices, Adam slots and logs bit for bit; off: no clip-count launch, no buffer"""
    import pytest
    args = tiny_args(["Cooperative"] * 4 + ["Malicious"])
    seeds = (11,)
    W, goals = EC.make_inputs(args, 5, seeds)
    out = {}
    for on in (False, True):
        proxy = RecountingLib(lib)
        eng, logs = run_engine(args, device, proxy, seeds, W, goals, on)
        out[on] = (eng, logs, proxy.calls)
    off, on = out[False], out[True]
    assert off[2] == 0 and off[0].clip is None and on[2] > 0
    with pytest.raises(ValueError, match="clip report is off"):
        off[0].clip_report()
    for net in off[0].theta:
        np.testing.assert_array_equal(_bits(off[0].theta[net].cpu().numpy()), _bits(on[0].theta[net].cpu().numpy()), err_msg=net)
    np.testing.assert_array_equal(_bits(off[0].adam_m.cpu().numpy()), _bits(on[0].adam_m.cpu().numpy()))
    np.testing.assert_array_equal(_bits(off[0].adam_v.cpu().numpy()), _bits(on[0].adam_v.cpu().numpy()))
    assert set(off[1]) == set(on[1])
    for k in off[1]:
        np.testing.assert_array_equal(off[1][k], on[1][k], err_msg=k)
    assert "clip_report" not in off[0].state_dict() and "clip_report" in on[0].state_dict()


def check_faulty_sender(device, lib):
    """Four cooperative agents and one Faulty agent (agent 4) whose hidden critic weights are all 1e3: every recipient trims every one
    of its hidden-layer values at every step -- above == steps x P_hid exactly -- and its sender_rate is 1, the team's largest."""
    args = tiny_args(["Cooperative"] * 4 + ["Faulty"])
    seeds = (11,)
    W, goals = EC.make_inputs(args, 5, seeds)
    for s in range(len(seeds)):
        for k in range(4):                                  # W1, b1, W2, b2
            W[s][4]["critic"][k][...] = np.float32(1e3)
    eng, _ = run_engine(args, device, lib, seeds, W, goals, True)
    r = eng.clip_report()["critic"]
    steps, P_hid = r["steps"], r["P_hid"]
    assert steps == 2 * args["n_epochs"] and P_hid == eng.P["critic"] - 21
    listeners = [(i, EC.CIRC5[i].index(4)) for i in range(4) if 4 in EC.CIRC5[i]]
    assert len(listeners) == 3
    for i, k in listeners:
        assert (r["above"][:, i, k] == steps * P_hid).all() and not r["below"][:, i, k].any()
    assert not r["above"][:, 4].any() and not r["below"][:, 4].any()       # the Faulty agent's own row: never counted for
    np.testing.assert_array_equal(r["sender_rate"][:, 4], 1.0)
    assert (r["sender_rate"][:, :4] < 1.0).all()


def check_checkpoint(device, lib, path):
    """the accumulators and the step count travel in the checkpoint; a file without them starts the report from zero"""
    args = tiny_args(["Cooperative"] * 4 + ["Malicious"])
    seeds = (11,)
    W, goals = EC.make_inputs(args, 5, seeds)
    a, _ = run_engine(args, device, lib, seeds, W, goals, True)                      # two blocks
    b, _ = run_engine(args, device, lib, seeds, W, goals, True, n_episodes=2)        # one block, saved ...
    b.save_checkpoint(path)
    c, _ = run_engine(args, device, lib, seeds, W, goals, True, n_episodes=0)        # ... and continued in a fresh engine
    c.load_checkpoint(path)
    assert c.clip_report()["critic"]["steps"] == args["n_epochs"]
    run_engine(args, device, lib, seeds, W, goals, True, n_episodes=2, eng=c)
    ra, rc = a.clip_report(), c.clip_report()
    for net in ra:
        assert ra[net]["steps"] == rc[net]["steps"] == 2 * args["n_epochs"]
        np.testing.assert_array_equal(ra[net]["below"], rc[net]["below"])
        np.testing.assert_array_equal(ra[net]["above"], rc[net]["above"])
    assert ra["critic"]["above"].sum() > 0
    # reset: the report it returns is the last one before zero
    last = c.clip_report(reset=True)
    np.testing.assert_array_equal(last["critic"]["above"], ra["critic"]["above"])
    z = c.clip_report()
    assert z["critic"]["steps"] == 0 and not z["critic"]["above"].any() and not z["tr"]["below"].any()
    # a checkpoint written with the switch off, loaded with the switch on: from zero
    off, _ = run_engine(args, device, lib, seeds, W, goals, False, n_episodes=2)
    sd = off.state_dict()
    assert "clip_report" not in sd
    a.load_state_dict(sd)
    z = a.clip_report()
    assert z["tr"]["steps"] == 0 and not z["critic"]["above"].any() and not z["critic"]["below"].any()
    # ... and the other way round: the key is ignored
    off.load_state_dict(b.state_dict())


def check_shard_refusal(device, lib):
    import pytest
    cfg = EngineConfig(4, ["Cooperative"] * 4, [[0, 1, 2], [1, 2, 3], [2, 3, 0], [3, 0, 1]], H=1, max_ep_len=3, n_ep_fixed=2, n_epochs=1,
                       buffer_size=6, critic_hid=32, lattice=False, clip_report=True)
    eng = RPBCACEngine(cfg, seeds=[1], device=device, lib=lib)
    with pytest.raises(ValueError, match="clip report"):
        eng.shard_agents(rank=0, world=2)


def check_graph_replay(device, lib, monkeypatch, seed=21):
    """GPU: a run that replays captured epochs reports what an uncaptured run reports, steps included"""
    args = EC.make_args(["Cooperative"] * 5, H=1, n_episodes=6, max_ep_len=3, n_ep_fixed=2, n_epochs=4, buffer_size=12, seed=seed)
    W, goals = EC.make_inputs(args, 5, (seed,))
    out = {}
    for graph in ("1", "0"):
        monkeypatch.setenv("RCMARL_GRAPH", graph)
        eng, _ = run_engine(args, device, lib, (seed,), W, goals, True)
        out[graph] = (eng, eng.clip_report())
    assert out["1"][0].graph_replays > 0 and out["1"][0].graph_captures > 0 and out["0"][0].graph_replays == 0
    for net in ("critic", "tr"):
        a, b = out["1"][1][net], out["0"][1][net]
        assert a["steps"] == b["steps"] == 3 * args["n_epochs"]
        np.testing.assert_array_equal(a["below"], b["below"])
        np.testing.assert_array_equal(a["above"], b["above"])
    assert out["0"][1]["critic"]["below"].sum() + out["0"][1]["critic"]["above"].sum() > 0


# ---- drop-in surface ------------------------------------------------------------------------------------------------------------
def _dropin_run(engine_hook, clip, seed=5):
    import dropin_checks as DC
    from rcmarl_amd import keras_compat as K
    from rcmarl_amd.agents.resilient_CAC_agents import RPBCAC_agent
    from rcmarl_amd.environments.grid_world import Grid_World
    from rcmarl_amd.training.train_agents import train_RPBCAC
    n = 5
    K.set_seed(seed)
    agents = []
    for _ in range(n):
        actor, critic, tr = DC.make_models(n)
        agents.append(RPBCAC_agent(actor, critic, tr, slow_lr=0.002, fast_lr=0.01, gamma=0.9, H=1))
    args = EC.make_args(["Cooperative"] * n, H=1, n_episodes=4, max_ep_len=3, n_ep_fixed=2, n_epochs=1, buffer_size=9, seed=seed)
    if clip is not None:
        args["clip_report"] = clip
    goals = np.random.default_rng(seed).integers(0, 5, size=(n, 2))
    np.random.seed(seed)
    env = Grid_World(nrow=5, ncol=5, n_agents=n, desired_state=goals, initial_state=goals, randomize_state=True, scaling=True)
    return train_RPBCAC(env, agents, args, engine_hook=engine_hook)


def check_dropin(engine_hook):
    """train_RPBCAC: args['clip_report'] puts the report of seed 0 into sim_data.attrs; columns and return types as before"""
    import pandas as pd
    w0, df0 = _dropin_run(engine_hook, None)
    w1, df1 = _dropin_run(engine_hook, True)
    assert "clip_report" not in df0.attrs
    assert isinstance(df1, pd.DataFrame) and list(df1.columns) == list(df0.columns) == ["True_team_returns", "True_adv_returns",
                                                                                       "Estimated_team_returns"]
    for col in df0.columns:
        np.testing.assert_array_equal(df0[col].to_numpy(), df1[col].to_numpy())
    assert isinstance(w1, list) and len(w1) == len(w0) == 5
    rep = df1.attrs["clip_report"]
    assert set(rep) == {"critic", "tr"}
    for net in rep:
        r = rep[net]
        assert r["below"].shape == r["above"].shape == (5, 4) and r["below"].dtype == np.int64 and r["sender_rate"].shape == (5,)
        assert r["steps"] == 2 and r["in_nodes"] == EC.CIRC5
        assert (r["below"].sum(axis=1) <= r["steps"] * r["P_hid"]).all() and (r["above"].sum(axis=1) <= r["steps"] * r["P_hid"]).all()
    assert rep["critic"]["below"].sum() + rep["critic"]["above"].sum() > 0


def check_main(engine_hook, tmp_path, monkeypatch):
    """main --clip_report writes clip_report.npz beside sim_data.pkl; without the flag no such file"""
    import os
    from rcmarl_amd import main as RM
    monkeypatch.chdir(tmp_path)
    argv = ["--n_agents", "5", "--H", "1", "--n_episodes", "2", "--n_ep_fixed", "2", "--max_ep_len", "3", "--n_epochs", "1",
            "--buffer_size", "6", "--random_seed", "5", "--slow_lr", "0.002"]
    RM.main(argv, engine_hook=engine_hook)
    assert os.path.exists("sim_data.pkl") and not os.path.exists("clip_report.npz")
    _, df = RM.main(argv + ["--clip_report"], engine_hook=engine_hook)
    z = np.load("clip_report.npz")
    rep = df.attrs["clip_report"]
    for net in ("critic", "tr"):
        np.testing.assert_array_equal(z[net + "_below"], rep[net]["below"])
        np.testing.assert_array_equal(z[net + "_above"], rep[net]["above"])
        assert int(z[net + "_steps"]) == 1 and int(z[net + "_P_hid"]) == rep[net]["P_hid"]
        assert z[net + "_sender_rate"].shape == (5,)
    np.testing.assert_array_equal(z["in_nodes"], np.asarray(EC.CIRC5))
