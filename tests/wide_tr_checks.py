"""Wide team-reward nets (EngineConfig.tr_hid != 20) -- checks shared by the hipemu and the GPU tests: the engine against oracle.train for
a wide team-reward net alone and beside a wide critic of the same and of another width (dense path, and both nets on packed
operands), the cross-epoch caches (a cached image is never reused after another net wrote its buffer), the routing by net, Greedy /
Malicious agents beside a wide team-reward net, rcmarl_wide_td_error against the three-launch form, the drop-in trainer, checkpoints
and refusals."""
import collections

import numpy as np
import pytest

import engine_checks as EC
from kernel_checks import pad64
from oracle import mlp_np as M
from oracle import rpbcac_oracle as O
from rcmarl_amd import capi
from rcmarl_amd.engine import EngineConfig, RPBCACEngine, net_numel

COOP = "Cooperative"
CIRC3 = [[0, 1, 2], [1, 2, 0], [2, 0, 1]]
N_ = 3
# (critic, team-reward net): a wide team-reward net alone, both wide at one width, both wide at different widths (scratch sizing)
WIDTH_PAIRS = ((20, 24), (24, 24), (32, 24))
PK_PAIR = (128, 128)              # both nets on the packed-operand path (lattice layer 1)
# the packed scratch is sized by the wider net and the narrower one uses a prefix: two packed widths with different tile sides (256:
# 256 x 256 tiles, 128: 128 x 128), and one packed net beside one on the dense path (which shares w_a2 / w_grads / w_est with it)
PK_MIXED_PAIRS = ((256, 128), (128, 24))
LATTICE_PAIR = (24, 40)           # lattice layer 1 (w1_split, dz pack + row sums at 3N columns), dense layers 2 and 3


def engine_args(n_episodes=4, seed=5, labels=None, in_nodes=None, n_epochs=2):
    labels = [COOP] * N_ if labels is None else labels
    return EC.make_args(labels, H=1, n_episodes=n_episodes, max_ep_len=3, n_ep_fixed=2, n_epochs=n_epochs, buffer_size=12, seed=seed,
                        in_nodes=CIRC3 if in_nodes is None else in_nodes)


def make_cfg(critic_hid=20, tr_hid=24, rng_mode="numpy", n_seeds=2, **kw):
    base = dict(H=1, max_ep_len=3, n_ep_fixed=2, n_epochs=2, buffer_size=12, nrow=3, ncol=3, n_seeds=n_seeds, rng_mode=rng_mode,
                critic_hid=critic_hid)
    if tr_hid is not None:                                            # None: built without the argument at all
        base["tr_hid"] = tr_hid
    labels, in_nodes = kw.pop("labels", [COOP] * N_), kw.pop("in_nodes", CIRC3)
    base.update(kw)
    return EngineConfig(len(labels), labels, in_nodes, **base)


def engine_inputs(seeds, critic_hid, tr_hid, n=N_, weight_seed=3, nrow=3):
    rng = np.random.default_rng(weight_seed)
    W = [[{"actor": M.init_mlp(rng, 2 * n, 20, 5), "critic": M.init_mlp(rng, 2 * n, critic_hid, 1), "tr": M.init_mlp(rng, 3 * n, tr_hid, 1)}
          for _ in range(n)] for _ in seeds]
    goals = [np.random.default_rng(100 + s).integers(0, nrow, size=(n, 2)) for s in range(len(seeds))]
    return W, goals


def make_engine(device, lib, seeds, W, goals, nrow=3, **kw):
    eng = RPBCACEngine(make_cfg(n_seeds=len(seeds), nrow=nrow, ncol=nrow, **kw), seeds=list(seeds), device=device, lib=lib)
    n = eng.N
    for s in range(len(seeds)):
        for i in range(n):
            for net in ("actor", "critic", "tr"):
                eng.set_weights(s, i, net, W[s][i][net])
    eng.set_goals(np.stack(goals))
    if eng.cfg.rng_mode == "numpy":
        eng.np_rngs = []
        for sd in seeds:
            r = np.random.RandomState(int(sd))
            r.randint([0, 0], [nrow, nrow], size=(n, 2))              # the env constructor's reset() draw (grid_world.py:28)
            eng.np_rngs.append(r)
    return eng


_ORACLE = {}


def oracle_run(seeds, critic_hid, tr_hid):
    """oracle.train of one width pair, computed once and shared (its networks are lists of arrays of any width)"""
    key = (tuple(seeds), critic_hid, tr_hid)
    if key not in _ORACLE:
        W, goals = engine_inputs(seeds, critic_hid, tr_hid)
        _ORACLE[key] = (W, goals) + tuple(EC.run_oracle(engine_args(), 3, 3, "numpy", seeds, W, goals))
    return _ORACLE[key]


def check_engine_vs_oracle(device, lib, critic_hid, tr_hid, lattice=False, seeds=(11, 12)):
    """Two seeds, two update blocks of two epochs against oracle.train at engine_checks.compare's default bars (weights 1e-4, strict
    actor), returns bit-identical.  lattice=True: layer 1 of both nets on the lattice kernels; with widths that are multiples of 128
    both nets then run on the packed-operand path."""
    W, goals, o_logs, o_w = oracle_run(seeds, critic_hid, tr_hid)
    eng = make_engine(device, lib, seeds, W, goals, critic_hid=critic_hid, tr_hid=tr_hid, lattice=lattice)
    P = net_numel(3 * N_, 1, tr_hid)
    assert eng.hid["tr"] == tr_hid and eng.P["tr"] == P and eng.ldp["tr"] == pad64(P)
    assert eng.msg["tr"].shape[-1] == eng.ldp["tr"] and eng.get_all_weights("tr").shape == (len(seeds), N_, P)
    assert eng.a1net["tr"].shape[1] == N_ * tr_hid
    assert eng.wide and eng.critic_wide == (critic_hid != 20)
    logs = eng.train(engine_args()["n_episodes"])
    assert eng.lat_active == lattice                                  # lattice: layer 1 of both nets on the lattice kernels
    for net, xkey, hid in (("critic", "s", critic_hid), ("tr", "sa", tr_hid)):
        assert bool(eng._pk_ok(net, xkey, eng.lat_B if lattice else 0)) == bool(lattice and hid % 128 == 0), net
    assert (eng.pk is not None) == bool(lattice and (critic_hid % 128 == 0 or tr_hid % 128 == 0))
    worst = EC.compare(eng, logs, o_logs, o_w)
    print("[wide tr] critic %d, team-reward net %d%s: worst |w - w_oracle| / max(1, |w|max): critic %.2e, team-reward net %.2e (bar 1e-4)"
          % (critic_hid, tr_hid, (", packed operands" if eng.pk is not None else ", lattice layer 1") if lattice else "", worst["critic"], worst["tr"]))
    return eng


def check_cache_invariant(device, lib, critic_hid, tr_hid, lattice=False, seeds=(11,)):
    """The same instance with the cross-epoch caches on (reuse_activations = True: step 0 of a local fit starts from the image the
    consensus step left) and off: bit-identical weights.  A cached image that another net's phase wrote into would show here."""
    W, goals = engine_inputs(seeds, critic_hid, tr_hid)
    out = []
    for reuse in (True, False):
        eng = make_engine(device, lib, seeds, W, goals, critic_hid=critic_hid, tr_hid=tr_hid, lattice=lattice)
        eng.reuse_activations = reuse
        eng.train(engine_args()["n_episodes"])
        if lattice:
            assert eng._pk_ok("tr", "sa", eng.lat_B) and eng._pk_ok("critic", "s", eng.lat_B)
            assert eng.a1_cached["tr"] == eng.a1_cached["critic"] == ("pk" if reuse else False)
        else:
            assert eng.a1_cached["tr"] == reuse
        out.append({k: eng.get_all_weights(k) for k in ("actor", "critic", "tr")})
    for k in out[0]:
        assert np.isfinite(out[0][k]).all()
        np.testing.assert_array_equal(out[0][k], out[1][k], err_msg=k)


class CountingLib:
    """the library with a launch counter per entry point in front; `tr_ptr`: also counts the calls that were handed the team-reward
    nets' parameter matrix"""

    def __init__(self, lib):
        self._lib, self.calls, self.tr_calls, self.tr_ptrs = lib, collections.Counter(), collections.Counter(), set()

    def __getattr__(self, name):
        fn = getattr(self._lib, name)
        if not callable(fn):
            return fn

        def call(*args):
            self.calls[name] += 1
            if any(isinstance(a, int) and a in self.tr_ptrs for a in args):
                self.tr_calls[name] += 1
            return fn(*args)
        return call


def _one_block(device, lib, critic_hid, tr_hid, n_epochs=2):
    seeds = (41,)
    W, goals = engine_inputs(seeds, critic_hid, 20 if tr_hid is None else tr_hid)
    cl = CountingLib(lib)
    eng = make_engine(device, cl, seeds, W, goals, critic_hid=critic_hid, tr_hid=tr_hid, rng_mode="device", n_epochs=n_epochs)
    cl.tr_ptrs = {eng.theta["tr"].data_ptr(), eng.msg["tr"].data_ptr()}
    eng.train(2)                                                      # one block: 2 episodes of 3 steps
    return eng, cl


def check_routing(device, lib):
    """A 20-unit team-reward net beside any critic takes exactly the launches of an engine built without the tr_hid argument; a wide
    one never reaches the 20-unit kernels and runs the wide consensus head once per epoch per wide net."""
    for critic_hid in (20, 24):
        _, a = _one_block(device, lib, critic_hid, 20)
        _, b = _one_block(device, lib, critic_hid, None)
        assert dict(a.calls) == dict(b.calls), (critic_hid, dict(a.calls), dict(b.calls))
        assert a.calls["rcmarl_wide_td_error"] == 0
    n_epochs = 2
    for critic_hid in (20, 24):
        eng, cl = _one_block(device, lib, critic_hid, 24, n_epochs)
        c, t = cl.calls, cl.tr_calls
        n_wide = 1 + (critic_hid != 20)
        assert c["rcmarl_wide_consensus_head"] == n_epochs * n_wide and t["rcmarl_wide_consensus_head"] == n_epochs, dict(c)
        assert c["rcmarl_wide_head_apply"] == n_epochs * n_wide and t["rcmarl_wide_head_apply"] == n_epochs
        for name in ("rcmarl_mid_value", "rcmarl_consensus_head", "rcmarl_head_apply", "rcmarl_mid_fit", "rcmarl_small_sgd",
                     "rcmarl_layer1_forward", "rcmarl_minibatch_fit"):
            assert t[name] == 0, (name, dict(t))
        assert t["rcmarl_consensus_params"] + t["rcmarl_consensus_params_circulant"] == n_epochs       # K1, g_hid = P - (hid + 1)
        if critic_hid == 20:
            assert c["rcmarl_consensus_head"] == n_epochs and c["rcmarl_td_error"] == 1 and c["rcmarl_wide_td_error"] == 0
        else:
            assert c["rcmarl_consensus_head"] == c["rcmarl_mid_value"] == c["rcmarl_td_error"] == 0 and c["rcmarl_wide_td_error"] == 1
        assert np.isfinite(eng.get_all_weights("tr")).all()


def check_adversary(device, lib, label, seeds=(44,)):
    """4 cooperative agents + 1 Greedy / Malicious one beside a 24-unit team-reward net (20-unit critic), one block against the oracle
    at the bars of the wide critic's adversary checks -- engine_checks.compare's defaults, as in
    test_engine_emu.test_engine_wide_critic_with_greedy_and_malicious_agents_matches_oracle and its GPU twin in test_engine_gpu.py.
    The adversary's team-reward fit takes its mini-batch steps through the dense entry points at the real width."""
    labels = [COOP] * 4 + [label]
    args = EC.make_args(labels, H=1, n_episodes=2, max_ep_len=3, n_ep_fixed=2, n_epochs=1, buffer_size=9, seed=44)
    W, goals = engine_inputs(seeds, 20, 24, n=5, nrow=5)
    o_logs, o_w = EC.run_oracle(args, 5, 5, "device", seeds, W, goals)
    cl = CountingLib(lib)
    cfg = EngineConfig(5, labels, EC.CIRC5, H=1, max_ep_len=3, n_ep_fixed=2, n_epochs=1, buffer_size=9, nrow=5, ncol=5,
                       n_seeds=len(seeds), rng_mode="device", lattice=False, critic_hid=20, tr_hid=24)
    eng = RPBCACEngine(cfg, seeds=list(seeds), device=device, lib=cl)
    for s in range(len(seeds)):
        for i in range(5):
            for net in ("actor", "critic", "tr"):
                eng.set_weights(s, i, net, W[s][i][net])
    eng.set_goals(np.stack(goals))
    cl.tr_ptrs = {eng.theta["tr"].data_ptr()}
    logs = eng.train(2)
    assert eng.wide and not eng.critic_wide and hasattr(eng, "adv") and eng.adv.fit
    assert cl.tr_calls["rcmarl_minibatch_fit"] == 0 and cl.calls["rcmarl_minibatch_fit_multi"] == 0
    EC.compare(eng, logs, o_logs, o_w)


def check_wide_td_error(bk, B, S=2, N=N_, tr_hid=384, c_hid=128):
    """rcmarl_wide_td_error against rcmarl_pk_head x3 + rcmarl_td_error, bit for bit, on rows 0..B: all three values as parts (the
    team-reward net's three parts per row, the critic's one), all three as finished head outputs, and mixed."""
    L, st = bk.lib, bk.stream
    rng = np.random.default_rng(50 + B)
    ldb, Z = pad64(B) + 64, S * N
    geo = {"tr": (3 * N, tr_hid), "c": (2 * N, c_hid)}
    parts = {k: L.rcmarl_pk_parts(h) for k, (_, h) in geo.items()}
    assert parts == {"tr": 3, "c": 1}
    ldp = {k: pad64(net_numel(i, 1, h)) for k, (i, h) in geo.items()}
    theta = {k: rng.normal(size=(S, N, ldp[k])).astype(np.float32) for k in geo}
    vp = {k: rng.normal(size=(Z, parts["tr" if k == "tr" else "c"], ldb)).astype(np.float32) for k in ("tr", "next", "cur")}
    d_th = {k: bk.dev(v) for k, v in theta.items()}
    d_vp = {k: bk.dev(v) for k, v in vp.items()}
    z = lambda: bk.dev(np.zeros((S, N, ldb), np.float32))
    d_v = {k: z() for k in vp}
    gamma = 0.9
    for k, net in (("tr", "tr"), ("next", "c"), ("cur", "c")):
        L.rcmarl_pk_head(bk.ptr(d_vp[k]), bk.ptr(d_th[net]), None, 0.0, 0, bk.ptr(d_v[k]), None, None, S, N, B, geo[net][0], geo[net][1],
                         ldp[net], ldb, st)
    d_want = z()
    L.rcmarl_td_error(bk.ptr(d_v["tr"]), bk.ptr(d_v["next"]), bk.ptr(d_v["cur"]), gamma, bk.ptr(d_want), S * N * ldb, st)
    want = np.array(bk.host(d_want))[:, :, :B]
    v = {k: np.array(bk.host(d_v[k]))[:, :, :B].astype(np.float64) for k in d_v}
    assert np.abs(want - (v["tr"] + gamma * v["next"] - v["cur"])).max() < 1e-5 and np.abs(want).max() > 0.5
    for mode in ("parts", "outputs", "mixed"):
        src = {k: (d_vp[k], parts["tr" if k == "tr" else "c"]) if mode == "parts" or (mode == "mixed" and k != "next") else (d_v[k], 0)
               for k in vp}
        d_got = bk.dev(np.full((S, N, ldb), -7.0, np.float32))
        L.rcmarl_wide_td_error(bk.ptr(src["tr"][0]), src["tr"][1], bk.ptr(d_th["tr"]), geo["tr"][0], geo["tr"][1], ldp["tr"],
                               bk.ptr(src["next"][0]), src["next"][1], bk.ptr(src["cur"][0]), src["cur"][1], bk.ptr(d_th["c"]),
                               geo["c"][0], geo["c"][1], ldp["c"], gamma, bk.ptr(d_got), S, N, B, ldb, st)
        got = np.array(bk.host(d_got))
        np.testing.assert_array_equal(got[:, :, :B], want, err_msg=mode)
        assert (got[:, :, B:] == -7.0).all(), mode                    # nothing written beyond row B


def check_wide_td_error_arguments(lib):
    p = 64                                                            # stands for "not NULL": refused before any pointer is looked at
    ok = [p, 3, p, 9, 384, pad64(net_numel(9, 1, 384)), p, 1, p, 1, p, 6, 128, pad64(net_numel(6, 1, 128)), 0.9, p, 2, 3, 7, 64, None]
    bad = []
    for pos, val in ((0, None), (6, None), (8, None), (15, None), (1, -1), (7, -1), (9, -1), (16, 0), (17, 0), (18, 0), (19, 6),
                     (2, None), (10, None), (5, 100), (13, 100), (4, 0), (12, 0)):
        a = list(ok)
        a[pos] = val
        bad.append(a)
    for a in bad:
        with pytest.raises(capi.RcmarlError, match="RCMARL_ERR_ARG"):
            lib.rcmarl_wide_td_error(*a)


def check_dropin(hook, seed=5):
    """keras_compat models with a 24-unit team-reward net through train_RPBCAC, which reads the width off the model objects: the
    returned weights' shape, that training changed them, parity with oracle.train on the same NumPy stream (returns bit-identical,
    critic / team-reward net to 1e-4 as in wide_actor_checks.check_dropin, the actor within 5 % of an Adam step per update); mixed
    team-reward widths are refused."""
    import dropin_checks as DC
    from rcmarl_amd import keras_compat as K
    from rcmarl_amd.agents.resilient_CAC_agents import RPBCAC_agent
    from rcmarl_amd.environments.grid_world import Grid_World
    from rcmarl_amd.training.train_agents import train_RPBCAC
    n = N_

    def mlp(width, hid, out, act):
        return K.Sequential([K.Input(shape=(n, width)), K.layers.Flatten(), K.layers.Dense(hid, activation=K.layers.LeakyReLU(alpha=0.1)),
                             K.layers.Dense(hid, activation=K.layers.LeakyReLU(alpha=0.1)), K.layers.Dense(out, activation=act)])

    def team(tr_hids):
        K.set_seed(seed)
        agents, W = [], []
        for h in tr_hids:
            actor, critic, tr = mlp(2, 20, 5, 'softmax'), mlp(2, 20, 1, None), mlp(3, h, 1, None)
            W.append([actor.get_weights(), critic.get_weights(), tr.get_weights()])
            agents.append(RPBCAC_agent(actor, critic, tr, slow_lr=0.002, fast_lr=0.01, gamma=0.9, H=1))
        return agents, W
    agents, W = team([24] * n)
    assert W[0][2][0].shape == (9, 24)
    args = engine_args(n_episodes=4, seed=seed)
    goals = np.random.default_rng(seed).integers(0, 3, size=(n, 2))
    np.random.seed(seed)
    env = Grid_World(nrow=3, ncol=3, n_agents=n, desired_state=goals, initial_state=goals, randomize_state=True, scaling=True)
    weights, df = train_RPBCAC(env, agents, args, engine_hook=hook)
    o_agents = [O.make_agent(COOP, [a.copy() for a in W[i][0]], [a.copy() for a in W[i][1]], [a.copy() for a in W[i][2]], 0.002, 0.01, 0.9, 1)
                for i in range(n)]
    np.random.seed(seed)
    ow, odf = O.train(O.GridWorldOracle(3, 3, n, goals, None, True, True), o_agents, args, rng_mode="numpy")
    np.testing.assert_array_equal(df["True_team_returns"].to_numpy(), odf["True_team_returns"].to_numpy(dtype=np.float64))
    for i in range(n):
        assert [a.shape for a in weights[i][2]] == [(9, 24), (24,), (24, 24), (24,), (24, 1), (1,)]
        assert any(np.abs(a - b).max() > 0 for a, b in zip(weights[i][2], W[i][2]))        # the team-reward net was trained
        for a, b in zip(weights[i][0], ow[i][0]):
            assert float(np.abs(a - b).max()) <= 0.05 * 0.002 * 2 + 1e-5, ("actor", i, float(np.abs(a - b).max()))
        for k in (1, 2):
            for a, b in zip(weights[i][k], ow[i][k]):
                DC.close(a, b, 1e-4, "wide team-reward net drop-in agent %d net %d" % (i, k))
    mixed, _ = team([24, 20, 24])
    with pytest.raises(ValueError, match="all team-reward nets must have the same width"):
        train_RPBCAC(env, mixed, args, engine_hook=hook)


def check_checkpoints(device, lib, path):
    """round trip (save after one block, a fresh engine resumes: the bits of the straight run), and a 20-unit file refused by a 24-unit
    engine and the reverse, in the existing message's form; a file without tr_hid is a 20-unit file"""
    import torch
    seeds = (31,)
    W, goals = engine_inputs(seeds, 20, 24)
    W20, _ = engine_inputs(seeds, 20, 20)
    mk = lambda: make_engine(device, lib, seeds, W, goals, tr_hid=24, rng_mode="device", n_epochs=1)
    a = mk()
    la = a.train(4)
    b = mk()
    lb = b.train(2)
    b.save_checkpoint(path)
    assert torch.load(path, map_location="cpu", weights_only=True)["shape"]["tr_hid"] == 24
    c = mk()
    c.init_glorot(base_seed=99)                                       # everything must come from the file
    c.load_checkpoint(path)
    lc = c.train(2)
    for k in la:
        np.testing.assert_array_equal(la[k], np.concatenate([lb[k], lc[k]], axis=0))
    for net in a.theta:
        np.testing.assert_array_equal(a.get_all_weights(net), c.get_all_weights(net))
    narrow = make_engine(device, lib, seeds, W20, goals, tr_hid=20, rng_mode="device", n_epochs=1)
    with pytest.raises(ValueError, match=r"checkpoint does not match this engine: \{'tr_hid': \(24, 20\)\}"):
        narrow.load_checkpoint(path)
    narrow.train(2)
    narrow.save_checkpoint(path + ".20")
    with pytest.raises(ValueError, match=r"checkpoint does not match this engine: \{'tr_hid': \(20, 24\)\}"):
        mk().load_checkpoint(path + ".20")
    sd = narrow.state_dict()
    del sd["shape"]["tr_hid"]
    torch.save(sd, path + ".old")
    again = make_engine(device, lib, seeds, W20, goals, tr_hid=20, rng_mode="device", n_epochs=1)
    again.load_checkpoint(path + ".old")
    np.testing.assert_array_equal(again.get_all_weights("tr"), narrow.get_all_weights("tr"))
    with pytest.raises(ValueError, match="tr_hid"):
        mk().load_checkpoint(path + ".old")


def check_validation(device, lib):
    with pytest.raises(ValueError, match="tr_hid must be positive"):
        make_cfg(tr_hid=0)
    with pytest.raises(ValueError, match="irregular"):
        make_cfg(tr_hid=24, in_nodes=[[0, 1, 2], [1, 2, 0], [2, 0]], H=0)
    with pytest.raises(ValueError, match="irregular"):
        make_cfg(tr_hid=24, H=[1, 1, 0])
    make_cfg(tr_hid=20, H=[1, 1, 0])                                  # the 20-unit team-reward net keeps the irregular graphs
    make_cfg(tr_hid=24, labels=[COOP, COOP, "Greedy"])                # ... and a wide one keeps the adversaries
    assert make_cfg(tr_hid=None).tr_hid == 20
    eng = RPBCACEngine(make_cfg(n_seeds=1, critic_hid=32, tr_hid=24), seeds=[1], device=device, lib=lib)
    with pytest.raises(ValueError, match="team-reward net"):
        eng.shard_agents(rank=0, world=2)
