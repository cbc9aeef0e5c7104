"""Engine-vs-oracle end-to-end checks shared by the hipemu (CPU) and GPU tests."""
import numpy as np

from oracle import mlp_np as M
from oracle import rpbcac_oracle as O
from rcmarl_amd.engine import EngineConfig, RPBCACEngine

CIRC5 = [[0, 1, 2, 3], [1, 2, 3, 4], [2, 3, 4, 0], [3, 4, 0, 1], [4, 0, 1, 2]]


def make_args(labels, H, n_episodes, max_ep_len, n_ep_fixed, n_epochs, buffer_size, seed, in_nodes=None,
              common_reward=False, slow_lr=0.002, fast_lr=0.01, gamma=0.9):
    n = len(labels)
    return {"n_agents": n, "agent_label": list(labels), "in_nodes": in_nodes or CIRC5, "n_actions": 5, "n_states": 2,
            "n_episodes": n_episodes, "max_ep_len": max_ep_len, "n_ep_fixed": n_ep_fixed, "n_epochs": n_epochs,
            "slow_lr": slow_lr, "fast_lr": fast_lr, "batch_size": 200, "buffer_size": buffer_size, "gamma": gamma, "H": H,
            "common_reward": common_reward, "summary_dir": "./", "pretrained_agents": False, "random_seed": seed}


def init_weights(rng, n_agents, critic_hid=20):
    out = []
    for _ in range(n_agents):
        out.append({"actor": M.init_mlp(rng, 2 * n_agents, 20, 5), "critic": M.init_mlp(rng, 2 * n_agents, critic_hid, 1),
                    "tr": M.init_mlp(rng, 3 * n_agents, 20, 1)})
    return out


def make_inputs(args, nrow, seeds, weight_seed=3, critic_hid=20):
    """Initial weights and goals of every seed (shared by the oracle run and the engine run)."""
    n = args["n_agents"]
    wrng = np.random.default_rng(weight_seed)
    W = [init_weights(wrng, n, critic_hid) for _ in seeds]
    goals = [np.random.default_rng(100 + s).integers(0, min(5, nrow), size=(n, 2)) for s in range(len(seeds))]
    return W, goals


# The packed-operand path of a wide critic (csrc/dense_pk.hip) carries 2^10 W2 as two f16 pieces and raises its flag when that leaves
# 65000 (csrc/dense_pk.hip, k_pk_pack_w2: `!(amax * RC_F16_W_SCALE <= 65000.f)`), i.e. at |W2| > 63.48.  70 is 1.10 of that bound.
PK_PLANT_W2 = 70.0


def plant_out_of_range_w2(critic, value=PK_PLANT_W2):
    """ONE entry W2[k][j] = value in a critic [W1, b1, W2, b2, W3, b3] (in place): enough to raise the range flag of the packed-operand
    path, and the gentlest such trigger -- k is the hidden unit with the smallest sum_c |W1[c][k]| + |b1[k]| (its layer-1 activation
    is small on every input), j the layer-2 unit with the smallest |W3[j]| (the value moves least), so a1, W2 W3 and dz1 stay in range
    and the float32 oracle is nowhere near diverging.  Under H >= 1 the entry is the one outlier of its column among the neighbours'
    messages, so the first hidden-layer consensus trims it away: the flag rises in the first block and the critics are ordinary
    afterwards.  Returns (k, j)."""
    k = int(np.argmin(np.abs(critic[0]).sum(axis=0) + np.abs(critic[1])))
    j = int(np.argmin(np.abs(critic[4][:, 0])))
    critic[2][k, j] = np.float32(value)
    return k, j


def _oracle_seed_job(payload):
    """one seed of run_oracle in a worker process (spawned: nothing of the parent's GPU state travels)"""
    import os
    import sys
    root, args, nrow, ncol, rng_mode, seed, W_s, goals_s, threads = payload
    for p in (root, os.path.join(root, "tests")):
        if p not in sys.path:
            sys.path.insert(0, p)
    try:
        import threadpoolctl
        threadpoolctl.threadpool_limits(threads)
    except Exception:
        pass
    logs, weights = run_oracle(args, nrow, ncol, rng_mode, (seed,), [W_s], [goals_s])
    return logs[0], weights[0]


def run_oracle_parallel(args, nrow, ncol, rng_mode, seeds, W, goals):
    """run_oracle with one worker process per seed (the seeds are independent runs; the GPU boxes have hundreds of host cores and
    the oracle's Python loops are serial).  Same results as run_oracle, in a fraction of the wall time."""
    import concurrent.futures as cf
    import multiprocessing as mp
    import os
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    ncpu = os.cpu_count() or 1
    workers = max(1, min(len(seeds), ncpu))
    threads = max(1, min(16, ncpu // workers))
    jobs = [(root, args, nrow, ncol, rng_mode, int(seeds[s]), W[s], goals[s], threads) for s in range(len(seeds))]
    if workers == 1:
        res = [_oracle_seed_job(j) for j in jobs]
    else:
        with cf.ProcessPoolExecutor(max_workers=workers, mp_context=mp.get_context("spawn")) as ex:
            res = list(ex.map(_oracle_seed_job, jobs))
    return [r[0] for r in res], [r[1] for r in res]


def snapshot_for_oracle(eng, seed_idx):
    """Everything oracle.update_block needs to repeat the engine's NEXT update block of one seed from identical state: every
    network of every agent, the actors' Adam slots and step count, the replay rows (fp32, as the reference casts them at
    training/train_agents.py:89-92)."""
    from rcmarl_amd.engine import unflatten_params
    N, B = eng.N, eng.B
    W = [{net: [a.copy() for a in eng.get_weights(seed_idx, i, net)] for net in ("actor", "critic", "tr")} for i in range(N)]
    adam = []
    for i in range(N):
        m, v, t = eng.dump_adam(seed_idx, i)
        adam.append((unflatten_params(m, eng.in_dim["actor"], eng.out_dim["actor"]), unflatten_params(v, eng.in_dim["actor"], eng.out_dim["actor"]), t))
    g = lambda k: eng.rp[k][seed_idx, :B].detach().cpu().numpy().copy()
    return {"W": W, "adam": adam, "s": g("s").reshape(B, N, 2), "ns": g("ns").reshape(B, N, 2), "r": g("r").reshape(B, N, 1),
            "a": g("a").reshape(B, N, 1)}


# ---- the oracle's update block with its per-agent loops spread over worker processes ----------------------------------------
# oracle.update_block (training/train_agents.py:100-153) walks the agents one after the other; for an all-cooperative team every step
# of an epoch is independent per agent given the previous step's results (phase I: the local fits; phase II: consensus + projection
# from the gathered messages; phase III: the actor step).  At 256 agents x 3000 rows one block takes ~4.5 minutes in one process --
# the GPU boxes have hundreds of cores -- so the SAME agent methods are called per agent in a process pool, epoch by epoch, and the
# results are those of the serial loop (checked bit for bit in tests/test_engine_emu.py).  Test infrastructure only.
_POOL_STATE = {}


def _set_oracle_mode(mode, seed):
    from oracle import mlp_np as M_
    from oracle import rpbcac_oracle as O_
    if not hasattr(M_, "_pristine_fit_mse"):
        M_._pristine_fit_mse = M_.fit_mse
    M_.fit_mse = M_._pristine_fit_mse
    M_.F32 = O_.F32 = np.float32
    M_.LEAK = np.float32(0.1)
    if mode == "f64":
        # the ARBITER: the same loop nest in float64.  Every array and every scalar the restatement forms through its F32 alias
        # becomes a double; the inputs are the fp32 snapshot widened.  (Constants such as lr and the LeakyReLU slope are then the
        # doubles 0.001 / 0.1 rather than their fp32 roundings: a relative 5e-8 on the update.)
        M_.F32 = O_.F32 = np.float64
        M_.LEAK = np.float64(0.1)
    elif mode == "f32_shuffled":
        # the CONTROL: fp32, the rows of every full-batch local fit in another order per epoch -- what Keras' fit(shuffle=True)
        # does to the single batch: the same sums, taken in another order
        orig, rng = M_._pristine_fit_mse, np.random.default_rng(seed)

        def fit_shuffled(params, x, y, lr, epochs, batch_size=None, perms=None, sample_weight=None):
            if batch_size is None and perms is None:
                B = np.asarray(x).shape[0]
                perms = np.stack([rng.permutation(B) for _ in range(epochs)])
            return orig(params, x, y, lr, epochs, batch_size=batch_size, perms=perms, sample_weight=sample_weight)
        M_.fit_mse = fit_shuffled
    return M_, O_


def _pool_init(root, data_dir, n_snaps, threads):
    import os
    import sys
    for p in (root, os.path.join(root, "tests")):
        if p not in sys.path:
            sys.path.insert(0, p)
    try:
        import threadpoolctl
        _POOL_STATE["tp"] = threadpoolctl.threadpool_limits(threads)
    except Exception:
        pass
    # per snapshot: s, ns, sa, r, a, r_coop (fp32), memory-mapped from files the parent wrote (one copy in the page cache for all workers)
    _POOL_STATE["data"] = [{key: np.load(os.path.join(data_dir, "%d_%s.npy" % (k, key)), mmap_mode="r")
                            for key in ("s", "ns", "sa", "r", "a", "r_coop")} for k in range(n_snaps)]


def _pool_task(task):
    kind, k, mode, i, agent, extra = task
    M_, O_ = _set_oracle_mode(mode, 12345 + 7919 * k + i)
    d = _POOL_STATE["data"][k]
    if kind == "fit":                        # phase I  (train_agents.py:105-121, cooperative branch)
        r_applied = d["r_coop"] if extra else d["r"][:, i]
        x, tl = agent.local_fit_tr(d["sa"], r_applied)
        y, cl = agent.local_fit_critic(d["s"], d["ns"], r_applied)
        return x, y, tl, cl
    if kind == "cons":                       # phase II (:125-145)
        c_in, t_in = extra
        agent.consensus_hidden_critic(c_in)
        agent.consensus_hidden_tr(t_in)
        c_agg = agent.consensus_estimates_critic(d["s"], c_in)
        t_agg = agent.consensus_estimates_tr(d["sa"], t_in)
        agent.projection_step_critic(d["s"], c_agg)
        agent.projection_step_tr(d["sa"], t_agg)
        return agent
    n_last = extra                           # phase III (:149-153)
    agent.actor_step(d["s"][-n_last:], d["ns"][-n_last:], d["sa"][-n_last:], d["a"][-n_last:, i])
    return agent


def _make_agents(args, snap, mode):
    M_, O_ = _set_oracle_mode(mode, 0)
    agents = []
    for i, lab in enumerate(args["agent_label"]):
        w = snap["W"][i]
        ag = O_.make_agent(lab, w["actor"], w["critic"], w["tr"], args["slow_lr"], args["fast_lr"], args["gamma"], args["H"])
        m, v, t = snap["adam"][i]
        ag.adam.m, ag.adam.v, ag.adam.t = [x.astype(M_.F32).copy() for x in m], [x.astype(M_.F32).copy() for x in v], int(t)
        agents.append(ag)
    return agents


def _oracle_block_job(payload):
    """oracle.update_block (training/train_agents.py:100-153) on one snapshot, in a worker process: the serial form"""
    import os
    import sys
    root, args, snap, threads = payload[:4]
    mode = payload[4] if len(payload) > 4 else "f32"
    for p in (root, os.path.join(root, "tests")):
        if p not in sys.path:
            sys.path.insert(0, p)
    try:
        import threadpoolctl
        threadpoolctl.threadpool_limits(threads)
    except Exception:
        pass
    M_, O_ = _set_oracle_mode(mode, 12345 + int(args.get("random_seed", 0)))
    agents = _make_agents(args, snap, mode)
    _set_oracle_mode(mode, 12345 + int(args.get("random_seed", 0)))
    O_.update_block(agents, args["agent_label"], args["in_nodes"], snap["s"], snap["ns"], snap["r"], snap["a"], args["n_epochs"],
                    args["common_reward"], args["max_ep_len"], args["n_ep_fixed"], O_.ShuffleStream(args.get("random_seed", 0)))
    return [ag.parameters() for ag in agents]


def run_oracle_blocks_parallel(args, snaps, modes=None, force_serial=False):
    """one oracle update block per snapshot -> per-snapshot weight lists [agent][actor, critic, tr].
    modes (per snapshot): "f32" (the oracle), "f64" (the same loop nest in float64), "f32_shuffled" (fp32, local-fit rows reordered).
    All-cooperative teams on a host with many cores: the per-agent loops of every epoch run in a process pool (see above);
    otherwise (adversaries draw from a shared shuffle stream in agent order; few cores) one serial oracle.update_block per process."""
    import concurrent.futures as cf
    import multiprocessing as mp
    import os
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    ncpu = os.cpu_count() or 1
    modes = ["f32"] * len(snaps) if modes is None else list(modes)
    labels = args["agent_label"]
    n = len(labels)
    spread = (not force_serial) and all(lab == "Cooperative" for lab in labels) and ncpu >= 8
    if not spread:
        workers = max(1, min(len(snaps), ncpu))
        threads = max(1, min(16, ncpu // workers))
        jobs = [(root, args, sn, threads, modes[k]) for k, sn in enumerate(snaps)]
        if workers == 1:
            return [_oracle_block_job(j) for j in jobs]
        with cf.ProcessPoolExecutor(max_workers=workers, mp_context=mp.get_context("spawn")) as ex:
            return list(ex.map(_oracle_block_job, jobs))
    import shutil
    import tempfile
    data_dir = tempfile.mkdtemp(prefix="rcmarl_oracle_", dir="/dev/shm" if os.path.isdir("/dev/shm") else None)
    for k, sn in enumerate(snaps):
        s, ns, r, a = (np.asarray(sn[key], np.float32) for key in ("s", "ns", "r", "a"))
        r_coop = np.zeros((r.shape[0], r.shape[2]), np.float32)
        for i in range(n):
            r_coop += r[:, i] / n                                          # train_agents.py:96-98 (all agents cooperative)
        for key, arr in (("s", s), ("ns", ns), ("sa", np.concatenate([s, a], axis=-1)), ("r", r), ("a", a), ("r_coop", r_coop)):
            np.save(os.path.join(data_dir, "%d_%s.npy" % (k, key)), np.ascontiguousarray(arr))
    agents = [_make_agents(args, sn, modes[k]) for k, sn in enumerate(snaps)]
    _set_oracle_mode("f32", 0)
    workers = max(1, min(ncpu, 192, len(snaps) * n))
    in_nodes, common, n_last = args["in_nodes"], bool(args["common_reward"]), args["max_ep_len"] * args["n_ep_fixed"]
    chunk = max(1, (len(snaps) * n) // (workers * 4))
    try:
        return _spread_epochs(cf, mp, workers, root, data_dir, snaps, modes, agents, n, args, in_nodes, common, n_last, chunk)
    finally:
        shutil.rmtree(data_dir, ignore_errors=True)


def _spread_epochs(cf, mp, workers, root, data_dir, snaps, modes, agents, n, args, in_nodes, common, n_last, chunk):
    with cf.ProcessPoolExecutor(max_workers=workers, mp_context=mp.get_context("spawn"), initializer=_pool_init,
                                initargs=(root, data_dir, len(snaps), 1)) as ex:
        for _ in range(args["n_epochs"]):
            fits = list(ex.map(_pool_task, [("fit", k, modes[k], i, agents[k][i], common) for k in range(len(snaps)) for i in range(n)],
                               chunksize=chunk))
            tasks = []
            for k in range(len(snaps)):
                tr_msgs = [fits[k * n + i][0] for i in range(n)]
                c_msgs = [fits[k * n + i][1] for i in range(n)]
                for i in range(n):
                    tasks.append(("cons", k, modes[k], i, agents[k][i], ([c_msgs[j] for j in in_nodes[i]], [tr_msgs[j] for j in in_nodes[i]])))
            res = list(ex.map(_pool_task, tasks, chunksize=chunk))
            for k in range(len(snaps)):
                agents[k] = res[k * n:(k + 1) * n]
        res = list(ex.map(_pool_task, [("actor", k, modes[k], i, agents[k][i], n_last) for k in range(len(snaps)) for i in range(n)],
                           chunksize=chunk))
    return [[ag.parameters() for ag in res[k * n:(k + 1) * n]] for k in range(len(snaps))]


def network_errors(eng, o_weights, nets=("critic", "tr")):
    """per-network worst |w - w_oracle| / max(1, |w|max) -> {net: float array over (seed, agent)}"""
    out = {}
    for k, net in ((1, "critic"), (2, "tr")):
        if net not in nets:
            continue
        errs = []
        for s in range(eng.S):
            for i in range(eng.N):
                e = 0.0
                for a, b in zip(eng.get_weights(s, i, net), o_weights[s][i][k]):
                    e = max(e, float(np.abs(a - b).max()) / max(1.0, float(np.abs(b).max())))
                errs.append(e)
        out[net] = np.asarray(errs)
    return out


def run_oracle(args, nrow, ncol, rng_mode, seeds, W, goals, return_agents=False):
    """oracle.train, one run per seed -> (per-seed DataFrames, per-seed weight lists[, per-seed agent objects])."""
    n = args["n_agents"]
    o_logs, o_weights, o_agents = [], [], []
    for s in range(len(seeds)):
        a = dict(args)
        a["random_seed"] = int(seeds[s])
        agents = [O.make_agent(lab, W[s][i]["actor"], W[s][i]["critic"], W[s][i]["tr"], a["slow_lr"], a["fast_lr"], a["gamma"], a["H"])
                  for i, lab in enumerate(a["agent_label"])]
        if rng_mode == "numpy":
            np.random.seed(int(seeds[s]))
            env = O.GridWorldOracle(nrow, ncol, n, goals[s], None, True, True)
            w, df = O.train(env, agents, a, rng_mode="numpy")
        else:
            env = O.GridWorldOracle(nrow, ncol, n, goals[s], None, True, True, rng_mode="device", seed=int(seeds[s]))
            w, df = O.train(env, agents, a, rng_mode="device")
        o_logs.append(df)
        o_weights.append(w)
        o_agents.append(agents)
    return (o_logs, o_weights, o_agents) if return_agents else (o_logs, o_weights)


def run_engine(args, nrow, ncol, rng_mode, device, lib, seeds, W, goals, lattice="auto", critic_hid=20, tweak=None):
    """The batched engine on all seeds from the same weights/goals.  tweak(eng): instance-level switches
    (e.g. eng.td_shortcut = False) applied before training."""
    n, S = args["n_agents"], len(seeds)
    cfg = EngineConfig(n, args["agent_label"], args["in_nodes"], H=args["H"], gamma=args["gamma"], slow_lr=args["slow_lr"],
                       fast_lr=args["fast_lr"], max_ep_len=args["max_ep_len"], n_ep_fixed=args["n_ep_fixed"],
                       n_epochs=args["n_epochs"], buffer_size=args["buffer_size"], common_reward=args["common_reward"],
                       nrow=nrow, ncol=ncol, n_seeds=S, rng_mode=rng_mode, lattice=lattice, critic_hid=critic_hid)
    eng = RPBCACEngine(cfg, seeds=list(seeds), device=device, lib=lib)
    for s in range(S):
        for i in range(n):
            for net in ("actor", "critic", "tr"):
                eng.set_weights(s, i, net, W[s][i][net])
    eng.set_goals(np.stack(goals))
    if tweak is not None:
        tweak(eng)
    if rng_mode == "numpy":
        eng.np_rngs = []
        for s in range(S):
            r = np.random.RandomState(int(seeds[s]))
            r.randint([0, 0], [nrow, ncol], size=(n, 2))       # the env constructor's reset() draw (grid_world.py:28)
            eng.np_rngs.append(r)
    logs = eng.train(args["n_episodes"])
    return eng, logs


def run_pair(args, nrow, ncol, rng_mode, device, lib, seeds=(11,), weight_seed=3, lattice="auto", critic_hid=20):
    """Run the oracle (one run per seed) and the engine (all seeds batched); return both results."""
    W, goals = make_inputs(args, nrow, seeds, weight_seed, critic_hid)
    o_logs, o_weights = run_oracle(args, nrow, ncol, rng_mode, seeds, W, goals)
    eng, logs = run_engine(args, nrow, ncol, rng_mode, device, lib, seeds, W, goals, lattice, critic_hid)
    return eng, logs, o_logs, o_weights


def compare(eng, logs, o_logs, o_weights, rtol_w=1e-4, actor="strict", outlier_frac=0.0, rtol_w_outlier=None, actor_outlier_frac=1e-4):
    """rtol_w: end-of-run critic / team-reward weights vs the oracle, |err| <= rtol_w * max(1, |w|max) per array -- SURVEY.md 8c's
    1e-4 (measured worst cases on the MI355X, profiles/r03f_parity_worst_cases.txt: <= 2.9e-5 everywhere except the 256-agent
    BASELINE configs[3] run, 9.3e-5, which therefore passes 2e-4 explicitly).  Prints the measured worst case.
    outlier_frac / rtol_w_outlier (hundreds of agents, wide inputs): that fraction of the (seed, agent, net) networks may miss rtol_w,
    none may miss rtol_w_outlier -- for runs where the distribution over networks was MEASURED and is the same in the exact operand
    form, i.e. a property of fp32 summation order on an ill-conditioned fit, not of this engine's arithmetic (the caller cites the file).
    actor="none": the caller judges the actor itself.  actor="strict": every actor parameter within 5 % of an Adam step per update.  actor="stat" (hundreds of agents):
    Adam turns a gradient of magnitude ~eps into anything in [-lr, lr] and a pre-activation within rounding of 0 flips its
    LeakyReLU slope, so among millions of parameters a few legitimately differ by more between any two fp32 summation
    orders: bulk within 5 % of a step, at most actor_outlier_frac (1e-4) of the entries beyond, none beyond two full steps (the bar
    of kernel_checks.check_actor_step)."""
    S, n = eng.S, eng.N
    steps = max(1, eng.adam_t)
    worst = {"critic": 0.0, "tr": 0.0, "critic_local": 0.0}        # measured max |err| / max(1, |w|max) per family
    n_nets, outliers = 0, []
    for s in range(S):
        df = o_logs[s]
        # identical action streams -> bit-identical float64 returns
        np.testing.assert_array_equal(logs["True_team_returns"][:, s], df["True_team_returns"].to_numpy(dtype=np.float64))
        np.testing.assert_array_equal(logs["True_adv_returns"][:, s], df["True_adv_returns"].to_numpy(dtype=np.float64))
        np.testing.assert_allclose(logs["Estimated_team_returns"][:, s], df["Estimated_team_returns"].to_numpy(dtype=np.float64),
                                   rtol=1e-4, atol=1e-5)
        actor_err = []
        for i in range(n):
            for k, net in enumerate(("actor", "critic", "tr")):
                got = eng.get_weights(s, i, net)
                for a, b in zip(got, o_weights[s][i][k]):
                    scale = max(1.0, float(np.abs(b).max()))
                    err = float(np.abs(a - b).max())
                    if net == "actor" and actor == "none":
                        continue
                    if net == "actor" and actor == "stat":
                        actor_err.append(np.abs(a - b).ravel())
                        continue
                    tol = rtol_w * scale if net != "actor" else 0.05 * eng.cfg.slow_lr * steps + 1e-5
                    if net != "actor":
                        worst[net] = max(worst[net], err / scale)
                        if err > tol and rtol_w_outlier is not None and err <= rtol_w_outlier * scale:
                            outliers.append((s, i, net, err / scale))
                            continue
                    assert err <= tol, (s, i, net, err, tol)
                n_nets += net != "actor"
            if len(o_weights[s][i]) == 4:                       # Malicious: private critic (adversarial:180-182)
                got = eng.get_weights(s, i, "critic_local")
                for a, b in zip(got, o_weights[s][i][3]):
                    scale = max(1.0, float(np.abs(b).max()))
                    worst["critic_local"] = max(worst["critic_local"], float(np.abs(a - b).max()) / scale)
                    assert float(np.abs(a - b).max()) <= rtol_w * scale, (s, i, "critic_local")
        if actor_err:
            e = np.concatenate(actor_err)
            lr = eng.cfg.slow_lr
            assert e.max() <= 2.0 * lr * steps + 1e-6, ("actor", float(e.max()))
            frac = float(np.mean(e > 0.05 * lr * steps + 1e-5))
            assert frac <= actor_outlier_frac, ("actor outliers", frac, float(e.max()))
            print("[parity] actor (statistical bar): %.2e of the parameters beyond 5 %% of an Adam step (bar %.0e), max |err| %.2e = %.2f steps"
                  % (frac, actor_outlier_frac, float(e.max()), float(e.max()) / max(lr * steps, 1e-30)))
    n_out = len({(s_, i_, net_) for s_, i_, net_, _ in outliers})
    assert n_out <= outlier_frac * n_nets, ("networks beyond rtol_w", n_out, n_nets, outliers[:5])
    print("[parity] N=%d S=%d worst |w - w_oracle| / max(1,|w|max): critic %.2e  tr %.2e%s  (bar %.0e%s)"
          % (n, S, worst["critic"], worst["tr"], "  critic_local %.2e" % worst["critic_local"] if worst["critic_local"] else "", rtol_w,
             "; %d of %d networks between that and %.0e" % (n_out, n_nets, rtol_w_outlier) if rtol_w_outlier else ""))
    return worst


def check_checkpoint_resume(labels, rng_mode, device, lib, path, n=5, nrow=5, max_ep_len=3, n_ep_fixed=2, n_epochs=1, buffer_size=9,
                            S=2, blocks=(1, 2), lattice=True, d=4):
    """Train blocks[0]+blocks[1] blocks straight vs blocks[0] -> save -> FRESH engine -> load -> blocks[1]: same logs, same
    bits (weights, Adam slots and step counts, replay rows, agent positions, RNG position all travel in the file)."""
    in_nodes = [[(i + k) % n for k in range(d)] for i in range(n)]

    def make():
        cfg = EngineConfig(n, labels, in_nodes, H=1, max_ep_len=max_ep_len, n_ep_fixed=n_ep_fixed, n_epochs=n_epochs,
                           buffer_size=buffer_size, nrow=nrow, ncol=nrow, n_seeds=S, rng_mode=rng_mode, lattice=lattice)
        eng = RPBCACEngine(cfg, seeds=[7 + s for s in range(S)], device=device, lib=lib)
        eng.init_glorot(base_seed=3)
        eng.set_goals(np.random.default_rng(9).integers(0, min(5, nrow), size=(n, 2)))
        if rng_mode == "numpy":
            eng.np_rngs = [np.random.RandomState(70 + s) for s in range(S)]
        return eng
    e1, e2 = blocks[0] * n_ep_fixed, blocks[1] * n_ep_fixed
    a = make()
    la = a.train(e1 + e2)
    b = make()
    lb1 = b.train(e1)
    b.save_checkpoint(path)
    c = make()
    c.init_glorot(base_seed=99)                       # different weights: everything must come from the file
    c.load_checkpoint(path)
    lc = c.train(e2)
    for k in la:
        np.testing.assert_array_equal(la[k], np.concatenate([lb1[k], lc[k]], axis=0))
    for net in a.theta:
        np.testing.assert_array_equal(a.get_all_weights(net), c.get_all_weights(net))
    np.testing.assert_array_equal(a.adam_m.cpu().numpy(), c.adam_m.cpu().numpy())
    np.testing.assert_array_equal(a.adam_v.cpu().numpy(), c.adam_v.cpu().numpy())
    for k in a.rp:
        np.testing.assert_array_equal(a.rp[k][:, :a.B].cpu().numpy(), c.rp[k][:, :c.B].cpu().numpy())
    # a checkpoint of a different scenario is refused, not silently loaded
    other = EngineConfig(n, labels, in_nodes, H=0, max_ep_len=max_ep_len, n_ep_fixed=n_ep_fixed, n_epochs=n_epochs,
                         buffer_size=buffer_size, nrow=nrow, ncol=nrow, n_seeds=S, rng_mode=rng_mode, lattice=lattice)
    wrong = RPBCACEngine(other, seeds=[7 + s for s in range(S)], device=device, lib=lib)
    try:
        wrong.load_checkpoint(path)
    except ValueError:
        pass
    else:
        raise AssertionError("a checkpoint written with H=1 loaded into an H=0 engine")


def check_probed_rows_vs_oracle(n, d, H, hid, nrow, device, lib, probe, fast_lr, n_ep_fixed=5, max_ep_len=20, rtol=1e-4):
    """ONE update epoch of a whole (wide-critic) instance on the engine; for the agents in `probe` the same epoch by the
    oracle's per-agent methods (agents/resilient_CAC_agents.py:103-206): the local fits of the agent's in-neighbourhood on
    the engine's own replay rows, hidden-layer consensus, estimate consensus, projection step.  The rows of an agent depend on
    its neighbourhood only, so a 1024-agent instance needs d local fits per probed agent, not 1024.  Returns the worst
    |w - w_oracle| / max(1, |w|max)."""
    from rcmarl_amd.engine import flatten_params  # noqa: F401  (kept importable from here for the callers)
    gamma = 0.9
    in_nodes = [[(i + k) % n for k in range(d)] for i in range(n)]
    cfg = EngineConfig(n, ["Cooperative"] * n, in_nodes, H=H, gamma=gamma, slow_lr=0.002, fast_lr=fast_lr, max_ep_len=max_ep_len,
                       n_ep_fixed=n_ep_fixed, n_epochs=1, buffer_size=n_ep_fixed * max_ep_len, nrow=nrow, ncol=nrow, n_seeds=1,
                       rng_mode="device", critic_hid=hid)
    eng = RPBCACEngine(cfg, seeds=[5], device=device, lib=lib)
    eng.init_glorot(base_seed=11)
    eng.set_goals(np.random.default_rng(2).integers(0, min(5, nrow), size=(1, n, 2)))
    assert eng.wide == (hid != 20)
    need = sorted({j for i in probe for j in in_nodes[i]})
    W0 = {j: {net: eng.get_weights(0, j, net) for net in ("critic", "tr")} for j in need}
    eng.rollout_block(cfg.n_ep_fixed)
    B = eng.B
    assert B == n_ep_fixed * max_ep_len
    rows = {k: eng.rp[k][0, :B].cpu().numpy() for k in ("s", "ns", "sa", "r")}
    s, ns, sa = rows["s"].reshape(B, n, 2), rows["ns"].reshape(B, n, 2), rows["sa"].reshape(B, n, 3)
    eng.update_block()
    eng.sync()
    assert all(bool(np.isfinite(v.cpu().numpy()).all()) for k, v in eng.theta.items() if k != "actor" or True)
    dummy_actor = M.init_mlp(np.random.default_rng(0), 2 * n, 20, 5)
    agents = {j: O.CoopAgent(dummy_actor, [a.copy() for a in W0[j]["critic"]], [a.copy() for a in W0[j]["tr"]], 0.002, fast_lr,
                             gamma, H) for j in need}
    msg_c, msg_t = {}, {}
    for j in need:
        msg_c[j], _ = agents[j].local_fit_critic(s, ns, rows["r"][:, j])
        msg_t[j], _ = agents[j].local_fit_tr(sa, rows["r"][:, j])
    worst = 0.0
    for i in probe:
        ag = agents[i]
        c_in, t_in = [msg_c[j] for j in in_nodes[i]], [msg_t[j] for j in in_nodes[i]]
        ag.consensus_hidden_critic(c_in)
        ag.consensus_hidden_tr(t_in)
        c_agg = ag.consensus_estimates_critic(s, c_in)
        t_agg = ag.consensus_estimates_tr(sa, t_in)
        ag.projection_step_critic(s, c_agg)
        ag.projection_step_tr(sa, t_agg)
        for net, want in (("critic", ag.critic), ("tr", ag.tr)):
            got = eng.get_weights(0, i, net)
            for a, b in zip(got, want):
                err = float(np.abs(a - b).max()) / max(1.0, float(np.abs(b).max()))
                worst = max(worst, err)
                assert err <= rtol, (i, net, a.shape, err)
    return worst


def check_actor_gradient(n, d, H, nrow, device, lib, fast_lr, n_ep_fixed=10, max_ep_len=20, rtol=2e-3):
    """One block, one epoch END TO END: after ONE Adam step m = (1 - beta1) g, so the engine's first-moment slots against the
    oracle's hold the actor GRADIENT (agents/resilient_CAC_agents.py:86-101) -- a deterministic bar where the parameters
    themselves only admit a statistical one (Adam turns a gradient of magnitude eps into +-lr).  The gradient is
    sum_b delta_b grad log pi with TD errors delta_b of both signs: the 1e-5-relative differences the TD errors inherit from
    ten fits and consensus steps are amplified by that cancellation (measured worst case at 256 agents: 8.3e-4 of the
    largest entry), hence `rtol` 2e-3 here; with IDENTICAL inputs the kernels hold 1e-4 (kernel_checks.check_actor_step, run
    at 256 agents by tests/test_kernels_gpu.py).  Returns the worst max|dm| / max|m|."""
    from rcmarl_amd.engine import flatten_params
    in_nodes = [[(i + k) % n for k in range(d)] for i in range(n)]
    args = make_args(["Cooperative"] * n, H=H, n_episodes=n_ep_fixed, max_ep_len=max_ep_len, n_ep_fixed=n_ep_fixed, n_epochs=1,
                     buffer_size=2 * n_ep_fixed * max_ep_len, seed=1000, in_nodes=in_nodes, fast_lr=fast_lr)
    seeds = (1000,)
    W, goals = make_inputs(args, nrow, seeds)
    o_logs, o_w, o_agents = run_oracle(args, nrow, nrow, "device", seeds, W, goals, return_agents=True)
    eng, logs = run_engine(args, nrow, nrow, "device", device, lib, seeds, W, goals)
    assert eng.adam_t == 1 and all(a.adam.t == 1 for a in o_agents[0])
    P = eng.P["actor"]
    got = eng.adam_m[0, :, :P].cpu().numpy()
    errs = []
    for i in range(n):
        want = flatten_params(o_agents[0][i].adam.m)
        scale = float(np.abs(want).max())
        assert scale > 0
        errs.append(float(np.abs(got[i] - want).max()) / scale)
    e = np.asarray(errs)
    # (a LeakyReLU pre-activation within rounding of 0 moves one gradient column by ~1 %: at most 2 % of the agents beyond rtol)
    assert float(np.mean(e > rtol)) <= 0.02 and float(e.max()) <= 5e-2, (float(e.max()), float(np.mean(e > rtol)))
    print("[parity] actor gradient end to end, %d agents: max|dm| / max|m| median %.2e, worst %.2e, beyond %.0e: %d"
          % (n, float(np.median(e)), float(e.max()), rtol, int(np.sum(e > rtol))))
    # (weights: this short 256-agent run leaves the team-reward net at 2.2e-4 of the oracle's -- 768 unscaled inputs at the
    # edge of the plain-SGD stability range amplify summation-order differences; the bars of this check are the gradient's)
    # the actor PARAMETERS after this single Adam step are +-lr wherever |g| >> eps: nothing to learn from them beyond the sign of
    # the gradient, which the bar above already holds (the statistical parameter bar sits at 1.2e-4 outliers on this 200-row run)
    # weights at hundreds of agents: SURVEY 8c's 1e-4 for at least 98 % of the networks, 3e-4 for all (round 4 held 5e-4 for all)
    if n >= 64:
        compare(eng, logs, o_logs, o_w, rtol_w=1e-4, actor="none", outlier_frac=0.02, rtol_w_outlier=3e-4)
    else:
        compare(eng, logs, o_logs, o_w, rtol_w=1e-4, actor="strict")
    return float(e.max())


def actor_stat(eng, o_weights, lr, steps=1):
    """(fraction of the actor parameters further than 5 % of `steps` Adam steps from the oracle's, largest |difference|)"""
    errs = []
    for s in range(eng.S):
        for i in range(eng.N):
            for a, b in zip(eng.get_weights(s, i, "actor"), o_weights[s][i][0]):
                errs.append(np.abs(a - b).ravel())
    e = np.concatenate(errs)
    return float(np.mean(e > 0.05 * lr * steps + 1e-5)), float(e.max())


def check_block_from_injected_state(args, nrow, ncol, device, lib, seeds, blocks_before=2, lattice="auto", tweak=None, oracle_later=False):
    """ONE update block against the oracle from IDENTICAL state: the engine runs `blocks_before` whole blocks and the rollout of the
    next one, its state (every network, the Adam slots, the replay rows) is handed to oracle.update_block, then both sides run the
    update.  Unlike a run from the initial weights this comparison does not need the two rollouts to stay in step, so it reaches the
    steady-state batch (B = buffer_size + one block of rows) with live actors.  Returns (engine, per-network errors)."""
    n, S = args["n_agents"], len(seeds)
    W, goals = make_inputs(args, nrow, seeds)
    cfg = EngineConfig(n, args["agent_label"], args["in_nodes"], H=args["H"], gamma=args["gamma"], slow_lr=args["slow_lr"],
                       fast_lr=args["fast_lr"], max_ep_len=args["max_ep_len"], n_ep_fixed=args["n_ep_fixed"],
                       n_epochs=args["n_epochs"], buffer_size=args["buffer_size"], common_reward=args["common_reward"],
                       nrow=nrow, ncol=ncol, n_seeds=S, rng_mode="device", lattice=lattice)
    eng = RPBCACEngine(cfg, seeds=list(seeds), device=device, lib=lib)
    for s in range(S):
        for i in range(n):
            for net in ("actor", "critic", "tr"):
                eng.set_weights(s, i, net, W[s][i][net])
    eng.set_goals(np.stack(goals))
    if tweak is not None:
        tweak(eng)
    for _ in range(blocks_before):
        eng.run_block()
    eng.rollout_block(cfg.n_ep_fixed)
    snaps = [snapshot_for_oracle(eng, s) for s in range(S)]
    if oracle_later:                                   # the caller batches the oracle jobs of several engines (one process each)
        return eng, snaps
    o_w = run_oracle_blocks_parallel(dict(args), snaps)
    eng.update_block()
    eng.sync()
    return eng, network_errors(eng, o_w), o_w


def _weight_errors(got, want):
    """{net: worst |w - w_oracle| / max(1, |w|max) over the agents} for got / want = [agent][actor, critic, tr] parameter lists"""
    out = {}
    for k, net in enumerate(("actor", "critic", "tr")):
        out[net] = max(float(np.abs(a - b).max()) / max(1.0, float(np.abs(b).max()))
                       for g_i, w_i in zip(got, want) for a, b in zip(g_i[k], w_i[k]))
    return out


def check_pk_range_fallback(device, lib, hid, monkeypatch, tmp_path, planted_label="Cooperative", n=5, nrow=5, max_ep_len=3, n_ep_fixed=2,
                            n_epochs=2, buffer_size=12, fast_lr=0.01, seed=91, rtol=1e-5, actor_tol=1e-5):
    """The range fallback of the packed-operand wide-critic path (RPBCACEngine._poll_pk_range) in ONE instance, end to end.

    Scenario: n agents on the circulant d = 4 graph, H = 1, critic width `hid` (a multiple of 128), lattice layer 1, n_epochs >= 2 (so
    the cached-a2 TD shortcut and _a2_rows_ok run).  The LAST agent -- Cooperative, or a Faulty one whose critic is frozen -- starts
    with ONE out-of-range operand: W2[k][j] = 70 (the bound is 65000 / 2^10 = 63.48) on the hidden unit k with the smallest layer-1
    weights and the layer-2 unit j with the smallest |W3| (plant_out_of_range_w2).  That is the gentlest trigger there is: a1, W2 W3
    and dz1 stay in range, a Cooperative agent's entry is trimmed away by the first hidden-layer consensus (H = 1: it is the one
    outlier of its column), a Faulty agent's stays in its frozen critic for good and reaches the neighbours only through the trimmed
    mean.  The reference's fast_lr = 0.01 needs no lowering for it: THE FLOAT32 ORACLE, run from the engine's state on every block of
    this test, STAYS FINITE WITH NO WEIGHT ABOVE 1e4 (asserted below on the oracle's side: the case cannot pass by both sides diverging).

    Checked: (control) the same scenario without the planted value never warns and stays on the packed path; (flagged block, through
    run_block(), not train()) ends with the RuntimeWarning -- which does not blame fast_lr: the row may be a frozen adversary's --,
    eng.pk None, weights finite; (next block) bit-identical to a fresh engine built with RCMARL_WIDE_PK=0 from the same checkpoint,
    and within `rtol` (critic, team-reward net) / `actor_tol` of oracle.update_block from the identical snapshot, the planted agent
    included; (sticky) the replay grows past `cap`, every row-sized buffer is re-allocated, the engine stays off the packed path and
    does not warn again.

    The flagged block itself ran on clipped operands and is not redone (that would cost a copy of every wide weight per block); its
    deviation from the oracle's block from identical state is printed and returned, not held to a bar.  Measured, worst
    |w - w_oracle| / max(1, |w|max) over the agents (actor / critic / team-reward net):
      hipemu, 5 agents, 128 units:  Cooperative 3.9e-7 / 2.2e-7 / 6.0e-8,  Faulty 7.2e-7 / 3.0e-8 / 6.0e-8
      MI355X, 8 agents, 128 units:  Cooperative 5.5e-7 / 2.2e-7 / 3.0e-8,  Faulty 1.8e-7 / 3.0e-8 / 3.0e-8
      MI355X, 8 agents, 512 units:  Cooperative 7.6e-7 / 1.8e-7 / 6.0e-8,  Faulty 2.0e-6 / 1.5e-8 / 6.0e-8
    (one entry clipped from 70 to the largest f16 / 2^10 = 63.97 on a unit with a small activation moves little; the block after it:
    at most 9e-8 on every network, both backends).
    Returns {"flagged": errors of the flagged block, "next": errors of the block after it}."""
    import warnings
    import pytest
    assert hid % 128 == 0
    labels = ["Cooperative"] * (n - 1) + [planted_label]
    in_nodes = [[(i + k) % n for k in range(4)] for i in range(n)]
    args = make_args(labels, H=1, n_episodes=0, max_ep_len=max_ep_len, n_ep_fixed=n_ep_fixed, n_epochs=n_epochs, buffer_size=buffer_size,
                     seed=seed, in_nodes=in_nodes, fast_lr=fast_lr)
    seeds = (seed,)
    W, goals = make_inputs(args, nrow, seeds, critic_hid=hid)

    def make(W_):
        cfg = EngineConfig(n, labels, in_nodes, H=1, gamma=args["gamma"], slow_lr=args["slow_lr"], fast_lr=fast_lr, max_ep_len=max_ep_len,
                           n_ep_fixed=n_ep_fixed, n_epochs=n_epochs, buffer_size=buffer_size, nrow=nrow, ncol=nrow, n_seeds=1,
                           rng_mode="device", lattice=True, critic_hid=hid)
        eng = RPBCACEngine(cfg, seeds=list(seeds), device=device, lib=lib)
        for i in range(n):
            for net in ("actor", "critic", "tr"):
                eng.set_weights(0, i, net, W_[0][i][net])
        eng.set_goals(np.stack(goals))
        return eng

    def weights(eng):
        return [[eng.get_weights(0, i, net) for net in ("actor", "critic", "tr")] for i in range(n)]

    # control: no planted value -> a block on the packed path, no warning
    ctl = make(W)
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        ctl.run_block()
        assert ctl.pk is not None and not ctl._pk_range_fallback
    assert ctl.wide and ctl.lat_active and ctl._pk_ok("critic", "s", ctl.lat_B)
    assert int(ctl.pk.ovf.item()) == 0

    Wp = [[{net: [a.copy() for a in W[0][i][net]] for net in W[0][i]} for i in range(n)]]
    k, j = plant_out_of_range_w2(Wp[0][n - 1]["critic"])
    eng = make(Wp)
    assert eng.pk is not None
    snaps, update_block = [], eng.update_block

    def update_block_snapped():                     # the state every update block starts from, for the oracle
        snaps.append(snapshot_for_oracle(eng, 0))
        return update_block()
    eng.update_block = update_block_snapped
    # the block in which the flag rises, through run_block()
    with pytest.warns(RuntimeWarning, match="packed-operand") as rec:
        eng.run_block()
    msgs = [str(w.message) for w in rec if "packed-operand" in str(w.message)]
    assert len(msgs) == 1 and "fast_lr" not in msgs[0] and "dense path" in msgs[0], msgs
    assert eng.pk is None and eng._pk_range_fallback and not eng._pk_ok("critic", "s", eng.B)
    after = {0: weights(eng)}
    assert all(bool(np.isfinite(a).all()) for ag in after[0] for net in ag for a in net)
    ck = str(tmp_path / ("pk_fallback_%d_%s.pt" % (hid, planted_label)))
    eng.save_checkpoint(ck)
    # the next block: (a) against an engine that never had the packed path, from the same checkpoint
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        eng.run_block()
        eng.sync()
        after[1] = weights(eng)
        monkeypatch.setenv("RCMARL_WIDE_PK", "0")
        dense = make(W)
        monkeypatch.delenv("RCMARL_WIDE_PK")
        assert dense.pk is None
        dense.load_checkpoint(ck)
        dense.run_block()
        dense.sync()
    assert eng.adam_t == dense.adam_t == 2
    for net in eng.theta:
        np.testing.assert_array_equal(eng.theta[net].cpu().numpy(), dense.theta[net].cpu().numpy(), err_msg=net)
    for net in eng.loss:
        np.testing.assert_array_equal(eng.loss[net].cpu().numpy(), dense.loss[net].cpu().numpy(), err_msg="loss " + net)
    np.testing.assert_array_equal(eng.adam_m.cpu().numpy(), dense.adam_m.cpu().numpy())
    np.testing.assert_array_equal(eng.adam_v.cpu().numpy(), dense.adam_v.cpu().numpy())
    for key in eng.rp:
        np.testing.assert_array_equal(eng.rp[key][:, :eng.B].cpu().numpy(), dense.rp[key][:, :dense.B].cpu().numpy())
    # sticky: the replay grows past cap (a trailing episode, then a second train() call), every row-sized buffer is re-allocated
    cap0 = eng.cap
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        eng.train(n_ep_fixed + 1)
        eng.train(n_ep_fixed)
    assert eng.cap > cap0 and eng.pk is None and eng._pk_range_fallback
    assert len(snaps) == 4
    # the oracle, one update block from each of those states
    o_w = run_oracle_blocks_parallel(dict(args), snaps)
    for b, ow in enumerate(o_w):
        big = max(float(np.abs(a).max()) for ag in ow for net in ag[:3] for a in net)
        assert all(bool(np.isfinite(a).all()) for ag in ow for net in ag[:3] for a in net) and big <= 1e4, \
            "the ORACLE does not stay finite and below 1e4 in block %d (largest |w| %g): not a case for this check" % (b, big)
    out = {"flagged": _weight_errors(after[0], o_w[0]), "next": _weight_errors(after[1], o_w[1])}
    print("[pk range fallback, %s, %d units, planted %s agent W2[%d][%d] = %g, fast_lr %g] worst |w - w_oracle| / max(1,|w|max): flagged block "
          "(clipped operands, no bar) actor %.2e critic %.2e tr %.2e | next block actor %.2e critic %.2e tr %.2e (bars %.0e / %.0e / %.0e)"
          % (device, hid, planted_label, k, j, PK_PLANT_W2, fast_lr, out["flagged"]["actor"], out["flagged"]["critic"], out["flagged"]["tr"],
             out["next"]["actor"], out["next"]["critic"], out["next"]["tr"], actor_tol, rtol, rtol))
    assert out["next"]["critic"] <= rtol and out["next"]["tr"] <= rtol and out["next"]["actor"] <= actor_tol, out
    return out
