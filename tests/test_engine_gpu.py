"""End-to-end parity on a real MI355X: the batched engine vs the oracle's train()
from identical initial weights and identical RNG streams."""
import pytest

import engine_checks as EC

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("rng_mode", ["device", "numpy"])
def test_engine_coop_H1(rng_mode):
    args = EC.make_args(["Cooperative"] * 5, H=1, n_episodes=45, max_ep_len=20, n_ep_fixed=10, n_epochs=3, buffer_size=400, seed=100)
    eng, logs, o_logs, o_w = EC.run_pair(args, 5, 5, rng_mode, "cuda", None, seeds=(100, 200, 300))
    EC.compare(eng, logs, o_logs, o_w)


def test_engine_coop_H0_common_reward():
    args = EC.make_args(["Cooperative"] * 5, H=0, n_episodes=20, max_ep_len=20, n_ep_fixed=10, n_epochs=2, buffer_size=300, seed=7,
                        common_reward=True)
    eng, logs, o_logs, o_w = EC.run_pair(args, 5, 5, "device", "cuda", None, seeds=(7,))
    EC.compare(eng, logs, o_logs, o_w)


@pytest.mark.parametrize("labels", [["Cooperative"] * 5, ["Cooperative"] * 4 + ["Malicious"], ["Cooperative", "Faulty", "Cooperative", "Cooperative", "Cooperative"]])
def test_engine_local_fits_as_matrix_core_chains(labels, monkeypatch):
    """RCMARL_FIT_CHAINS=1: the cooperative agents' 5-step full-batch local fits of the small networks through rcmarl_minibatch_fit
    (batch_size = B, no shuffle: one matrix-core wavefront per network, activations never leave the registers; the default from
    1024 networks per launch on -- the batched BASELINE configs[0] / [1] workloads) vs the oracle, steady-state buffer included."""
    monkeypatch.setenv("RCMARL_FIT_CHAINS", "1")
    args = EC.make_args(labels, H=1, n_episodes=45, max_ep_len=20, n_ep_fixed=10, n_epochs=3, buffer_size=400, seed=100)
    eng, logs, o_logs, o_w = EC.run_pair(args, 5, 5, "device", "cuda", None, seeds=(100, 200, 300))
    assert eng._fit_as_chains("critic", eng.coop) and eng._fit_as_chains("tr", eng.coop)
    EC.compare(eng, logs, o_logs, o_w)


def test_engine_12_agents_H2():
    n = 12
    in_nodes = [[(i + k) % n for k in range(6)] for i in range(n)]
    args = EC.make_args(["Cooperative"] * n, H=2, n_episodes=10, max_ep_len=10, n_ep_fixed=5, n_epochs=2, buffer_size=80, seed=9,
                        in_nodes=in_nodes)
    eng, logs, o_logs, o_w = EC.run_pair(args, 8, 8, "device", "cuda", None, seeds=(9, 10))
    EC.compare(eng, logs, o_logs, o_w)


@pytest.mark.parametrize("labels", [["Cooperative"] * 4 + ["Malicious"], ["Cooperative", "Greedy", "Cooperative", "Cooperative", "Faulty"]])
def test_engine_with_adversaries(labels):
    """BASELINE configs[1] (4 cooperative + 1 Malicious, H=1) and a Greedy+Faulty mix: shuffled
    mini-batch fits (32 x 10 epochs) and shuffled actor fits (200-row Adam mini-batches)."""
    args = EC.make_args(labels, H=1, n_episodes=30, max_ep_len=20, n_ep_fixed=15, n_epochs=2, buffer_size=450, seed=300)
    eng, logs, o_logs, o_w = EC.run_pair(args, 5, 5, "device", "cuda", None, seeds=(300, 301))
    EC.compare(eng, logs, o_logs, o_w)


@pytest.mark.parametrize("n,nrow,ncol,labels", [(5, 5, 5, None), (20, 16, 12, None), (5, 5, 5, ["Cooperative"] * 4 + ["Malicious"])])
def test_engine_lattice_path(n, nrow, ncol, labels):
    """Layer-1 GEMMs on the exact bf16x3 (lattice) kernels: same parity bar as the f32-MFMA path.
    n=20 is above the engine's own "auto" threshold; n=5 forces the path on the reference's config."""
    labels = labels or ["Cooperative"] * n
    d = 4 if n == 5 else 6
    in_nodes = [[(i + k) % n for k in range(d)] for i in range(n)]
    args = EC.make_args(labels, H=1 if n == 5 else 2, n_episodes=20, max_ep_len=20, n_ep_fixed=10, n_epochs=3, buffer_size=300,
                        seed=41, in_nodes=in_nodes)
    eng, logs, o_logs, o_w = EC.run_pair(args, nrow, ncol, "device", "cuda", None, seeds=(41, 42), lattice=True if n == 5 else "auto")
    assert eng.lat_enabled and eng.lat_active
    EC.compare(eng, logs, o_logs, o_w)


def test_engine_full_size_lattice_equals_f32_path():
    """BASELINE configs[3] shape (256 agents, 32x32 grid, H=8, d=18; 2 of the 16 seeds of a GPU shard): one whole
    training block with the layer-1 GEMMs on the lattice kernels vs on the f32-MFMA kernels.  The rollout is
    identical (it precedes the first update), the updated weights agree to fp32 roundoff accumulated over the block."""
    import numpy as np
    from rcmarl_amd.engine import EngineConfig, RPBCACEngine
    n, d = 256, 18
    in_nodes = [[(i + k) % n for k in range(d)] for i in range(n)]
    out = {}
    for lat in (False, True):
        # fast_lr 0.0025: the reference's 0.01 makes the plain-SGD local fits diverge to NaN at 768 inputs (see bench.py)
        cfg = EngineConfig(n, ["Cooperative"] * n, in_nodes, H=8, max_ep_len=20, n_ep_fixed=50, n_epochs=2, buffer_size=2000,
                           fast_lr=0.0025, nrow=32, ncol=32, n_seeds=2, rng_mode="device", lattice=lat)
        eng = RPBCACEngine(cfg, seeds=[1000, 1001])
        eng.init_glorot(base_seed=1)
        eng.set_goals(np.stack([np.random.RandomState(s).randint(0, 5, size=(n, 2)) for s in (1000, 1001)]))
        logs = eng.train(50)
        assert eng.lat_active == lat
        out[lat] = (logs, {k: eng.get_all_weights(k) for k in ("actor", "critic", "tr")})
        assert all(np.isfinite(v).all() for v in out[lat][1].values())
    for k in out[False][0]:
        if k == "Estimated_team_returns":
            np.testing.assert_allclose(out[True][0][k], out[False][0][k], rtol=1e-5, atol=1e-6)
        else:
            np.testing.assert_array_equal(out[True][0][k], out[False][0][k])
    for net in ("critic", "tr"):
        a, b = out[True][1][net], out[False][1][net]
        # 20 SGD steps + 2 clipped consensus rounds amplify fp32 roundoff on a few columns; noise, not bias:
        diff = np.abs(a - b)
        assert float(diff.max()) <= 1e-3 * max(1.0, float(np.abs(b).max())) and float(diff.mean()) <= 5e-6, \
            (net, float(diff.max()), float(diff.mean()))
    # the actor's first Adam step is lr*g/(|g|+eps) ~ lr*sign(g): entries whose gradient is ~0 may flip, so the
    # statement for the actor is statistical
    a, b = out[True][1]["actor"], out[False][1]["actor"]
    diff = np.abs(a - b)
    assert float(diff.mean()) <= 1e-5 and float((diff > 1e-4).mean()) <= 1e-3, (float(diff.mean()), float((diff > 1e-4).mean()))


@pytest.mark.parametrize("labels", [["Cooperative"] * 5, ["Cooperative"] * 4 + ["Malicious"], ["Cooperative"] * 20])
def test_engine_run_to_run_bit_identical(labels):
    """No atomics, no unordered reductions, every LDS-DMA waited for: the same scenario twice gives the same bits
    (256 seeds x 5 agents is the shape that exposed a missing wait in the consensus kernel)."""
    import numpy as np
    from rcmarl_amd.engine import EngineConfig, RPBCACEngine
    n = len(labels)
    S = 256 if n == 5 else 32                      # 20 agents: the lattice (bf16x3) layer-1 path
    in_nodes = EC.CIRC5 if n == 5 else [[(i + k) % n for k in range(4)] for i in range(n)]
    res = []
    for rep in range(2):
        cfg = EngineConfig(n, labels, in_nodes, H=1, n_seeds=S, rng_mode="device", max_ep_len=20, n_ep_fixed=20, n_epochs=4,
                           buffer_size=800, nrow=8 if n > 5 else 5, ncol=8 if n > 5 else 5)
        eng = RPBCACEngine(cfg, seeds=list(range(100, 100 + S)))
        eng.init_glorot(base_seed=1)
        eng.set_goals(np.stack([np.random.RandomState(s).randint(0, 5, size=(n, 2)) for s in range(S)]))
        logs = eng.train(40)
        res.append((logs, {k: eng.theta[k].detach().cpu().numpy().copy() for k in eng.theta}))
    for k in res[0][0]:
        np.testing.assert_array_equal(res[0][0][k], res[1][0][k])
    for k in res[0][1]:
        assert np.isfinite(res[0][1][k]).all()
        np.testing.assert_array_equal(res[0][1][k], res[1][1][k])


@pytest.mark.parametrize("n,S,nrow", [(5, 1, 5), (20, 2, 8), (64, 1, 16)])
def test_engine_epochs_replayed_from_a_hipgraph_are_bit_identical(n, S, nrow, monkeypatch):
    """RCMARL_GRAPH: from the second epoch of a block on, an epoch is one captured hipGraph (engine._epoch) -- same launches, same
    arguments, replayed; growing replay buffer (a capture per B) into steady state (the same graph across blocks).  Bits equal
    the eager run's; the default (on for small instances) actually replays."""
    import numpy as np
    from rcmarl_amd.engine import EngineConfig, RPBCACEngine
    in_nodes = EC.CIRC5 if n == 5 else [[(i + k) % n for k in range(4)] for i in range(n)]
    res = {}
    for mode in ("0", "1", None):
        if mode is None:
            monkeypatch.delenv("RCMARL_GRAPH", raising=False)
        else:
            monkeypatch.setenv("RCMARL_GRAPH", mode)
        cfg = EngineConfig(n, ["Cooperative"] * n, in_nodes, H=1, n_seeds=S, rng_mode="device", max_ep_len=20, n_ep_fixed=10,
                           n_epochs=4, buffer_size=400, nrow=nrow, ncol=nrow)
        eng = RPBCACEngine(cfg, seeds=list(range(100, 100 + S)))
        eng.init_glorot(base_seed=1)
        eng.set_goals(np.stack([np.random.RandomState(s).randint(0, 5, size=(n, 2)) for s in range(S)]))
        logs = eng.train(50)                       # 5 blocks: B = 200, 400, 600, 600, 600
        res[mode] = (logs, {k: eng.theta[k].detach().cpu().numpy().copy() for k in eng.theta}, eng.graph_captures, eng.graph_replays)
    assert res["0"][2:] == (0, 0)
    assert res["1"][2] == 3 and res["1"][3] == 5 * 3, res["1"][2:]          # one capture per distinct B, three replays per block
    assert res[None][3] == 5 * 3                                              # S * N <= 256: on by default
    for mode in ("1", None):
        for k in res["0"][0]:
            np.testing.assert_array_equal(res["0"][0][k], res[mode][0][k])
        for k in res["0"][1]:
            assert np.isfinite(res["0"][1][k]).all()
            np.testing.assert_array_equal(res["0"][1][k], res[mode][1][k])


@pytest.mark.parametrize("labels,S", [(["Cooperative"] * 4 + ["Malicious"], 1), (["Greedy", "Cooperative", "Cooperative", "Malicious", "Faulty"], 2),
                                      (["Cooperative", "Faulty", "Cooperative", "Cooperative", "Faulty"], 1)])
def test_engine_epochs_with_adversaries_replayed_from_a_hipgraph_are_bit_identical(labels, S, monkeypatch):
    """The reference's own headline scenario (main.py:88-104 with a Malicious agent) as captured epochs.  Round 5: all fits of an
    epoch are ONE rcmarl_minibatch_fit_multi launch on the capture stream (no side streams), so the DEFAULT engine captures such
    instances too.  The per-family launches stay behind RCMARL_ADV_MULTI=0: inline on the capture stream (RCMARL_ADV_ASYNC=0) they
    capture as well; on their side streams the capture crashes this ROCm's runtime, so that combination keeps the instance eager
    (asserted).  The shuffle stream's call counter lives on the device (engine_adversaries._draw), the out-of-range flags are consumed
    by the fix-up launch.  Weights, logs and the number of shuffle draws equal the eager per-family run's bit for bit in every
    mode, and epochs really are replayed."""
    import numpy as np
    from rcmarl_amd.engine import EngineConfig, RPBCACEngine
    n = len(labels)
    fits = any(l in ("Greedy", "Malicious") for l in labels)
    res = {}
    for graph, asyn, multi in (("0", "1", "0"), ("1", "0", "0"), ("1", "1", "0"), ("0", "1", "1"), ("1", "1", "1")):
        monkeypatch.setenv("RCMARL_GRAPH", graph)
        monkeypatch.setenv("RCMARL_ADV_ASYNC", asyn)
        monkeypatch.setenv("RCMARL_ADV_MULTI", multi)
        cfg = EngineConfig(n, labels, EC.CIRC5, H=1, n_seeds=S, rng_mode="device", max_ep_len=20, n_ep_fixed=10, n_epochs=4,
                           buffer_size=400, nrow=5, ncol=5)
        eng = RPBCACEngine(cfg, seeds=list(range(200, 200 + S)))
        eng.init_glorot(base_seed=2)
        eng.set_goals(np.stack([np.random.RandomState(s).randint(0, 5, size=(n, 2)) for s in range(S)]))
        logs = eng.train(50)                       # 5 blocks: B = 200, 400, 600, 600, 600
        res[(graph, asyn, multi)] = (logs, {k: eng.theta[k].detach().cpu().numpy().copy() for k in eng.theta}, eng.graph_captures,
                                     eng.graph_replays, list(eng.adv.calls))
    eager, inline, side = res[("0", "1", "0")], res[("1", "0", "0")], res[("1", "1", "0")]
    eager_multi, dflt = res[("0", "1", "1")], res[("1", "1", "1")]
    assert eager[2:4] == (0, 0) and eager_multi[2:4] == (0, 0)
    assert inline[2] == 3 and inline[3] == 5 * 3, inline[2:4]
    assert side[2:4] == ((0, 0) if fits else (3, 15))                         # per-family fits on side streams: the engine stays eager
    assert dflt[2:4] == (3, 15), dflt[2:4]                                    # the default (one multi launch): captured and replayed
    for other in (inline, side, eager_multi, dflt):
        assert eager[4] == other[4]                                           # the same number of shuffle draws was consumed
        for k in eager[0]:
            np.testing.assert_array_equal(eager[0][k], other[0][k])
        for k in eager[1]:
            assert np.isfinite(eager[1][k]).all()
            np.testing.assert_array_equal(eager[1][k], other[1][k])


@pytest.mark.parametrize("n,critic_hid,H,d,rng_mode,lattice", [(5, 64, 1, 4, "device", False), (12, 512, 2, 6, "device", False),
                                                               (5, 128, 0, 4, "numpy", False), (12, 512, 2, 6, "device", True),
                                                               (20, 96, 1, 5, "device", "auto")])
def test_engine_wide_critic(n, critic_hid, H, d, rng_mode, lattice):
    """BASELINE configs[4] in miniature: a critic wider than the reference's 20 units (512 in one case) takes the
    dense f32-MFMA GEMM path for local fits, TD targets, estimate consensus and start-state values; everything else
    (team-reward net, actor, rollout) stays on the 20-unit kernels.  Same oracle, same tolerances."""
    in_nodes = [[(i + k) % n for k in range(d)] for i in range(n)]
    args = EC.make_args(["Cooperative"] * n, H=H, n_episodes=12, max_ep_len=10, n_ep_fixed=4, n_epochs=2, buffer_size=60, seed=51,
                        in_nodes=in_nodes, fast_lr=0.005)
    eng, logs, o_logs, o_w = EC.run_pair(args, 6, 6, rng_mode, "cuda", None, seeds=(51, 52), critic_hid=critic_hid, lattice=lattice)
    assert eng.wide and eng.lat_active == (lattice is not False)
    EC.compare(eng, logs, o_logs, o_w)


@pytest.mark.parametrize("n,critic_hid,lattice,labels", [(6, 64, False, {1: "Greedy", 4: "Malicious"}), (16, 64, True, {0: "Malicious", 9: "Malicious"})])
def test_engine_wide_critic_with_greedy_and_malicious_agents(n, critic_hid, lattice, labels):
    """Byzantine agents beside a wide critic (VERDICT r02 missing #3; agents/adversarial_CAC_agents.py:121-165,228-253 take any
    Keras model): two adversaries, 64-unit critic, vs the oracle.  Their mini-batch message generators run through the dense
    per-agent GEMM entry points, 32 permuted rows at a time (engine_adversaries._fit_critic_family) -- correct, not fast."""
    d = 4
    in_nodes = [[(i + k) % n for k in range(d)] for i in range(n)]
    lab = ["Cooperative"] * n
    for i, v in labels.items():
        lab[i] = v
    args = EC.make_args(lab, H=1, n_episodes=8, max_ep_len=10, n_ep_fixed=4, n_epochs=2, buffer_size=60, seed=58,
                        in_nodes=in_nodes, fast_lr=0.005)
    eng, logs, o_logs, o_w = EC.run_pair(args, 6, 6, "device", "cuda", None, seeds=(58,), critic_hid=critic_hid, lattice=lattice)
    assert eng.wide and hasattr(eng, "adv") and eng.adv.fit and eng.lat_active == lattice
    EC.compare(eng, logs, o_logs, o_w)


@pytest.mark.parametrize("n,critic_hid,lattice", [(6, 64, False), (16, 512, True)])
def test_engine_wide_critic_with_faulty_agents(n, critic_hid, lattice):
    """Faulty agents (frozen critic / team-reward messages, learning actor: adversarial_CAC_agents.py:5-55) beside a wide
    critic: the frozen wide message enters its neighbours' aggregations, the Faulty actors take their mini-batch Adam steps
    from TD errors of their own wide critic."""
    d = 4
    in_nodes = [[(i + k) % n for k in range(d)] for i in range(n)]
    labels = ["Cooperative"] * n
    labels[2] = labels[n - 1] = "Faulty"
    args = EC.make_args(labels, H=1, n_episodes=12, max_ep_len=10, n_ep_fixed=4, n_epochs=2, buffer_size=60, seed=57,
                        in_nodes=in_nodes, fast_lr=0.005)
    eng, logs, o_logs, o_w = EC.run_pair(args, 6, 6, "device", "cuda", None, seeds=(57, 58), critic_hid=critic_hid, lattice=lattice)
    assert eng.wide and hasattr(eng, "adv") and eng.lat_active == lattice
    EC.compare(eng, logs, o_logs, o_w)


@pytest.mark.parametrize("critic_hid", [128, 512])
@pytest.mark.parametrize("planted_label", ["Cooperative", "Faulty"])
def test_packed_operand_range_fallback(planted_label, critic_hid, monkeypatch, tmp_path):
    """tests/engine_checks.check_pk_range_fallback on the gfx950 kernels: an out-of-range operand in ONE agent's critic, the block
    after the fallback bit-identical to the dense path and within 1e-4 of the oracle from identical state (the bar of the wide-critic
    probed-row checks, check_probed_rows_vs_oracle), the actors within 5 % of an Adam step (compare()'s bar)."""
    EC.check_pk_range_fallback("cuda", None, critic_hid, monkeypatch, tmp_path, planted_label=planted_label, n=8, nrow=6, max_ep_len=5,
                               n_ep_fixed=4, n_epochs=2, buffer_size=40, rtol=1e-4, actor_tol=0.05 * 0.002 + 1e-5)


def test_engine_wide_critic_cfg5_shape_paths_agree():
    """BASELINE configs[4] shape at an eighth of the agents (128 agents, 512-unit critic, H=32, circulant d=66, 32x32 grid,
    B = 1000..): one training block with layer 1 of the critic on the bf16x3 lattice kernels + the circulant consensus
    kernel vs on the dense f32-MFMA GEMM + the general consensus kernel.  Independent implementations of the same
    fp32 math: identical rollouts, weights equal to accumulated fp32 roundoff, all finite."""
    import os
    import numpy as np
    from rcmarl_amd.engine import EngineConfig, RPBCACEngine
    n, d = 128, 66
    in_nodes = [[(i + k) % n for k in range(d)] for i in range(n)]
    out = {}
    for fast in (False, True):
        os.environ["RCMARL_K1_CIRC"] = "1" if fast else "0"
        try:
            cfg = EngineConfig(n, ["Cooperative"] * n, in_nodes, H=32, max_ep_len=20, n_ep_fixed=50, n_epochs=2, buffer_size=2000,
                               fast_lr=0.002, nrow=32, ncol=32, n_seeds=1, rng_mode="device", lattice=fast, critic_hid=512)
            eng = RPBCACEngine(cfg, seeds=[2000])
        finally:
            os.environ.pop("RCMARL_K1_CIRC", None)
        assert eng.wide and eng.k1_circulant == fast
        eng.init_glorot(base_seed=2)
        eng.set_goals(np.random.RandomState(7).randint(0, 5, size=(n, 2)))
        logs = eng.train(50)
        assert eng.lat_active == fast
        out[fast] = (logs, {k: eng.get_all_weights(k) for k in ("critic", "tr")})
        assert all(np.isfinite(v).all() for v in out[fast][1].values())
    for k in ("True_team_returns", "True_adv_returns"):
        np.testing.assert_array_equal(out[True][0][k], out[False][0][k])
    for net in ("critic", "tr"):
        a, b = out[True][1][net], out[False][1][net]
        diff = np.abs(a - b)
        assert float(diff.max()) <= 1e-3 * max(1.0, float(np.abs(b).max())) and float(diff.mean()) <= 5e-6, \
            (net, float(diff.max()), float(diff.mean()))


@pytest.mark.parametrize("labels,rng_mode,n", [(["Cooperative"] * 4 + ["Malicious"], "device", 5), (["Cooperative"] * 5, "numpy", 5),
                                               (["Cooperative"] * 19 + ["Greedy"], "device", 20)])
def test_checkpoint_resume_is_bit_identical(labels, rng_mode, n, tmp_path):
    """Mid-run checkpoint on the GPU (the reference only saves final weights, main.py:119-121): 2 blocks -> save -> fresh
    engine -> load -> 2 blocks equals 4 blocks straight, bit for bit; n = 20 runs the lattice GEMMs and the TD shortcut."""
    EC.check_checkpoint_resume(labels, rng_mode, "cuda", None, str(tmp_path / "ck.pt"), n=n, nrow=5 if n == 5 else 8,
                               max_ep_len=20, n_ep_fixed=10, n_epochs=3, buffer_size=300, S=3, blocks=(2, 2),
                               lattice=True if n == 5 else "auto")

