"""Wide actors (EngineConfig.actor_hid != 20) -- checks shared by the hipemu and the GPU tests: the two forward kernels of the rollout
(csrc/rollout.hip: plain, any width; matrix core, episode-parallel) against oracle/mlp_np and the oracle's Philox draw, the Adam
step (head kernel, Adam epilogue of the weight-gradient GEMMs, small Adam kernel) against the oracle's Keras Adam, the engine
against oracle.train, checkpoints, refusals and the routing of widths the matrix-core kernel does not serve."""
import collections

import numpy as np
import pytest

import engine_checks as EC
from kernel_checks import pad64, pack_rows, unpack_row
from oracle import mlp_np as M
from oracle import philox_np as PX
from oracle import rpbcac_oracle as O
from rcmarl_amd import capi
from rcmarl_amd.engine import EngineConfig, RPBCACEngine

A = 5
COOP = "Cooperative"
CIRC3 = [[0, 1, 2], [1, 2, 0], [2, 0, 1]]
# S, N, E of every kernel case: in_dim 6 (no multiple of the 16-wide contraction step), 5 episodes in 64 lanes
S_, N_, E_ = 2, 3, 5
NROW = 5
SEEDS = (1000, 1017)              # Philox keys of the two seeds; check_seed_has_no_knife_edge holds them to the 1e-6 margin
EPISODE0, STEP = 4, 1


def actor_params(rng, S, N, in_dim, hid, bias_scale=0.3):
    out = []
    for s in range(S):
        row = []
        for n in range(N):
            p = M.init_mlp(rng, in_dim, hid, A)
            for k in (1, 3, 5):
                p[k] += (bias_scale * rng.normal(size=p[k].shape)).astype(np.float32)
            row.append(p)
        out.append(row)
    return out


def ageom(in_dim, hid):
    o_b1 = in_dim * hid
    o_W2 = o_b1 + hid
    o_b2 = o_W2 + hid * hid
    o_W3 = o_b2 + hid
    o_b3 = o_W3 + hid * A
    return dict(o_b1=o_b1, o_W2=o_W2, o_b2=o_b2, o_W3=o_W3, o_b3=o_b3, P=o_b3 + A)


class _Scene:
    """start states of E episodes of S seeds (Philox resets), actors of one width, the oracle's probabilities and draws"""

    def __init__(self, hid, plant=False):
        S, N, E = S_, N_, E_
        self.hid, self.in_dim = hid, 2 * N
        rng = np.random.default_rng(700 + hid)
        self.params = actor_params(rng, S, N, self.in_dim, hid)
        if plant:
            # one weight beyond the range of the two-piece f16 form (2^10 |w| > 65000, i.e. |w| > 63.5): that (seed, agent)'s
            # workgroup redoes both layers on the fp32 values
            self.params[1][2][0][3, 5] = np.float32(90.0)
        self.ldp = pad64(ageom(self.in_dim, hid)["P"])
        self.theta = pack_rows(self.params, self.ldp)
        self.goal = rng.integers(0, NROW, size=(S, N, 2)).astype(np.int32)
        self.seeds = np.array(SEEDS, dtype=np.uint64)
        mean, std = np.mean(np.arange(NROW)), np.std(np.arange(NROW))
        self.scale = np.array([mean, mean, std, std])
        self.pos = np.stack([np.stack([PX.reset_positions(N, NROW, NROW, int(self.seeds[s]), EPISODE0 + e) for e in range(E)])
                             for s in range(S)]).astype(np.int32)                              # [S][E][N][2]
        self.x = ((self.pos.astype(np.float64) - mean) / std).astype(np.float32).reshape(S, E, 2 * N)
        # oracle: probabilities [S][E][N][A], draws [S][E][N]
        self.probs = np.stack([np.stack([M.softmax(M.forward(self.params[s][i], self.x[s])) for i in range(N)], axis=1) for s in range(S)])
        self.acts = np.stack([np.stack([PX.sample_actions(self.probs[s, e], int(self.seeds[s]), EPISODE0 + e, STEP, 0.1) for e in range(E)])
                              for s in range(S)])
        self.margins = np.stack([PX.action_margins(self.probs[s], int(self.seeds[s]), EPISODE0 + np.arange(E)[:, None], STEP)
                                 for s in range(S)])


_SCENES = {}


def scene(hid, plant=False):
    key = (hid, plant)
    if key not in _SCENES:
        _SCENES[key] = _Scene(hid, plant)
    return _SCENES[key]


def check_seed_has_no_knife_edge():
    """none of the 2 * 3 * 5 draws of any scene a test runs (the GPU-only 512-unit one included) sits within 1e-6 of a
    cumulative-probability boundary (CPU only)"""
    for hid, plant in ((24, False), (32, False), (96, False), (32, True), (512, False)):
        sc = scene(hid, plant)
        assert sc.margins.shape == (S_, E_, N_) and float(sc.margins.min()) > 1e-6, (hid, plant, float(sc.margins.min()))


def _close(got, want, rtol, what):
    err = np.abs(np.asarray(got, np.float64) - np.asarray(want, np.float64))
    bad = err > rtol * np.abs(want)
    assert not bad.any(), (what, float((err / np.abs(want)).max()))


def _next_positions(sc, acts):
    """Grid_World.step (environments/grid_world.py:52-55) of every (seed, episode, agent)"""
    mv = np.array([[0, 0], [-1, 0], [1, 0], [0, -1], [0, 1]])
    return np.clip(sc.pos + mv[acts], 0, NROW - 1).astype(np.int32)


def run_plain(bk, sc):
    """rcmarl_policy_probs_wide and one rcmarl_rollout_step_wide per episode -> probs [S][E][N][A], actions [S][E][N], next positions"""
    S, N, E, L = S_, N_, E_, bk.lib
    d_th, d_goal, d_seeds, d_scale = bk.dev(sc.theta), bk.dev(sc.goal), bk.dev(sc.seeds), bk.dev(sc.scale)
    probs, acts, nxt = np.zeros((S, E, N, A), np.float32), np.zeros((S, E, N), np.int64), np.zeros((S, E, N, 2), np.int32)
    for e in range(E):
        d_xs, d_pos = bk.dev(np.ascontiguousarray(sc.x[:, e])), bk.dev(np.ascontiguousarray(sc.pos[:, e]))
        d_p = bk.dev(np.zeros((S, N, A), np.float32))
        L.rcmarl_policy_probs_wide(bk.ptr(d_xs), bk.ptr(d_th), bk.ptr(d_p), S, N, 2 * N, sc.hid, A, sc.ldp, bk.stream)
        probs[:, e] = bk.host(d_p)
        rp = {k: bk.dev(np.zeros((S, 2, w * N), np.float32)) for k, w in (("s", 2), ("ns", 2), ("sa", 3), ("a", 1), ("r", 1))}
        d_pn, d_xn = bk.dev(np.zeros((S, N, 2), np.int32)), bk.dev(np.zeros((S, 2 * N), np.float32))
        d_ret, d_act = bk.dev(np.zeros((S, N), np.float64)), bk.dev(np.full((S, N), -1, np.int32))
        L.rcmarl_rollout_step_wide(bk.ptr(d_xs), bk.ptr(d_pos), bk.ptr(d_goal), bk.ptr(d_th), bk.ptr(d_seeds), NROW, NROW, bk.ptr(d_scale),
                                   bk.ptr(rp["s"]), bk.ptr(rp["ns"]), bk.ptr(rp["sa"]), bk.ptr(rp["a"]), bk.ptr(rp["r"]), 2, 1,
                                   bk.ptr(d_pn), bk.ptr(d_xn), bk.ptr(d_ret), 0.9, EPISODE0 + e, STEP, 0.1, S, N, sc.hid, A, sc.ldp,
                                   bk.ptr(d_act), bk.stream)
        acts[:, e], nxt[:, e] = bk.host(d_act), bk.host(d_pn)
        np.testing.assert_array_equal(bk.host(rp["a"])[:, 1, :], acts[:, e].astype(np.float32))
        np.testing.assert_array_equal(bk.host(rp["s"])[:, 1, :], sc.x[:, e])
        assert not bk.host(rp["a"])[:, 0].any()                       # row 0 of the replay tensors untouched
    return probs, acts, nxt


def run_matrix_core(bk, sc):
    """rcmarl_policy_probs_episodes_wide and one rcmarl_rollout_step_episodes_wide -> the same three arrays"""
    S, N, E, L = S_, N_, E_, bk.lib
    EP, ep_len = pad64(E), STEP + 2
    xsT = np.zeros((S, 2 * N, EP), np.float32)
    xsT[:, :, :E] = sc.x.transpose(0, 2, 1)
    posT = np.zeros((S, N, 2, EP), np.int32)
    posT[:, :, :, :E] = sc.pos.transpose(0, 2, 3, 1)
    d_th, d_goal, d_seeds, d_scale = bk.dev(sc.theta), bk.dev(sc.goal), bk.dev(sc.seeds), bk.dev(sc.scale)
    d_xs, d_pos = bk.dev(xsT), bk.dev(posT)
    d_p = bk.dev(np.full((S, N, EP, A), -7.0, np.float32))
    L.rcmarl_policy_probs_episodes_wide(bk.ptr(d_xs), bk.ptr(d_th), bk.ptr(d_p), S, N, E, EP, sc.hid, A, sc.ldp, bk.stream)
    p = bk.host(d_p)
    assert (p[:, :, E:] == -7.0).all()                                # idle lanes write nothing
    cap = E * ep_len + 3
    rp = {k: bk.dev(np.full((S, cap, w * N), -7.0, np.float32)) for k, w in (("s", 2), ("ns", 2), ("sa", 3), ("a", 1), ("r", 1))}
    d_pn, d_xn = bk.dev(np.full((S, N, 2, EP), -7, np.int32)), bk.dev(np.full((S, 2 * N, EP), -7.0, np.float32))
    d_ret = bk.dev(np.zeros((S, N, EP), np.float64))
    L.rcmarl_rollout_step_episodes_wide(bk.ptr(d_xs), bk.ptr(d_pos), bk.ptr(d_goal), bk.ptr(d_th), bk.ptr(d_seeds), NROW, NROW,
                                        bk.ptr(d_scale), bk.ptr(rp["s"]), bk.ptr(rp["ns"]), bk.ptr(rp["sa"]), bk.ptr(rp["a"]), bk.ptr(rp["r"]),
                                        cap, 2, ep_len, bk.ptr(d_pn), bk.ptr(d_xn), bk.ptr(d_ret), 0.9, EPISODE0, STEP, 0.1, S, N, E, EP,
                                        sc.hid, A, sc.ldp, bk.stream)
    rows = 2 + np.arange(E) * ep_len + STEP
    a = bk.host(rp["a"])
    acts = a[:, rows, :].astype(np.int64)
    untouched = np.ones(cap, bool)
    untouched[rows] = False
    assert (a[:, untouched] == -7.0).all()                            # only the E rows of this step are written
    np.testing.assert_array_equal(bk.host(rp["s"])[:, rows, :], sc.x)
    pn = bk.host(d_pn)
    assert (pn[:, :, :, E:] == -7).all()
    return p[:, :, :E].transpose(0, 2, 1, 3), acts, pn[:, :, :, :E].transpose(0, 3, 1, 2)


def check_forward_plain(bk, hid):
    sc = scene(hid)
    probs, acts, nxt = run_plain(bk, sc)
    _close(probs, sc.probs, 1e-5, "plain kernel: probabilities, hid %d" % hid)
    np.testing.assert_array_equal(acts, sc.acts)
    np.testing.assert_array_equal(nxt, _next_positions(sc, sc.acts))


def check_forward_matrix_core(bk, hid, plant=False):
    sc = scene(hid, plant)
    probs, acts, nxt = run_matrix_core(bk, sc)
    _close(probs, sc.probs, 1e-5, "matrix-core kernel: probabilities, hid %d%s" % (hid, ", planted weight" if plant else ""))
    np.testing.assert_array_equal(acts, sc.acts)
    np.testing.assert_array_equal(nxt, _next_positions(sc, sc.acts))
    if hid == 32 and not plant:                                       # the width both kernels take: the same bits out of both
        _, acts_p, nxt_p = run_plain(bk, sc)
        np.testing.assert_array_equal(acts, acts_p)
        np.testing.assert_array_equal(nxt, nxt_p)


# ---- Adam step -----------------------------------------------------------------------------------------------------------------
def actor_step(bk, bufs, d_x, x_stride, d_th, d_m, d_v, d_act, d_delta, ldy, d_mask, d_loss, S, N, B, in_dim, hid, ldp, ldb, alpha):
    """the launch sequence of engine._actor_step_wide"""
    g, L, st = ageom(in_dim, hid), bk.lib, bk.stream
    a1, a2, dz, dz3, lp = (bk.ptr(t) for t in bufs)
    th, m, v, mask = bk.ptr(d_th), bk.ptr(d_m), bk.ptr(d_v), bk.ptr(d_mask)
    adam = (float(alpha), float(np.float32(0.1)), float(np.float32(1 - 0.999)), float(np.float32(1e-7)), st)
    L.rcmarl_dense_forward(bk.ptr(d_x), x_stride, 0, 1, in_dim, th, 0, g["o_b1"], a1, S, N, B, in_dim, hid, ldp, ldb, st)
    L.rcmarl_dense_forward(a1, N * hid * ldb, hid * ldb, 0, ldb, th, g["o_W2"], g["o_b2"], a2, S, N, B, hid, hid, ldp, ldb, st)
    L.rcmarl_wide_actor_head(a2, th, bk.ptr(d_act), bk.ptr(d_delta), ldy, dz3, lp, S, N, B, in_dim, hid, A, ldp, ldb, st)
    L.rcmarl_dense_backward_data(dz3, th, g["o_W3"], a2, dz, S, N, B, hid, A, ldp, ldb, st)
    L.rcmarl_dense_backward_adam(a2, N * hid * ldb, hid * ldb, 0, ldb, dz3, th, m, v, g["o_W3"], mask, S, N, B, hid, A, ldp, ldb, *adam)
    L.rcmarl_dense_backward_data(dz, th, g["o_W2"], a1, a2, S, N, B, hid, hid, ldp, ldb, st)
    L.rcmarl_dense_backward_adam(a1, N * hid * ldb, hid * ldb, 0, ldb, dz, th, m, v, g["o_W2"], mask, S, N, B, hid, hid, ldp, ldb, *adam)
    L.rcmarl_dense_backward_adam(bk.ptr(d_x), x_stride, 0, 1, in_dim, a2, th, m, v, 0, mask, S, N, B, in_dim, hid, ldp, ldb, *adam)
    L.rcmarl_wide_actor_small_adam(a2, dz, dz3, lp, th, m, v, mask, bk.ptr(d_loss), S, N, B, in_dim, hid, A, ldp, ldb, *adam)


def check_adam_step(bk, B, hid, lr=0.002):
    """Two consecutive Adam steps (bias correction with t = 1 and t = 2) on the head kernel, the Adam epilogue and the small Adam
    kernel against the oracle's Keras Adam (oracle/keras_np.Model._train_step = mlp_np.sparse_ce_loss_and_dlogits, backward,
    adam_apply) from identical weights and slots: weights, m and v to 1e-6 max(1, |x|), the loss to rtol 1e-5.  One agent is masked."""
    S, N = S_, N_
    in_dim = 2 * N
    rng = np.random.default_rng(900 + 7 * B + hid)
    g = ageom(in_dim, hid)
    ldp, ldb, ldy = pad64(g["P"]), pad64(B), pad64(B) + 64
    params = actor_params(rng, S, N, in_dim, hid)
    theta = pack_rows(params, ldp)
    pos = rng.integers(0, NROW, size=(S, B, in_dim))
    x = ((pos - np.mean(np.arange(NROW))) / np.std(np.arange(NROW))).astype(np.float32)          # grid-world states
    act = rng.integers(0, A, size=(S, N, ldy)).astype(np.float32)
    delta = rng.normal(size=(S, N, ldy)).astype(np.float32)
    mask = np.ones(N, np.int32)
    mask[1] = 0
    z = lambda *sh: bk.dev(np.zeros(sh, np.float32))
    bufs = (z(S, N * hid, ldb), z(S, N * hid, ldb), z(S, N * hid, ldb), z(S, N * A, ldb), z(S, N, (B + 255) // 256))
    d_x, d_th, d_m, d_v = bk.dev(x), bk.dev(theta), bk.dev(np.zeros_like(theta)), bk.dev(np.zeros_like(theta))
    d_act, d_delta, d_mask, d_loss = bk.dev(act), bk.dev(delta), bk.dev(mask), z(S, N)
    oracle = [[(M.copy_params(params[s][n]), None) for n in range(N)] for s in range(S)]
    oracle = [[(p, M.AdamState(p, lr)) for p, _ in row] for row in oracle]
    worst = {"w": 0.0, "m": 0.0, "v": 0.0, "loss": 0.0}
    for t in (1, 2):
        alpha = np.float32(lr * np.sqrt(1.0 - 0.999 ** t) / (1.0 - 0.9 ** t))
        actor_step(bk, bufs, d_x, B * in_dim, d_th, d_m, d_v, d_act, d_delta, ldy, d_mask, d_loss, S, N, B, in_dim, hid, ldp, ldb, alpha)
        th, mm, vv, loss = bk.host(d_th), bk.host(d_m), bk.host(d_v), bk.host(d_loss)
        for s in range(S):
            for n in range(N):
                if not mask[n]:
                    np.testing.assert_array_equal(th[s, n], theta[s, n])
                    assert not mm[s, n].any() and not vv[s, n].any()
                    continue
                p, st = oracle[s][n]
                want_loss = M.fit_actor_ce(p, st, x[s], act[s, n, :B], delta[s, n, :B], epochs=1)[0]
                assert st.t == t
                rel = abs(float(loss[s, n]) - float(want_loss)) / abs(float(want_loss))
                worst["loss"] = max(worst["loss"], rel)
                for key, got_row, want in (("w", th, p), ("m", mm, st.m), ("v", vv, st.v)):
                    got = unpack_row(got_row[s, n], in_dim, A, hid)
                    for a_, b_ in zip(got, want):
                        worst[key] = max(worst[key], float((np.abs(a_ - b_) / np.maximum(1.0, np.abs(b_))).max()))
    print("[wide actor] Adam step B=%d hid=%d: worst |x - oracle| / max(1, |x|): weights %.2e, m %.2e, v %.2e (bar 1e-6); loss rel %.2e "
          "(bar 1e-5)" % (B, hid, worst["w"], worst["m"], worst["v"], worst["loss"]))
    assert worst["w"] <= 1e-6 and worst["m"] <= 1e-6 and worst["v"] <= 1e-6, worst
    assert worst["loss"] <= 1e-5, worst


# ---- engine ----------------------------------------------------------------------------------------------------------------------
def engine_args(n_episodes=4, seed=5):
    return EC.make_args([COOP] * 3, H=1, n_episodes=n_episodes, max_ep_len=3, n_ep_fixed=2, n_epochs=2, buffer_size=12, seed=seed,
                        in_nodes=CIRC3)


def make_cfg(actor_hid=32, critic_hid=20, rng_mode="numpy", n_seeds=2, **kw):
    base = dict(H=1, max_ep_len=3, n_ep_fixed=2, n_epochs=2, buffer_size=12, nrow=3, ncol=3, n_seeds=n_seeds, rng_mode=rng_mode,
                actor_hid=actor_hid, critic_hid=critic_hid)
    labels, in_nodes = kw.pop("labels", [COOP] * 3), kw.pop("in_nodes", CIRC3)
    base.update(kw)
    return EngineConfig(3, labels, in_nodes, **base)


def engine_inputs(seeds, actor_hid, critic_hid, weight_seed=3):
    rng = np.random.default_rng(weight_seed)
    W = [[{"actor": M.init_mlp(rng, 6, actor_hid, A), "critic": M.init_mlp(rng, 6, critic_hid, 1), "tr": M.init_mlp(rng, 9, 20, 1)}
          for _ in range(3)] for _ in seeds]
    goals = [np.random.default_rng(100 + s).integers(0, 3, size=(3, 2)) for s in range(len(seeds))]
    return W, goals


def make_engine(device, lib, seeds, W, goals, **kw):
    eng = RPBCACEngine(make_cfg(n_seeds=len(seeds), **kw), seeds=list(seeds), device=device, lib=lib)
    for s in range(len(seeds)):
        for i in range(3):
            for net in ("actor", "critic", "tr"):
                eng.set_weights(s, i, net, W[s][i][net])
    eng.set_goals(np.stack(goals))
    if eng.cfg.rng_mode == "numpy":
        eng.np_rngs = []
        for sd in seeds:
            r = np.random.RandomState(int(sd))
            r.randint([0, 0], [3, 3], size=(3, 2))                    # the env constructor's reset() draw (grid_world.py:28)
            eng.np_rngs.append(r)
    return eng


def check_oracle_runs_with_a_wide_actor():
    """oracle.train with a 32-unit actor on the CPU (its networks are lists of arrays of any width)"""
    args = engine_args()
    W, goals = engine_inputs((11,), 32, 20)
    o_logs, o_w = EC.run_oracle(args, 3, 3, "numpy", (11,), W, goals)
    assert o_w[0][0][0][0].shape == (6, 32) and len(o_logs[0]) == 4


def check_engine_vs_oracle(device, lib, critic_hid, seeds=(11, 12)):
    """two update blocks against oracle.train at engine_checks.compare's default bars; returns bit-identical while actions are"""
    args = engine_args()
    W, goals = engine_inputs(seeds, 32, critic_hid)
    o_logs, o_w = EC.run_oracle(args, 3, 3, "numpy", seeds, W, goals)
    eng = make_engine(device, lib, seeds, W, goals, actor_hid=32, critic_hid=critic_hid)
    assert eng.hid["actor"] == 32 and eng.P["actor"] == 6 * 32 + 32 + 32 * 32 + 32 + 32 * 5 + 5 and eng.ldp["actor"] == pad64(eng.P["actor"])
    assert eng.adam_m.shape[-1] == eng.ldp["actor"] and eng.get_all_weights("actor").shape == (len(seeds), 3, eng.P["actor"])
    logs = eng.train(args["n_episodes"])
    assert eng.adam_t == 2                                            # one Adam step per update block, as on the 20-unit path
    assert eng.wa_alias == (critic_hid != 20)
    EC.compare(eng, logs, o_logs, o_w)
    return eng


def check_engine_device_mode(device, lib, critic_hid=20):
    seeds = (21,)
    W, goals = engine_inputs(seeds, 32, critic_hid)
    out = []
    for _ in range(2):
        eng = make_engine(device, lib, seeds, W, goals, actor_hid=32, critic_hid=critic_hid, rng_mode="device", n_epochs=1)
        assert eng.actor_mx
        logs = eng.train(4)
        assert eng.adam_t == 2
        out.append((logs, {k: eng.get_all_weights(k) for k in ("actor", "critic", "tr")}, eng.adam_m.cpu().numpy(), eng.adam_v.cpu().numpy()))
    (la, wa, ma, va), (lb, wb, mb, vb) = out
    for k in la:
        assert np.isfinite(la[k]).all()
        np.testing.assert_array_equal(la[k], lb[k])
    for k in wa:
        assert np.isfinite(wa[k]).all()
        np.testing.assert_array_equal(wa[k], wb[k])
    np.testing.assert_array_equal(ma, mb)
    np.testing.assert_array_equal(va, vb)
    assert np.abs(ma).max() > 0


def check_checkpoints(device, lib, path):
    seeds = (31,)
    W, goals = engine_inputs(seeds, 32, 20)
    W20, _ = engine_inputs(seeds, 20, 20)
    mk = lambda: make_engine(device, lib, seeds, W, goals, actor_hid=32, rng_mode="device", n_epochs=1)
    a = mk()
    la = a.train(4)
    b = mk()
    lb = b.train(2)
    b.save_checkpoint(path)
    import torch
    assert torch.load(path, map_location="cpu", weights_only=True)["shape"]["actor_hid"] == 32
    c = mk()
    c.init_glorot(base_seed=99)                                       # everything must come from the file
    c.load_checkpoint(path)
    lc = c.train(2)
    for k in la:
        np.testing.assert_array_equal(la[k], np.concatenate([lb[k], lc[k]], axis=0))
    for net in a.theta:
        np.testing.assert_array_equal(a.get_all_weights(net), c.get_all_weights(net))
    np.testing.assert_array_equal(a.adam_m.cpu().numpy(), c.adam_m.cpu().numpy())
    np.testing.assert_array_equal(a.adam_v.cpu().numpy(), c.adam_v.cpu().numpy())
    assert a.adam_t == c.adam_t == 2
    # a 32-unit file is refused by a 20-unit engine and the reverse, in the existing message's shape
    narrow = make_engine(device, lib, seeds, W20, goals, actor_hid=20, rng_mode="device", n_epochs=1)
    with pytest.raises(ValueError, match=r"checkpoint does not match this engine: \{'actor_hid': \(32, 20\)\}"):
        narrow.load_checkpoint(path)
    narrow.train(2)
    narrow.save_checkpoint(path + ".20")
    with pytest.raises(ValueError, match=r"checkpoint does not match this engine: \{'actor_hid': \(20, 32\)\}"):
        mk().load_checkpoint(path + ".20")
    # a file written before actors could be wide carries no actor_hid: it is a 20-unit file
    sd = narrow.state_dict()
    del sd["shape"]["actor_hid"]
    torch.save(sd, path + ".old")
    again = make_engine(device, lib, seeds, W20, goals, actor_hid=20, rng_mode="device", n_epochs=1)
    again.load_checkpoint(path + ".old")
    np.testing.assert_array_equal(again.get_all_weights("actor"), narrow.get_all_weights("actor"))
    with pytest.raises(ValueError, match="actor_hid"):
        mk().load_checkpoint(path + ".old")


def check_refusals(device, lib):
    for lab in ("Greedy", "Malicious", "Faulty"):
        with pytest.raises(ValueError, match="wide actor"):
            make_cfg(labels=[COOP, COOP, lab])
    with pytest.raises(ValueError, match="irregular"):
        make_cfg(in_nodes=[[0, 1, 2], [1, 2, 0], [2, 0]], H=0)
    with pytest.raises(ValueError, match="irregular"):
        make_cfg(H=[1, 1, 0])
    with pytest.raises(ValueError, match="actor_hid must be positive"):
        make_cfg(actor_hid=0)
    make_cfg(actor_hid=20, labels=[COOP, COOP, "Greedy"])             # the 20-unit actor keeps every combination
    eng = RPBCACEngine(make_cfg(n_seeds=1, critic_hid=32), seeds=[1], device=device, lib=lib)
    with pytest.raises(ValueError, match="wide actor"):
        eng.shard_agents(rank=0, world=2)


class CountingLib:
    """the library with a launch counter per entry point in front"""

    def __init__(self, lib):
        self._lib, self.calls = lib, collections.Counter()

    def __getattr__(self, name):
        fn = getattr(self._lib, name)
        if not callable(fn):
            return fn

        def call(*args):
            self.calls[name] += 1
            return fn(*args)
        return call


def check_routing(device, lib):
    """rng_mode 'device': a multiple of 32 steps its episodes together on the matrix-core kernel; any other width goes episode by
    episode through the plain kernel (and trains: finite weights, one Adam step per block)"""
    seeds = (41,)
    for hid, mx in ((32, True), (24, False)):
        W, goals = engine_inputs(seeds, hid, 20)
        cl = CountingLib(lib)
        eng = make_engine(device, cl, seeds, W, goals, actor_hid=hid, rng_mode="device", n_epochs=1)
        assert eng.actor_mx == mx
        eng.train(2)                                                  # one block: 2 episodes of 3 steps
        c = cl.calls
        assert c["rcmarl_rollout_step_episodes"] == c["rcmarl_rollout_step"] == c["rcmarl_mid_actor"] == c["rcmarl_small_adam"] == 0
        assert (c["rcmarl_rollout_step_episodes_wide"], c["rcmarl_rollout_step_wide"]) == ((3, 0) if mx else (0, 6)), dict(c)
        assert c["rcmarl_dense_backward_adam"] == 3 and c["rcmarl_wide_actor_head"] == 1 and c["rcmarl_wide_actor_small_adam"] == 1
        assert eng.adam_t == 1 and np.isfinite(eng.get_all_weights("actor")).all()
    # the 20-unit actor takes exactly the launches it took before
    W, goals = engine_inputs(seeds, 20, 20)
    cl = CountingLib(lib)
    eng = make_engine(device, cl, seeds, W, goals, actor_hid=20, rng_mode="device", n_epochs=1)
    eng.train(2)
    c = cl.calls
    assert c["rcmarl_rollout_step_episodes"] == 3 and c["rcmarl_mid_actor"] == c["rcmarl_small_adam"] == c["rcmarl_layer1_backward_adam"] == 1
    assert not any(c[k] for k in ("rcmarl_rollout_step_episodes_wide", "rcmarl_rollout_step_wide", "rcmarl_policy_probs_wide",
                                  "rcmarl_dense_backward_adam", "rcmarl_wide_actor_head", "rcmarl_wide_actor_small_adam"))


def check_dropin(hook, seed=5):
    """The route a user takes: keras_compat.Sequential models -- the actor 32 units wide -- handed to RPBCAC_agent, a Grid_World and
    train_RPBCAC, which reads the actor's width off the model objects as it does for the critic; against oracle.train on the same
    NumPy stream (returns bit-identical, critic / team-reward net to 1e-4, the actor within 5 % of an Adam step per update)."""
    import dropin_checks as DC
    from rcmarl_amd import keras_compat as K
    from rcmarl_amd.agents.resilient_CAC_agents import RPBCAC_agent
    from rcmarl_amd.environments.grid_world import Grid_World
    from rcmarl_amd.training.train_agents import train_RPBCAC
    n = 3

    def mlp(width, hid, out, act):
        return K.Sequential([K.Input(shape=(n, width)), K.layers.Flatten(), K.layers.Dense(hid, activation=K.layers.LeakyReLU(alpha=0.1)),
                             K.layers.Dense(hid, activation=K.layers.LeakyReLU(alpha=0.1)), K.layers.Dense(out, activation=act)])

    def team(actor_hids):
        K.set_seed(seed)
        agents, W = [], []
        for h in actor_hids:
            actor, critic, tr = mlp(2, h, A, 'softmax'), mlp(2, 20, 1, None), mlp(3, 20, 1, None)
            W.append([actor.get_weights(), critic.get_weights(), tr.get_weights()])
            agents.append(RPBCAC_agent(actor, critic, tr, slow_lr=0.002, fast_lr=0.01, gamma=0.9, H=1))
        return agents, W
    agents, W = team([32] * n)
    assert W[0][0][0].shape == (6, 32)
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
        assert weights[i][0][0].shape == (6, 32)
        assert any(np.abs(a - b).max() > 0 for a, b in zip(weights[i][0], W[i][0]))        # the actor was trained
        for a, b in zip(weights[i][0], ow[i][0]):
            assert float(np.abs(a - b).max()) <= 0.05 * 0.002 * 2 + 1e-5, ("actor", i, float(np.abs(a - b).max()))
        for k in (1, 2):
            for a, b in zip(weights[i][k], ow[i][k]):
                DC.close(a, b, 1e-4, "wide actor drop-in agent %d net %d" % (i, k))
    mixed, _ = team([32, 24, 32])
    with pytest.raises(ValueError, match="all actors the same width"):
        train_RPBCAC(env, mixed, args, engine_hook=hook)


def check_argument_validation(lib):
    """bad calls of the new entry points come back as RCMARL_ERR_ARG / RCMARL_ERR_UNSUPPORTED before anything is launched"""
    q = lib.rcmarl_rollout_wide_supported
    assert [q(h) for h in (32, 96, 512, 24, 20, 544, 0, -32)] == [1, 1, 1, 0, 0, 0, 0, 0]
    bad = [
        ("rcmarl_policy_probs_wide", (None, None, None, 1, 3, 6, 32, 5, 1472, None)),
        ("rcmarl_rollout_step_wide", (None,) * 5 + (3, 3, None) + (None,) * 5 + (8, 0, None, None, None, 1.0, 0, 0, 0.1, 1, 3, 32, 5, 1472, None, None)),
        ("rcmarl_policy_probs_episodes_wide", (None, None, None, 1, 3, 5, 64, 32, 5, 1472, None)),
        ("rcmarl_rollout_step_episodes_wide", (None,) * 5 + (3, 3, None) + (None,) * 5 + (40, 0, 3, None, None, None, 1.0, 0, 0, 0.1, 1, 3, 5, 64, 32, 5,
                                                                                          1472, None)),
        ("rcmarl_dense_backward_adam", (None, 0, 0, 1, 6, None, None, None, None, 0, None, 1, 3, 7, 6, 32, 1472, 64, 0.002, 0.1, 0.001, 1e-7, None)),
        ("rcmarl_wide_actor_head", (None, None, None, None, 64, None, None, 1, 3, 7, 6, 32, 5, 1472, 64, None)),
        ("rcmarl_wide_actor_small_adam", (None,) * 9 + (1, 3, 7, 6, 32, 5, 1472, 64, 0.002, 0.1, 0.001, 1e-7, None)),
    ]
    for name, args in bad:
        with pytest.raises(capi.RcmarlError, match="RCMARL_ERR_ARG"):
            getattr(lib, name)(*args)
    # a width the matrix-core kernel does not serve: refused before any pointer is looked at (64 stands for "not NULL")
    p = 64
    for hid in (24, 544):
        with pytest.raises(capi.RcmarlError, match="RCMARL_ERR_UNSUPPORTED"):
            lib.rcmarl_rollout_step_episodes_wide(p, p, p, p, p, 3, 3, p, p, p, p, p, p, 40, 0, 3, p, p, p, 1.0, 0, 0, 0.1, 1, 3, 5, 64, hid, 5,
                                                  1472, None)
        with pytest.raises(capi.RcmarlError, match="RCMARL_ERR_UNSUPPORTED"):
            lib.rcmarl_policy_probs_episodes_wide(p, p, p, 1, 3, 5, 64, hid, 5, 1472, None)
