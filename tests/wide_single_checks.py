"""Per-agent classes at any hidden width -- checks shared by the hipemu, the GPU and the CPU-only C-ABI tests:
rcmarl_minibatch_actor_wide (csrc/minibatch_actor_wide.hip: one workgroup per (seed, adversary) chain, a mini-batch walked in 32-row
tiles, one Adam pass per mini-batch) against oracle/mlp_np.fit_actor_ce and against the nine-launch wide Adam step run once per
mini-batch, its query and refusals; and single.RowOps / keras_compat / the agent classes with nets of 24, 40 and 32 hidden units
against the oracle's agents, with the launches counted."""
import contextlib

import numpy as np
import pytest

import dropin_checks as DC
import wide_actor_checks as WAC
from kernel_checks import pad64, pack_rows, unpack_row
from oracle import mlp_np as M
from oracle import rpbcac_oracle as O
from rcmarl_amd import capi
from rcmarl_amd import keras_compat as K
from rcmarl_amd import single
from rcmarl_amd.agents import adversarial_CAC_agents as ADV
from rcmarl_amd.agents.resilient_CAC_agents import RPBCAC_agent

A = 5
S_, N_, ADVS = 2, 3, (0, 2)
LR = 0.002
B1, B2, EPS = 0.9, 0.999, 1e-7
# name -> hid, in_dim, B, batch_size, t0, shuffled
CASES = {
    "partial_tile": (24, 6, 100, 40, 0, True),         # row tiles 32 + 8; the last mini-batch is 20 rows
    "two_unit_tiles": (40, 6, 70, 32, 0, True),
    "two_chunks": (32, 70, 64, 32, 0, True),           # more inputs than one staged chunk
    "one_step": (24, 6, 50, 200, 0, True),             # batch_size >= B: exactly one wide Adam step
    "warm_slots": (24, 6, 100, 40, 7, True),           # t0 = 7, planted non-zero m, v
    "natural_order": (24, 6, 100, 40, 0, False),       # perm = NULL
    "reference_batch": (64, 6, 450, 200, 0, True),     # mini-batches 200, 200, 50; seven row tiles, the last of 8 rows (GPU only)
    "widest": (384, 6, 64, 32, 0, True),               # (GPU only)
}


def _alpha(t):
    return np.float32(LR * np.sqrt(1.0 - B2 ** t) / (1.0 - B1 ** t))


class _Case:
    """inputs of one kernel case and the oracle's result for every chain, computed once"""

    def __init__(self, name):
        self.name = name
        self.hid, self.in_dim, self.B, self.bs, self.t0, self.shuffle = CASES[name]
        hid, in_dim, B, S, N = self.hid, self.in_dim, self.B, S_, N_
        rng = np.random.default_rng(1300 + sorted(CASES).index(name))
        self.g = WAC.ageom(in_dim, hid)
        self.ldp, self.ldb = pad64(self.g["P"]), pad64(B)
        self.params = WAC.actor_params(rng, S, N, in_dim, hid)
        self.theta = pack_rows(self.params, self.ldp)
        pos = rng.integers(0, WAC.NROW, size=(S, B, in_dim))
        self.x = ((pos - np.mean(np.arange(WAC.NROW))) / np.std(np.arange(WAC.NROW))).astype(np.float32)       # grid-world states
        self.act = rng.integers(0, A, size=(S, N, self.ldb)).astype(np.float32)
        self.delta = rng.normal(size=(S, N, self.ldb)).astype(np.float32)
        self.perm = np.stack([[[rng.permutation(B)] for _ in ADVS] for _ in range(S)]).astype(np.int32)          # [S][n_adv][1][B]
        if self.t0:                                     # as kernel_checks.check_minibatch_actor plants them
            self.m0 = (0.01 * rng.normal(size=self.theta.shape)).astype(np.float32)
            self.v0 = (1e-4 * rng.random(size=self.theta.shape)).astype(np.float32)
            self.m0[:, :, self.g["P"]:] = 0
            self.v0[:, :, self.g["P"]:] = 0
        else:
            self.m0, self.v0 = np.zeros_like(self.theta), np.zeros_like(self.theta)
        self.nsteps = (B + min(self.bs, B) - 1) // min(self.bs, B)
        self.oracle = {}
        for s in range(S):
            for k, n in enumerate(ADVS):
                pw = M.copy_params(self.params[s][n])
                st = M.AdamState(pw, LR)
                st.t = self.t0
                st.m, st.v = unpack_row(self.m0[s, n], in_dim, A, hid), unpack_row(self.v0[s, n], in_dim, A, hid)
                loss = M.fit_actor_ce(pw, st, self.x[s], self.act[s, n, :B], self.delta[s, n, :B], epochs=1, batch_size=self.bs,
                                      perms=self.perm[s, k] if self.shuffle else None)[0]
                assert st.t == self.t0 + self.nsteps
                self.oracle[s, n] = (pw, st.m, st.v, float(loss))

    def order(self, s, k):
        return self.perm[s, k, 0] if self.shuffle else np.arange(self.B)


_CASES = {}


def case(name):
    if name not in _CASES:
        _CASES[name] = _Case(name)
    return _CASES[name]


def run_chain(bk, c):
    """one rcmarl_minibatch_actor_wide launch over all chains of the case -> theta, m, v, loss"""
    S, N = S_, N_
    assert bk.lib.rcmarl_minibatch_actor_wide_supported(c.in_dim, c.hid, A, c.bs) == 1
    d_x, d_th, d_m, d_v = bk.dev(c.x), bk.dev(c.theta), bk.dev(c.m0), bk.dev(c.v0)
    d_grad = bk.dev(np.full((S, len(ADVS), c.ldp), 3.0, np.float32))          # the kernel zeroes its scratch itself
    d_adv, d_act, d_delta, d_perm = bk.dev(np.asarray(ADVS, np.int32)), bk.dev(c.act), bk.dev(c.delta), bk.dev(c.perm)
    d_loss = bk.dev(np.zeros((S, N), np.float32))
    rc = bk.lib.rcmarl_minibatch_actor_wide(bk.ptr(d_x), c.B * c.in_dim, bk.ptr(d_th), bk.ptr(d_m), bk.ptr(d_v), bk.ptr(d_grad), bk.ptr(d_adv),
                                            len(ADVS), bk.ptr(d_act), bk.ptr(d_delta), bk.ptr(d_perm) if c.shuffle else None, S, N, c.B,
                                            c.in_dim, c.hid, A, c.ldp, c.ldb, c.bs, 1, LR, B1, B2, EPS, c.t0, bk.ptr(d_loss), bk.stream)
    assert rc in (0, None)
    return bk.host(d_th).copy(), bk.host(d_m).copy(), bk.host(d_v).copy(), bk.host(d_loss).copy()


def run_composition(bk, c):
    """the nine-launch wide Adam step (wide_actor_checks.actor_step: the launch sequence of engine._actor_step_wide) once per
    mini-batch on the gathered rows, chain by chain -> theta, m, v, loss in run_chain's layout"""
    th, mm, vv, loss = c.theta.copy(), c.m0.copy(), c.v0.copy(), np.zeros((S_, N_), np.float32)
    z = lambda *sh: bk.dev(np.zeros(sh, np.float32))
    d_mask = bk.dev(np.ones(1, np.int32))
    for s in range(S_):
        for k, n in enumerate(ADVS):
            d_th, d_m, d_v = (bk.dev(a[s:s + 1, n:n + 1]) for a in (th, mm, vv))
            order, tot = c.order(s, k), 0.0
            bs = min(c.bs, c.B)
            for step, lo in enumerate(range(0, c.B, bs)):
                idx = order[lo:lo + bs]
                nb, ldn = len(idx), pad64(len(idx))
                row = lambda a: np.concatenate([a[s, n, idx], np.zeros(ldn - nb, np.float32)]).reshape(1, 1, ldn)
                bufs = (z(1, c.hid, ldn), z(1, c.hid, ldn), z(1, c.hid, ldn), z(1, A, ldn), z(1, 1, (nb + 255) // 256))
                d_loss = z(1, 1)
                WAC.actor_step(bk, bufs, bk.dev(c.x[s][idx]), nb * c.in_dim, d_th, d_m, d_v, bk.dev(row(c.act)), bk.dev(row(c.delta)), ldn,
                               d_mask, d_loss, 1, 1, nb, c.in_dim, c.hid, c.ldp, ldn, _alpha(c.t0 + step + 1))
                tot += float(bk.host(d_loss)[0, 0]) * nb
            th[s, n], mm[s, n], vv[s, n] = bk.host(d_th)[0, 0], bk.host(d_m)[0, 0], bk.host(d_v)[0, 0]
            loss[s, n] = tot / c.B
    return th, mm, vv, loss


def _deviation(c, th, mm, vv):
    """worst |x - oracle| / max(1, |x|) over the chains: weights, m, v"""
    worst = {"w": 0.0, "m": 0.0, "v": 0.0}
    for (s, n), (pw, om, ov, _) in c.oracle.items():
        for key, rows, want in (("w", th, pw), ("m", mm, om), ("v", vv, ov)):
            for a_, b_ in zip(unpack_row(rows[s, n], c.in_dim, A, c.hid), want):
                worst[key] = max(worst[key], float((np.abs(a_ - b_) / np.maximum(1.0, np.abs(b_))).max()))
    return worst


def check_kernel(bk, name):
    """The chain against oracle/mlp_np.fit_actor_ce: weights to 0.02 lr nsteps + 1e-6 (kernel_checks.check_minibatch_actor's bar),
    the first-epoch loss to 2e-5 relative; `one_step` also to check_adam_step's bars (weights, m, v 1e-6 max(1, |x|), loss 1e-5).
    m and v after several steps: the chain may be at most twice as far from the oracle as the nine-launch composition, plus 1e-6
    (the same fp32 arithmetic in another summation order).  Rows of the agent that is no adversary: bit-unchanged.  Two runs from
    the same state: bit-identical."""
    c = case(name)
    th, mm, vv, loss = run_chain(bk, c)
    th2, mm2, vv2, loss2 = run_chain(bk, c)
    for a_, b_ in ((th, th2), (mm, mm2), (vv, vv2), (loss, loss2)):
        np.testing.assert_array_equal(a_, b_)
    for n in range(N_):
        if n not in ADVS:
            np.testing.assert_array_equal(th[:, n], c.theta[:, n])
            np.testing.assert_array_equal(mm[:, n], c.m0[:, n])
            np.testing.assert_array_equal(vv[:, n], c.v0[:, n])
    assert not np.array_equal(th[:, ADVS[0]], c.theta[:, ADVS[0]])
    cth, cmm, cvv, closs = run_composition(bk, c)
    dev, cdev = _deviation(c, th, mm, vv), _deviation(c, cth, cmm, cvv)
    worst_abs, worst_loss, worst_closs = 0.0, 0.0, 0.0
    for (s, n), (pw, _, _, want) in c.oracle.items():
        for a_, b_ in zip(unpack_row(th[s, n], c.in_dim, A, c.hid), pw):
            worst_abs = max(worst_abs, float(np.abs(a_ - b_).max()))
        worst_loss = max(worst_loss, abs(float(loss[s, n]) - want) / abs(want))
        worst_closs = max(worst_closs, abs(float(closs[s, n]) - want) / abs(want))
    print("[wide actor fit] %s hid=%d in=%d B=%d bs=%d (%d Adam steps): worst |x - oracle| / max(1, |x|): chain weights %.2e, m %.2e, v %.2e; "
          "nine-launch composition weights %.2e, m %.2e, v %.2e; weights |w - oracle| %.2e (bar %.2e); loss rel: chain %.2e, composition "
          "%.2e (bar 2e-5)" % (name, c.hid, c.in_dim, c.B, c.bs, c.nsteps, dev["w"], dev["m"], dev["v"], cdev["w"], cdev["m"], cdev["v"],
                               worst_abs, 0.02 * LR * c.nsteps + 1e-6, worst_loss, worst_closs))
    assert worst_abs <= 0.02 * LR * c.nsteps + 1e-6, worst_abs
    assert worst_loss <= 2e-5, worst_loss
    if c.nsteps == 1:
        assert dev["w"] <= 1e-6 and dev["m"] <= 1e-6 and dev["v"] <= 1e-6, dev
        assert worst_loss <= 1e-5, worst_loss
    for key in ("m", "v"):
        assert dev[key] <= 2.0 * cdev[key] + 1e-6, (key, dev, cdev)


# ---- query and refusals (no GPU needed) ----------------------------------------------------------------------------------------------
def check_query(lib):
    q = lib.rcmarl_minibatch_actor_wide_supported
    for in_dim in (6, 70, 2048):
        for hid in (1, 24, 32, 256, 384):
            for bs in (32, 200):
                assert q(in_dim, hid, A, bs) == 1, (in_dim, hid, bs)
    for args in ((0, 64, A, 200), (6, 0, A, 200), (6, 64, 0, 200), (6, 64, A, 0), (-6, 64, A, 200), (6, -64, A, 200), (6, 64, -A, 200),
                 (6, 64, A, -200), (6, 64, 1, 200), (6, 64, 9, 200), (6, 1 << 30, A, 200)):
        assert q(*args) == 0, args
    assert q(6, 64, 2, 1) == 1 and q(6, 64, 8, 1) == 1


def check_argument_validation(lib):
    """bad calls come back as RCMARL_ERR_ARG / RCMARL_ERR_UNSUPPORTED before the HIP runtime is touched (64 stands for "not NULL")"""
    p = 64
    hid, in_dim, B = 32, 6, 100
    ldp, ldb = pad64(WAC.ageom(in_dim, hid)["P"]), pad64(B)

    def call(x=p, th=p, m=p, v=p, grad=p, agents=p, n_adv=2, act=p, delta=p, S=2, N=3, B=B, in_dim=in_dim, hid=hid, n_actions=A, ldp=ldp,
             ldb=ldb, bs=200, epochs=1, t0=0):
        return lib.rcmarl_minibatch_actor_wide(x, B * in_dim, th, m, v, grad, agents, n_adv, act, delta, None, S, N, B, in_dim, hid, n_actions,
                                               ldp, ldb, bs, epochs, LR, B1, B2, EPS, t0, None, None)
    for kw in (dict(x=None), dict(th=None), dict(m=None), dict(v=None), dict(grad=None), dict(agents=None), dict(act=None), dict(delta=None),
               dict(n_adv=0), dict(S=0), dict(N=0), dict(B=0), dict(in_dim=0), dict(hid=0), dict(n_actions=0), dict(bs=0), dict(epochs=0),
               dict(t0=-1), dict(ldp=ldp + 32), dict(ldp=ldp - 64), dict(ldb=B - 1)):
        with pytest.raises(capi.RcmarlError, match="RCMARL_ERR_ARG"):
            call(**kw)
    wide_ldp = pad64(WAC.ageom(in_dim, 600)["P"])
    for kw in (dict(hid=600, ldp=wide_ldp), dict(n_actions=1), dict(n_actions=9), dict(hid=1 << 30)):
        with pytest.raises(capi.RcmarlError, match="RCMARL_ERR_UNSUPPORTED"):
            call(**kw)


# ---- the per-agent classes ---------------------------------------------------------------------------------------------------------------
HIDS = {"actor": 32, "critic": 24, "tr": 40}           # all three differ from 20 and from each other


def make_models(n_agents, weights=None, hids=None):
    """dropin_checks.make_models with the widths of HIDS"""
    hids = HIDS if hids is None else hids

    def mlp(width, hid, out, act):
        return K.Sequential([K.Input(shape=(n_agents, width)), K.layers.Flatten(), K.layers.Dense(hid, activation=K.layers.LeakyReLU(alpha=0.1)),
                             K.layers.Dense(hid, activation=K.layers.LeakyReLU(alpha=0.1)), K.layers.Dense(out, activation=act)])
    trio = [mlp(2, hids["actor"], A, 'softmax'), mlp(2, hids["critic"], 1, None), mlp(3, hids["tr"], 1, None)]
    if weights is not None:
        for m, w in zip(trio, weights):
            m.set_weights(w)
    return trio


@contextlib.contextmanager
def wide_models():
    """dropin_checks' method checks build their models through its module-level make_models: hand them the wide ones"""
    saved, DC.make_models = DC.make_models, make_models
    try:
        yield
    finally:
        DC.make_models = saved


def check_agent_methods(B=100):
    """every RPBCAC_agent method on wide models: dropin_checks.check_agent_methods, its tolerances unchanged"""
    with wide_models():
        DC.check_agent_methods(H=1, n=5, B=B)


def check_adversary_methods(B=100):
    """every adversary method on wide models: dropin_checks.check_adversary_methods, its tolerances unchanged"""
    with wide_models():
        DC.check_adversary_methods(n=5, B=B)


def _batch(rng, B, n):
    s = rng.normal(size=(B, n, 2)).astype(np.float32)
    ns = rng.normal(size=(B, n, 2)).astype(np.float32)
    a = rng.integers(0, A, size=(B, n, 1)).astype(np.float32)
    r = rng.normal(size=(B, 1)).astype(np.float32)
    return s, ns, a, r


def _adversaries(n):
    """the three adversary classes on wide models, each beside its oracle twin"""
    out = []
    for cls, ocls, fast in ((ADV.Faulty_CAC_agent, O.FaultyAgent, False), (ADV.Greedy_CAC_agent, O.GreedyAgent, True),
                            (ADV.Malicious_CAC_agent, O.MaliciousAgent, True)):
        actor, critic, tr = make_models(n)
        kw = dict(fast_lr=0.01) if fast else {}
        out.append((cls(actor, critic, tr, slow_lr=LR, gamma=0.9, **kw),
                    ocls(actor.get_weights(), critic.get_weights(), tr.get_weights(), LR, gamma=0.9, **kw), actor))
    return out


def check_adversary_actor_updates(B, n=5, seed=21):
    """actor_update of Faulty / Greedy / Malicious agents with a 32-unit actor and a 24-unit critic, twice in a row (the Adam slots
    persist): B <= 200 takes the rows in their natural order as the reference does, B > 200 the shuffle of set_shuffle_seed.  Loss to
    dropin_checks' 5e-5, weights to kernel_checks.check_minibatch_actor's 0.02 lr nsteps + 1e-6."""
    rng = np.random.default_rng(seed + B)
    K.set_seed(seed)
    s, ns, a, r = _batch(rng, B, n)
    ADV.set_shuffle_seed(77)
    sh = O.ShuffleStream(77)
    nsteps = 2 * ((B + 199) // 200)
    for ag, ref, actor in _adversaries(n):
        for _ in range(2):
            la = ag.actor_update(s, ns, r, a[:, 0])
            lw = ref.actor_step(s, ns, r, a[:, 0], sh)
            assert abs(la - lw) <= 5e-5 * max(1, abs(lw)), (type(ag).__name__, la, lw)
        assert ag._adam["t"] == ref.adam.t == nsteps
        for x, y in zip(actor.get_weights(), ref.actor):
            assert x.shape == y.shape and float(np.abs(x - y).max()) <= 0.02 * LR * nsteps + 1e-6, (type(ag).__name__, float(np.abs(x - y).max()))
    assert ADV._shuffle["calls"] == sh.calls == (6 if B > 200 else 0)


def check_keras_compat_views(B=7, n=5, seed=4):
    """model(x) and predict of keras_compat models of 24, 40 and 32 units"""
    rng = np.random.default_rng(seed)
    K.set_seed(seed)
    actor, critic, tr = make_models(n)
    s = rng.normal(size=(B, n, 2)).astype(np.float32)
    sa = rng.normal(size=(B, n, 3)).astype(np.float32)
    assert actor.get_weights()[0].shape == (2 * n, 32) and critic.get_weights()[2].shape == (24, 24) and tr.get_weights()[4].shape == (40, 1)
    for model, x in ((critic, s), (tr, sa)):
        want = M.forward(model.get_weights(), x.reshape(B, -1))
        DC.close(model(x), want, 1e-5, "wide model(x)")
        DC.close(model.predict(x), want, 1e-5, "wide model.predict")
    want = M.softmax(M.forward(actor.get_weights(), s.reshape(B, -1)))
    DC.close(actor.predict(s), want, 1e-5, "wide actor.predict")
    DC.close(actor(s), want, 1e-5, "wide actor(x)")


def check_minibatch_fit_host_loop(B=40, n=5, seed=8):
    """a 600-unit critic is beyond both one-launch mini-batch kernels: the Greedy agent's fit takes one SGD step per mini-batch on
    the gathered rows, against M.fit_mse (through the oracle's GreedyAgent) at dropin_checks' 5e-5"""
    ops = single.get_ops()
    assert ops.lib.rcmarl_minibatch_fit_wide_supported(2 * n, 600, 32) == 0 and ops.lib.rcmarl_minibatch_fit_wide2_supported(2 * n, 600, 32) == 0
    rng = np.random.default_rng(seed)
    K.set_seed(seed)
    s, ns, _, r = _batch(rng, B, n)
    actor, critic, tr = make_models(n, hids=dict(HIDS, critic=600))
    cl = WAC.CountingLib(ops.lib)
    ops.lib = cl
    try:
        g = ADV.Greedy_CAC_agent(actor, critic, tr, slow_lr=LR, fast_lr=0.01, gamma=0.9)
        g._fit32 = lambda model, x, y: _fit_one_epoch(g, model, x, y)
        ref = O.GreedyAgent(actor.get_weights(), critic.get_weights(), tr.get_weights(), LR, 0.01, 0.9)
        ADV.set_shuffle_seed(5)
        sh = O.ShuffleStream(5)
        got, lg = g.critic_update_local(s, ns, r)
        target = r + np.float32(0.9) * M.forward(ref.critic, ns.reshape(B, -1))
        lw = M.fit_mse(ref.critic, s.reshape(B, -1), target, 0.01, epochs=1, batch_size=32, perms=sh.perms(1, B))[0]
    finally:
        ops.lib = cl._lib
    for p, q in zip(got, ref.critic):
        DC.close(p, q, 5e-5, "600-unit critic, host-loop mini-batch fit")
    assert abs(lg - lw) <= 5e-5 * max(1, abs(lw)), (lg, lw)
    assert cl.calls["rcmarl_minibatch_fit_wide"] == cl.calls["rcmarl_minibatch_fit_wide2"] == cl.calls["rcmarl_minibatch_fit"] == 0
    assert cl.calls["rcmarl_wide_head_fit"] == cl.calls["rcmarl_wide_small_sgd"] == 2, dict(cl.calls)          # mini-batches of 32 and 8 rows


def _fit_one_epoch(agent, model, x, y):
    """_Adversary._fit32 with epochs = 1 (the host loop at ten epochs is ten times the same code)"""
    B = int(np.asarray(x).shape[0])
    new, loss = single.get_ops().minibatch_fit(model.get_weights(), x, y, agent.fast_lr, batch_size=32, epochs=1, perms=ADV._perms(1, B))
    model.set_weights(new)
    return new, loss


WIDE_ONLY = ("rcmarl_dense_forward", "rcmarl_dense_backward_data", "rcmarl_dense_backward_sgd", "rcmarl_dense_backward_adam",
             "rcmarl_wide_head_value", "rcmarl_wide_head_fit", "rcmarl_wide_bias_grad", "rcmarl_wide_small_sgd", "rcmarl_wide_consensus_head",
             "rcmarl_wide_head_apply", "rcmarl_wide_actor_head", "rcmarl_wide_actor_small_adam", "rcmarl_policy_probs_wide",
             "rcmarl_minibatch_fit_wide", "rcmarl_minibatch_fit_wide2", "rcmarl_minibatch_actor_wide", "rcmarl_minibatch_actor_wide_supported",
             "rcmarl_minibatch_fit_wide_supported", "rcmarl_minibatch_fit_wide2_supported")
NARROW_ONLY = ("rcmarl_layer1_forward", "rcmarl_mid_value", "rcmarl_mid_fit", "rcmarl_small_sgd", "rcmarl_layer1_backward_sgd", "rcmarl_mid_actor",
               "rcmarl_small_adam", "rcmarl_layer1_backward_adam", "rcmarl_consensus_head", "rcmarl_projection_residual", "rcmarl_head_apply",
               "rcmarl_policy_probs", "rcmarl_minibatch_fit", "rcmarl_minibatch_actor")


def check_launch_counts(B=450, n=5, seed=12):
    """A counting proxy around the library: a wide adversary's actor_update is ONE rcmarl_minibatch_actor_wide launch after the two
    value passes of its TD error (two dense forward GEMMs and a head each) and touches no 20-unit entry point; the same calls on
    20-unit models touch only the 20-unit entry points, in today's numbers."""
    ops = single.get_ops()
    rng = np.random.default_rng(seed)
    K.set_seed(seed)
    s, ns, a, r = _batch(rng, B, n)
    sa = np.concatenate([s, a], axis=-1)
    real = ops.lib
    try:
        # wide
        ops.lib = cl = WAC.CountingLib(real)
        actor, critic, tr = make_models(n)
        ADV.set_shuffle_seed(3)
        ADV.Greedy_CAC_agent(actor, critic, tr, slow_lr=LR, fast_lr=0.01, gamma=0.9).actor_update(s, ns, r, a[:, 0])
        c = cl.calls
        assert c["rcmarl_minibatch_actor_wide"] == 1 and c["rcmarl_dense_forward"] == 4 and c["rcmarl_wide_head_value"] == 2, dict(c)
        assert c["rcmarl_shuffle_perms"] == 1 and c["rcmarl_wide_actor_head"] == c["rcmarl_dense_backward_adam"] == 0, dict(c)
        assert not any(c[k] for k in NARROW_ONLY), dict(c)
        cl.calls.clear()
        ag = RPBCAC_agent(actor, critic, tr, slow_lr=LR, fast_lr=0.01, gamma=0.9, H=1)
        ag.actor_update(s, ns, sa, a[:, 0])
        assert c["rcmarl_dense_forward"] == 3 * 2 + 2 and c["rcmarl_wide_head_value"] == 3 and c["rcmarl_wide_actor_head"] == 1, dict(c)
        assert c["rcmarl_dense_backward_data"] == 2 and c["rcmarl_dense_backward_adam"] == 3 and c["rcmarl_wide_actor_small_adam"] == 1, dict(c)
        ag.critic_update_local(s, ns, r)
        assert c["rcmarl_wide_head_fit"] == c["rcmarl_wide_bias_grad"] == c["rcmarl_wide_small_sgd"] == 5 and c["rcmarl_dense_backward_sgd"] == 10, dict(c)
        assert not any(c[k] for k in NARROW_ONLY), dict(c)
        # 20 units
        ops.lib = cl = WAC.CountingLib(real)
        actor, critic, tr = DC.make_models(n)
        ADV.Greedy_CAC_agent(actor, critic, tr, slow_lr=LR, fast_lr=0.01, gamma=0.9).actor_update(s, ns, r, a[:, 0])
        c = cl.calls
        assert c["rcmarl_minibatch_actor"] == 1 and c["rcmarl_layer1_forward"] == 2 and c["rcmarl_mid_value"] == 2 and c["rcmarl_shuffle_perms"] == 1, dict(c)
        ag = RPBCAC_agent(actor, critic, tr, slow_lr=LR, fast_lr=0.01, gamma=0.9, H=1)
        ag.actor_update(s, ns, sa, a[:, 0])
        ag.critic_update_local(s, ns, r)
        assert c["rcmarl_mid_actor"] == c["rcmarl_small_adam"] == c["rcmarl_layer1_backward_adam"] == 1, dict(c)
        assert c["rcmarl_mid_fit"] == c["rcmarl_small_sgd"] == c["rcmarl_layer1_backward_sgd"] == 5, dict(c)
        assert not any(c[k] for k in WIDE_ONLY), dict(c)
    finally:
        ops.lib = real
