"""Wide actors beside adversaries in the batched engine -- checks shared by the hipemu, the GPU and the CPU-only C-ABI tests:
rcmarl_minibatch_actor_wide2 (csrc/minibatch_actor_wide.hip, the two-image layout: 385 .. 576 units) against
oracle/mlp_np.fit_actor_ce and the nine-launch composition at the bars of wide_single_checks.check_kernel, its query (never 1
together with rcmarl_minibatch_actor_wide_supported) and refusals; and EngineConfig(adv_actor=...): Greedy / Malicious / Faulty agents
beside 32-, 24- and 416-unit actors against oracle.train with the route of every phase-III fit counted, the cooperative step's mask,
checkpoints, construction and the drop-in trainer."""
import collections

import numpy as np
import pytest

import dropin_checks as DC
import engine_checks as EC
import wide_actor_checks as WAC
import wide_single_checks as WS
from kernel_checks import pad64, pack_rows, unpack_row
from oracle import mlp_np as M
from oracle import rpbcac_oracle as O
from rcmarl_amd import capi
from rcmarl_amd import engine_adversaries as EA
from rcmarl_amd.engine import EngineConfig, RPBCACEngine

A, S_, N_, ADVS, LR = WS.A, WS.S_, WS.N_, WS.ADVS, WS.LR
B1, B2, EPS = WS.B1, WS.B2, WS.EPS
COOP, FAULTY, GREEDY, MAL = "Cooperative", "Faulty", "Greedy", "Malicious"
# name -> hid, in_dim, B, batch_size, t0, shuffled, data seed
CASES = {
    "partial_unit_tile": (400, 6, 70, 32, 0, True, 1),      # 13 unit tiles on four wavefronts (wavefront 0 owns four); row tiles 32 + 6
    # exactly one Adam step.  The sample weights carry both signs, so the loss cancels: the data seed is the first of 1, 2, ... at
    # which every chain's oracle loss has |loss| >= ONE_STEP_MIN_LOSS (asserted by the check), so that the 1e-5 bar on the loss
    # tests the kernel and not the oracle's own fp32 rounding
    "one_step": (416, 6, 50, 200, 0, True, 1),
    "two_chunks": (416, 70, 64, 32, 0, True, 1),            # more inputs than one staged chunk
    "warm_natural": (400, 6, 70, 32, 7, False, 1),          # t0 = 7, planted non-zero m and v, perm = NULL
    "widest": (576, 6, 64, 32, 0, True, 1),                 # the LDS limit: 18 unit tiles, five on two of the wavefronts
}
ONE_STEP_MIN_LOSS = 1e-2


class _Case:
    """wide_single_checks._Case for the shapes above: inputs of one kernel case and the oracle's result for every chain, once"""

    def __init__(self, name):
        self.name = name
        self.hid, self.in_dim, self.B, self.bs, self.t0, self.shuffle, seed = CASES[name]
        hid, in_dim, B, S, N = self.hid, self.in_dim, self.B, S_, N_
        rng = np.random.default_rng([1600, seed, hid, in_dim, B])
        self.g = WAC.ageom(in_dim, hid)
        self.ldp, self.ldb = pad64(self.g["P"]), pad64(B)
        self.params = WAC.actor_params(rng, S, N, in_dim, hid)
        self.theta = pack_rows(self.params, self.ldp)
        pos = rng.integers(0, WAC.NROW, size=(S, B, in_dim))
        self.x = ((pos - np.mean(np.arange(WAC.NROW))) / np.std(np.arange(WAC.NROW))).astype(np.float32)       # grid-world states
        self.act = rng.integers(0, A, size=(S, N, self.ldb)).astype(np.float32)
        self.delta = rng.normal(size=(S, N, self.ldb)).astype(np.float32)
        self.perm = np.stack([[[rng.permutation(B)] for _ in ADVS] for _ in range(S)]).astype(np.int32)          # [S][n_adv][1][B]
        if self.t0:
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


def run_chain(bk, c, entry="rcmarl_minibatch_actor_wide2"):
    """one launch of `entry` over all chains of the case -> theta, m, v, loss"""
    S, N = S_, N_
    d_x, d_th, d_m, d_v = bk.dev(c.x), bk.dev(c.theta), bk.dev(c.m0), bk.dev(c.v0)
    d_grad = bk.dev(np.full((S, len(ADVS), c.ldp), 3.0, np.float32))          # the kernel zeroes its scratch itself
    d_adv, d_act, d_delta, d_perm = bk.dev(np.asarray(ADVS, np.int32)), bk.dev(c.act), bk.dev(c.delta), bk.dev(c.perm)
    d_loss = bk.dev(np.zeros((S, N), np.float32))
    rc = getattr(bk.lib, entry)(bk.ptr(d_x), c.B * c.in_dim, bk.ptr(d_th), bk.ptr(d_m), bk.ptr(d_v), bk.ptr(d_grad), bk.ptr(d_adv),
                                len(ADVS), bk.ptr(d_act), bk.ptr(d_delta), bk.ptr(d_perm) if c.shuffle else None, S, N, c.B,
                                c.in_dim, c.hid, A, c.ldp, c.ldb, c.bs, 1, LR, B1, B2, EPS, c.t0, bk.ptr(d_loss), bk.stream)
    assert rc in (0, None)
    return bk.host(d_th).copy(), bk.host(d_m).copy(), bk.host(d_v).copy(), bk.host(d_loss).copy()


def check_one_step_loss_is_well_conditioned():
    """the input condition of the one-step case's 1e-5 loss bar (CPU only)"""
    c = case("one_step")
    assert c.nsteps == 1
    worst = min(abs(want) for (_, _, _, want) in c.oracle.values())
    assert worst >= ONE_STEP_MIN_LOSS, worst


def check_kernel(bk, name):
    """wide_single_checks.check_kernel on rcmarl_minibatch_actor_wide2: the chain against oracle/mlp_np.fit_actor_ce -- weights to
    0.02 lr nsteps + 1e-6, the first-epoch loss to 2e-5 relative; m and v at most twice as far from the oracle as the nine-launch
    composition, plus 1e-6; the one-step case also to 1e-6 max(1, |x|) on weights, m and v and 1e-5 on the loss.  Rows of the agent
    that is no adversary: bit-unchanged.  Two runs from the same state: bit-identical."""
    c = case(name)
    assert bk.lib.rcmarl_minibatch_actor_wide2_supported(c.in_dim, c.hid, A, c.bs) == 1
    assert bk.lib.rcmarl_minibatch_actor_wide_supported(c.in_dim, c.hid, A, c.bs) == 0
    if c.nsteps == 1:
        check_one_step_loss_is_well_conditioned()
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
    cth, cmm, cvv, closs = WS.run_composition(bk, c)
    dev, cdev = WS._deviation(c, th, mm, vv), WS._deviation(c, cth, cmm, cvv)
    worst_abs, worst_loss, worst_closs = 0.0, 0.0, 0.0
    for (s, n), (pw, _, _, want) in c.oracle.items():
        for a_, b_ in zip(unpack_row(th[s, n], c.in_dim, A, c.hid), pw):
            worst_abs = max(worst_abs, float(np.abs(a_ - b_).max()))
        worst_loss = max(worst_loss, abs(float(loss[s, n]) - want) / abs(want))
        worst_closs = max(worst_closs, abs(float(closs[s, n]) - want) / abs(want))
    print("[wide2 actor fit] %s hid=%d in=%d B=%d bs=%d (%d Adam steps): worst |x - oracle| / max(1, |x|): chain weights %.2e, m %.2e, v %.2e; "
          "nine-launch composition weights %.2e, m %.2e, v %.2e; weights |w - oracle| %.2e (bar %.2e); loss rel: chain %.2e, composition "
          "%.2e (bar %s)" % (name, c.hid, c.in_dim, c.B, c.bs, c.nsteps, dev["w"], dev["m"], dev["v"], cdev["w"], cdev["m"], cdev["v"],
                             worst_abs, 0.02 * LR * c.nsteps + 1e-6, worst_loss, worst_closs, "1e-5" if c.nsteps == 1 else "2e-5"))
    assert worst_abs <= 0.02 * LR * c.nsteps + 1e-6, worst_abs
    assert worst_loss <= 2e-5, worst_loss
    if c.nsteps == 1:
        assert dev["w"] <= 1e-6 and dev["m"] <= 1e-6 and dev["v"] <= 1e-6, dev
        assert worst_loss <= 1e-5, worst_loss
    for key in ("m", "v"):
        assert dev[key] <= 2.0 * cdev[key] + 1e-6, (key, dev, cdev)


# ---- query and refusals (no GPU needed) ----------------------------------------------------------------------------------------------
def check_query(lib):
    q2, q1 = lib.rcmarl_minibatch_actor_wide2_supported, lib.rcmarl_minibatch_actor_wide_supported
    assert [q2(6, h, A, 200) for h in (384, 385, 576, 577)] == [0, 1, 1, 0]
    assert q2(6, 512, 1, 200) == 0 and q2(6, 512, 9, 200) == 0 and q2(6, 512, 2, 1) == 1 and q2(6, 512, 8, 1) == 1
    for args in ((0, 512, A, 200), (6, 0, A, 200), (6, 512, 0, 200), (6, 512, A, 0), (-6, 512, A, 200), (6, -512, A, 200), (6, 512, -A, 200),
                 (6, 512, A, -200), (6, 1 << 30, A, 200)):
        assert q2(*args) == 0, args
    for in_dim in (6, 70, 2048):
        for hid in (1, 24, 384, 385, 512, 576, 577, 600):
            for bs in (32, 200):
                a, b = q1(in_dim, hid, A, bs), q2(in_dim, hid, A, bs)
                assert a in (0, 1) and b in (0, 1) and a + b <= 1, (in_dim, hid, bs)
                assert b == (1 if 385 <= hid <= 576 else 0) and a == (1 if hid <= 384 else 0), (in_dim, hid, bs)


def check_argument_validation(lib):
    """wide_single_checks.check_argument_validation on the new entry point: bad calls come back as RCMARL_ERR_ARG /
    RCMARL_ERR_UNSUPPORTED before the HIP runtime is touched (64 stands for "not NULL")"""
    p = 64
    hid, in_dim, B = 416, 6, 100
    ldp, ldb = pad64(WAC.ageom(in_dim, hid)["P"]), pad64(B)

    def call(x=p, th=p, m=p, v=p, grad=p, agents=p, n_adv=2, act=p, delta=p, S=2, N=3, B=B, in_dim=in_dim, hid=hid, n_actions=A, ldp=ldp,
             ldb=ldb, bs=200, epochs=1, t0=0):
        return lib.rcmarl_minibatch_actor_wide2(x, B * in_dim, th, m, v, grad, agents, n_adv, act, delta, None, S, N, B, in_dim, hid, n_actions,
                                                ldp, ldb, bs, epochs, LR, B1, B2, EPS, t0, None, None)
    for kw in (dict(x=None), dict(th=None), dict(m=None), dict(v=None), dict(grad=None), dict(agents=None), dict(act=None), dict(delta=None),
               dict(n_adv=0), dict(S=0), dict(N=0), dict(B=0), dict(in_dim=0), dict(hid=0), dict(n_actions=0), dict(bs=0), dict(epochs=0),
               dict(t0=-1), dict(ldp=ldp + 32), dict(ldp=ldp - 64), dict(ldb=B - 1)):
        with pytest.raises(capi.RcmarlError, match="RCMARL_ERR_ARG"):
            call(**kw)
    for h in (32, 384, 600):                           # the sibling's widths and a width beyond both layouts
        with pytest.raises(capi.RcmarlError, match="RCMARL_ERR_UNSUPPORTED"):
            call(hid=h, ldp=pad64(WAC.ageom(in_dim, h)["P"]))
    for kw in (dict(n_actions=1), dict(n_actions=9), dict(hid=1 << 30)):
        with pytest.raises(capi.RcmarlError, match="RCMARL_ERR_UNSUPPORTED"):
            call(**kw)


# ---- the engine ------------------------------------------------------------------------------------------------------------------
LABELS_GM = (COOP, COOP, COOP, GREEDY, MAL)
LABELS_FM = (COOP, COOP, COOP, FAULTY, MAL)
LABELS_M = (MAL, COOP, COOP, COOP, COOP)
ONE_LAUNCH = ("rcmarl_minibatch_actor_wide", "rcmarl_minibatch_actor_wide2")


class CountingLib:
    """the library with a launch counter per entry point in front; `loop_steps` counts the rcmarl_wide_actor_head calls of the
    adversaries' launch-per-step loop: (seed, agent) = (1, 1) views.  serve=False: both one-launch queries answer 0, as a library
    does for a shape beyond its layouts."""

    def __init__(self, lib, serve=True):
        self._lib, self.calls, self.loop_steps, self.serve = lib, collections.Counter(), 0, serve

    def __getattr__(self, name):
        fn = getattr(self._lib, name)
        if not callable(fn):
            return fn

        def call(*args):
            self.calls[name] += 1
            if name == "rcmarl_wide_actor_head" and args[7:9] == (1, 1):
                self.loop_steps += 1
            if name in ("rcmarl_minibatch_actor_wide_supported", "rcmarl_minibatch_actor_wide2_supported") and not self.serve:
                return 0
            return fn(*args)
        return call


def engine_inputs(seeds, actor_hid, critic_hid, n=5, nrow=5, weight_seed=3):
    rng = np.random.default_rng(weight_seed)
    W = [[{"actor": M.init_mlp(rng, 2 * n, actor_hid, 5), "critic": M.init_mlp(rng, 2 * n, critic_hid, 1), "tr": M.init_mlp(rng, 3 * n, 20, 1)}
          for _ in range(n)] for _ in seeds]
    goals = [np.random.default_rng(100 + s).integers(0, nrow, size=(n, 2)) for s in range(len(seeds))]
    return W, goals


SHAPE = dict(max_ep_len=3, n_ep_fixed=2, n_epochs=2, buffer_size=9)
_ORACLE = {}


def _oracle(labels, actor_hid, critic_hid, seeds, blocks, shape):
    key = (tuple(labels), actor_hid, critic_hid, tuple(seeds), blocks, tuple(sorted(shape.items())))
    if key not in _ORACLE:
        args = EC.make_args(list(labels), H=1, n_episodes=blocks * shape["n_ep_fixed"], seed=44, **shape)
        W, goals = engine_inputs(seeds, actor_hid, critic_hid)
        _ORACLE[key] = (W, goals) + tuple(EC.run_oracle(args, 5, 5, "device", seeds, W, goals))
    return _ORACLE[key]


def make_engine(device, lib, labels, actor_hid, critic_hid, seeds, W, goals, adv_actor, shape=SHAPE):
    cfg = EngineConfig(5, list(labels), EC.CIRC5, H=1, nrow=5, ncol=5, n_seeds=len(seeds), rng_mode="device", lattice=False,
                       actor_hid=actor_hid, critic_hid=critic_hid, adv_actor=adv_actor, **shape)
    eng = RPBCACEngine(cfg, seeds=list(seeds), device=device, lib=lib)
    for s in range(len(seeds)):
        for i in range(5):
            for net in ("actor", "critic", "tr"):
                eng.set_weights(s, i, net, W[s][i][net])
    eng.set_goals(np.stack(goals))
    return eng


def run_engine(device, lib, labels, actor_hid, critic_hid=20, adv_actor="launch", seeds=(44, 45), blocks=2, shape=SHAPE, serve=True):
    """5 agents on EC.CIRC5, H = 1, a 5 x 5 grid, rng_mode="device": `blocks` update blocks against oracle.train at
    engine_checks.compare's default bars; returns the engine and the counting wrapper it ran on"""
    W, goals, o_logs, o_w = _oracle(labels, actor_hid, critic_hid, seeds, blocks, shape)
    cl = CountingLib(lib, serve)
    eng = make_engine(device, cl, labels, actor_hid, critic_hid, seeds, W, goals, adv_actor, shape)
    logs = eng.train(blocks * shape["n_ep_fixed"])
    assert eng.actor_wide and hasattr(eng, "adv") and eng.adv.adv
    worst = EC.compare(eng, logs, o_logs, o_w)
    print("[wide actor adv] %s actor %d, critic %d, adv_actor=%s, %d seed(s), %d block(s): oracle met; worst critic %.2e, team-reward net "
          "%.2e (bar 1e-4)" % ("/".join(l[0] for l in labels), actor_hid, critic_hid, adv_actor, len(seeds), blocks, worst["critic"],
                               worst["tr"]))
    return eng, cl, W


def _steps_per_fit(shape):
    nl = shape["max_ep_len"] * shape["n_ep_fixed"]
    return (nl + EA.ACTOR_BATCH - 1) // EA.ACTOR_BATCH


def _check_adversaries_moved(eng, W, labels, blocks, shape=SHAPE):
    """the adversaries' actor rows moved, their Adam slots are non-zero, their step count is that of `blocks` fits"""
    assert eng.adv.adam_t == blocks * _steps_per_fit(shape) and eng.adam_t == blocks
    m = eng.adam_m.cpu().numpy()
    for s in range(eng.S):
        for i, lab in enumerate(labels):
            if lab == COOP:
                continue
            assert any(np.abs(a - b).max() > 0 for a, b in zip(eng.get_weights(s, i, "actor"), W[s][i]["actor"])), (s, i)
            assert np.abs(m[s, i]).max() > 0, (s, i)


def _check_route(cl, entry, blocks, shape=SHAPE, n_chains=None):
    """entry: the one-launch entry point every phase-III fit must have taken (one call per block for all seeds and adversaries), or
    None for the loop (n_chains x ceil(n_last / 200) steps per block)"""
    c = cl.calls
    assert c["rcmarl_minibatch_actor"] == 0, dict(c)
    for name in ONE_LAUNCH:
        assert c[name] == (blocks if name == entry else 0), (name, dict(c))
    assert cl.loop_steps == (0 if entry else blocks * n_chains * _steps_per_fit(shape)), (cl.loop_steps, dict(c))


def check_engine_two_blocks(device, lib, adv_actor="launch"):
    """C C C Greedy Malicious, actor 32, critic 20, seeds (44, 45), two blocks"""
    eng, cl, W = run_engine(device, lib, LABELS_GM, 32, 20, adv_actor)
    assert eng.actor_mx
    _check_route(cl, None if adv_actor == "loop" else "rcmarl_minibatch_actor_wide", 2, n_chains=4)
    _check_adversaries_moved(eng, W, LABELS_GM, 2)
    assert eng.adv.adam_t == 2


def check_engine_auto(device, lib):
    """adv_actor="auto": a library whose two queries answer 0 takes the loop; with the real queries the route follows the measured
    constant and the chain count"""
    eng, cl, W = run_engine(device, lib, LABELS_GM, 32, 20, "auto", blocks=1, serve=False)
    _check_route(cl, None, 1, n_chains=4)
    _check_adversaries_moved(eng, W, LABELS_GM, 1)
    eng, cl, W = run_engine(device, lib, LABELS_GM, 32, 20, "auto", blocks=1)
    chains = eng.S * len(eng.adv.adv)
    assert chains == 4
    _check_route(cl, "rcmarl_minibatch_actor_wide" if chains >= EA.ACTOR_WIDE_MIN_CHAINS else None, 1, n_chains=chains)
    _check_adversaries_moved(eng, W, LABELS_GM, 1)


def check_engine_shuffled(device, lib, adv_actor="launch"):
    """220 rows in the one block: mini-batches of 200 and 20 rows, permutations drawn in the reference's call order"""
    shape = dict(max_ep_len=110, n_ep_fixed=2, n_epochs=2, buffer_size=220)
    eng, cl, W = run_engine(device, lib, LABELS_GM, 32, 20, adv_actor, blocks=1, shape=shape)
    assert eng.n_last == 220 and eng.n_last > EA.ACTOR_BATCH
    _check_route(cl, None if adv_actor == "loop" else "rcmarl_minibatch_actor_wide", 1, shape, n_chains=4)
    assert eng.adv.adam_t == 2 and eng.adv.calls == [2 * 1 * 5 + 2] * 2          # 5 fits per epoch (G: 2, M: 3) + one draw per adversary's actor
    _check_adversaries_moved(eng, W, LABELS_GM, 1, shape)


def check_engine_plain_rollout(device, lib):
    """C C C Faulty Malicious with a 24-unit actor: no multiple of 32, so the rollout goes episode by episode on the plain kernel"""
    eng, cl, W = run_engine(device, lib, LABELS_FM, 24, 20, "launch")
    assert not eng.actor_mx and cl.calls["rcmarl_rollout_step_wide"] > 0 and cl.calls["rcmarl_rollout_step_episodes_wide"] == 0
    _check_route(cl, "rcmarl_minibatch_actor_wide", 2)
    _check_adversaries_moved(eng, W, LABELS_FM, 2)


def check_engine_wide_critic(device, lib):
    """Malicious C C C C, a 24-unit critic beside the 32-unit actor: the TD error comes from the wide private critic.  (The critic's
    scratch is smaller than the actor's here, so the actor keeps its own.)"""
    eng, cl, W = run_engine(device, lib, LABELS_M, 32, 24, "launch")
    assert eng.wide and not eng.wa_alias
    _check_route(cl, "rcmarl_minibatch_actor_wide", 2)
    _check_adversaries_moved(eng, W, LABELS_M, 2)


def check_engine_wide_critic_aliased(device, lib):
    """the same team with a 40-unit critic on the loop: the actor's scratch, which the loop works in, aliases the wide critic's"""
    eng, cl, W = run_engine(device, lib, LABELS_M, 32, 40, "loop")
    assert eng.wide and eng.wa_alias
    _check_route(cl, None, 2, n_chains=2)
    _check_adversaries_moved(eng, W, LABELS_M, 2)


def check_engine_wide2(device, lib):
    """the new kernel end to end: a 416-unit actor, one rcmarl_minibatch_actor_wide2 call per block"""
    eng, cl, W = run_engine(device, lib, LABELS_GM, 416, 20, "launch", seeds=(44,))
    _check_route(cl, "rcmarl_minibatch_actor_wide2", 2)
    _check_adversaries_moved(eng, W, LABELS_GM, 2)


def check_cooperative_step_leaves_adversaries_alone(device, lib):
    """after one cooperative _actor_step_wide the adversaries' rows of theta["actor"], adam_m and adam_v keep their bits"""
    seeds = (44, 45)
    W, goals = engine_inputs(seeds, 32, 20)
    eng = make_engine(device, lib, LABELS_GM, 32, 20, seeds, W, goals, "launch")
    eng._rollout(eng.cfg.n_ep_fixed)
    eng._require_adversary_support()
    rng = np.random.default_rng(5)
    import torch
    eng.adam_m.copy_(torch.from_numpy((0.01 * rng.normal(size=tuple(eng.adam_m.shape))).astype(np.float32)))
    eng.adam_v.copy_(torch.from_numpy((1e-4 * rng.random(size=tuple(eng.adam_v.shape))).astype(np.float32)))
    before = [t.detach().cpu().numpy().copy() for t in (eng.theta["actor"], eng.adam_m, eng.adam_v)]
    eng._actor_update(eng.B)
    eng.sync()
    after = [t.detach().cpu().numpy() for t in (eng.theta["actor"], eng.adam_m, eng.adam_v)]
    for i, lab in enumerate(LABELS_GM):
        for b, a in zip(before, after):
            if lab == COOP:
                assert not np.array_equal(a[:, i], b[:, i]), i
            else:
                np.testing.assert_array_equal(a[:, i], b[:, i])


def check_checkpoint(device, lib, path, adv_actor="launch"):
    """two blocks against one block, save, load into a fresh engine, one more: logs, weights, Adam slots and both step counts"""
    seeds = (44, 45)
    W, goals = engine_inputs(seeds, 32, 20)
    mk = lambda: make_engine(device, lib, LABELS_GM, 32, 20, seeds, W, goals, adv_actor)
    a = mk()
    la = a.train(4)
    b = mk()
    lb = b.train(2)
    b.save_checkpoint(path)
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
    assert a.adam_t == c.adam_t == 2 and a.adv.adam_t == c.adv.adam_t == 2
    assert np.abs(a.adam_m.cpu().numpy()[:, 3:]).max() > 0


NARROW_COUNTED = ("rcmarl_minibatch_actor", "rcmarl_mid_actor", "rcmarl_small_adam", "rcmarl_layer1_backward_adam", "rcmarl_rollout_step_episodes",
                  "rcmarl_minibatch_fit_multi", "rcmarl_minibatch_fit", "rcmarl_shuffle_perms", "rcmarl_td_error")


def check_construction(device, lib):
    cfg = lambda **kw: EngineConfig(5, kw.pop("labels", list(LABELS_GM)), kw.pop("in_nodes", EC.CIRC5), **dict(dict(H=1, nrow=5, ncol=5, actor_hid=32,
                                                                                                                  **SHAPE), **kw))
    for lab in (GREEDY, MAL, FAULTY):
        with pytest.raises(ValueError, match="wide actor"):
            cfg(labels=[COOP, COOP, COOP, COOP, lab])
        with pytest.raises(ValueError, match="wide actor"):
            cfg(labels=[COOP, COOP, COOP, COOP, lab], adv_actor="refuse")
        for mode in ("auto", "launch", "loop"):
            assert cfg(labels=[COOP, COOP, COOP, COOP, lab], adv_actor=mode).adv_actor == mode
    for bad in ("on", True, None, "Launch"):
        with pytest.raises(ValueError, match="adv_actor"):
            cfg(adv_actor=bad)
        with pytest.raises(ValueError, match="adv_actor"):
            cfg(adv_actor=bad, actor_hid=20)
    ragged = [[0, 1, 2, 3], [1, 2, 3, 4], [2, 3, 4, 0], [3, 4, 0, 1], [4, 0, 1]]
    for mode in ("refuse", "auto", "launch", "loop"):
        labels = [COOP] * 5 if mode == "refuse" else list(LABELS_GM)      # ("refuse" beside adversaries: the wide-actor refusal comes first)
        with pytest.raises(ValueError, match="irregular"):
            cfg(labels=labels, in_nodes=ragged, adv_actor=mode)
        with pytest.raises(ValueError, match="irregular"):
            cfg(labels=labels, H=[1, 1, 1, 0, 1], adv_actor=mode)
        with pytest.raises(ValueError):
            cfg(in_nodes=ragged, adv_actor=mode)
    W, goals = engine_inputs((44,), 32, 20)
    eng = make_engine(device, lib, LABELS_GM, 32, 20, (44,), W, goals, "auto")
    with pytest.raises(ValueError, match="wide actor"):
        eng.shard_agents(rank=0, world=2)
    # a 20-unit actor beside a Greedy agent: the keyword changes no launch
    W, goals = engine_inputs((44,), 20, 20)
    counts = []
    for mode in ("refuse", "auto", "launch", "loop"):
        cl = CountingLib(lib)
        eng = make_engine(device, cl, [COOP, COOP, COOP, COOP, GREEDY], 20, 20, (44,), W, goals, mode)
        eng.train(2)
        assert cl.calls["rcmarl_minibatch_actor"] == 1 and cl.loop_steps == 0 and not any(cl.calls[k] for k in ONE_LAUNCH), dict(cl.calls)
        assert not any(cl.calls[k + "_supported"] for k in ONE_LAUNCH), dict(cl.calls)
        counts.append(dict(cl.calls))
    assert counts[0]["rcmarl_mid_actor"] == 1 and all(c == counts[0] for c in counts[1:]), counts


def check_dropin(hook, seed=5):
    """keras_compat models with 32-unit actors handed to the three adversary classes and RPBCAC_agent, then to train_RPBCAC on the
    NumPy stream, against O.train as wide_actor_checks.check_dropin compares: returns bit-identical, critic and team-reward net to
    1e-4, the actors within 5 % of the Adam steps taken"""
    from rcmarl_amd import keras_compat as K
    from rcmarl_amd.agents import adversarial_CAC_agents as ADV
    from rcmarl_amd.agents.resilient_CAC_agents import RPBCAC_agent
    from rcmarl_amd.environments.grid_world import Grid_World
    from rcmarl_amd.training.train_agents import train_RPBCAC
    n = 5
    labels = [COOP, COOP, FAULTY, GREEDY, MAL]
    hids = dict(actor=32, critic=20, tr=20)
    K.set_seed(seed)
    agents, W = [], []
    for lab in labels:
        actor, critic, tr = WS.make_models(n, hids=hids)
        W.append([actor.get_weights(), critic.get_weights(), tr.get_weights()])
        if lab == COOP:
            agents.append(RPBCAC_agent(actor, critic, tr, slow_lr=0.002, fast_lr=0.01, gamma=0.9, H=1))
        elif lab == FAULTY:
            agents.append(ADV.Faulty_CAC_agent(actor, critic, tr, slow_lr=0.002, gamma=0.9))
        else:
            cls = ADV.Greedy_CAC_agent if lab == GREEDY else ADV.Malicious_CAC_agent
            agents.append(cls(actor, critic, tr, slow_lr=0.002, fast_lr=0.01, gamma=0.9))
    assert W[0][0][0].shape == (10, 32)
    args = EC.make_args(labels, H=1, n_episodes=4, seed=seed, **SHAPE)
    goals = np.random.default_rng(seed).integers(0, 5, size=(n, 2))
    np.random.seed(seed)
    env = Grid_World(nrow=5, ncol=5, n_agents=n, desired_state=goals, initial_state=goals, randomize_state=True, scaling=True)
    weights, df = train_RPBCAC(env, agents, args, engine_hook=hook)
    o_agents = [O.make_agent(lab, [a.copy() for a in W[i][0]], [a.copy() for a in W[i][1]], [a.copy() for a in W[i][2]], 0.002, 0.01, 0.9, 1)
                for i, lab in enumerate(labels)]
    np.random.seed(seed)
    ow, odf = O.train(O.GridWorldOracle(5, 5, n, goals, None, True, True), o_agents, args, rng_mode="numpy")
    np.testing.assert_array_equal(df["True_team_returns"].to_numpy(), odf["True_team_returns"].to_numpy(dtype=np.float64))
    np.testing.assert_array_equal(df["True_adv_returns"].to_numpy(), odf["True_adv_returns"].to_numpy(dtype=np.float64))
    steps = 2                                                          # two blocks; an adversary's fit of 6 rows is one step as well
    for i in range(n):
        assert weights[i][0][0].shape == (10, 32)
        assert any(np.abs(a - b).max() > 0 for a, b in zip(weights[i][0], W[i][0])), i       # every actor was trained
        for a, b in zip(weights[i][0], ow[i][0]):
            assert float(np.abs(a - b).max()) <= 0.05 * 0.002 * steps + 1e-5, ("actor", i, float(np.abs(a - b).max()))
        for k in (1, 2):
            for a, b in zip(weights[i][k], ow[i][k]):
                DC.close(a, b, 1e-4, "wide actor beside adversaries, drop-in agent %d net %d" % (i, k))
