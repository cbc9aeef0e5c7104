"""Adversaries beside wide critic-family nets -- checks shared by the hipemu, the GPU and the argument-validation tests:
rcmarl_minibatch_fit_wide (csrc/minibatch_wide.hip: one workgroup per (job, seed, adversary) chain, all chains of a consensus epoch
in one launch) against oracle/mlp_np.fit_mse, its multi-job form against single-job calls, its query and refusals, and the engine
with Greedy / Malicious agents beside wide nets against oracle.train, with the routing counted and the launch-per-step fallback
kept under test."""
import collections
import ctypes

import numpy as np
import pytest

import engine_checks as EC
from kernel_checks import pad64, pack_rows, unpack_row, rel_close
from oracle import mlp_np as M
from rcmarl_amd import capi
from rcmarl_amd.engine import EngineConfig, RPBCACEngine
from wide_checks import wgeom, wide_params

COOP, GREEDY, MAL = "Cooperative", "Greedy", "Malicious"
KNIFE_MIN = 1e-6                 # five times the 2e-7 knife threshold of wide_checks.check_pk_fit
# (in_dim, hid, B, adversaries, S, data seed).  The data seeds are picked so that no LeakyReLU input of any chain is a knife edge
# (minibatch_knife_ratio >= KNIFE_MIN, asserted by the check): random Glorot nets give 1e-6 ... 6e-5 for most seeds, a few fall below.
SHAPES = {
    "partial_tile": (6, 24, 70, (3, 4), 2, 1),        # partial unit tile; two full batches + one of 6 rows
    "odd_in_one_batch": (9, 40, 32, (4,), 2, 1),      # odd in_dim; exactly one batch; two unit tiles, two idle wavefronts
    "two_chunks": (70, 96, 70, (0, 4), 2, 5),        # more input columns than one staging chunk; three tiles on four wavefronts
    "short_batch": (10, 160, 5, (2,), 2, 1),          # B below one batch; five tiles, so one wavefront owns two
    # the largest width the query must serve (GPU only).  Its 8 chains pass ~1.8 million LeakyReLU inputs: one data seed in several
    # hundred keeps all of them above KNIFE_MIN (1.13e-6 for this one; 1082 of the first 1083 seeds fall below)
    "widest": (15, 256, 200, (1, 3), 4, 1083),
}
MULTI_JOBS = ((10, 24, (4,)), (15, 40, (3, 4)), (10, 24, (3, 4)))


def minibatch_knife_ratio(p0, x, y, lr, epochs, bs, perms):
    """The mini-batch form of wide_checks.knife_edge_ratio: a float64 replay of one chain (Keras SGD on the MSE loss, the batches of
    oracle/mlp_np.fit_mse) from p0; the smallest |pre-activation| / sum |terms| over both hidden layers, all rows of all mini-batches
    and all steps.  A LeakyReLU input within fp32 rounding of zero (ratio ~1e-7) takes the other slope in one of two fp32 chains that
    differ in summation order; a chain well above that is held to the fp32 bar on every network."""
    W1, b1, W2, b2, W3, b3 = [np.asarray(q, np.float64).copy() for q in p0]
    x, y = np.asarray(x, np.float64), np.asarray(y, np.float64).reshape(-1, 1)
    B = x.shape[0]
    bs = min(bs, B)
    worst = np.inf
    for ep in range(epochs):
        order = np.arange(B) if perms is None else np.asarray(perms[ep])
        for lo in range(0, B, bs):
            idx = order[lo:lo + bs]
            xb, yb, nb = x[idx], y[idx], len(idx)
            z1 = xb @ W1 + b1
            a1 = np.where(z1 > 0, z1, 0.1 * z1)
            z2 = a1 @ W2 + b2
            a2 = np.where(z2 > 0, z2, 0.1 * z2)
            s1 = np.abs(xb) @ np.abs(W1) + np.abs(b1)
            s2 = np.abs(a1) @ np.abs(W2) + np.abs(b2)
            worst = min(worst, float((np.abs(z1) / s1).min()), float((np.abs(z2) / s2).min()))
            dv = 2.0 * (a2 @ W3 + b3 - yb) / nb
            dz2 = (dv @ W3.T) * np.where(z2 > 0, 1.0, 0.1)
            dz1 = (dz2 @ W2.T) * np.where(z1 > 0, 1.0, 0.1)
            W3 -= lr * (a2.T @ dv); b3 -= lr * dv.sum(0)
            W2 -= lr * (a1.T @ dz2); b2 -= lr * dz2.sum(0)
            W1 -= lr * (xb.T @ dz1); b1 -= lr * dz1.sum(0)
    return worst


def _case(in_dim, hid, B, advs, S, N, seed, epochs):
    rng = np.random.default_rng([seed, in_dim, hid, B])
    g = wgeom(in_dim, hid)
    ldp, ldb, cap = pad64(g["P"]) + 64, pad64(B), B + 5            # (+ 64: columns P..ldp the kernel must not touch)
    params = wide_params(rng, S, N, in_dim, hid)
    theta = pack_rows(params, ldp)
    theta[:, :, g["P"]:] = rng.normal(size=(S, N, ldp - g["P"])).astype(np.float32)
    x = rng.normal(size=(S, cap, in_dim)).astype(np.float32)
    y = rng.normal(size=(S, N, ldb)).astype(np.float32)
    advs = np.asarray(advs, np.int32)
    perm = np.stack([[[rng.permutation(B) for _ in range(epochs)] for _ in advs] for _ in range(S)]).astype(np.int32)
    return dict(in_dim=in_dim, hid=hid, B=B, advs=advs, S=S, N=N, ldp=ldp, ldb=ldb, cap=cap, P=g["P"], params=params, theta=theta,
                x=x, y=y, perm=perm)


def _launch(bk, cases, epochs, bs=32, lr=0.01, shuffle=True):
    """one rcmarl_minibatch_fit_wide call over `cases` (jobs of one S, N, B) -> [(theta, loss)] per job"""
    c0 = cases[0]
    dev = [dict(x=bk.dev(c["x"]), th=bk.dev(c["theta"]), y=bk.dev(c["y"]), adv=bk.dev(c["advs"]), perm=bk.dev(c["perm"]),
                loss=bk.dev(np.full((c["S"], c["N"]), -3.0, np.float32))) for c in cases]
    arr = (capi.MbJob * len(cases))(*[capi.MbJob(bk.ptr(d["x"]), c["cap"] * c["in_dim"], bk.ptr(d["th"]), bk.ptr(d["adv"]), len(c["advs"]),
                                                 c["in_dim"], c["ldp"], 0, bk.ptr(d["y"]), bk.ptr(d["perm"]) if shuffle else None,
                                                 bk.ptr(d["loss"]), None) for c, d in zip(cases, dev)])
    hid = (ctypes.c_int * len(cases))(*[c["hid"] for c in cases])
    rc = bk.lib.rcmarl_minibatch_fit_wide(arr, hid, len(cases), c0["S"], c0["N"], c0["B"], c0["ldb"], bs, epochs, lr, bk.stream)
    assert rc in (0, None)
    return [(np.array(bk.host(d["th"])), np.array(bk.host(d["loss"]))) for d in dev]


def check_fit(bk, name, epochs=2, lr=0.01, shuffle=True, bs=32, N=5):
    """One job against oracle/mlp_np.fit_mse with the same permutations, at the bars of kernel_checks.check_minibatch_fit: every
    parameter within 2e-5 * max(1, |w|max), the loss within 2e-5 * max(1, |loss|), NO network exempt -- on inputs that are asserted
    not to be LeakyReLU knife edges.  Rows of non-adversaries and columns P..ldp keep their bits."""
    in_dim, hid, B, advs, S, seed = SHAPES[name]
    assert bk.lib.rcmarl_minibatch_fit_wide_supported(in_dim, hid, bs) == 1
    c = _case(in_dim, hid, B, advs, S, N, seed, epochs)
    (th_new, loss), = _launch(bk, [c], epochs, bs, lr, shuffle)
    worst_w, worst_l, ratio, fitted = 0.0, 0.0, np.inf, []
    for s in range(S):
        for n in range(N):
            if n not in c["advs"]:
                np.testing.assert_array_equal(th_new[s, n], c["theta"][s, n])
                assert loss[s, n] == -3.0
                continue
            np.testing.assert_array_equal(th_new[s, n, c["P"]:], c["theta"][s, n, c["P"]:])
            k = list(c["advs"]).index(n)
            perms = c["perm"][s, k] if shuffle else None
            ratio = min(ratio, minibatch_knife_ratio(c["params"][s][n], c["x"][s, :B], c["y"][s, n, :B], lr, epochs, bs, perms))
            pw = M.copy_params(c["params"][s][n])
            hist = M.fit_mse(pw, c["x"][s, :B], c["y"][s, n, :B], lr, epochs=epochs, batch_size=bs,
                             perms=perms if shuffle else np.tile(np.arange(B), (epochs, 1)))
            got = unpack_row(th_new[s, n], in_dim, 1, hid)
            fitted.append((s, n, got, pw, hist))
            for q in range(6):
                worst_w = max(worst_w, float(np.abs(got[q] - pw[q]).max()) / max(1.0, float(np.abs(pw[q]).max())))
            worst_l = max(worst_l, abs(float(loss[s, n]) - float(hist[0])) / max(1.0, abs(float(hist[0]))))
    print("[wide adv] %s (in %d, hid %d, B %d): knife ratio %.2e (needs >= %.0e), worst parameter %.2e, worst loss %.2e (bars 2e-5)"
          % (name, in_dim, hid, B, ratio, KNIFE_MIN, worst_w, worst_l))
    assert ratio >= KNIFE_MIN, ratio                                  # the input condition of the comparison
    assert len(fitted) == S * len(c["advs"])
    for s, n, got, pw, hist in fitted:
        for q in range(6):
            rel_close(got[q], pw[q], 2e-5, "wide minibatch fit %s, net (%d, %d), param %d" % (name, s, n, q))
        assert abs(loss[s, n] - hist[0]) <= 2e-5 * max(1.0, abs(hist[0])), (loss[s, n], hist[0])
    return th_new, loss


def check_determinism(bk, name="partial_tile"):
    in_dim, hid, B, advs, S, seed = SHAPES[name]
    c = _case(in_dim, hid, B, advs, S, 5, seed, 2)
    (a, la), = _launch(bk, [c], 2)
    (b, lb), = _launch(bk, [c], 2)
    np.testing.assert_array_equal(a, b)
    np.testing.assert_array_equal(la, lb)
    assert not np.array_equal(a, c["theta"])


def check_multi_job(bk, S=2, N=5, B=40, epochs=2):
    """three jobs of different (in_dim, hid, adversary set) in ONE call: the bits of three single-job calls"""
    cases = [_case(in_dim, hid, B, advs, S, N, 7 + j, epochs) for j, (in_dim, hid, advs) in enumerate(MULTI_JOBS)]
    multi = _launch(bk, cases, epochs)
    for j, c in enumerate(cases):
        (th, loss), = _launch(bk, [c], epochs)
        np.testing.assert_array_equal(multi[j][0], th, err_msg="job %d parameters" % j)
        np.testing.assert_array_equal(multi[j][1], loss, err_msg="job %d losses" % j)
        assert not np.array_equal(th, c["theta"])


def check_query(lib):
    for hid in (1, 20, 24, 40, 64, 96, 160, 255, 256):
        for in_dim in (1, 9, 15, 70, 2048):
            for bs in (1, 7, 32):
                assert lib.rcmarl_minibatch_fit_wide_supported(in_dim, hid, bs) == 1, (in_dim, hid, bs)
    assert lib.rcmarl_minibatch_fit_wide_supported(10, 64, 33) == 0
    assert lib.rcmarl_minibatch_fit_wide_supported(10, 64, 0) == 0
    assert lib.rcmarl_minibatch_fit_wide_supported(0, 64, 32) == 0
    assert lib.rcmarl_minibatch_fit_wide_supported(10, 0, 32) == 0
    assert lib.rcmarl_minibatch_fit_wide_supported(10, 512, 32) == 0       # 3 x [32][512] fp32 = 192 KiB: beyond the 160 KiB of a CU
    assert lib.rcmarl_minibatch_fit_wide_supported(10, 1 << 30, 32) == 0


def check_argument_validation(lib):
    """RCMARL_ERR_ARG / RCMARL_ERR_UNSUPPORTED before the HIP runtime is touched (64 stands for "not NULL": refused before any pointer
    is looked at -- every call here is refused)"""
    p, hid, ldp = 64, 64, pad64(wgeom(10, 64)["P"])

    def job(**kw):
        f = dict(x=p, x_seed_stride=100, theta=p, agents=p, n_adv=1, in_dim=10, ldp=ldp, reserved_=0, y=p, perm=None, loss_out=None,
                 ovf_flags=None)
        f.update(kw)
        return capi.MbJob(*[f[k] for k, _ in capi.MbJob._fields_])

    def call(jobs, hids, njobs=None, S=2, N=5, B=40, ldb=64, bs=32, epochs=2):
        arr = (capi.MbJob * max(1, len(jobs)))(*jobs) if jobs is not None else None
        h = (ctypes.c_int * max(1, len(hids)))(*hids) if hids is not None else None
        return lib.rcmarl_minibatch_fit_wide(arr, h, len(jobs) if njobs is None else njobs, S, N, B, ldb, bs, epochs, 0.01, None)

    bad = [lambda: call(None, [hid], njobs=1), lambda: call([job()], None),
           lambda: call([job(x=None)], [hid]), lambda: call([job(theta=None)], [hid]), lambda: call([job(agents=None)], [hid]),
           lambda: call([job(y=None)], [hid]), lambda: call([job(n_adv=0)], [hid]), lambda: call([job(n_adv=-1)], [hid]),
           lambda: call([job()], [hid], njobs=0), lambda: call([job()] * 5, [hid] * 5), lambda: call([job(ldp=ldp + 32)], [hid]),
           lambda: call([job(in_dim=0)], [hid]), lambda: call([job()], [0]), lambda: call([job()], [hid], S=0),
           lambda: call([job()], [hid], N=0), lambda: call([job()], [hid], B=0), lambda: call([job()], [hid], bs=0),
           lambda: call([job()], [hid], epochs=0), lambda: call([job()], [hid], ldb=39),
           lambda: call([job(), job(theta=None)], [hid, hid])]
    for f in bad:
        with pytest.raises(capi.RcmarlError, match="RCMARL_ERR_ARG"):
            f()
    for f in (lambda: call([job()], [hid], bs=33), lambda: call([job(ldp=pad64(wgeom(10, 512)["P"]))], [512]),
              lambda: call([job(), job(ldp=pad64(wgeom(10, 512)["P"]))], [hid, 512])):
        with pytest.raises(capi.RcmarlError, match="RCMARL_ERR_UNSUPPORTED"):
            f()


# ---- the engine ------------------------------------------------------------------------------------------------------------------
ENGINE_CASES = [([COOP, COOP, COOP, GREEDY, MAL], 24, 24), ([COOP, COOP, COOP, GREEDY, MAL], 24, 40),
                ([MAL, COOP, COOP, COOP, COOP], 24, 24), ([MAL, COOP, COOP, COOP, COOP], 24, 40)]
N_EPOCHS = 2


class CountingLib:
    """the library with a launch counter per entry point in front (as wide_tr_checks.CountingLib); `adv_steps` counts the
    rcmarl_wide_head_fit calls of the adversaries' launch-per-step loop: (seed, agent) = (1, 1) views of at most 32 rows.
    serve_wide=False: rcmarl_minibatch_fit_wide_supported answers 0, as a library does for a width beyond its LDS layout."""

    def __init__(self, lib, serve_wide=True):
        self._lib, self.calls, self.adv_steps, self.serve_wide = lib, collections.Counter(), 0, serve_wide

    def __getattr__(self, name):
        fn = getattr(self._lib, name)
        if not callable(fn):
            return fn

        def call(*args):
            self.calls[name] += 1
            if name == "rcmarl_wide_head_fit" and args[6:8] == (1, 1) and args[8] <= 32:
                self.adv_steps += 1
            if name == "rcmarl_minibatch_fit_wide_supported" and not self.serve_wide:
                return 0
            return fn(*args)
        return call


def engine_inputs(seeds, critic_hid, tr_hid, n=5, nrow=5, weight_seed=3):
    rng = np.random.default_rng(weight_seed)
    W = [[{"actor": M.init_mlp(rng, 2 * n, 20, 5), "critic": M.init_mlp(rng, 2 * n, critic_hid, 1), "tr": M.init_mlp(rng, 3 * n, tr_hid, 1)}
          for _ in range(n)] for _ in seeds]
    goals = [np.random.default_rng(100 + s).integers(0, nrow, size=(n, 2)) for s in range(len(seeds))]
    return W, goals


_ORACLE = {}


def _oracle(labels, critic_hid, tr_hid, seeds):
    key = (tuple(labels), critic_hid, tr_hid, tuple(seeds))
    if key not in _ORACLE:
        args = EC.make_args(list(labels), H=1, n_episodes=2, max_ep_len=3, n_ep_fixed=2, n_epochs=N_EPOCHS, buffer_size=9, seed=44)
        W, goals = engine_inputs(seeds, critic_hid, tr_hid)
        _ORACLE[key] = (W, goals) + tuple(EC.run_oracle(args, 5, 5, "device", seeds, W, goals))
    return _ORACLE[key]


def run_engine(device, lib, labels, critic_hid, tr_hid, seeds=(44,), serve_wide=True):
    """5 agents on EC.CIRC5, H = 1, 5 x 5 grid, one block of two consensus epochs against oracle.train at engine_checks.compare's
    default bars; returns the engine and the counting wrapper it ran on"""
    W, goals, o_logs, o_w = _oracle(labels, critic_hid, tr_hid, seeds)
    cl = CountingLib(lib, serve_wide)
    cfg = EngineConfig(5, list(labels), EC.CIRC5, H=1, max_ep_len=3, n_ep_fixed=2, n_epochs=N_EPOCHS, buffer_size=9, nrow=5, ncol=5,
                       n_seeds=len(seeds), rng_mode="device", lattice=False, critic_hid=critic_hid, tr_hid=tr_hid)
    eng = RPBCACEngine(cfg, seeds=list(seeds), device=device, lib=cl)
    for s in range(len(seeds)):
        for i in range(5):
            for net in ("actor", "critic", "tr"):
                eng.set_weights(s, i, net, W[s][i][net])
    eng.set_goals(np.stack(goals))
    logs = eng.train(2)
    assert eng.wide and hasattr(eng, "adv") and eng.adv.fit
    worst = EC.compare(eng, logs, o_logs, o_w)
    print("[wide adv] %s critic %d, team-reward net %d, %d seed(s), %s: worst |w - w_oracle| / max(1, |w|max): critic %.2e, "
          "team-reward net %.2e (bar 1e-4)" % ("/".join(l[0] for l in labels), critic_hid, tr_hid, len(seeds),
                                               "one launch per epoch" if serve_wide else "launch-per-step fallback",
                                               worst["critic"], worst["tr"]))
    return eng, cl


def check_engine(device, lib, labels, critic_hid, tr_hid):
    """both nets wide: ONE rcmarl_minibatch_fit_wide call per consensus epoch, no step of the launch-per-step loop, no 20-unit fit"""
    eng, cl = run_engine(device, lib, labels, critic_hid, tr_hid)
    assert eng.critic_wide
    assert cl.calls["rcmarl_minibatch_fit_wide"] == N_EPOCHS, dict(cl.calls)
    assert cl.adv_steps == 0 and cl.calls["rcmarl_minibatch_fit"] == 0 and cl.calls["rcmarl_minibatch_fit_multi"] == 0


def check_engine_mixed(device, lib, seeds=(44, 45, 46)):
    """a 20-unit critic beside a 24-unit team-reward net, three seeds batched: the critic stays on rcmarl_minibatch_fit, the
    team-reward net goes to the new entry point -- one call each per consensus epoch, for all seeds"""
    eng, cl = run_engine(device, lib, [COOP, COOP, COOP, COOP, GREEDY], 20, 24, seeds=seeds)
    assert not eng.critic_wide and eng.S == 3
    assert cl.calls["rcmarl_minibatch_fit_wide"] == N_EPOCHS and cl.calls["rcmarl_minibatch_fit"] == N_EPOCHS, dict(cl.calls)
    assert cl.adv_steps == 0 and cl.calls["rcmarl_minibatch_fit_multi"] == 0


def check_engine_fallback(device, lib, labels=(COOP, COOP, COOP, GREEDY, MAL), critic_hid=24, tr_hid=40):
    """the query answers 0: no rcmarl_minibatch_fit_wide call, the launch-per-step loop (10 epochs x 1 mini-batch per chain; a
    Greedy agent has two chains, a Malicious one three), and the oracle is met at the same bars"""
    eng, cl = run_engine(device, lib, list(labels), critic_hid, tr_hid, serve_wide=False)
    assert cl.calls["rcmarl_minibatch_fit_wide"] == 0
    chains = sum(3 if l == MAL else 2 for l in labels if l in (GREEDY, MAL))
    assert cl.adv_steps == N_EPOCHS * chains * 10, (cl.adv_steps, dict(cl.calls))
