"""Adversaries beside critic-family nets of 385 .. 576 units -- checks shared by the hipemu, the GPU and the argument-validation
tests: rcmarl_minibatch_fit_wide2 (csrc/minibatch_wide2.hip: two activation images in LDS, dz1 over a1, the layer-1 chunks staged
once per step) against oracle/mlp_np.fit_mse by the method of wide_adv_checks.check_fit, its multi-job form against single-job
calls, its query (never 1 together with rcmarl_minibatch_fit_wide_supported) and refusals, and the engine with Greedy / Malicious
agents beside such nets against oracle.train, with the routing counted on the forced launch and on the forced loop."""
import ctypes

import numpy as np
import pytest

import engine_checks as EC
import wide_adv_checks as WA
from kernel_checks import pad64, unpack_row, rel_close
from oracle import mlp_np as M
from rcmarl_amd import capi
from rcmarl_amd.engine import EngineConfig, RPBCACEngine
from wide_checks import wgeom

COOP, GREEDY, MAL = WA.COOP, WA.GREEDY, WA.MAL
KNIFE_MIN = WA.KNIFE_MIN
# (in_dim, hid, B, adversaries, S, data seed): the data seeds keep every LeakyReLU input of every chain off the knife edge
# (minibatch_knife_ratio >= KNIFE_MIN, asserted by the check; found by a scan over seeds 1..40, alternates in the comments)
SHAPES = {
    # the smallest width the query serves: a last unit tile of ONE column, 13 tiles on four wavefronts (uneven ownership),
    # batches of 32 + 8 rows  (3.2e-6; then 3, 9, 10, 11, 13)
    "first_unserved": (6, 385, 40, (3, 4), 1, 1),
    # the same shape for the run in natural row order (perm = NULL), whose chains are other chains: of the seeds above, 11 is the
    # first that meets the condition there (7.0e-6; 1, 3, 9 and 10 give 2.0e-7, 6.1e-8, 5.8e-7 and 7.0e-7)
    "first_unserved_natural": (6, 385, 40, (3, 4), 1, 11),
    # BASELINE configs[4]'s width: 16 full tiles; two seeds  (4.4e-6; then 5, 15, 7)
    "cfg5_width": (10, 512, 40, (2,), 2, 9),
    # the widest width: 18 tiles, five on one wavefront (all accumulators live); four staging chunks, the last of 8 columns;
    # batches of 32 + 1 row  (3.6e-6; then 22, 32, 18)
    "widest_chunks": (200, 576, 33, (0, 4), 1, 27),
}
MULTI_JOBS = ((10, 416, (4,)), (15, 512, (3, 4)), (10, 416, (3, 4)))


def _launch(bk, cases, epochs, bs=32, lr=0.01, shuffle=True):
    """one rcmarl_minibatch_fit_wide2 call over `cases` (jobs of one S, N, B) -> [(theta, loss)] per job"""
    c0 = cases[0]
    dev = [dict(x=bk.dev(c["x"]), th=bk.dev(c["theta"]), y=bk.dev(c["y"]), adv=bk.dev(c["advs"]), perm=bk.dev(c["perm"]),
                loss=bk.dev(np.full((c["S"], c["N"]), -3.0, np.float32))) for c in cases]
    arr = (capi.MbJob * len(cases))(*[capi.MbJob(bk.ptr(d["x"]), c["cap"] * c["in_dim"], bk.ptr(d["th"]), bk.ptr(d["adv"]), len(c["advs"]),
                                                 c["in_dim"], c["ldp"], 0, bk.ptr(d["y"]), bk.ptr(d["perm"]) if shuffle else None,
                                                 bk.ptr(d["loss"]), None) for c, d in zip(cases, dev)])
    hid = (ctypes.c_int * len(cases))(*[c["hid"] for c in cases])
    rc = bk.lib.rcmarl_minibatch_fit_wide2(arr, hid, len(cases), c0["S"], c0["N"], c0["B"], c0["ldb"], bs, epochs, lr, bk.stream)
    assert rc in (0, None)
    return [(np.array(bk.host(d["th"])), np.array(bk.host(d["loss"]))) for d in dev]


def check_fit(bk, name, epochs=2, lr=0.01, shuffle=True, bs=32, N=5):
    """wide_adv_checks.check_fit on the new entry point: one job against oracle/mlp_np.fit_mse with the same permutations, every
    parameter array within 2e-5 * max(1, |w|max), the loss within 2e-5 * max(1, |loss|), NO network exempt -- on inputs that are
    asserted not to be LeakyReLU knife edges.  Rows of non-adversaries and columns P..ldp keep their bits."""
    in_dim, hid, B, advs, S, seed = SHAPES[name]
    assert bk.lib.rcmarl_minibatch_fit_wide2_supported(in_dim, hid, bs) == 1
    assert bk.lib.rcmarl_minibatch_fit_wide_supported(in_dim, hid, bs) == 0
    c = WA._case(in_dim, hid, B, advs, S, N, seed, epochs)
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
            ratio = min(ratio, WA.minibatch_knife_ratio(c["params"][s][n], c["x"][s, :B], c["y"][s, n, :B], lr, epochs, bs, perms))
            pw = M.copy_params(c["params"][s][n])
            hist = M.fit_mse(pw, c["x"][s, :B], c["y"][s, n, :B], lr, epochs=epochs, batch_size=bs,
                             perms=perms if shuffle else np.tile(np.arange(B), (epochs, 1)))
            got = unpack_row(th_new[s, n], in_dim, 1, hid)
            fitted.append((s, n, got, pw, hist))
            for q in range(6):
                worst_w = max(worst_w, float(np.abs(got[q] - pw[q]).max()) / max(1.0, float(np.abs(pw[q]).max())))
            worst_l = max(worst_l, abs(float(loss[s, n]) - float(hist[0])) / max(1.0, abs(float(hist[0]))))
    print("[wide2 adv] %s (in %d, hid %d, B %d): knife ratio %.2e (needs >= %.0e), worst parameter %.2e, worst loss %.2e (bars 2e-5)"
          % (name, in_dim, hid, B, ratio, KNIFE_MIN, worst_w, worst_l))
    assert ratio >= KNIFE_MIN, ratio                                  # the input condition of the comparison
    assert len(fitted) == S * len(c["advs"])
    for s, n, got, pw, hist in fitted:
        for q in range(6):
            rel_close(got[q], pw[q], 2e-5, "wide2 minibatch fit %s, net (%d, %d), param %d" % (name, s, n, q))
        assert abs(loss[s, n] - hist[0]) <= 2e-5 * max(1.0, abs(hist[0])), (loss[s, n], hist[0])
    return th_new, loss


def check_determinism(bk, name="first_unserved"):
    in_dim, hid, B, advs, S, seed = SHAPES[name]
    c = WA._case(in_dim, hid, B, advs, S, 5, seed, 2)
    (a, la), = _launch(bk, [c], 2)
    (b, lb), = _launch(bk, [c], 2)
    np.testing.assert_array_equal(a, b)
    np.testing.assert_array_equal(la, lb)
    assert not np.array_equal(a, c["theta"])


def check_multi_job(bk, S=2, N=5, B=40, epochs=2):
    """three jobs of different (in_dim, hid, adversary set) in ONE call: the bits of three single-job calls"""
    cases = [WA._case(in_dim, hid, B, advs, S, N, 7 + j, epochs) for j, (in_dim, hid, advs) in enumerate(MULTI_JOBS)]
    multi = _launch(bk, cases, epochs)
    for j, c in enumerate(cases):
        (th, loss), = _launch(bk, [c], epochs)
        np.testing.assert_array_equal(multi[j][0], th, err_msg="job %d parameters" % j)
        np.testing.assert_array_equal(multi[j][1], loss, err_msg="job %d losses" % j)
        assert not np.array_equal(th, c["theta"])


def check_query(lib):
    q2, q1 = lib.rcmarl_minibatch_fit_wide2_supported, lib.rcmarl_minibatch_fit_wide_supported
    tried = []
    for hid in (385, 416, 512, 576):
        for in_dim in (1, 9, 70, 2048):
            for bs in (1, 7, 32):
                assert q2(in_dim, hid, bs) == 1, (in_dim, hid, bs)
                tried.append((in_dim, hid, bs))
    for hid in (1, 20, 24, 256, 384, 577, 608, 1 << 30):
        for in_dim in (1, 10, 2048):
            assert q2(in_dim, hid, 32) == 0, (in_dim, hid)
            tried.append((in_dim, hid, 32))
    for bs in (0, 33):
        assert q2(10, 512, bs) == 0
        tried.append((10, 512, bs))
    assert q2(0, 512, 32) == 0
    tried += [(0, 512, 32), (10, 0, 32), (10, -5, 32), (-1, 512, 32), (10, 512, -1)]
    for a in tried:
        assert q2(*a) in (0, 1) and q1(*a) in (0, 1) and q1(*a) + q2(*a) <= 1, a        # every shape keeps at most one path


def check_argument_validation(lib):
    """the bad-argument list of wide_adv_checks.check_argument_validation at hid = 512 with a matching ldp: RCMARL_ERR_ARG /
    RCMARL_ERR_UNSUPPORTED before the HIP runtime is touched (64 stands for "not NULL": every call here is refused)"""
    p, hid, ldp = 64, 512, pad64(wgeom(10, 512)["P"])

    def job(**kw):
        f = dict(x=p, x_seed_stride=100, theta=p, agents=p, n_adv=1, in_dim=10, ldp=ldp, reserved_=0, y=p, perm=None, loss_out=None,
                 ovf_flags=None)
        f.update(kw)
        return capi.MbJob(*[f[k] for k, _ in capi.MbJob._fields_])

    def call(jobs, hids, njobs=None, S=2, N=5, B=40, ldb=64, bs=32, epochs=2):
        arr = (capi.MbJob * max(1, len(jobs)))(*jobs) if jobs is not None else None
        h = (ctypes.c_int * max(1, len(hids)))(*hids) if hids is not None else None
        return lib.rcmarl_minibatch_fit_wide2(arr, h, len(jobs) if njobs is None else njobs, S, N, B, ldb, bs, epochs, 0.01, None)

    bad = [lambda: call(None, [hid], njobs=1), lambda: call([job()], None),
           lambda: call([job(x=None)], [hid]), lambda: call([job(theta=None)], [hid]), lambda: call([job(agents=None)], [hid]),
           lambda: call([job(y=None)], [hid]), lambda: call([job(n_adv=0)], [hid]), lambda: call([job(n_adv=-1)], [hid]),
           lambda: call([job()], [hid], njobs=0), lambda: call([job()] * 5, [hid] * 5), lambda: call([job(ldp=ldp + 32)], [hid]),
           lambda: call([job(in_dim=0)], [hid]), lambda: call([job()], [0]), lambda: call([job()], [hid], S=0),
           lambda: call([job()], [hid], N=0), lambda: call([job()], [hid], B=0), lambda: call([job()], [hid], bs=0),
           lambda: call([job()], [hid], epochs=0), lambda: call([job()], [hid], ldb=39),
           lambda: call([job(), job(theta=None)], [hid, hid]),
           lambda: call([job(ldp=ldp - 64)], [hid])]                   # (in_dim + hid + 3) * hid + 1 > ldp: the net does not fit its row
    for f in bad:
        with pytest.raises(capi.RcmarlError, match="RCMARL_ERR_ARG"):
            f()
    refused = [lambda: call([job()], [hid], bs=33)]
    for h in (64, 608):
        lp = pad64(wgeom(10, h)["P"])
        refused += [lambda h=h, lp=lp: call([job(ldp=lp)], [h]), lambda h=h, lp=lp: call([job(), job(ldp=lp)], [hid, h])]
    refused.append(lambda: call([job(), job()], [hid, hid], bs=33))
    for f in refused:
        with pytest.raises(capi.RcmarlError, match="RCMARL_ERR_UNSUPPORTED"):
            f()


# ---- the engine ------------------------------------------------------------------------------------------------------------------
N_EPOCHS = WA.N_EPOCHS
LABELS_GM, LABELS_M = (COOP, COOP, COOP, GREEDY, MAL), (MAL, COOP, COOP, COOP, COOP)


class CountingLib(WA.CountingLib):
    """wide_adv_checks.CountingLib that also keeps the job count of every rcmarl_minibatch_fit_wide2 call"""

    def __init__(self, lib):
        super().__init__(lib)
        self.wide2_jobs = []

    def __getattr__(self, name):
        call = super().__getattr__(name)
        if name != "rcmarl_minibatch_fit_wide2":
            return call

        def counted(*args):
            self.wide2_jobs.append(args[2])
            return call(*args)
        return counted


def run_engine(device, lib, labels, critic_hid, tr_hid, adv_wide2, seeds=(44,)):
    """the set-up of wide_adv_checks.run_engine (5 agents on EC.CIRC5, H = 1, 5 x 5 grid, buffer_size 9, two consensus epochs,
    rng_mode="device") with the 385 .. 576-unit fits forced onto the launch (adv_wide2=True) or onto the loop (False), against
    oracle.train at engine_checks.compare's default bars; returns the engine and the counting wrapper it ran on"""
    W, goals, o_logs, o_w = WA._oracle(labels, critic_hid, tr_hid, seeds)
    cl = CountingLib(lib)
    cfg = EngineConfig(5, list(labels), EC.CIRC5, H=1, max_ep_len=3, n_ep_fixed=2, n_epochs=N_EPOCHS, buffer_size=9, nrow=5, ncol=5,
                       n_seeds=len(seeds), rng_mode="device", lattice=False, critic_hid=critic_hid, tr_hid=tr_hid, adv_wide2=adv_wide2)
    eng = RPBCACEngine(cfg, seeds=list(seeds), device=device, lib=cl)
    for s in range(len(seeds)):
        for i in range(5):
            for net in ("actor", "critic", "tr"):
                eng.set_weights(s, i, net, W[s][i][net])
    eng.set_goals(np.stack(goals))
    logs = eng.train(2)
    assert eng.wide and hasattr(eng, "adv") and eng.adv.fit
    worst = EC.compare(eng, logs, o_logs, o_w)
    print("[wide2 adv] %s critic %d, team-reward net %d, %s: worst |w - w_oracle| / max(1, |w|max): critic %.2e, team-reward net %.2e "
          "(bar 1e-4)" % ("/".join(l[0] for l in labels), critic_hid, tr_hid,
                          "one launch per epoch" if adv_wide2 else "launch-per-step loop", worst["critic"], worst["tr"]))
    return eng, cl


def _loop_steps(labels, nets):
    """steps of the launch-per-step loop: 10 epochs x 1 mini-batch per chain and consensus epoch; `nets` names the looping families
    ("local" exists for a Malicious agent only)"""
    chains = sum(len(nets) - (0 if l == MAL or "local" not in nets else 1) for l in labels if l in (GREEDY, MAL))
    return N_EPOCHS * chains * 10


def check_engine_narrow_tr(device, lib, on=True):
    """C C C Greedy Malicious, critic 400 beside a 20-unit team-reward net"""
    eng, cl = run_engine(device, lib, LABELS_GM, 400, 20, on)
    assert cl.calls["rcmarl_minibatch_fit"] == N_EPOCHS and cl.calls["rcmarl_minibatch_fit_wide"] == 0, dict(cl.calls)
    if on:
        assert cl.calls["rcmarl_minibatch_fit_wide2"] == N_EPOCHS and cl.wide2_jobs == [2] * N_EPOCHS, dict(cl.calls)
        assert cl.adv_steps == 0
    else:
        assert cl.calls["rcmarl_minibatch_fit_wide2"] == 0, dict(cl.calls)
        assert cl.adv_steps == _loop_steps(LABELS_GM, ("local", "critic")), (cl.adv_steps, dict(cl.calls))


def check_engine_both_wide2(device, lib, on=True):
    """Malicious C C C C, critic 512 beside a 448-unit team-reward net: three jobs in the one call"""
    eng, cl = run_engine(device, lib, LABELS_M, 512, 448, on)
    assert cl.calls["rcmarl_minibatch_fit"] == 0 and cl.calls["rcmarl_minibatch_fit_wide"] == 0, dict(cl.calls)
    if on:
        assert cl.calls["rcmarl_minibatch_fit_wide2"] == N_EPOCHS and cl.wide2_jobs == [3] * N_EPOCHS, (dict(cl.calls), cl.wide2_jobs)
        assert cl.adv_steps == 0
    else:
        assert cl.calls["rcmarl_minibatch_fit_wide2"] == 0, dict(cl.calls)
        assert cl.adv_steps == _loop_steps(LABELS_M, ("local", "tr", "critic")), (cl.adv_steps, dict(cl.calls))


def check_engine_mixed(device, lib, on=True):
    """C C C Greedy Malicious, critic 400 beside a 40-unit team-reward net: one call of each wide entry point per epoch"""
    eng, cl = run_engine(device, lib, LABELS_GM, 400, 40, on)
    assert cl.calls["rcmarl_minibatch_fit_wide"] == N_EPOCHS and cl.calls["rcmarl_minibatch_fit"] == 0, dict(cl.calls)
    if on:
        assert cl.calls["rcmarl_minibatch_fit_wide2"] == N_EPOCHS and cl.wide2_jobs == [2] * N_EPOCHS, dict(cl.calls)
        assert cl.adv_steps == 0
    else:
        assert cl.calls["rcmarl_minibatch_fit_wide2"] == 0, dict(cl.calls)
        assert cl.adv_steps == _loop_steps(LABELS_GM, ("local", "critic")), (cl.adv_steps, dict(cl.calls))


def check_engine_crossover(device, lib, monkeypatch):
    """adv_wide2="auto": the named crossover decides -- above the epoch's chain count the loop, at it the launch (3 chains here)"""
    from rcmarl_amd import engine_adversaries as EA
    W, goals, _, _ = WA._oracle(LABELS_GM, 400, 20, (44,))
    for min_chains, launches in ((4, 0), (3, 1)):
        monkeypatch.setattr(EA, "WIDE2_MIN_CHAINS", min_chains)
        cl = CountingLib(lib)
        cfg = EngineConfig(5, list(LABELS_GM), EC.CIRC5, H=1, max_ep_len=3, n_ep_fixed=2, n_epochs=1, buffer_size=9, nrow=5, ncol=5,
                           n_seeds=1, rng_mode="device", lattice=False, critic_hid=400, tr_hid=20)
        eng = RPBCACEngine(cfg, seeds=[44], device=device, lib=cl)
        for i in range(5):
            for net in ("actor", "critic", "tr"):
                eng.set_weights(0, i, net, W[0][i][net])
        eng.set_goals(np.stack(goals))
        eng.train(2)                              # one block = one consensus epoch here
        assert cl.calls["rcmarl_minibatch_fit_wide2"] == launches, (min_chains, dict(cl.calls))
        assert cl.adv_steps == (0 if launches else 3 * 10), (min_chains, cl.adv_steps)
