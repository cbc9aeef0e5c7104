"""Checks of the local fit that starts from the live net (rcmarl_small_sgd_from, EngineConfig.fit_from_live) and of the first
epoch's TD target taken from the fit's own forward pass (RPBCACEngine.td_from_fit_forward), shared by the hipemu (CPU), GPU and
C-ABI tests.  The yardstick is always the same run with the switch off, and the comparison is word for word."""
import os

import numpy as np

import engine_checks as EC
from kernel_checks import HID, geom, pad64

# ---- the small step with a separate source ----------------------------------------------------------------------------------------
S, N, IN_DIM, B_SMALL, MASKED = 2, 7, 300, 70, 3
SENTINEL = np.float32(-12345.5)


def check_small_sgd_from(bk, lr=0.01):
    """dst = src - lr * sum(partials) on the five small arrays: every word of dst equals the in-place call on a copy of src (W1 and
    the columns P..ldp: untouched, i.e. the sentinel dst was filled with), the masked agent's row keeps its sentinel, src and the loss
    of the masked agent are unchanged."""
    L = bk.lib
    rng = np.random.default_rng(14)
    P, _ = geom(IN_DIM, 1)
    ldp = pad64(P)
    nrec = -(-B_SMALL // int(L.rcmarl_rows_per_chunk()))            # an upper bound of the records the step sums (it sums a prefix)
    psize = int(L.rcmarl_fit_partial_size(HID))
    partials = rng.normal(size=(S, N, nrec, psize)).astype(np.float32)
    src = rng.uniform(-0.3, 0.3, size=(S, N, ldp)).astype(np.float32)
    mask = np.ones(N, np.int32)
    mask[MASKED] = 0
    d_part, d_mask = bk.dev(partials), bk.dev(mask)
    d_inpl, d_loss0 = bk.dev(src.copy()), bk.dev(np.full((S, N), SENTINEL, np.float32))
    L.rcmarl_small_sgd(bk.ptr(d_part), bk.ptr(d_inpl), bk.ptr(d_mask), bk.ptr(d_loss0), S, N, B_SMALL, IN_DIM, HID, ldp, lr, bk.stream)
    d_src, d_dst, d_loss1 = bk.dev(src.copy()), bk.dev(np.full((S, N, ldp), SENTINEL, np.float32)), bk.dev(np.full((S, N), SENTINEL, np.float32))
    L.rcmarl_small_sgd_from(bk.ptr(d_part), bk.ptr(d_src), bk.ptr(d_dst), bk.ptr(d_mask), bk.ptr(d_loss1), S, N, B_SMALL, IN_DIM, HID, ldp,
                            lr, bk.stream)
    inpl, dst = bk.host(d_inpl).reshape(S, N, ldp), bk.host(d_dst).reshape(S, N, ldp)
    np.testing.assert_array_equal(bk.host(d_src).reshape(S, N, ldp).view(np.uint32), src.view(np.uint32))          # src is only read
    np.testing.assert_array_equal(bk.host(d_loss1).view(np.uint32), bk.host(d_loss0).view(np.uint32))
    assert bk.host(d_loss1).reshape(S, N)[0, MASKED] == SENTINEL
    small = slice(IN_DIM * HID, P)
    live = mask != 0
    np.testing.assert_array_equal(dst[:, live, small].view(np.uint32), inpl[:, live, small].view(np.uint32))
    assert not np.array_equal(inpl[:, live, small], src[:, live, small])                                            # the step did happen
    assert (np.abs(inpl[:, live, small] - src[:, live, small]) > 0).mean() > 0.99                                   # ... on every small array
    np.testing.assert_array_equal(dst[:, live, :IN_DIM * HID], SENTINEL)                                             # W1 is not this kernel's
    np.testing.assert_array_equal(dst[:, live, P:], SENTINEL)
    np.testing.assert_array_equal(dst[:, MASKED], SENTINEL)                                                          # masked: untouched
    np.testing.assert_array_equal(inpl[:, MASKED], src[:, MASKED])
    # the in-place entry point is the new one with src == dst
    d_same = bk.dev(src.copy())
    L.rcmarl_small_sgd_from(bk.ptr(d_part), bk.ptr(d_same), bk.ptr(d_same), bk.ptr(d_mask), None, S, N, B_SMALL, IN_DIM, HID, ldp, lr, bk.stream)
    np.testing.assert_array_equal(bk.host(d_same).reshape(S, N, ldp).view(np.uint32), inpl.view(np.uint32))


# ---- engine ---------------------------------------------------------------------------------------------------------------------
WATCHED = {"rcmarl_mid_fit_lattice": (1,), "rcmarl_small_sgd": (1,), "rcmarl_small_sgd_from": (1, 2), "rcmarl_w1_split": (0,),
           "rcmarl_layer1_forward_lattice": (6,), "rcmarl_layer1_backward_sgd_lattice_tiled": (7,),
           "rcmarl_layer1_backward_sgd_lattice": (7,), "rcmarl_mid_fit": (1,), "rcmarl_layer1_backward_sgd": (3,)}
B_ARG = {"rcmarl_layer1_forward_lattice": 10}


class CountingLib:
    """the library with a record of the local fit's launches: (entry point, the parameter matrices it was handed, B where watched)"""

    def __init__(self, lib):
        self._lib = lib
        self.calls = []
        self.names = {}                   # data_ptr -> "theta:critic", "msg:tr", ...

    def __getattr__(self, name):
        fn = getattr(self._lib, name)
        if name not in WATCHED:
            return fn

        def counted(*a):
            ptrs = tuple(self.names.get(a[i], "other") for i in WATCHED[name])
            self.calls.append((name, ptrs, a[B_ARG[name]] if name in B_ARG else None))
            return fn(*a)
        return counted


N_AG, EP_LEN, N_EP, BLOCK_B = 16, 10, 10, 100
COOP16 = ["Cooperative"] * N_AG
GREEDY16 = ["Cooperative"] * 7 + ["Greedy"] + ["Cooperative"] * 8


_RUNS = {}


def run(device, lib, labels, fit_from_live, w1_tiled="auto", td_from_fit_forward=True):
    """one engine run per combination of switches, shared by the checks below (nobody changes what it returns)"""
    key = (device, id(lib), tuple(labels), fit_from_live, w1_tiled, td_from_fit_forward)
    if key not in _RUNS:
        _RUNS[key] = _run(device, lib, labels, fit_from_live, w1_tiled, td_from_fit_forward)
    return _RUNS[key]


def _run(device, lib, labels, fit_from_live, w1_tiled, td_from_fit_forward, seeds=(51,)):
    """16 agents on a ring, H = 1, 5 x 5 grid, one block of B = 100 rows and two epochs.  Before every epoch the parameters of both
    messages are overwritten with NaN (whoever relies on a value of the previous epoch's message shows), after every epoch theta, msg
    and the losses of both nets are kept.  -> engine, launches per epoch, snapshots per epoch"""
    from rcmarl_amd import capi
    from rcmarl_amd.engine import EngineConfig, RPBCACEngine
    n = N_AG
    in_nodes = [[i, (i + 1) % n, (i - 1) % n] for i in range(n)]               # a ring, own value first
    wrng = np.random.default_rng(5)
    M = EC.M
    W = [[{"actor": M.init_mlp(wrng, 2 * n, 20, 5), "critic": M.init_mlp(wrng, 2 * n, 20, 1), "tr": M.init_mlp(wrng, 3 * n, 20, 1)}
          for _ in range(n)] for _ in seeds]
    goals = np.stack([np.random.default_rng(100 + s).integers(0, 5, size=(n, 2)) for s in range(len(seeds))])
    cfg = EngineConfig(n, labels, in_nodes, H=1, max_ep_len=EP_LEN, n_ep_fixed=N_EP, n_epochs=2, buffer_size=BLOCK_B, nrow=5, ncol=5,
                       n_seeds=len(seeds), rng_mode="device", lattice=True, w1_tiled=w1_tiled, fit_from_live=fit_from_live)
    clib = CountingLib(lib if lib is not None else capi.load())
    eng = RPBCACEngine(cfg, seeds=list(seeds), device=device, lib=clib)
    eng.td_from_fit_forward = td_from_fit_forward
    for net in ("critic", "tr"):
        clib.names[eng.theta[net].data_ptr()] = "theta:" + net
        clib.names[eng.msg[net].data_ptr()] = "msg:" + net
    for s in range(len(seeds)):
        for i in range(n):
            for net in ("actor", "critic", "tr"):
                eng.set_weights(s, i, net, W[s][i][net])
    eng.set_goals(goals)
    epochs, snaps = [], []
    inner = eng._epoch

    def epoch(B, e, t0):
        assert B == BLOCK_B
        for net in ("critic", "tr"):
            eng.msg[net][:, :, :eng.P[net]] = float("nan")
        first = len(clib.calls)
        r = inner(B, e, t0)
        eng.sync()
        epochs.append(clib.calls[first:])
        snaps.append({"%s:%s" % (what, net): t[net].detach().cpu().numpy().copy()
                      for what, t in (("theta", eng.theta), ("msg", eng.msg), ("loss", eng.loss)) for net in ("critic", "tr")})
        return r
    eng._epoch = epoch
    eng.train(N_EP)
    eng.sync()
    assert len(epochs) == 2 and eng.lat_active and eng.lat_B == BLOCK_B
    return eng, epochs, snaps


def assert_same_snapshots(a, b):
    assert len(a) == len(b) == 2
    for e, (x, y) in enumerate(zip(a, b)):
        for k in x:
            assert np.isfinite(x[k]).all(), (e, k)
            np.testing.assert_array_equal(x[k].view(np.uint32), y[k].view(np.uint32), err_msg="%s after epoch %d" % (k, e))


def fits(calls):
    """the launches of one epoch grouped per local fit: {net: {entry point: [pointer names ...]}}, in launch order"""
    out = {}
    for name, ptrs, _ in calls:
        if name in ("rcmarl_w1_split", "rcmarl_layer1_forward_lattice") or ptrs[-1] == "other":       # (other: an adversary's own fit)
            continue
        net = ptrs[-1].split(":")[1]
        out.setdefault(net, []).append((name, ptrs))
    return out


def check_engine_live_equals_copy(device, lib):
    """All-cooperative team: the rule holds for both nets.  Results word for word those of the run that copies; step 0 of every fit
    is handed theta, the later steps msg."""
    eng_on, ep_on, snap_on = run(device, lib, COOP16, True)
    eng_off, ep_off, snap_off = run(device, lib, COOP16, False)
    for net, xkey in (("critic", "s"), ("tr", "sa")):
        assert eng_on._fit_from_live(net, xkey, BLOCK_B, eng_on.coop) and not eng_off._fit_from_live(net, xkey, BLOCK_B, eng_off.coop)
    assert_same_snapshots(snap_on, snap_off)
    steps = eng_on.cfg.local_fit_steps
    assert steps == 5
    for e in range(2):
        f_on, f_off = fits(ep_on[e]), fits(ep_off[e])
        assert list(f_on) == list(f_off) == ["tr", "critic"]
        for net in ("tr", "critic"):
            th, msg = "theta:" + net, "msg:" + net
            want_on = [("rcmarl_mid_fit_lattice", (th,)), ("rcmarl_small_sgd_from", (th, msg)), ("rcmarl_layer1_backward_sgd_lattice_tiled", (th,))]
            want_rest = [("rcmarl_mid_fit_lattice", (msg,)), ("rcmarl_small_sgd", (msg,)), ("rcmarl_layer1_backward_sgd_lattice_tiled", (msg,))]
            assert f_on[net] == want_on + want_rest * (steps - 1), f_on[net]
            assert f_off[net] == want_rest * steps, f_off[net]
    # the forward passes and W1 splits: the same in both runs, except that step 0 of an uncached fit reads theta (epoch 0: the
    # team-reward net; the critic's activations are those the TD target's forward left)
    fw = lambda calls: [(n, p, b) for n, p, b in calls if n in ("rcmarl_w1_split", "rcmarl_layer1_forward_lattice")]
    for e in range(2):
        a, b = fw(ep_on[e]), fw(ep_off[e])
        assert len(a) == len(b) and [(n, bb) for n, _, bb in a] == [(n, bb) for n, _, bb in b]
        diff = [(x, y) for x, y in zip(a, b) if x != y]
        want = [("theta:tr",), ("msg:tr",)]
        assert all([x[1], y[1]] == want for x, y in diff) and len(diff) == (2 if e == 0 else 0), diff
    return eng_on


def check_engine_td_from_fit_forward(device, lib):
    """The first epoch's TD target from the forward pass that opens the critic's fit, against a TD target that runs its own forward
    pass over the ns rows (td_from_fit_forward off: the engine as it was): the same results word for word, one full-size forward
    launch and one W1 split less -- in their place the small forward over the last next state of every episode, as in every later
    epoch."""
    fw = lambda calls: [(n, p, b) for n, p, b in calls if n in ("rcmarl_w1_split", "rcmarl_layer1_forward_lattice")]
    eng_on, ep_on, snap_on = run(device, lib, COOP16, True)
    eng_td, ep_td, snap_td = run(device, lib, COOP16, True, td_from_fit_forward=False)
    assert_same_snapshots(snap_on, snap_td)
    count = lambda calls, name, B=None: sum(1 for n, _, b in calls if n == name and (B is None or b == B))
    nt = BLOCK_B // EP_LEN                                                     # the last next state of every episode: a forward of its own
    assert count(ep_td[0], "rcmarl_w1_split") - count(ep_on[0], "rcmarl_w1_split") == 1
    assert count(ep_td[0], "rcmarl_layer1_forward_lattice", BLOCK_B) - count(ep_on[0], "rcmarl_layer1_forward_lattice", BLOCK_B) == 1
    assert count(ep_on[0], "rcmarl_layer1_forward_lattice", nt) == 1 and count(ep_td[0], "rcmarl_layer1_forward_lattice", nt) == 0
    assert fw(ep_on[1]) == fw(ep_td[1])                                        # later epochs: nothing changed


def check_engine_rule_off(device, lib, labels, w1_tiled="auto"):
    """A team with a Greedy agent, or W1 strided between the steps: fit_from_live=True changes nothing -- the same launches with the
    same parameter matrices (msg everywhere) as with False, the copy in front of every epoch (without it the NaN the run plants in
    the messages would reach the weights), the same results."""
    eng_on, ep_on, snap_on = run(device, lib, labels, True, w1_tiled=w1_tiled)
    eng_off, ep_off, snap_off = run(device, lib, labels, False, w1_tiled=w1_tiled)
    for net, xkey in (("critic", "s"), ("tr", "sa")):
        assert not eng_on._fit_from_live(net, xkey, BLOCK_B, eng_on.coop)
    assert ep_on == ep_off
    for calls in ep_on:
        f = fits(calls)
        assert list(f) == ["tr", "critic"]
        for net in f:
            assert len(f[net]) == 15 and all(p == ("msg:" + net,) for _, p in f[net]), f[net]
            assert not any(n == "rcmarl_small_sgd_from" for n, _ in f[net])
    assert_same_snapshots(snap_on, snap_off)


# ---- no GPU -----------------------------------------------------------------------------------------------------------------------
def check_arg_errors(lib):
    """bad calls come back as RCMARL_ERR_ARG before the HIP runtime is touched (the pointers below are never dereferenced)"""
    import pytest
    from rcmarl_amd.capi import RcmarlError
    fake = 0x10000
    good = [fake, fake, fake, None, None, 1, 5, 100, 10, HID, 704, 0.01, None]
    bad = {"NULL src": {1: None}, "NULL dst": {2: None}, "NULL partials": {0: None}, "no seeds": {5: 0}, "no agents": {6: 0}, "no rows": {7: 0}}
    for what, change in bad.items():
        args = list(good)
        for k, v in change.items():
            args[k] = v
        with pytest.raises(RcmarlError, match="RCMARL_ERR_ARG"):
            lib.rcmarl_small_sgd_from(*args)
    args = list(good)
    args[9] = 21                                                               # a width the 20-unit kernels are not compiled for
    with pytest.raises(RcmarlError, match="RCMARL_ERR_UNSUPPORTED"):
        lib.rcmarl_small_sgd_from(*args)
    with pytest.raises(RcmarlError, match="RCMARL_ERR_ARG"):                   # the in-place entry point is the new one with src == dst
        lib.rcmarl_small_sgd(fake, None, None, None, 1, 5, 100, 10, HID, 704, 0.01, None)


def check_exports(lib_path):
    import re
    import subprocess
    from rcmarl_amd import capi
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = subprocess.run(["nm", "-D", "--defined-only", lib_path], capture_output=True, text=True).stdout
    exported = set(re.findall(r"\bT (rcmarl_\w+)", out))
    header = open(os.path.join(root, "include", "rcmarl.h")).read()
    for name in ("rcmarl_small_sgd_from", "rcmarl_small_sgd"):
        assert name in exported and re.search(r"\bint\s+%s\s*\(" % name, header), name
    # the new launch takes the old one's arguments with (src, dst) in the place of theta
    old, new = capi.SIGNATURES["rcmarl_small_sgd"], capi.SIGNATURES["rcmarl_small_sgd_from"]
    assert new == old[:1] + [old[1], old[1]] + old[2:]


def check_config_switch():
    import pytest
    from rcmarl_amd import engine as E
    in_nodes = [[i, (i + 1) % 5, (i + 2) % 5, (i + 3) % 5] for i in range(5)]
    assert E.EngineConfig(5, ["Cooperative"] * 5, in_nodes, H=1).fit_from_live == "auto" and isinstance(E.FIT_FROM_LIVE_AUTO, bool)
    for v in (True, False):
        assert E.EngineConfig(5, ["Cooperative"] * 5, in_nodes, H=1, fit_from_live=v).fit_from_live is v
    with pytest.raises(ValueError, match="fit_from_live"):
        E.EngineConfig(5, ["Cooperative"] * 5, in_nodes, H=1, fit_from_live=1)
