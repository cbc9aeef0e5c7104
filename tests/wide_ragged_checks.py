"""Wide nets (any hidden width) on irregular communication graphs: rcmarl_wide_consensus_head_ragged (csrc/wide_head_ragged.hip)
and the engine's ragged_wide switch, shared by the hipemu (CPU) tests and the GPU tests.

Kernel checks take a *backend* (bk.lib, bk.dev, bk.ptr, bk.host, bk.stream), engine checks (device, lib), as ragged_checks.py.  The
references are the oracle (fp32 bars of wide_checks.check_wide_consensus_head: the forward pass runs in its fp32 form here) and the
uniform entry rcmarl_wide_consensus_head called once per class with a dense table and the class mask (bits)."""
import contextlib
import ctypes

import numpy as np

import engine_checks as EC
import ragged_checks as RC
import wide_checks as WC
from kernel_checks import circulant, pack_rows, pad64, random_regular, unpack_row
from oracle import mlp_np as M
from oracle import rpbcac_oracle as O
from rcmarl_amd import capi
from rcmarl_amd.engine import EngineConfig, RPBCACEngine
from wide_checks import WideBuffers, forward2, rel_close, wide_params

DEGREES_A = RC.K1_DEGREES                   # (1, 3, 4, 5, 7, 12, 21) on N = 24
DEGREES_B = (1, 4, 21, 31, 32, 33)          # on N = 36: d + 1 straddling one and two head tiles
SENTINEL = np.float32(-7.25e9)              # what the outputs hold before a call: a row the kernel must not write keeps it


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


@contextlib.contextmanager
def fp32_form(lib):
    """the dense layers of wide nets in their fp32 form (rcmarl_wide_set_f16_mode(0)) inside, the form found on entry afterwards"""
    prev = lib.rcmarl_wide_f16_mode()
    lib.rcmarl_wide_set_f16_mode(0)
    try:
        yield
    finally:
        lib.rcmarl_wide_set_f16_mode(prev)


# ---- inputs ---------------------------------------------------------------------------------------------------------------
def make_case(S, N, B, hid, seed, degrees=DEGREES_A, in_dim=10, graph=None, n_noncoop=3):
    """live nets, messages (one outlier head, x50, as wide_checks), replay rows and an irregular graph (graph = (in_nodes, H, coop)
    overrides ragged_checks.ragged_graph)"""
    rng = np.random.default_rng(seed)
    g = WC.wgeom(in_dim, hid)
    ldp, ldb = pad64(g["P"]), pad64(B)
    live, msgp = wide_params(rng, S, N, in_dim, hid), wide_params(rng, S, N, in_dim, hid)
    theta, msg = pack_rows(live, ldp), pack_rows(msgp, ldp)
    x = rng.normal(size=(S, B, in_dim)).astype(np.float32)
    in_nodes, H, coop = RC.ragged_graph(N, rng, degrees=degrees, n_noncoop=n_noncoop) if graph is None else graph
    if graph is None:                   # the extreme H of every degree (and H = 0 where a second agent allows it) among the COOPERATIVE agents
        for d in degrees:
            idx = [i for i in range(N) if len(in_nodes[i]) == d and coop[i]]
            H[idx[0]] = (d - 1) // 2
            if len(idx) > 1:
                H[idx[1]] = 0
    for s in range(S):
        msg[s, 1, g["P_hid"]:g["P"]] *= np.float32(50.0)
        msgp[s][1][4] = msgp[s][1][4] * np.float32(50.0)
        msgp[s][1][5] = msgp[s][1][5] * np.float32(50.0)
    return dict(S=S, N=N, B=B, hid=hid, in_dim=in_dim, g=g, ldp=ldp, ldb=ldb, live=live, msgp=msgp, theta=theta, msg=msg, x=x,
                in_nodes=in_nodes, H=list(H), coop=np.asarray(coop, np.int32), rng=rng)


def features(bk, c):
    """phi = layer-2 activations of the live nets in the fp32 form, [S][N*hid][ldb] on the host; computed once per case"""
    if "phi" not in c:
        S, N, B, hid, in_dim, ldp, ldb = (c[k] for k in ("S", "N", "B", "hid", "in_dim", "ldp", "ldb"))
        wb = WideBuffers(bk, S, N, B, hid)
        with fp32_form(bk.lib):
            forward2(bk, wb, bk.dev(c["x"]), B * in_dim, bk.dev(c["theta"]), S, N, B, in_dim, hid, ldp, ldb)
        c["phi"] = np.array(bk.host(wb.a2))
        a2 = c["phi"].reshape(S, N, hid, ldb).astype(np.float64)
        h2 = max(1, hid // 2)            # |phi|^2 as two parts, summed in fp64 on the host (wide_checks.check_wide_consensus_head)
        c["nparts"] = np.stack([(a2[:, :, :h2] ** 2).sum(axis=2), (a2[:, :, h2:] ** 2).sum(axis=2)], axis=2).astype(np.float32)
    return c["phi"]


def run_ragged(bk, c, classes=None, seeds=None, nparts=False, dbg=True):
    """one call of the ragged entry (all classes, or the given subset of the class table; `seeds`: a slice of the seeds) on outputs
    pre-filled with SENTINEL, then the head apply.  Returns the host copies."""
    N, B, hid, in_dim, ldp, ldb = (c[k] for k in ("N", "B", "hid", "in_dim", "ldp", "ldb"))
    phi = features(bk, c)
    sl = slice(0, c["S"]) if seeds is None else seeds
    S = len(range(*sl.indices(c["S"])))
    off, idx, order, all_classes, _ = RC.csr_and_classes(c["in_nodes"], c["H"], c["coop"])
    classes = all_classes if classes is None else classes
    table = (capi.RaggedClass * len(classes))(*[capi.RaggedClass(*k) for k in classes])
    lde = max(k[0] for k in all_classes) + 2                       # one slot more than needed: it must stay untouched
    L = bk.lib
    gs = L.rcmarl_wide_grad_size(hid)
    fill = lambda *sh: bk.dev(np.full(sh, SENTINEL, np.float32))
    d_ebuf, d_grads, d_agg = fill(S, N, ldb), fill(S, N, gs), fill(S, N, ldb)
    d_est = fill(S, N, lde, ldb) if dbg else None
    d_phi, d_th, d_msg = bk.dev(phi[sl]), bk.dev(c["theta"][sl]), bk.dev(c["msg"][sl])
    d_np = bk.dev(c["nparts"][sl]) if nparts else None
    d_off, d_idx, d_order = bk.dev(off), bk.dev(idx), bk.dev(order)
    L.rcmarl_wide_consensus_head_ragged(bk.ptr(d_phi), bk.ptr(d_np) if nparts else None, 2 if nparts else 0, bk.ptr(d_th), bk.ptr(d_msg),
                                        bk.ptr(d_off), bk.ptr(d_idx), bk.ptr(d_order), table, len(classes), bk.ptr(d_ebuf),
                                        bk.ptr(d_grads), bk.ptr(d_agg), bk.ptr(d_est) if dbg else None, lde if dbg else 0, S, N, B,
                                        in_dim, hid, ldp, ldb, bk.stream)
    out = dict(ebuf=np.array(bk.host(d_ebuf)), grads=np.array(bk.host(d_grads)), agg=np.array(bk.host(d_agg)),
               est=np.array(bk.host(d_est)) if dbg else None, classes=classes, order=order, lde=lde)
    listed = np.zeros(N, np.int32)
    for _, _, first, count in classes:
        listed[order[first:first + count]] = 1
    L.rcmarl_wide_head_apply(bk.ptr(d_grads), bk.ptr(d_th), bk.ptr(bk.dev(listed)), S, N, B, in_dim, hid, ldp, bk.stream)
    out["theta"], out["listed"] = np.array(bk.host(d_th)), listed
    return out


def run_uniform_class(bk, c, members, d, h, nparts=False):
    """rcmarl_wide_consensus_head[_nrm] for ONE class: dense table of its rows, coop masked to the class (hmat / hb / est scratch
    sized by this d), then the head apply with the same mask"""
    S, N, B, hid, in_dim, ldp, ldb = (c[k] for k in ("S", "N", "B", "hid", "in_dim", "ldp", "ldb"))
    nbr, mask = RC.dense_table_of_class(c["in_nodes"], members, d)
    wb = WideBuffers(bk, S, N, B, hid, d)
    L = bk.lib
    d_phi, d_th, d_msg, d_nbr, d_mask = bk.dev(features(bk, c)), bk.dev(c["theta"]), bk.dev(c["msg"]), bk.dev(nbr), bk.dev(mask)
    d_agg = bk.dev(np.zeros((S, N, ldb), np.float32))
    with fp32_form(L):
        if nparts:
            d_np = bk.dev(c["nparts"])
            L.rcmarl_wide_consensus_head_nrm(bk.ptr(d_phi), bk.ptr(d_np), 2, bk.ptr(d_th), bk.ptr(d_msg), bk.ptr(d_nbr), bk.ptr(d_mask),
                                             bk.ptr(wb.hmat), bk.ptr(wb.hb), bk.ptr(wb.est), bk.ptr(wb.ebuf), bk.ptr(wb.grads),
                                             bk.ptr(d_agg), S, N, B, in_dim, hid, ldp, ldb, d, h, bk.stream)
        else:
            L.rcmarl_wide_consensus_head(bk.ptr(d_phi), bk.ptr(d_th), bk.ptr(d_msg), bk.ptr(d_nbr), bk.ptr(d_mask), None, bk.ptr(wb.hmat),
                                         bk.ptr(wb.hb), bk.ptr(wb.est), bk.ptr(wb.ebuf), bk.ptr(wb.grads), bk.ptr(d_agg), S, N, B,
                                         in_dim, hid, ldp, ldb, d, h, bk.stream)
    out = dict(ebuf=np.array(bk.host(wb.ebuf)), grads=np.array(bk.host(wb.grads)), agg=np.array(bk.host(d_agg)),
               est=np.array(bk.host(wb.est)))
    L.rcmarl_wide_head_apply(bk.ptr(wb.grads), bk.ptr(d_th), bk.ptr(d_mask), S, N, B, in_dim, hid, ldp, bk.stream)
    out["theta"] = np.array(bk.host(d_th))
    return out


# ---- the checks ------------------------------------------------------------------------------------------------------------
def check_untouched(c, out):
    """nothing else is written: rows of agents that are not listed, columns b >= B, slots of est_dbg beyond d_i"""
    B, hid = c["B"], c["hid"]
    sent = _bits(np.asarray([SENTINEL]))[0]
    for i in range(c["N"]):
        if not out["listed"][i]:
            assert (_bits(out["ebuf"][:, i]) == sent).all() and (_bits(out["grads"][:, i]) == sent).all(), "agent %d is not listed" % i
            assert (_bits(out["agg"][:, i]) == sent).all()
            np.testing.assert_array_equal(_bits(out["theta"][:, i]), _bits(c["theta"][:out["theta"].shape[0], i]))
            if out["est"] is not None:
                assert (_bits(out["est"][:, i]) == sent).all()
            continue
        d = len(c["in_nodes"][i])
        assert (_bits(out["ebuf"][:, i, B:]) == sent).all() and (_bits(out["agg"][:, i, B:]) == sent).all(), "columns b >= B, agent %d" % i
        assert (_bits(out["grads"][:, i, hid + 1:]) == sent).all(), "grads beyond [gW3 | gb3], agent %d" % i
        assert not (_bits(out["ebuf"][:, i, :B]) == sent).any() and not (_bits(out["grads"][:, i, :hid + 1]) == sent).any()
        if out["est"] is not None:
            assert (_bits(out["est"][:, i, d + 1:]) == sent).all(), "est_dbg slots beyond d_i, agent %d" % i
            assert (_bits(out["est"][:, i, :d + 1, B:]) == sent).all()
            assert not (_bits(out["est"][:, i, :d + 1, :B]) == sent).any()


def check_oracle(c, out):
    """check 1: aggregates and W3, b3 after the apply against the oracle agent at the fp32 bars of
    wide_checks.check_wide_consensus_head (aggregate 1e-5 up to 128 units, W3 / b3 3e-5); hidden layers bit-unchanged"""
    S, N, B, hid, in_dim = (c[k] for k in ("S", "N", "B", "hid", "in_dim"))
    assert hid <= 128
    worst = {"agg": 0.0, "W3": 0.0}
    for s in range(S):
        for i in range(N):
            if not out["listed"][i]:
                continue
            ag = O.CoopAgent(M.init_mlp(c["rng"], in_dim, 20, 5), c["live"][s][i], c["live"][s][i], 0.002, 0.01, 0.9, c["H"][i])
            want = ag.consensus_estimates_critic(c["x"][s], [c["msgp"][s][j] for j in c["in_nodes"][i]])
            what = "agent %d (d %d, H %d)" % (i, len(c["in_nodes"][i]), c["H"][i])
            rel_close(out["agg"][s, i, :B], want[:, 0], 1e-5, "estimate aggregate, " + what)
            worst["agg"] = max(worst["agg"], float(np.abs(out["agg"][s, i, :B] - want[:, 0]).max()) / max(1.0, float(np.abs(want).max())))
            ag.projection_step_critic(c["x"][s], want)
            got = unpack_row(out["theta"][s, i], in_dim, 1, hid)
            for k in range(4):
                np.testing.assert_array_equal(got[k], c["live"][s][i][k])          # hidden layers frozen
            rel_close(got[4], ag.critic[4], 3e-5, "W3 after projection, " + what)
            rel_close(got[5], ag.critic[5], 3e-5, "b3 after projection, " + what)
            worst["W3"] = max(worst["W3"], float(np.abs(got[4] - ag.critic[4]).max()) / max(1.0, float(np.abs(ag.critic[4]).max())))
    print("[parity] ragged wide head (%d units): worst aggregate %.2e (bar 1e-5), W3 after projection %.2e (bar 3e-5)"
          % (hid, worst["agg"], worst["W3"]))


def check_aggregation_alone(c, out):
    """check 2: from the kernel's own estimates (est_dbg) the aggregate is within 1e-6 max(1, |x|) of oracle.resilient_aggregate
    (the K1 bar) and inside the window of oracle.aggregation_bounds.  "Inside" for an fp32 mean: the exact mean of d values clipped
    into [lo, hi] lies in the window, the computed one carries d - 1 roundings of the running sum and one of the division, each at
    most 2^-24 relative -- so it may leave the window by d 2^-24 max(|lo|, |hi|) and no more (H = (d - 1) / 2 makes lo == hi: seven
    copies of one value do not always sum and divide back to it)."""
    B = c["B"]
    for s in range(out["agg"].shape[0]):
        for i in range(c["N"]):
            if not out["listed"][i]:
                continue
            d, h = len(c["in_nodes"][i]), c["H"][i]
            vals = out["est"][s, i, :d, :B]
            want = O.resilient_aggregate(vals, h)
            got = out["agg"][s, i, :B]
            assert (np.abs(got - want) / np.maximum(1.0, np.abs(want))).max() <= 1e-6, (i, d, h)
            lo, hi, _ = O.aggregation_bounds(vals, h)
            slack = d * 2.0 ** -24 * np.maximum(np.abs(lo), np.abs(hi))
            assert (got >= lo - slack).all() and (got <= hi + slack).all(), (i, d, h)


def check_classes_against_uniform(bk, c, out, out_nrm=None, classes=None):
    """check 3: per class, rcmarl_wide_consensus_head in its fp32 form with the dense table and the class mask: aggregates and
    estimates bit-equal, ebuf and theta after the apply within 2e-6 (only the |phi|^2 summation differs, wide_checks.py:210); with
    the same nparts handed to both entries (out_nrm) ebuf and grads bit-equal too"""
    B, hid, P = c["B"], c["hid"], c["g"]["P"]
    for d, h, first, count in (out["classes"] if classes is None else classes):
        members = [int(i) for i in out["order"][first:first + count]]
        uni = run_uniform_class(bk, c, members, d, h)
        uni_n = run_uniform_class(bk, c, members, d, h, nparts=True) if out_nrm is not None else None
        for i in members:
            what = "agent %d of class (d %d, H %d)" % (i, d, h)
            np.testing.assert_array_equal(_bits(out["agg"][:, i, :B]), _bits(uni["agg"][:, i, :B]), err_msg="aggregate, " + what)
            np.testing.assert_array_equal(_bits(out["est"][:, i, :d + 1, :B]), _bits(uni["est"][:, i, :, :B]), err_msg="estimates, " + what)
            rel_close(out["ebuf"][:, i, :B], uni["ebuf"][:, i, :B], 2e-6, "ebuf, " + what)
            rel_close(out["theta"][:, i, :P], uni["theta"][:, i, :P], 2e-6, "theta after the apply, " + what)
            if out_nrm is not None:
                np.testing.assert_array_equal(_bits(out_nrm["agg"][:, i, :B]), _bits(uni_n["agg"][:, i, :B]))
                np.testing.assert_array_equal(_bits(out_nrm["ebuf"][:, i, :B]), _bits(uni_n["ebuf"][:, i, :B]), err_msg="ebuf (nparts), " + what)
                np.testing.assert_array_equal(_bits(out_nrm["grads"][:, i, :hid + 1]), _bits(uni_n["grads"][:, i, :hid + 1]),
                                              err_msg="grads (nparts), " + what)
                np.testing.assert_array_equal(_bits(out_nrm["theta"][:, i]), _bits(uni_n["theta"][:, i]))


def check_kernel(bk, hid, B, S, degrees=DEGREES_A, N=24, seed=0, uniform_classes=None):
    """checks 1, 2, 3 and the sentinel check on one irregular instance (and with nparts where hid is 128: the packed path's width)"""
    c = make_case(S, N, B, hid, 1000 * hid + 10 * B + S + seed, degrees=degrees)
    assert sorted(set(len(r) for r in c["in_nodes"])) == sorted(degrees) and int((c["coop"] == 0).sum()) == 3
    out = run_ragged(bk, c)
    assert {d for d, _, _, _ in out["classes"]} == set(degrees) and any(h == 0 for _, h, _, _ in out["classes"])
    assert all(any(h == (d - 1) // 2 for dd, h, _, _ in out["classes"] if dd == d) for d in degrees)     # every degree with its extreme H
    check_untouched(c, out)
    check_oracle(c, out)
    check_aggregation_alone(c, out)
    out_nrm = run_ragged(bk, c, nparts=True) if hid == 128 else None
    if out_nrm is not None:
        check_untouched(c, out_nrm)
        np.testing.assert_array_equal(_bits(out_nrm["agg"]), _bits(out["agg"]))          # (the aggregate does not depend on the norm)
        np.testing.assert_array_equal(_bits(out_nrm["est"]), _bits(out["est"]))
    pick = out["classes"] if uniform_classes is None else [k for k in out["classes"] if k[0] in uniform_classes]
    assert pick
    check_classes_against_uniform(bk, c, out, out_nrm, classes=pick)
    return c, out


def check_regular_as_one_class(bk, N, d, H, graph, hid=24, B=70, S=2):
    """check 4: a regular graph handed over as ONE class gives what a single uniform call gives (check 3's statements)"""
    rng = np.random.default_rng(N * 100 + d * 7 + H)
    nbr = circulant(N, d) if graph == "circ" else random_regular(N, d, rng)
    coop = np.ones(N, np.int32)
    coop[N - 1] = 0
    c = make_case(S, N, B, hid, N + d + H, graph=([[int(j) for j in row] for row in nbr], [H] * N, coop))
    out = run_ragged(bk, c)
    assert out["classes"] == [(d, H, 0, N - 1)]
    check_untouched(c, out)
    check_aggregation_alone(c, out)
    check_classes_against_uniform(bk, c, out, run_ragged(bk, c, nparts=True))


def check_independence(bk, hid=24, B=130, S=2):
    """check 5: the full call against a call listing one class only and against a call with S = 1 on seed 0's slices: the listed
    agents' ebuf, grads and aggregates are bit-equal"""
    c = make_case(S, 24, B, hid, 77)
    full = run_ragged(bk, c, dbg=False)
    one = full["classes"][len(full["classes"]) // 2]
    alone = run_ragged(bk, c, classes=[one], dbg=False)
    check_untouched(c, alone)
    members = full["order"][one[2]:one[2] + one[3]]
    assert len(members) and int(alone["listed"].sum()) == len(members)
    for key in ("ebuf", "grads", "agg", "theta"):
        np.testing.assert_array_equal(_bits(alone[key][:, members]), _bits(full[key][:, members]), err_msg=key + ", one class alone")
    s0 = run_ragged(bk, c, seeds=slice(0, 1), dbg=False)
    for key in ("ebuf", "grads", "agg", "theta"):
        np.testing.assert_array_equal(_bits(s0[key][0]), _bits(full[key][0]), err_msg=key + ", seed 0 alone")


def check_more_than_32_classes(bk, N=60, hid=24, B=40, seed=8, uniform_classes=None):
    """check 6: the 54 classes of ragged_checks.check_k1_ragged_more_classes_than_one_launch_takes: check 1's bars, check 3's bits
    (uniform_classes: the degrees whose classes are compared with the uniform entry; default all)"""
    rng = np.random.default_rng(seed)
    pairs = [(d, h) for d in range(3, 20, 2) for h in range((d - 1) // 2 + 1)]
    assert len(pairs) == 54 and N >= len(pairs)
    pairs = pairs + [pairs[int(k)] for k in rng.integers(0, len(pairs), size=N - len(pairs))]
    pairs = [pairs[k] for k in rng.permutation(N)]
    in_nodes = [[i] + [int(j) for j in rng.permutation([j for j in range(N) if j != i])[:d - 1]] for i, (d, _) in enumerate(pairs)]
    c = make_case(1, N, B, hid, seed, graph=(in_nodes, [h for _, h in pairs], np.ones(N, np.int32)))
    out = run_ragged(bk, c)
    assert len(out["classes"]) == 54
    check_untouched(c, out)
    check_oracle(c, out)
    check_aggregation_alone(c, out)
    check_classes_against_uniform(bk, c, out, classes=[k for k in out["classes"] if uniform_classes is None or k[0] in uniform_classes])


def check_determinism(bk, hid=33, B=130, S=2):
    """check 7: two identical calls give identical bits"""
    c = make_case(S, 24, B, hid, 5)
    a, b = run_ragged(bk, c), run_ragged(bk, c)
    for key in ("ebuf", "grads", "agg", "est", "theta"):
        np.testing.assert_array_equal(_bits(a[key]), _bits(b[key]), err_msg=key)


# ---- argument validation and the coverage query (no GPU) --------------------------------------------------------------------
def check_argument_validation(lib):
    """check 8: every RCMARL_ERR_ARG case with a never-dereferenced non-null pointer; RCMARL_ERR_UNSUPPORTED and the query's 0 for
    a d beyond the kernel's LDS tile; the query's 1 at BASELINE configs[4]'s (512 units, d = 66)"""
    import pytest
    one = ctypes.c_void_p(64)
    cls = lambda d, h, first, count: (capi.RaggedClass * 1)(capi.RaggedClass(d, h, first, count))
    # phi, nparts, n_parts, theta, msg, nbr_off, nbr_idx, order, classes, n_classes, ebuf, grads, agg_out, est_dbg, lde, S, N, B,
    # in_dim, hid, ldp, ldb, stream
    good = [one, None, 0, one, one, one, one, one, cls(3, 1, 0, 2), 1, one, one, None, None, 0, 1, 5, 100, 10, 32, 1472, 128, None]
    bad = [{0: None}, {3: None}, {4: None}, {5: None}, {6: None}, {7: None}, {8: None}, {10: None}, {11: None},       # required pointers
           {1: one, 2: 0}, {1: one, 2: -1},                                                                            # nparts without parts
           {13: one, 14: 3}, {13: one, 14: 0},                                                                         # lde < max d + 1
           {8: cls(2, 1, 0, 2)}, {8: cls(6, 1, 0, 2)}, {8: cls(3, -1, 0, 2)}, {8: cls(3, 1, 0, 0)}, {8: cls(3, 1, -1, 2)},
           {8: cls(0, 0, 0, 2)}, {8: cls(3, 1, 4, 2)},
           {9: 0}, {9: -1},                                                                                            # n_classes
           {15: 0}, {16: 0}, {17: 0}, {18: 0}, {19: 0}, {20: 0}, {21: 64}]                                             # w_dims_ok
    for change in bad:
        args = list(good)
        for k, v in change.items():
            args[k] = v
        with pytest.raises(capi.RcmarlError, match="RCMARL_ERR_ARG"):
            lib.rcmarl_wide_consensus_head_ragged(*args)
    q = lib.rcmarl_wide_consensus_head_ragged_supported
    assert q(512, 66) == 1 and q(24, 1) == 1 and q(1, 33) == 1 and q(2048, 66) == 1
    assert q(0, 4) == 0 and q(32, 0) == 0
    far = 4000                              # (d + 1) x 128 estimates alone are 2 MB: beyond any CU's 160 KiB
    assert q(32, far) == 0
    args = list(good)
    args[8], args[16] = cls(far, 1, 0, 2), far + 5
    with pytest.raises(capi.RcmarlError, match="RCMARL_ERR_UNSUPPORTED"):
        lib.rcmarl_wide_consensus_head_ragged(*args)
    d_end = max(d for d in range(1, far) if q(32, d))
    assert d_end >= 66 and all(q(32, d) == 1 for d in range(1, d_end + 1)) and q(32, d_end + 1) == 0
    assert (d_end + 1) * 128 * 4 <= 160 * 1024
    args[8], args[16] = cls(d_end + 1, 1, 0, 2), far + 5
    with pytest.raises(capi.RcmarlError, match="RCMARL_ERR_UNSUPPORTED"):
        lib.rcmarl_wide_consensus_head_ragged(*args)


# ---- engine against the oracle ------------------------------------------------------------------------------------------------
def engine_inputs(args, seeds, critic_hid, tr_hid, actor_hid=20, weight_seed=3):
    """initial weights of the given widths and goals of every seed (engine_checks.make_inputs with a width per net)"""
    n = args["n_agents"]
    rng = np.random.default_rng(weight_seed)
    W = [[{"actor": M.init_mlp(rng, 2 * n, actor_hid, 5), "critic": M.init_mlp(rng, 2 * n, critic_hid, 1),
           "tr": M.init_mlp(rng, 3 * n, tr_hid, 1)} for _ in range(n)] for _ in seeds]
    goals = [np.random.default_rng(100 + s).integers(0, 5, size=(n, 2)) for s in range(len(seeds))]
    return W, goals


def make_engine(args, rng_mode, device, lib, seeds, W, goals, critic_hid=20, tr_hid=20, actor_hid=20, lattice=False, **kw):
    """engine_checks.run_engine's engine with a width per net and ragged_wide='auto' (kw: further EngineConfig keywords)"""
    n, S = args["n_agents"], len(seeds)
    kw.setdefault("ragged_wide", "auto")
    if kw["ragged_wide"] is None:                       # built without the keyword at all
        del kw["ragged_wide"]
    cfg = EngineConfig(n, args["agent_label"], args["in_nodes"], H=args["H"], gamma=args["gamma"], slow_lr=args["slow_lr"],
                       fast_lr=args["fast_lr"], max_ep_len=args["max_ep_len"], n_ep_fixed=args["n_ep_fixed"], n_epochs=args["n_epochs"],
                       buffer_size=args["buffer_size"], common_reward=args["common_reward"], nrow=5, ncol=5, n_seeds=S, rng_mode=rng_mode,
                       lattice=lattice, critic_hid=critic_hid, tr_hid=tr_hid, actor_hid=actor_hid, **kw)
    eng = RPBCACEngine(cfg, seeds=list(seeds), device=device, lib=lib)
    for s in range(S):
        for i in range(n):
            for net in ("actor", "critic", "tr"):
                eng.set_weights(s, i, net, W[s][i][net])
    eng.set_goals(np.stack(goals))
    if rng_mode == "numpy":
        eng.np_rngs = []
        for s in range(S):
            r = np.random.RandomState(int(seeds[s]))
            r.randint([0, 0], [5, 5], size=(n, 2))             # the env constructor's reset() draw (grid_world.py:28)
            eng.np_rngs.append(r)
    return eng


def assert_no_head_scratch(eng):
    assert eng.wide and not eng.cfg.regular
    assert eng.w_est is None and eng.w_hmat is None and eng.w_hb is None


def check_engine_vs_oracle(name, rng_mode, device, lib, critic_hid, tr_hid, seeds=(11, 12, 13), lattice=False, **kw):
    """the engine with wide critic-family nets on an irregular instance against oracle.train, engine_checks.compare at its default
    bars; lattice=True: layer 1 on the lattice kernels, and a width that is a multiple of 128 then takes the packed-operand forward,
    whose |phi|^2 parts the ragged head receives -- which path ran is asserted"""
    args, sc = RC.scenario_args(name, **kw)
    W, goals = engine_inputs(args, seeds, critic_hid, tr_hid)
    o_logs, o_w = RC.run_oracle_ragged(args, sc["H"], 5, 5, rng_mode, seeds, W, goals)
    seen = []

    class Spy:
        """the library with the ragged head's nparts argument recorded"""
        def __init__(self, lib_):
            self._lib = lib_

        def __getattr__(self, fn_name):
            fn = getattr(self._lib, fn_name)
            if fn_name != "rcmarl_wide_consensus_head_ragged":
                return fn

            def call(*a):
                seen.append((a[19], a[1] is not None, a[2]))          # (hid, nparts given, n_parts)
                return fn(*a)
            return call
    eng = make_engine(args, rng_mode, device, Spy(lib), seeds, W, goals, critic_hid=critic_hid, tr_hid=tr_hid, lattice=lattice)
    assert not eng.cfg.regular and eng.cfg.degrees == [len(r) for r in sc["in_nodes"]] and eng.cfg.H_per_agent == list(sc["H"])
    assert_no_head_scratch(eng)
    logs = eng.train(args["n_episodes"])
    assert eng.adam_t == args["n_episodes"] // args["n_ep_fixed"]
    assert eng.lat_active == bool(lattice)
    n_wide = sum(h != 20 for h in (critic_hid, tr_hid))
    assert len(seen) == n_wide * eng.adam_t * args["n_epochs"], (len(seen), n_wide)        # one call per wide net and epoch
    for net, xkey, hid in (("critic", "s", critic_hid), ("tr", "sa", tr_hid)):
        pk = bool(lattice and hid != 20 and hid % 128 == 0)
        assert bool(eng._pk_ok(net, xkey, eng.lat_B if lattice else 0)) == pk, net
        if hid != 20:
            calls = [c for c in seen if c[0] == hid]
            assert calls and all(given == pk and (n_parts == lib.rcmarl_pk_parts(hid) if pk else n_parts == 0)
                                 for _, given, n_parts in calls), (net, calls[:3])
    worst = EC.compare(eng, logs, o_logs, o_w)
    print("[wide ragged] %s, critic %d, team-reward net %d%s: worst |w - w_oracle| / max(1, |w|max): critic %.2e, team-reward net %.2e "
          "(bar 1e-4)" % (name, critic_hid, tr_hid, ", lattice layer 1" if lattice else "", worst["critic"], worst["tr"]))
    return eng


def check_engine_wide_actor(name, device, lib, adv_actor="refuse", seeds=(11, 12), **kw):
    """a 32-unit actor beside 20-unit critic-family nets on an irregular instance (the actor never reads the graph), judged as
    wide_actor_checks judges the actor: oracle.train on the same NumPy stream, engine_checks.compare at its default bars (every actor
    parameter within 5 % of an Adam step per update)"""
    kw.setdefault("n_episodes", 4)
    kw.setdefault("buffer_size", 9)
    args, sc = RC.scenario_args(name, **kw)
    W, goals = engine_inputs(args, seeds, 20, 20, actor_hid=32)
    o_logs, o_w = RC.run_oracle_ragged(args, sc["H"], 5, 5, "numpy", seeds, W, goals)
    eng = make_engine(args, "numpy", device, lib, seeds, W, goals, actor_hid=32, adv_actor=adv_actor)
    assert eng.actor_wide and not eng.wide and not eng.cfg.regular and eng.hid["actor"] == 32
    logs = eng.train(args["n_episodes"])
    assert hasattr(eng, "adv") == any(lab != "Cooperative" for lab in sc["labels"])
    assert eng.adam_t == args["n_episodes"] // args["n_ep_fixed"]
    EC.compare(eng, logs, o_logs, o_w)
    return eng


def check_clip_report(device, lib, monkeypatch):
    """clip_report=True on "six" with (32, 24): the counts equal the NumPy recount from the messages at every count call
    (clip_report_checks.RecountingLib: independent of the nets' width)"""
    import clip_report_checks as CR
    monkeypatch.setenv("RCMARL_GRAPH", "0")            # the recount reads the message matrix at every call: no captured epochs
    args, sc = RC.scenario_args("six", n_episodes=4, buffer_size=9)
    seeds = (11,)
    W, goals = engine_inputs(args, seeds, 32, 24)
    proxy = CR.RecountingLib(lib)
    eng = make_engine(args, "device", device, proxy, seeds, W, goals, critic_hid=32, tr_hid=24, clip_report=True)
    proxy.eng = eng
    eng.train(args["n_episodes"])
    assert_no_head_scratch(eng)
    assert proxy.calls == 2 * 2 * args["n_epochs"]          # nets x blocks x epochs
    rep = CR.assert_report_equals_recount(eng, proxy)
    assert rep["critic"]["P_hid"] == eng.P["critic"] - 33 and rep["tr"]["P_hid"] == eng.P["tr"] - 25
    return rep


def check_regular_engine_unchanged(device, lib, seeds=(11, 12), n_episodes=4):
    """a regular wide engine built with ragged_wide='auto' trains bit-identically to one built without the keyword, and keeps the
    uniform head's scratch"""
    args = EC.make_args(["Cooperative"] * 5, H=1, n_episodes=n_episodes, max_ep_len=3, n_ep_fixed=2, n_epochs=2, buffer_size=9, seed=11)
    W, goals = engine_inputs(args, seeds, 32, 24)
    out = []
    for switch in ("auto", None):
        eng = make_engine(args, "device", device, lib, seeds, W, goals, critic_hid=32, tr_hid=24, ragged_wide=switch)
        assert eng.cfg.regular and eng.cfg.ragged_wide == ("auto" if switch else "refuse")
        assert eng.w_est is not None and eng.w_hmat is not None and eng.w_hb is not None
        logs = eng.train(args["n_episodes"])
        out.append((logs, {k: eng.get_all_weights(k) for k in ("actor", "critic", "tr")}))
    for k in out[0][0]:
        np.testing.assert_array_equal(out[0][0][k], out[1][0][k])
    for k in out[0][1]:
        np.testing.assert_array_equal(_bits(out[0][1][k]), _bits(out[1][1][k]), err_msg=k)


def check_switch(device, lib, construction=True):
    """the default stays 'refuse': every refusal the existing checks pin still raises with the keyword absent, and the message names
    the switch; a bad value raises; 'auto' lifts the three refusals; shard_agents on an irregular wide engine is still refused"""
    import pytest
    import wide_actor_adv_checks as WAA
    import wide_actor_checks as WA
    import wide_tr_checks as WT
    RC.check_refusals(device, lib)
    WT.check_validation(device, lib)
    WA.check_refusals(device, lib)
    if construction:                    # (trains four engines; the emulation suite runs it once, in test_wide_actor_adv_emu.py)
        WAA.check_construction(device, lib)
    sc = RC.SCENARIOS["six"]
    mk = lambda **kw: EngineConfig(6, sc["labels"], sc["in_nodes"], H=sc["H"], max_ep_len=3, n_ep_fixed=2, n_epochs=1, buffer_size=6, **kw)
    assert mk().ragged_wide == "refuse"
    for kw, what in ((dict(critic_hid=32), "20-unit critic"), (dict(tr_hid=24), "20-unit team-reward net"), (dict(actor_hid=32), "20-unit actor")):
        for extra in ({}, {"ragged_wide": "refuse"}):
            with pytest.raises(ValueError, match="irregular.*%s.*ragged_wide='auto'" % what):
                mk(**kw, **extra)
        cfg = mk(ragged_wide="auto", **kw)
        assert cfg.ragged_wide == "auto" and not cfg.regular
    for bad in ("on", True, None, "Auto", ""):
        with pytest.raises(ValueError, match="ragged_wide must be"):
            mk(ragged_wide=bad)
        with pytest.raises(ValueError, match="ragged_wide must be"):
            EngineConfig(5, ["Cooperative"] * 5, EC.CIRC5, H=1, ragged_wide=bad)          # ... on a regular graph too
    mal = RC.SCENARIOS["malicious"]
    with pytest.raises(ValueError, match="wide actor"):                                     # adv_actor still has its own say
        EngineConfig(5, mal["labels"], mal["in_nodes"], H=mal["H"], actor_hid=32, ragged_wide="auto")
    EngineConfig(5, mal["labels"], mal["in_nodes"], H=mal["H"], actor_hid=32, ragged_wide="auto", adv_actor="auto")
    eng = RPBCACEngine(mk(ragged_wide="auto", critic_hid=32, tr_hid=24), seeds=[1], device=device, lib=lib)
    assert_no_head_scratch(eng)
    with pytest.raises(ValueError, match="regular communication graph"):
        eng.shard_agents(rank=0, world=2)

    class NoRoom:
        """the library whose coverage query says no: the constructor must raise"""
        def __init__(self, lib_):
            self._lib = lib_

        def __getattr__(self, name):
            if name == "rcmarl_wide_consensus_head_ragged_supported":
                return lambda hid, d: 0
            return getattr(self._lib, name)
    with pytest.raises(ValueError, match="fused ragged head"):
        RPBCACEngine(mk(ragged_wide="auto", critic_hid=32), seeds=[1], device=device, lib=NoRoom(lib))


def check_checkpoints(device, lib, path, rng_mode="device", seeds=(7, 8)):
    """round trip on "six" with (32, 24), as ragged_checks.check_checkpoints: save after one block, a fresh engine with other weights
    resumes from the file -- the bits of the straight run; the switch is not part of the checkpoint's shape"""
    args, sc = RC.scenario_args("six", n_episodes=4, buffer_size=9)
    W, goals = engine_inputs(args, seeds, 32, 24)
    make = lambda: make_engine(args, rng_mode, device, lib, seeds, W, goals, critic_hid=32, tr_hid=24)
    a = make()
    la = a.train(4)
    b = make()
    lb1 = b.train(2)
    b.save_checkpoint(path)
    assert "ragged_wide" not in b.state_dict()["shape"]
    c = make()
    c.init_glorot(base_seed=99)                       # different weights: everything must come from the file
    c.load_checkpoint(path)
    lc = c.train(2)
    for k in la:
        np.testing.assert_array_equal(la[k], np.concatenate([lb1[k], lc[k]], axis=0))
    for net in a.theta:
        np.testing.assert_array_equal(_bits(a.get_all_weights(net)), _bits(c.get_all_weights(net)))
    np.testing.assert_array_equal(a.adam_m.cpu().numpy(), c.adam_m.cpu().numpy())


# ---- drop-in -----------------------------------------------------------------------------------------------------------------
def check_dropin(engine_hook, name="six", seed=5):
    """train_RPBCAC with ragged args['in_nodes'], agents of differing H and 32-unit critic / 24-unit team-reward models against
    oracle.train on the same NumPy stream, at ragged_checks.check_dropin's bars; ragged_wide='refuse' in args brings the refusal back"""
    import pytest
    import dropin_checks as DC
    from rcmarl_amd import keras_compat as K
    from rcmarl_amd.agents.resilient_CAC_agents import RPBCAC_agent
    from rcmarl_amd.environments.grid_world import Grid_World
    from rcmarl_amd.training.train_agents import train_RPBCAC
    sc = RC.SCENARIOS[name]
    n = len(sc["labels"])

    def mlp(width, hid, out, act):
        return K.Sequential([K.Input(shape=(n, width)), K.layers.Flatten(), K.layers.Dense(hid, activation=K.layers.LeakyReLU(alpha=0.1)),
                             K.layers.Dense(hid, activation=K.layers.LeakyReLU(alpha=0.1)), K.layers.Dense(out, activation=act)])

    def team():
        K.set_seed(seed)
        agents, W = [], []
        for i in range(n):
            actor, critic, tr = mlp(2, 20, 5, 'softmax'), mlp(2, 32, 1, None), mlp(3, 24, 1, None)
            W.append([actor.get_weights(), critic.get_weights(), tr.get_weights()])
            agents.append(RPBCAC_agent(actor, critic, tr, slow_lr=0.002, fast_lr=0.01, gamma=0.9, H=sc["H"][i]))
        return agents, W
    agents, W = team()
    args = EC.make_args(sc["labels"], H=0, n_episodes=4, max_ep_len=3, n_ep_fixed=2, n_epochs=1, buffer_size=9, seed=seed,
                        in_nodes=[list(r) for r in sc["in_nodes"]])
    goals = np.random.default_rng(seed).integers(0, 5, size=(n, 2))
    np.random.seed(seed)
    env = Grid_World(nrow=5, ncol=5, n_agents=n, desired_state=goals, initial_state=goals, randomize_state=True, scaling=True)
    weights, df = train_RPBCAC(env, agents, args, engine_hook=engine_hook)
    o_agents = [O.make_agent("Cooperative", [a.copy() for a in W[i][0]], [a.copy() for a in W[i][1]], [a.copy() for a in W[i][2]],
                             0.002, 0.01, 0.9, sc["H"][i]) for i in range(n)]
    np.random.seed(seed)
    ow, odf = O.train(O.GridWorldOracle(5, 5, n, goals, None, True, True), o_agents, args, rng_mode="numpy")
    np.testing.assert_array_equal(df["True_team_returns"].to_numpy(), odf["True_team_returns"].to_numpy(dtype=np.float64))
    np.testing.assert_allclose(df["Estimated_team_returns"].to_numpy(), odf["Estimated_team_returns"].to_numpy(dtype=np.float64),
                               rtol=1e-4, atol=1e-5)
    for i in range(n):
        assert weights[i][1][0].shape == (2 * n, 32) and weights[i][2][0].shape == (3 * n, 24)
        for k in (1, 2):                                  # critic, team-reward net
            for a, b in zip(weights[i][k], ow[i][k]):
                DC.close(a, b, 1e-4, "agent %d net %d" % (i, k))
    again, _ = team()
    with pytest.raises(ValueError, match="irregular.*ragged_wide='auto'"):
        train_RPBCAC(env, again, dict(args, ragged_wide="refuse"), engine_hook=engine_hook)
