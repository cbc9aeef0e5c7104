"""Checks of irregular communication graphs and per-agent H, shared by the hipemu (CPU) tests and the GPU tests.

Kernel checks take a *backend* as tests/kernel_checks.py does (bk.lib, bk.dev, bk.ptr, bk.host, bk.stream); engine checks take
(device, lib) as tests/engine_checks.py does.  The reference is the oracle throughout: oracle.aggregation_bounds /
resilient_aggregate work for any d, oracle.make_agent takes H per agent and oracle.update_block indexes in_nodes[i] per agent, so
the helpers here only have to build the oracle's agents with H[i] (engine_checks.run_oracle hands one scalar H to every agent).
"""
import os

import numpy as np

import engine_checks as EC
import kernel_checks as KC
from oracle import mlp_np as M
from oracle import rpbcac_oracle as O
from rcmarl_amd import capi
from rcmarl_amd.engine import EngineConfig, RPBCACEngine

HID = 20
K1_DEGREES = (1, 3, 4, 5, 7, 12, 21)            # 21: no generated selection network -> rank counting inside the same launch


# ---- graphs ---------------------------------------------------------------------------------------------------------------
def ragged_graph(N, rng, degrees=K1_DEGREES, n_noncoop=3):
    """N agents: every degree of `degrees` present, H_i drawn from 0 .. (d_i - 1) // 2 with both ends present for the larger
    degrees, a few non-cooperative agents.  Returns (in_nodes, H, coop)."""
    assert N >= len(degrees) and max(degrees) <= N
    deg = list(degrees) + [int(rng.choice(degrees)) for _ in range(N - len(degrees))]
    deg = [deg[k] for k in rng.permutation(N)]
    in_nodes, H = [], []
    for i, d in enumerate(deg):
        others = rng.permutation([j for j in range(N) if j != i])[:d - 1]
        in_nodes.append([i] + [int(j) for j in others])
        H.append(int(rng.integers(0, (d - 1) // 2 + 1)))
    for d in degrees:                            # the extreme H of every degree at least once where an agent allows it
        idx = [i for i in range(N) if deg[i] == d]
        H[idx[0]] = (d - 1) // 2
        if len(idx) > 1:
            H[idx[1]] = 0
    coop = np.ones(N, np.int32)
    seen = set()
    for i in rng.permutation(N):                 # never the only agent of its degree: every degree keeps a cooperative agent
        if len(seen) == n_noncoop:
            break
        if sum(1 for j in range(N) if deg[j] == deg[i] and coop[j]) > 1:
            coop[i] = 0
            seen.add(int(i))
    return in_nodes, H, coop


def csr_and_classes(in_nodes, H, coop):
    """CSR image, order[] and the class table, built here independently of EngineConfig.consensus_classes()."""
    N = len(in_nodes)
    off = np.zeros(N + 1, np.int32)
    for i, row in enumerate(in_nodes):
        off[i + 1] = off[i] + len(row)
    idx = np.asarray([j for row in in_nodes for j in row], np.int32)
    groups = {}
    for i in range(N):
        if coop[i]:
            groups.setdefault((len(in_nodes[i]), int(H[i])), []).append(i)
    order, classes = [], []
    for (d, h) in sorted(groups):
        classes.append((d, h, len(order), len(groups[(d, h)])))
        order += groups[(d, h)]
    table = (capi.RaggedClass * len(classes))(*[capi.RaggedClass(*k) for k in classes])
    return off, idx, np.asarray(order, np.int32), classes, table


def dense_table_of_class(in_nodes, members, d):
    """nbr[N][d] for one rcmarl_consensus_params / rcmarl_consensus_head call on the class `members` (the other rows are masked out
    by coop and only have to be valid: the agent itself, d times)."""
    N = len(in_nodes)
    nbr = np.asarray([[i] * d for i in range(N)], np.int32)
    for i in members:
        nbr[i] = in_nodes[i]
    mask = np.zeros(N, np.int32)
    mask[list(members)] = 1
    return nbr, mask


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


# ---- K1 -------------------------------------------------------------------------------------------------------------------
def k1_messages(rng, S, N, ldp, in_nodes):
    msg = rng.normal(size=(S, N, ldp)).astype(np.float32)
    msg[:, :, 5] = msg[:, :1, 5]                                       # every value equal (= equal to the own value)
    msg[:, :, 7] = np.round(msg[:, :, 7])                              # duplicates
    msg[:, :, 9] = np.where(rng.random((S, N)) < 0.5, np.float32(0.0), np.float32(-0.0))      # +-0 only
    msg[:, :, 11] = np.where(rng.random((S, N)) < 0.5, msg[:, :, 11], np.float32(0.0)) * np.where(rng.random((S, N)) < 0.5, 1, -1)
    for i, row in enumerate(in_nodes):                                 # some neighbours carry exactly the agent's own value
        for j in row[1::2]:
            msg[:, j, 13] = msg[:, i, 13]
    msg[:, int(rng.integers(N))] = np.float32(1e3)                     # an adversarial row
    return msg


def run_k1_ragged(bk, msg, theta0, in_nodes, H, coop, P_hid):
    S, N, ldp = msg.shape
    off, idx, order, classes, table = csr_and_classes(in_nodes, H, coop)
    d_msg, d_theta = bk.dev(msg), bk.dev(theta0)
    d_lo, d_hi = bk.dev(np.zeros_like(theta0)), bk.dev(np.zeros_like(theta0))
    d_off, d_idx, d_order = bk.dev(off), bk.dev(idx), bk.dev(order)
    bk.lib.rcmarl_consensus_params_ragged(bk.ptr(d_msg), bk.ptr(d_theta), bk.ptr(d_off), bk.ptr(d_idx), bk.ptr(d_order), table,
                                          len(classes), S, N, ldp, P_hid, bk.ptr(d_lo), bk.ptr(d_hi), bk.stream)
    return bk.host(d_theta), bk.host(d_lo), bk.host(d_hi), classes, order


def run_k1_per_class(bk, msg, theta0, in_nodes, H, coop, P_hid):
    """the alternative: one rcmarl_consensus_params launch per class, coop masked to the class, a dense table of its rows"""
    S, N, ldp = msg.shape
    _, _, order, classes, _ = csr_and_classes(in_nodes, H, coop)
    d_msg, d_theta = bk.dev(msg), bk.dev(theta0)
    d_lo, d_hi = bk.dev(np.zeros_like(theta0)), bk.dev(np.zeros_like(theta0))
    for d, h, first, count in classes:
        nbr, mask = dense_table_of_class(in_nodes, order[first:first + count], d)
        d_nbr, d_mask = bk.dev(nbr), bk.dev(mask)
        bk.lib.rcmarl_consensus_params(bk.ptr(d_msg), bk.ptr(d_theta), bk.ptr(d_nbr), bk.ptr(d_mask), S, N, ldp, P_hid, d, h,
                                       bk.ptr(d_lo), bk.ptr(d_hi), bk.stream)
        bk.host(d_theta)                                               # (the tables of this class live until its launch is done)
    return bk.host(d_theta), bk.host(d_lo), bk.host(d_hi)


def check_k1_ragged(bk, N=24, S=2, P=215, P_hid=150, seed=1):
    """rcmarl_consensus_params_ragged against the oracle at the project's bars (clip window bit-equal to
    oracle.aggregation_bounds, means within 1e-6 max(1, |x|) of oracle.resilient_aggregate) and bit for bit against one masked
    rcmarl_consensus_params launch per class."""
    rng = np.random.default_rng(seed)
    ldp = KC.pad64(P)
    assert P_hid % 64 and P_hid < P
    in_nodes, H, coop = ragged_graph(N, rng)
    assert sorted(set(len(r) for r in in_nodes)) == sorted(K1_DEGREES) and (coop == 0).any()
    msg = k1_messages(rng, S, N, ldp, in_nodes)
    theta0 = rng.normal(size=(S, N, ldp)).astype(np.float32)
    theta, lo, hi, classes, _ = run_k1_ragged(bk, msg, theta0, in_nodes, H, coop, P_hid)
    assert any(d == 21 for d, _, _, _ in classes) and len({h for _, h, _, _ in classes}) > 2
    worst = 0.0
    for s in range(S):
        for i in range(N):
            if not coop[i]:
                np.testing.assert_array_equal(_bits(theta[s, i]), _bits(theta0[s, i]))
                continue
            vals = msg[s, in_nodes[i], :P_hid]
            wl, wh, _ = O.aggregation_bounds(vals, H[i])
            np.testing.assert_array_equal(lo[s, i, :P_hid], wl, err_msg="lower bound, agent %d (d %d, H %d)" % (i, len(in_nodes[i]), H[i]))
            np.testing.assert_array_equal(hi[s, i, :P_hid], wh, err_msg="upper bound, agent %d" % i)
            want = O.resilient_aggregate(vals, H[i])
            err = np.abs(theta[s, i, :P_hid] - want) / np.maximum(1.0, np.abs(want))
            worst = max(worst, float(err.max()))
            assert err.max() <= 1e-6, (i, len(in_nodes[i]), H[i], float(err.max()))
    print("[parity] ragged K1: worst |mean - oracle| / max(1, |x|) = %.2e (bar 1e-6)" % worst)
    np.testing.assert_array_equal(_bits(theta[:, :, P_hid:]), _bits(theta0[:, :, P_hid:]))       # output layer, padding
    t2, lo2, hi2 = run_k1_per_class(bk, msg, theta0, in_nodes, H, coop, P_hid)
    np.testing.assert_array_equal(_bits(theta), _bits(t2))
    np.testing.assert_array_equal(_bits(lo), _bits(lo2))
    np.testing.assert_array_equal(_bits(hi), _bits(hi2))


def check_k1_ragged_more_classes_than_one_launch_takes(bk, N=60, S=1, P=100, P_hid=70, seed=8):
    """More than 32 (d, H) classes: the entry point issues one launch per 32 of them.  Degrees 3, 5, .., 19 with every H give 54
    classes; oracle bars and the per-class uniform launches as in check_k1_ragged."""
    rng = np.random.default_rng(seed)
    ldp = KC.pad64(P)
    pairs = [(d, h) for d in range(3, 20, 2) for h in range((d - 1) // 2 + 1)]
    assert len(pairs) == 54 and N >= len(pairs)
    pairs = pairs + [pairs[int(k)] for k in rng.integers(0, len(pairs), size=N - len(pairs))]
    pairs = [pairs[k] for k in rng.permutation(N)]
    in_nodes = [[i] + [int(j) for j in rng.permutation([j for j in range(N) if j != i])[:d - 1]] for i, (d, _) in enumerate(pairs)]
    H = [h for _, h in pairs]
    coop = np.ones(N, np.int32)
    msg = k1_messages(rng, S, N, ldp, in_nodes)
    theta0 = rng.normal(size=(S, N, ldp)).astype(np.float32)
    theta, lo, hi, classes, _ = run_k1_ragged(bk, msg, theta0, in_nodes, H, coop, P_hid)
    assert len(classes) == 54
    for s in range(S):
        for i in range(N):
            vals = msg[s, in_nodes[i], :P_hid]
            wl, wh, _ = O.aggregation_bounds(vals, H[i])
            np.testing.assert_array_equal(lo[s, i, :P_hid], wl, err_msg="lower bound, agent %d" % i)
            np.testing.assert_array_equal(hi[s, i, :P_hid], wh, err_msg="upper bound, agent %d" % i)
            want = O.resilient_aggregate(vals, H[i])
            assert (np.abs(theta[s, i, :P_hid] - want) / np.maximum(1.0, np.abs(want))).max() <= 1e-6, i
    t2, lo2, hi2 = run_k1_per_class(bk, msg, theta0, in_nodes, H, coop, P_hid)
    np.testing.assert_array_equal(_bits(theta), _bits(t2))
    np.testing.assert_array_equal(_bits(lo), _bits(lo2))
    np.testing.assert_array_equal(_bits(hi), _bits(hi2))


def check_k1_ragged_on_a_regular_graph(bk, N=12, d=4, H=1, S=2, P=215, P_hid=150, graph="rand", seed=2):
    """on a regular graph the ragged entry gives the bits of the uniform entry"""
    rng = np.random.default_rng(seed)
    ldp = KC.pad64(P)
    nbr = KC.circulant(N, d) if graph == "circ" else KC.random_regular(N, d, rng)
    in_nodes = [[int(j) for j in row] for row in nbr]
    coop = np.ones(N, np.int32)
    coop[N - 1] = 0
    msg = k1_messages(rng, S, N, ldp, in_nodes)
    theta0 = rng.normal(size=(S, N, ldp)).astype(np.float32)
    theta, lo, hi, classes, _ = run_k1_ragged(bk, msg, theta0, in_nodes, [H] * N, coop, P_hid)
    assert classes == [(d, H, 0, N - 1)]
    d_msg, d_theta, d_nbr, d_coop = bk.dev(msg), bk.dev(theta0), bk.dev(nbr), bk.dev(coop)
    d_lo, d_hi = bk.dev(np.zeros_like(theta0)), bk.dev(np.zeros_like(theta0))
    bk.lib.rcmarl_consensus_params(bk.ptr(d_msg), bk.ptr(d_theta), bk.ptr(d_nbr), bk.ptr(d_coop), S, N, ldp, P_hid, d, H,
                                   bk.ptr(d_lo), bk.ptr(d_hi), bk.stream)
    np.testing.assert_array_equal(_bits(theta), _bits(bk.host(d_theta)))
    np.testing.assert_array_equal(_bits(lo), _bits(bk.host(d_lo)))
    np.testing.assert_array_equal(_bits(hi), _bits(bk.host(d_hi)))


# ---- K2 + K3 --------------------------------------------------------------------------------------------------------------
def k2_inputs(S, N, B, in_dim, seed, outlier=50.0):
    """the inputs of kernel_checks.check_consensus_head on an irregular graph"""
    rng = np.random.default_rng(seed)
    P, P_hid = KC.geom(in_dim, 1)
    ldp, ldb = KC.pad64(P), KC.pad64(B)
    live = KC.random_params(rng, S, N, in_dim, 1)
    msgp = KC.random_params(rng, S, N, in_dim, 1)
    theta, msg = KC.pack_rows(live, ldp), KC.pack_rows(msgp, ldp)
    x = rng.normal(size=(S, B, in_dim)).astype(np.float32)
    in_nodes, H, coop = ragged_graph(N, rng)
    for s in range(S):                              # an outlier head among the messages
        msg[s, 1, P_hid:P] *= np.float32(outlier)
        msgp[s][1][4] = msgp[s][1][4] * np.float32(outlier)
        msgp[s][1][5] = msgp[s][1][5] * np.float32(outlier)
    return dict(S=S, N=N, B=B, in_dim=in_dim, ldp=ldp, ldb=ldb, live=live, msgp=msgp, theta=theta, msg=msg, x=x, in_nodes=in_nodes,
                H=H, coop=coop, rng=rng)


def run_k2(bk, inp, ragged):
    """layer 1 -> consensus head (ragged entry | one rcmarl_consensus_head per class) -> head apply; (theta, agg, partials)"""
    S, N, B, in_dim, ldp, ldb = (inp[k] for k in ("S", "N", "B", "in_dim", "ldp", "ldb"))
    in_nodes, H, coop = inp["in_nodes"], inp["H"], inp["coop"]
    off, idx, order, classes, table = csr_and_classes(in_nodes, H, coop)
    nchunk = (B + 255) // 256
    d_x, d_th, d_msg, d_coop = bk.dev(inp["x"]), bk.dev(inp["theta"]), bk.dev(inp["msg"]), bk.dev(coop)
    d_a = bk.dev(np.zeros((S, N * HID, ldb), np.float32))
    d_part = bk.dev(np.zeros((S, N, nchunk, HID + 1), np.float32))
    d_agg = bk.dev(np.zeros((S, N, ldb), np.float32))
    L = bk.lib
    KC._layer1(bk, d_x, B * in_dim, d_th, d_a, S, N, B, in_dim, ldp, ldb)
    if ragged:
        d_off, d_idx, d_order = bk.dev(off), bk.dev(idx), bk.dev(order)
        L.rcmarl_consensus_head_ragged(bk.ptr(d_a), bk.ptr(d_th), bk.ptr(d_msg), bk.ptr(d_off), bk.ptr(d_idx), bk.ptr(d_order), table,
                                       len(classes), bk.ptr(d_part), bk.ptr(d_agg), S, N, B, in_dim, HID, ldp, ldb, bk.stream)
    else:
        for d, h, first, count in classes:
            nbr, mask = dense_table_of_class(in_nodes, order[first:first + count], d)
            d_nbr, d_mask = bk.dev(nbr), bk.dev(mask)
            L.rcmarl_consensus_head(bk.ptr(d_a), bk.ptr(d_th), bk.ptr(d_msg), bk.ptr(d_nbr), bk.ptr(d_mask), bk.ptr(d_part),
                                    bk.ptr(d_agg), S, N, B, in_dim, HID, ldp, ldb, d, h, bk.stream)
            bk.host(d_agg)
    part, agg = bk.host(d_part).copy(), bk.host(d_agg).copy()
    L.rcmarl_head_apply(bk.ptr(d_part), bk.ptr(d_th), bk.ptr(d_coop), S, N, B, in_dim, HID, ldp, bk.stream)
    return bk.host(d_th), agg, part


def check_k2_ragged(bk, S=1, N=24, B=270, in_dim=10, seed=4):
    """rcmarl_consensus_head_ragged: aggregates and the projection step against the oracle at the bars of
    kernel_checks.check_consensus_head, and bit for bit against per-class calls of rcmarl_consensus_head."""
    inp = k2_inputs(S, N, B, in_dim, seed)
    in_nodes, H, coop, live, msgp, x, rng = (inp[k] for k in ("in_nodes", "H", "coop", "live", "msgp", "x", "rng"))
    th_new, agg, part = run_k2(bk, inp, ragged=True)
    f16 = os.environ.get("RCMARL_K2_MX", "1") not in ("0",) and bk.lib.rcmarl_lattice_f16_mode() != 0
    nets = generated_networks()
    worst = {"agg": 0.0, "W3": 0.0}
    for s in range(S):
        for i in range(N):
            if not coop[i]:
                np.testing.assert_array_equal(th_new[s, i], inp["theta"][s, i])
                continue
            ag = O.CoopAgent(M.init_mlp(rng, in_dim, HID, 5), live[s][i], live[s][i], 0.002, 0.01, 0.9, H[i])
            want_agg = ag.consensus_estimates_critic(x[s], [msgp[s][j] for j in in_nodes[i]])
            # the matrix-core kernel (two-piece f16 operands: 3e-5, see check_consensus_head) serves a class only when a selection
            # network is generated for it; every other class runs fp32 lane code: 5e-6
            mx = f16 and len(in_nodes[i]) + 1 <= 32 and (len(in_nodes[i]), H[i]) in nets
            KC.rel_close(agg[s, i, :B], want_agg[:, 0], 3e-5 if mx else 5e-6, "estimate aggregate, agent %d (d %d, H %d)" % (i, len(in_nodes[i]), H[i]))
            worst["agg"] = max(worst["agg"], float(np.abs(agg[s, i, :B] - want_agg[:, 0]).max()) / max(1.0, float(np.abs(want_agg).max())))
            ag.projection_step_critic(x[s], want_agg)
            got = KC.unpack_row(th_new[s, i], in_dim, 1)
            for k in range(4):
                np.testing.assert_array_equal(got[k], live[s][i][k])          # hidden layers frozen
            KC.rel_close(got[4], ag.critic[4], 2e-5, "W3 after projection, agent %d" % i)
            KC.rel_close(got[5], ag.critic[5], 2e-5, "b3 after projection, agent %d" % i)
            worst["W3"] = max(worst["W3"], float(np.abs(got[4] - ag.critic[4]).max()) / max(1.0, float(np.abs(ag.critic[4]).max())))
    print("[parity] ragged K2 (f16 form %s): worst aggregate %.2e, W3 after projection %.2e" % (f16, worst["agg"], worst["W3"]))
    th2, agg2, part2 = run_k2(bk, inp, ragged=False)
    for i in range(N):
        if coop[i]:
            np.testing.assert_array_equal(_bits(part[:, i]), _bits(part2[:, i]), err_msg="records, agent %d" % i)
            np.testing.assert_array_equal(_bits(agg[:, i]), _bits(agg2[:, i]), err_msg="aggregates, agent %d" % i)
    np.testing.assert_array_equal(_bits(th_new), _bits(th2))


def generated_networks():
    """the (d, H) with a generated selection network (csrc/gen_selnet.py: RCMARL_SELNET_COMBOS)"""
    import sys
    import rcmarl_amd.build as B
    sys.path.insert(0, B.CSRC)
    try:
        import gen_selnet
        return set(gen_selnet.combos())
    finally:
        sys.path.remove(B.CSRC)


def uniform_head_outputs(bk, cases=((2, 5, 300, 10, 4, 1, "circ"), (1, 6, 100, 18, 3, 0, "rand"), (1, 12, 70, 24, 11, 2, "rand"),
                                    (1, 30, 70, 12, 23, 5, "rand"))):
    """(theta after the projection step, aggregates) of rcmarl_consensus_head on fixed inputs: what two builds of the library are
    compared on, bit for bit, by tools/diag_head_two_builds.py (the kernels gained two optional parameters; the existing entry
    passes null for both)."""
    return [KC.check_consensus_head(bk, *c, compare=False) for c in cases]


# ---- argument validation (no GPU) -------------------------------------------------------------------------------------------
def check_argument_validation(lib):
    import ctypes
    import pytest
    ok = (capi.RaggedClass * 1)(capi.RaggedClass(3, 1, 0, 2))
    one = ctypes.c_void_p(64)                     # a non-null pointer that is never dereferenced: validation comes first
    k1_good = [one, one, one, one, one, ok, 1, 1, 5, 64, 40, None, None, None]
    k2_good = [one, one, one, one, one, one, ok, 1, one, None, 1, 5, 100, 10, 20, 704, 128, None]

    def bad_class(d, h, first, count):
        return (capi.RaggedClass * 1)(capi.RaggedClass(d, h, first, count))
    k1_bad = [{0: None}, {1: None}, {2: None}, {3: None}, {4: None}, {5: None}, {6: 0}, {7: 0}, {8: 0}, {9: 65}, {10: 0}, {10: 65},
              {11: one}, {5: bad_class(2, 1, 0, 2)}, {5: bad_class(0, 0, 0, 2)}, {5: bad_class(3, -1, 0, 2)},
              {5: bad_class(3, 1, -1, 2)}, {5: bad_class(3, 1, 0, 0)}, {5: bad_class(3, 1, 4, 2)}]
    k2_bad = [{0: None}, {1: None}, {2: None}, {3: None}, {4: None}, {5: None}, {6: None}, {7: 0}, {8: None}, {10: 0}, {11: 0},
              {12: 0}, {6: bad_class(2, 1, 0, 2)}, {6: bad_class(3, 1, 4, 2)}, {6: bad_class(3, 1, 0, 0)}]
    for name, good, bads in (("rcmarl_consensus_params_ragged", k1_good, k1_bad), ("rcmarl_consensus_head_ragged", k2_good, k2_bad)):
        for change in bads:
            args = list(good)
            for k, v in change.items():
                args[k] = v
            with pytest.raises(capi.RcmarlError, match="RCMARL_ERR_ARG"):
                getattr(lib, name)(*args)
    # the [N][4] tile image of K1 beyond the LDS / a class whose estimates exceed the rank-counting kernel's LDS: unsupported
    big = [one, one, one, one, one, (capi.RaggedClass * 1)(capi.RaggedClass(3, 1, 0, 2)), 1, 1, 5000, 64, 40, None, None, None]
    with pytest.raises(capi.RcmarlError, match="RCMARL_ERR_UNSUPPORTED"):
        lib.rcmarl_consensus_params_ragged(*big)
    wide = list(k2_good)
    wide[6], wide[11] = (capi.RaggedClass * 1)(capi.RaggedClass(70, 1, 0, 2)), 100
    with pytest.raises(capi.RcmarlError, match="RCMARL_ERR_UNSUPPORTED"):
        lib.rcmarl_consensus_head_ragged(*wide)


# ---- engine against the oracle ----------------------------------------------------------------------------------------------
def ring_rows(degrees):
    """in_nodes[i] = [i, i+1, ..] of length degrees[i] (mod N)"""
    n = len(degrees)
    return [[(i + k) % n for k in range(d)] for i, d in enumerate(degrees)]


SCENARIOS = {
    # 6 cooperative agents, degrees (3, 3, 4, 5, 5, 6), H (1, 1, 1, 2, 2, 2)
    "six": dict(labels=["Cooperative"] * 6, in_nodes=ring_rows((3, 3, 4, 5, 5, 6)), H=[1, 1, 1, 2, 2, 2]),
    # 4 cooperative + 1 Malicious (agent 4): only its out-neighbours (agents 0, 1) have d = 5, H = 1; the rest d = 3, H = 0
    "malicious": dict(labels=["Cooperative"] * 4 + ["Malicious"],
                      in_nodes=[[0, 1, 2, 3, 4], [1, 2, 3, 4, 0], [2, 3, 0], [3, 0, 1], [4]], H=[1, 1, 0, 0, 0]),
    # an agent that listens to nobody (d = 1)
    "loner": dict(labels=["Cooperative"] * 5, in_nodes=[[0], [1, 2, 3], [2, 3, 4], [3, 4, 0, 1], [4, 0, 1, 2]], H=[0, 1, 1, 1, 1]),
}


def run_oracle_ragged(args, H, nrow, ncol, rng_mode, seeds, W, goals):
    """engine_checks.run_oracle with the oracle's agents built with H[i]"""
    n = args["n_agents"]
    o_logs, o_weights = [], []
    for s in range(len(seeds)):
        a = dict(args)
        a["random_seed"] = int(seeds[s])
        agents = [O.make_agent(lab, W[s][i]["actor"], W[s][i]["critic"], W[s][i]["tr"], a["slow_lr"], a["fast_lr"], a["gamma"], H[i])
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
    return o_logs, o_weights


def scenario_args(name, n_episodes=6, max_ep_len=3, n_ep_fixed=2, n_epochs=2, buffer_size=12, seed=11):
    sc = SCENARIOS[name]
    args = EC.make_args(sc["labels"], H=list(sc["H"]), n_episodes=n_episodes, max_ep_len=max_ep_len, n_ep_fixed=n_ep_fixed,
                        n_epochs=n_epochs, buffer_size=buffer_size, seed=seed, in_nodes=[list(r) for r in sc["in_nodes"]])
    return args, sc


def check_engine_vs_oracle(name, rng_mode, device, lib, seeds=(11, 12, 13), **kw):
    """the engine on an irregular instance against oracle.train, engine_checks.compare at its default bars"""
    args, sc = scenario_args(name, **kw)
    W, goals = EC.make_inputs(args, 5, seeds)
    o_logs, o_w = run_oracle_ragged(args, sc["H"], 5, 5, rng_mode, seeds, W, goals)
    eng, logs = EC.run_engine(args, 5, 5, rng_mode, device, lib, seeds, W, goals)
    assert not eng.cfg.regular and eng.cfg.degrees == [len(r) for r in sc["in_nodes"]] and eng.cfg.H_per_agent == list(sc["H"])
    assert eng.adam_t == args["n_episodes"] // args["n_ep_fixed"]
    EC.compare(eng, logs, o_logs, o_w)
    return eng


def check_graph_replay(device, lib, monkeypatch, name="six", seed=21):
    """a single instance on an irregular graph replays its captured epochs, and the replayed run has the bits of an uncaptured one"""
    args, sc = scenario_args(name, n_episodes=6, n_epochs=4, seed=seed)
    W, goals = EC.make_inputs(args, 5, (seed,))
    out = {}
    for graph in ("1", "0"):
        monkeypatch.setenv("RCMARL_GRAPH", graph)
        eng, _ = EC.run_engine(args, 5, 5, "device", device, lib, (seed,), W, goals)
        out[graph] = eng
    assert out["1"].graph_replays > 0 and out["1"].graph_captures > 0 and out["0"].graph_replays == 0
    for net in ("actor", "critic", "tr"):
        np.testing.assert_array_equal(_bits(out["1"].get_all_weights(net)), _bits(out["0"].get_all_weights(net)))


# ---- configuration, refusals, checkpoints ----------------------------------------------------------------------------------
def check_config():
    import pytest
    sc = SCENARIOS["six"]
    cfg = EngineConfig(6, sc["labels"], sc["in_nodes"], H=sc["H"])
    assert cfg.degrees == [3, 3, 4, 5, 5, 6] and cfg.H_per_agent == [1, 1, 1, 2, 2, 2] and not cfg.regular
    order, classes = cfg.consensus_classes()
    assert order == [0, 1, 2, 3, 4, 5] and classes == [(3, 1, 0, 2), (4, 1, 2, 1), (5, 2, 3, 2), (6, 2, 5, 1)]
    reg = EngineConfig(5, ["Cooperative"] * 5, EC.CIRC5, H=1)
    assert reg.regular and reg.d == 4 and reg.H == 1 and reg.degrees == [4] * 5 and reg.H_per_agent == [1] * 5
    assert EngineConfig(5, ["Cooperative"] * 5, EC.CIRC5, H=[1] * 5).regular
    assert not EngineConfig(5, ["Cooperative"] * 5, EC.CIRC5, H=[1, 1, 0, 1, 1]).regular            # one graph, mixed H
    with pytest.raises(ValueError, match="2H\\+1"):
        EngineConfig(6, sc["labels"], sc["in_nodes"], H=[1, 1, 2, 2, 2, 2])                           # agent 2: d = 4 < 5
    with pytest.raises(ValueError, match="one int per agent"):
        EngineConfig(6, sc["labels"], sc["in_nodes"], H=[1, 1])
    with pytest.raises(ValueError, match="must be i"):
        EngineConfig(3, ["Cooperative"] * 3, [[0, 1], [2, 1], [2]], H=0)
    # rows of non-cooperative agents are never used for consensus: any length, any H
    mal = SCENARIOS["malicious"]
    EngineConfig(5, mal["labels"], mal["in_nodes"], H=[1, 1, 0, 0, 7])


def check_refusals(device, lib):
    """out of scope, each with a clear ValueError: an irregular graph with a wide critic, an irregular graph with shard_agents"""
    import pytest
    sc = SCENARIOS["six"]
    with pytest.raises(ValueError, match="irregular.*20-unit critic"):
        EngineConfig(6, sc["labels"], sc["in_nodes"], H=sc["H"], critic_hid=32)
    cfg = EngineConfig(6, sc["labels"], sc["in_nodes"], H=sc["H"], max_ep_len=3, n_ep_fixed=2, n_epochs=1, buffer_size=6)
    eng = RPBCACEngine(cfg, seeds=[1], device=device, lib=lib)
    with pytest.raises(ValueError, match="regular communication graph"):
        eng.shard_agents(rank=0, world=2)


def _make_engine(sc, H, rng_mode, device, lib, S=2):
    n = len(sc["labels"])
    cfg = EngineConfig(n, sc["labels"], sc["in_nodes"], H=H, max_ep_len=3, n_ep_fixed=2, n_epochs=2, buffer_size=9, nrow=5, ncol=5,
                       n_seeds=S, rng_mode=rng_mode, lattice=False)
    eng = RPBCACEngine(cfg, seeds=[7 + s for s in range(S)], device=device, lib=lib)
    eng.init_glorot(base_seed=3)
    eng.set_goals(np.random.default_rng(9).integers(0, 5, size=(n, 2)))
    if rng_mode == "numpy":
        eng.np_rngs = [np.random.RandomState(70 + s) for s in range(S)]
    return eng


def check_checkpoints(device, lib, path, rng_mode="device"):
    import pytest
    sc = SCENARIOS["six"]
    make = lambda H=sc["H"]: _make_engine(sc, H, rng_mode, device, lib)
    a = make()
    la = a.train(4)
    b = make()
    lb1 = b.train(2)
    b.save_checkpoint(path)
    c = make()
    c.init_glorot(base_seed=99)                       # different weights: everything must come from the file
    c.load_checkpoint(path)
    lc = c.train(2)
    for k in la:
        np.testing.assert_array_equal(la[k], np.concatenate([lb1[k], lc[k]], axis=0))
    for net in a.theta:
        np.testing.assert_array_equal(_bits(a.get_all_weights(net)), _bits(c.get_all_weights(net)))
    np.testing.assert_array_equal(a.adam_m.cpu().numpy(), c.adam_m.cpu().numpy())
    for k in a.rp:
        np.testing.assert_array_equal(a.rp[k][:, :a.B].cpu().numpy(), c.rp[k][:, :c.B].cpu().numpy())
    sd = b.state_dict()
    assert sd["shape"]["H"] == sc["H"]                # per agent when it is not uniform
    # another H list on the same graph: refused, in the existing message's shape
    other = make(H=[1, 1, 1, 2, 2, 1])
    with pytest.raises(ValueError, match=r"checkpoint does not match this engine: \{'H'"):
        other.load_checkpoint(path)
    # a regular engine: H stays the scalar of checkpoints written before per-agent H, and such a dict loads
    reg_sc = dict(labels=["Cooperative"] * 5, in_nodes=EC.CIRC5)
    r1 = _make_engine(reg_sc, 1, rng_mode, device, lib)
    r1.train(2)
    old = r1.state_dict()
    assert old["shape"]["H"] == 1 and isinstance(old["shape"]["H"], int)
    r2 = _make_engine(reg_sc, [1] * 5, rng_mode, device, lib)
    r2.load_state_dict(old)
    np.testing.assert_array_equal(_bits(r1.get_all_weights("critic")), _bits(r2.get_all_weights("critic")))
    r3 = _make_engine(reg_sc, 0, rng_mode, device, lib)
    with pytest.raises(ValueError, match="checkpoint does not match this engine"):
        r3.load_state_dict(old)


# ---- drop-in ---------------------------------------------------------------------------------------------------------------
def check_dropin(engine_hook, name="six", seed=5):
    """train_RPBCAC with ragged args['in_nodes'] and agents of differing H against oracle.train on the same NumPy stream"""
    import dropin_checks as DC
    from rcmarl_amd import keras_compat as K
    from rcmarl_amd.agents.resilient_CAC_agents import RPBCAC_agent
    from rcmarl_amd.environments.grid_world import Grid_World
    from rcmarl_amd.training.train_agents import train_RPBCAC
    sc = SCENARIOS[name]
    n = len(sc["labels"])
    assert all(lab == "Cooperative" for lab in sc["labels"])
    K.set_seed(seed)
    agents, W = [], []
    for i in range(n):
        actor, critic, tr = DC.make_models(n)
        W.append([actor.get_weights(), critic.get_weights(), tr.get_weights()])
        agents.append(RPBCAC_agent(actor, critic, tr, slow_lr=0.002, fast_lr=0.01, gamma=0.9, H=sc["H"][i]))
    args = EC.make_args(sc["labels"], H=0, n_episodes=4, max_ep_len=3, n_ep_fixed=2, n_epochs=1, buffer_size=9, seed=seed,
                        in_nodes=[list(r) for r in sc["in_nodes"]])
    goals = np.random.default_rng(seed).integers(0, 5, size=(n, 2))
    np.random.seed(seed)
    env = Grid_World(nrow=5, ncol=5, n_agents=n, desired_state=goals, initial_state=goals, randomize_state=True, scaling=True)
    weights, df = train_RPBCAC(env, agents, args, engine_hook=engine_hook)
    o_agents = [O.make_agent("Cooperative", [a.copy() for a in W[i][0]], [a.copy() for a in W[i][1]], [a.copy() for a in W[i][2]],
                             0.002, 0.01, 0.9, sc["H"][i]) for i in range(n)]
    np.random.seed(seed)
    oenv = O.GridWorldOracle(5, 5, n, goals, None, True, True)
    ow, odf = O.train(oenv, o_agents, args, rng_mode="numpy")
    np.testing.assert_array_equal(df["True_team_returns"].to_numpy(), odf["True_team_returns"].to_numpy(dtype=np.float64))
    np.testing.assert_allclose(df["Estimated_team_returns"].to_numpy(), odf["Estimated_team_returns"].to_numpy(dtype=np.float64),
                               rtol=1e-4, atol=1e-5)
    for i in range(n):
        for k in (1, 2):                                  # critic, team-reward net
            for a, b in zip(weights[i][k], ow[i][k]):
                DC.close(a, b, 1e-4, "agent %d net %d" % (i, k))


def check_main_in_nodes(engine_hook, tmp_path, monkeypatch):
    """main.py: a ragged --in_nodes value (JSON) reaches train_RPBCAC exactly as given, and the run goes through the engine"""
    import json
    from rcmarl_amd import main as RM
    in_nodes = [[0, 1, 2], [1, 2, 3, 4], [2, 3, 4, 0, 1], [3, 4, 0], [4, 0, 1, 2]]
    seen = {}
    real = RM.training.train_RPBCAC

    def spy(env, agents, args, **kw):
        seen["in_nodes"], seen["H"] = args["in_nodes"], [ag.H for ag in agents]
        return real(env, agents, args, **kw)
    monkeypatch.setattr(RM.training, "train_RPBCAC", spy)
    monkeypatch.chdir(tmp_path)
    argv = ["--n_agents", "5", "--in_nodes", json.dumps(in_nodes), "--H", "1", "--n_episodes", "2", "--n_ep_fixed", "2", "--max_ep_len",
            "3", "--n_epochs", "1", "--buffer_size", "6", "--random_seed", "5", "--slow_lr", "0.002"]
    weights, df = RM.main(argv, engine_hook=engine_hook)
    assert seen["in_nodes"] == in_nodes and seen["H"] == [1] * 5
    assert len(df) == 2 and len(weights) == 5 and all(np.isfinite(a).all() for w in weights for net in w for a in net)
