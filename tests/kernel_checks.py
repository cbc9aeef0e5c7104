"""Kernel-vs-oracle parity checks shared by the hipemu (CPU) tests and the
GPU tests.  A *backend* supplies memory + the bound C-ABI library:

    bk.lib              CLib (emu build or the product librcmarl_hip.so)
    bk.dev(np_array)    -> device handle holding a copy
    bk.ptr(handle)      -> raw pointer for the C-ABI
    bk.host(handle)     -> numpy copy (synchronises)
    bk.stream           -> hipStream_t or None
"""
import os

import numpy as np

from oracle import mlp_np as M
from oracle import rpbcac_oracle as O

HID = 20


_FLAG_BUFS = {}


def _mid_flags(bk, S, N):
    """caller-owned out-of-range flags of rcmarl_mid_fit_lattice: int32[S*N + 1], zero at first use, reused across calls"""
    key = ("mid", id(bk), S, N)
    if key not in _FLAG_BUFS:
        _FLAG_BUFS[key] = bk.dev(np.zeros(S * N + 1, np.int32))
    return _FLAG_BUFS[key]


def _mb_flags(bk, n=4096):
    """... of rcmarl_minibatch_fit: int32[S * n_adv], zero at first use (the fix-up clears what it consumes)"""
    key = ("mb", id(bk), n)
    if key not in _FLAG_BUFS:
        _FLAG_BUFS[key] = bk.dev(np.zeros(n, np.int32))
    return _FLAG_BUFS[key]


def pad64(n):
    return (n + 63) // 64 * 64


def geom(in_dim, out_dim, hid=HID):
    P = in_dim * hid + hid + hid * hid + hid + hid * out_dim + out_dim
    return P, P - (hid * out_dim + out_dim)


def pack_rows(params_sn, ldp):
    """params_sn[s][n] = [W1..b3] -> theta[S][N][ldp] fp32 (padding = 0)."""
    S, N = len(params_sn), len(params_sn[0])
    th = np.zeros((S, N, ldp), np.float32)
    for s in range(S):
        for n in range(N):
            v = np.concatenate([np.asarray(a, np.float32).ravel() for a in params_sn[s][n]])
            th[s, n, :len(v)] = v
    return th


def unpack_row(row, in_dim, out_dim, hid=HID):
    shapes = [(in_dim, hid), (hid,), (hid, hid), (hid,), (hid, out_dim), (out_dim,)]
    out, o = [], 0
    for sh in shapes:
        n = int(np.prod(sh))
        out.append(row[o:o + n].reshape(sh).copy())
        o += n
    return out


def random_params(rng, S, N, in_dim, out_dim, bias_scale=0.1):
    out = []
    for s in range(S):
        row = []
        for n in range(N):
            p = M.init_mlp(rng, in_dim, HID, out_dim)
            for k in (1, 3, 5):
                p[k] += (bias_scale * rng.normal(size=p[k].shape)).astype(np.float32)
            row.append(p)
        out.append(row)
    return out


def circulant(N, d):
    return np.array([[(i + k) % N for k in range(d)] for i in range(N)], dtype=np.int32)


def random_regular(N, d, rng):
    nbr = np.zeros((N, d), np.int32)
    for i in range(N):
        others = rng.permutation([j for j in range(N) if j != i])[:d - 1]
        nbr[i] = [i] + list(others)
    return nbr


def rel_close(got, want, rtol, what=""):
    scale = max(1.0, float(np.abs(want).max()))
    err = float(np.abs(got - want).max())
    assert err <= rtol * scale, "%s: max abs err %.3e > %.1e * %.3g" % (what, err, rtol, scale)


# ------------------------------------------------------------------------------------------
def check_consensus_params(bk, N, d, H, P, P_hid, graph, S=2):
    rng = np.random.default_rng(N * 100 + d)
    ldp = pad64(P)
    nbr = circulant(N, d) if graph == "circ" else random_regular(N, d, rng)
    coop = np.ones(N, np.int32)
    coop[N - 1] = 0
    base = rng.normal(size=(S, 1, ldp)).astype(np.float32)
    msg = (base + 0.01 * rng.normal(size=(S, N, ldp))).astype(np.float32)
    msg[:, N - 1] = 1e3                       # adversarial row
    msg[:, :, 5] = msg[:, :1, 5]              # ties
    theta0 = rng.normal(size=(S, N, ldp)).astype(np.float32)
    d_msg, d_theta, d_nbr, d_coop = bk.dev(msg), bk.dev(theta0), bk.dev(nbr), bk.dev(coop)
    d_lo, d_hi = bk.dev(np.zeros_like(theta0)), bk.dev(np.zeros_like(theta0))
    bk.lib.rcmarl_consensus_params(bk.ptr(d_msg), bk.ptr(d_theta), bk.ptr(d_nbr), bk.ptr(d_coop), S, N, ldp, P_hid, d,
                                   H, bk.ptr(d_lo), bk.ptr(d_hi), bk.stream)
    theta, lo, hi = bk.host(d_theta), bk.host(d_lo), bk.host(d_hi)
    want = theta0.copy()
    for s in range(S):
        for i in range(N):
            if not coop[i]:
                continue
            vals = msg[s, nbr[i], :P_hid]
            want[s, i, :P_hid] = O.resilient_aggregate(vals, H)
            wl, wh, _ = O.aggregation_bounds(vals, H)
            # order-statistic bounds: bit-exact
            np.testing.assert_array_equal(lo[s, i, :P_hid], wl)
            np.testing.assert_array_equal(hi[s, i, :P_hid], wh)
    # means: fp32 summation order only (|x| up to 1e3 in the adversarial columns)
    np.testing.assert_allclose(theta, want, rtol=2e-6, atol=2e-6)
    # untouched: output-layer columns, padding, non-cooperative rows
    np.testing.assert_array_equal(theta[:, :, P_hid:], theta0[:, :, P_hid:])
    np.testing.assert_array_equal(theta[:, N - 1], theta0[:, N - 1])


def check_consensus_params_circulant(bk, N, d, H, P, P_hid, S=2):
    """The circulant-graph kernel: same oracle checks as check_consensus_params AND bit-identical to the general kernel."""
    assert bk.lib.rcmarl_consensus_params_circulant_supported(N, d, H) == 1
    rng = np.random.default_rng(N * 100 + d + 1)
    ldp = pad64(P)
    nbr = circulant(N, d)
    coop = np.ones(N, np.int32)
    coop[N - 1] = 0
    coop[min(2, N - 1)] = 0
    base = rng.normal(size=(S, 1, ldp)).astype(np.float32)
    msg = (base + 0.01 * rng.normal(size=(S, N, ldp))).astype(np.float32)
    msg[:, N - 1] = 1e3                       # adversarial row
    msg[:, :, 5] = msg[:, :1, 5]              # ties
    msg[:, ::3, 7] = msg[:, :1, 7]            # partial ties
    theta0 = rng.normal(size=(S, N, ldp)).astype(np.float32)
    d_msg, d_nbr, d_coop = bk.dev(msg), bk.dev(nbr), bk.dev(coop)
    out = []
    for circ in (True, False):
        d_theta = bk.dev(theta0)
        d_lo, d_hi = bk.dev(np.zeros_like(theta0)), bk.dev(np.zeros_like(theta0))
        if circ:
            bk.lib.rcmarl_consensus_params_circulant(bk.ptr(d_msg), bk.ptr(d_theta), bk.ptr(d_coop), S, N, ldp, P_hid, d, H,
                                                     bk.ptr(d_lo), bk.ptr(d_hi), bk.stream)
        else:
            bk.lib.rcmarl_consensus_params(bk.ptr(d_msg), bk.ptr(d_theta), bk.ptr(d_nbr), bk.ptr(d_coop), S, N, ldp, P_hid, d,
                                           H, bk.ptr(d_lo), bk.ptr(d_hi), bk.stream)
        out.append((bk.host(d_theta), bk.host(d_lo), bk.host(d_hi)))
    (theta, lo, hi), (theta_g, lo_g, hi_g) = out
    np.testing.assert_array_equal(lo, lo_g)
    np.testing.assert_array_equal(hi, hi_g)
    np.testing.assert_array_equal(theta, theta_g)         # same clip window, same summation order
    for s in range(S):
        for i in range(N):
            if not coop[i]:
                np.testing.assert_array_equal(theta[s, i], theta0[s, i])
                continue
            vals = msg[s, nbr[i], :P_hid]
            wl, wh, _ = O.aggregation_bounds(vals, H)
            np.testing.assert_array_equal(lo[s, i, :P_hid], wl)
            np.testing.assert_array_equal(hi[s, i, :P_hid], wh)
            np.testing.assert_allclose(theta[s, i, :P_hid], O.resilient_aggregate(vals, H), rtol=2e-6, atol=2e-6)
    np.testing.assert_array_equal(theta[:, :, P_hid:], theta0[:, :, P_hid:])


def check_consensus_params_exact(bk, N, d, H, P_hid, S, seed, graph="circ"):
    """K1 against the reference's arithmetic BIT FOR BIT on awkward data: clip bounds = the two order statistics
    (agents/resilient_CAC_agents.py:48-53), mean = the d clipped values added IN NEIGHBOUR ORDER in fp32 and divided by d
    (np.mean over axis 0 of a [d, P] fp32 array is that sequential sum).  Columns of zeros, of subnormal-range values (the
    guarded slow path of the 3-instruction division), of 1e30-scale values, exact ties and an adversarial row; random
    cooperation mask; N not a multiple of the kernel's agent group.  Circulant graphs run both kernels (equal bits)."""
    rng = np.random.default_rng(seed)
    ldp = pad64(P_hid + 21)
    nbr = circulant(N, d) if graph == "circ" else random_regular(N, d, rng)
    coop = (rng.random(N) < 0.8).astype(np.int32)
    coop[int(rng.integers(N))] = 1
    msg = rng.normal(size=(S, N, ldp)).astype(np.float32)
    kinds = rng.integers(0, 6, size=ldp)
    msg[:, :, kinds == 1] = 0.0
    msg[:, :, kinds == 2] *= np.float32(1e-38)                 # sums with subnormal quotients
    msg[:, :, kinds == 3] *= np.float32(1e30)
    msg[:, :, kinds == 4] = np.round(msg[:, :, kinds == 4])     # many exact ties
    msg[:, int(rng.integers(N))] = np.float32(1e3)              # an adversarial row
    theta0 = rng.normal(size=(S, N, ldp)).astype(np.float32)
    d_msg, d_nbr, d_coop = bk.dev(msg), bk.dev(nbr), bk.dev(coop)
    results = []
    kernels = ["general"] + (["circ"] if graph == "circ" and bk.lib.rcmarl_consensus_params_circulant_supported(N, d, H) == 1 else [])
    for kern in kernels:
        d_theta = bk.dev(theta0)
        d_lo, d_hi = bk.dev(np.zeros_like(theta0)), bk.dev(np.zeros_like(theta0))
        if kern == "circ":
            bk.lib.rcmarl_consensus_params_circulant(bk.ptr(d_msg), bk.ptr(d_theta), bk.ptr(d_coop), S, N, ldp, P_hid, d, H,
                                                     bk.ptr(d_lo), bk.ptr(d_hi), bk.stream)
        else:
            bk.lib.rcmarl_consensus_params(bk.ptr(d_msg), bk.ptr(d_theta), bk.ptr(d_nbr), bk.ptr(d_coop), S, N, ldp, P_hid, d,
                                           H, bk.ptr(d_lo), bk.ptr(d_hi), bk.stream)
        results.append((kern, bk.host(d_theta), bk.host(d_lo), bk.host(d_hi)))
    want = theta0.copy()
    with np.errstate(over="ignore", under="ignore"):
        for s in range(S):
            for i in range(N):
                if not coop[i]:
                    continue
                vals = msg[s, nbr[i], :P_hid]
                srt = np.sort(vals, axis=0)
                lo = np.minimum(srt[H], vals[0])
                hi = np.maximum(srt[d - H - 1], vals[0])
                acc = np.zeros(P_hid, np.float32)
                for k in range(d):
                    acc = (acc + np.clip(vals[k], lo, hi)).astype(np.float32)
                want[s, i, :P_hid] = acc / np.float32(d)
                for kern, _, klo, khi in results:
                    np.testing.assert_array_equal(klo[s, i, :P_hid], lo, err_msg=kern)
                    np.testing.assert_array_equal(khi[s, i, :P_hid], hi, err_msg=kern)
    for kern, theta, _, _ in results:
        np.testing.assert_array_equal(theta.view(np.uint32), want.view(np.uint32), err_msg=kern)      # bits, incl. signed zeros


# ------------------------------------------------------------------------------------------
def _layer1(bk, d_x, x_stride, d_theta, d_a1t, S, N, B, in_dim, ldp, ldb):
    bk.lib.rcmarl_layer1_forward(bk.ptr(d_x), x_stride, bk.ptr(d_theta), bk.ptr(d_a1t), S, N, B, in_dim, HID, ldp, ldb,
                                 bk.stream)


def check_layer1_forward(bk, S, N, B, in_dim):
    rng = np.random.default_rng(B + in_dim)
    P, _ = geom(in_dim, 1)
    ldp, ldb = pad64(P), pad64(B)
    params = random_params(rng, S, N, in_dim, 1)
    theta = pack_rows(params, ldp)
    x = rng.normal(size=(S, B, in_dim)).astype(np.float32)
    d_x, d_th = bk.dev(x), bk.dev(theta)
    d_a = bk.dev(np.full((S, N * HID, ldb), np.nan, np.float32))
    _layer1(bk, d_x, B * in_dim, d_th, d_a, S, N, B, in_dim, ldp, ldb)
    a1t = bk.host(d_a)
    for s in range(S):
        for n in range(N):
            want = M.lrelu(x[s] @ params[s][n][0] + params[s][n][1])          # [B, HID]
            rel_close(a1t[s, n * HID:(n + 1) * HID, :B].T, want, 2e-6, "a1")


def check_sgd_fit(bk, S, N, B, in_dim, steps=2, lr=0.01, gamma=0.9, masked_agent=None, knife_edge_agents=0):
    """knife_edge_agents: that many (seed, agent) fits may miss the 1e-5 bar, up to 1e-4 -- a pre-activation within rounding of 0
    takes the other LeakyReLU slope in a kernel whose products round differently from the oracle's (measured: one agent of 128 at
    B = 333, in_dim = 256 with the f16-piece mid kernel; every form shows the same at B = 1000, tools/diag_mid_forms.py)."""
    """`steps` full-batch SGD steps of the local fit (layer1_forward -> mid_fit ->
    small_sgd -> layer1_backward_sgd) incl. the TD target (mid_value) vs the oracle."""
    rng = np.random.default_rng(S * 1000 + N * 100 + B + in_dim)
    P, _ = geom(in_dim, 1)
    ldp, ldb = pad64(P), pad64(B)
    params = random_params(rng, S, N, in_dim, 1)
    theta = pack_rows(params, ldp)
    x = rng.normal(size=(S, B, in_dim)).astype(np.float32)
    nx = rng.normal(size=(S, B, in_dim)).astype(np.float32)
    r_applied = rng.normal(size=(S, N, ldb)).astype(np.float32)
    mask = np.ones(N, np.int32)
    if masked_agent is not None:
        mask[masked_agent] = 0
    nchunk = (B + 255) // 256
    psz = bk.lib.rcmarl_fit_partial_size(HID)
    d_x, d_nx, d_th, d_r, d_mask = bk.dev(x), bk.dev(nx), bk.dev(theta), bk.dev(r_applied), bk.dev(mask)
    d_msg = bk.dev(theta.copy())
    d_a = bk.dev(np.zeros((S, N * HID, ldb), np.float32))
    d_y = bk.dev(np.zeros((S, N, ldb), np.float32))
    d_part = bk.dev(np.zeros((S, N, nchunk, psz), np.float32))
    d_loss = bk.dev(np.zeros((S, N), np.float32))
    L = bk.lib
    # target from the pre-fit weights (agents/resilient_CAC_agents.py:114-115)
    _layer1(bk, d_nx, B * in_dim, d_th, d_a, S, N, B, in_dim, ldp, ldb)
    L.rcmarl_mid_value(bk.ptr(d_a), bk.ptr(d_th), bk.ptr(d_r), gamma, bk.ptr(d_y), S, N, B, in_dim, HID, ldp, ldb,
                       bk.stream)
    for st in range(steps):
        _layer1(bk, d_x, B * in_dim, d_msg, d_a, S, N, B, in_dim, ldp, ldb)
        L.rcmarl_mid_fit(bk.ptr(d_a), bk.ptr(d_msg), bk.ptr(d_y), bk.ptr(d_part), S, N, B, in_dim, HID, ldp, ldb, bk.stream)
        L.rcmarl_small_sgd(bk.ptr(d_part), bk.ptr(d_msg), bk.ptr(d_mask), bk.ptr(d_loss) if st == 0 else None, S, N, B,
                           in_dim, HID, ldp, lr, bk.stream)
        L.rcmarl_layer1_backward_sgd(bk.ptr(d_x), B * in_dim, bk.ptr(d_a), bk.ptr(d_msg), bk.ptr(d_mask), S, N, B, in_dim,
                                     HID, ldp, ldb, lr, bk.stream)
    knife = set()
    msg, y, loss = bk.host(d_msg), bk.host(d_y), bk.host(d_loss)
    for s in range(S):
        for n in range(N):
            p0 = params[s][n]
            target = r_applied[s, n, :B, None] + np.float32(gamma) * M.forward(p0, nx[s])
            rel_close(y[s, n, :B], target[:, 0], 3e-6, "td target")
            if not mask[n]:
                np.testing.assert_array_equal(msg[s, n], theta[s, n])
                continue
            pw = M.copy_params(p0)
            hist = M.fit_mse(pw, x[s], target, lr, epochs=steps)
            got = unpack_row(msg[s, n], in_dim, 1)
            for k in range(6):
                try:
                    rel_close(got[k], pw[k], 1e-5, "fit param %d" % k)
                except AssertionError:
                    knife.add((s, n))
                    rel_close(got[k], pw[k], 1e-4, "fit param %d (knife-edge allowance)" % k)
            assert abs(loss[s, n] - hist[0]) <= 1e-5 * max(1.0, abs(hist[0])), (loss[s, n], hist[0])
    assert len(knife) <= knife_edge_agents, sorted(knife)
    np.testing.assert_array_equal(bk.host(d_th), theta)           # live weights untouched (rollback)


def check_consensus_head(bk, S, N, B, in_dim, d, H, graph="circ", outlier=50.0, compare=True, big_x_rows=None):
    """K2+K3: estimate consensus + projection step of the output layer.  compare=False: only run, return (theta after, aggregate)."""
    rng = np.random.default_rng(S + N * 10 + B + d * 7 + H)
    P, P_hid = geom(in_dim, 1)
    ldp, ldb = pad64(P), pad64(B)
    live = random_params(rng, S, N, in_dim, 1)
    msgp = random_params(rng, S, N, in_dim, 1)
    theta, msg = pack_rows(live, ldp), pack_rows(msgp, ldp)
    x = rng.normal(size=(S, B, in_dim)).astype(np.float32)
    if big_x_rows is not None:                      # replay rows whose layer-1 activations leave the f16 range of the matrix-core form
        x[:, big_x_rows] *= np.float32(3.0e6)
    nbr = circulant(N, d) if graph == "circ" else random_regular(N, d, rng)
    coop = np.ones(N, np.int32)
    coop[0] = 0
    for s in range(S):                              # an outlier head among the messages
        msg[s, 1, P_hid:P] *= np.float32(outlier)
        msgp[s][1][4] = msgp[s][1][4] * np.float32(outlier)
        msgp[s][1][5] = msgp[s][1][5] * np.float32(outlier)
    nchunk = (B + 255) // 256
    d_x, d_th, d_msg, d_nbr, d_coop = bk.dev(x), bk.dev(theta), bk.dev(msg), bk.dev(nbr), bk.dev(coop)
    d_a = bk.dev(np.zeros((S, N * HID, ldb), np.float32))
    d_part = bk.dev(np.zeros((S, N, nchunk, HID + 1), np.float32))
    d_agg = bk.dev(np.zeros((S, N, ldb), np.float32))
    L = bk.lib
    _layer1(bk, d_x, B * in_dim, d_th, d_a, S, N, B, in_dim, ldp, ldb)
    L.rcmarl_consensus_head(bk.ptr(d_a), bk.ptr(d_th), bk.ptr(d_msg), bk.ptr(d_nbr), bk.ptr(d_coop), bk.ptr(d_part),
                            bk.ptr(d_agg), S, N, B, in_dim, HID, ldp, ldb, d, H, bk.stream)
    L.rcmarl_head_apply(bk.ptr(d_part), bk.ptr(d_th), bk.ptr(d_coop), S, N, B, in_dim, HID, ldp, bk.stream)
    th_new, agg = bk.host(d_th), bk.host(d_agg)
    if not compare:
        return th_new, agg
    for s in range(S):
        for i in range(N):
            if not coop[i]:
                np.testing.assert_array_equal(th_new[s, i], theta[s, i])
                continue
            ag = O.CoopAgent(M.init_mlp(rng, in_dim, HID, 5), live[s][i], live[s][i], 0.002, 0.01, 0.9, H)
            want_agg = ag.consensus_estimates_critic(x[s], [msgp[s][j] for j in nbr[i]])
            # fp32 lane code (RCMARL_K2_MX=0): summation order only, 5e-6.  Matrix-core form (the default for 20 units and at most 31
            # neighbours): layer 2 and the heads carry two-piece f16 operands -- each to 2^-22 of ITS magnitude -- and the test plants
            # a head 50 times the others' size: where that estimate sits inside the clip window its error, 50 x 2.4e-7 x sum|terms|,
            # enters the mean; measured 1.6e-5 on the MI355X shapes (profiles/r06f_*) -> 3e-5, i.e. 6e-7 of the planted head
            mx = os.environ.get("RCMARL_K2_MX", "1") not in ("0",) and d + 1 <= 32 and bk.lib.rcmarl_lattice_f16_mode() != 0
            rel_close(agg[s, i, :B], want_agg[:, 0], 3e-5 if mx else 5e-6, "estimate aggregate")
            ag.projection_step_critic(x[s], want_agg)
            got = unpack_row(th_new[s, i], in_dim, 1)
            for k in range(4):
                np.testing.assert_array_equal(got[k], live[s][i][k])          # hidden layers frozen
            rel_close(got[4], ag.critic[4], 2e-5, "W3 after projection")
            rel_close(got[5], ag.critic[5], 2e-5, "b3 after projection")


def _ptr_add(ptr, nbytes):
    """device pointer (int on the GPU backend, ctypes.c_void_p on the emulation) + a byte offset"""
    import ctypes
    return ctypes.c_void_p(ptr.value + nbytes) if isinstance(ptr, ctypes.c_void_p) else ptr + nbytes


def check_mid_value(bk, S, N, B, in_dim, row_off=0, big_w2_agent=None, big_a1_rows=None, gamma=0.9, compare=True, entry="rcmarl_mid_value"):
    """rcmarl_mid_value on cached layer-1 activations: v = head(layer2(a1)) [r + gamma v], against the oracle's layers 2-3 in fp32.
    row_off: the base pointer the engine passes for shifted rows (a1 + row_off rows, B - row_off rows).  big_w2_agent: that agent's W2
    beyond the f16 range of the matrix-core form; big_a1_rows: activations beyond it in those rows -> the fp32 lane code, bit for bit."""
    rng = np.random.default_rng(S * 7 + N * 3 + B + in_dim)
    P, _ = geom(in_dim, 1)
    ldp, ldb = pad64(P), pad64(B)
    params = random_params(rng, S, N, in_dim, 1)
    if big_w2_agent is not None:
        for s in range(S):
            params[s][big_w2_agent][2][3, 5] = np.float32(2000.0)
    theta = pack_rows(params, ldp)
    a1 = rng.normal(size=(S, N * HID, ldb)).astype(np.float32)
    if big_a1_rows is not None:
        a1[:, 7, big_a1_rows] = np.float32(1.0e5)
    r_applied = rng.normal(size=(S, N, ldb)).astype(np.float32)
    d_a, d_th, d_r = bk.dev(a1), bk.dev(theta), bk.dev(r_applied)
    d_y = bk.dev(np.full((S, N, ldb), np.float32(-7.0)))
    nrows = B - row_off
    out = {}
    for with_r in (True, False):
        getattr(bk.lib, entry)(_ptr_add(bk.ptr(d_a), 4 * row_off), bk.ptr(d_th), bk.ptr(d_r) if with_r else None, gamma, bk.ptr(d_y), S, N, nrows,
                                in_dim, HID, ldp, ldb, bk.stream)
        y = bk.host(d_y)
        out[with_r] = y.copy()
        if not compare:
            continue
        assert np.all(y[:, :, nrows:] == np.float32(-7.0))            # nothing written beyond the rows asked for
        for s in range(S):
            for n in range(N):
                W1, b1, W2, b2, W3, b3 = params[s][n]
                a = a1[s, n * HID:(n + 1) * HID, row_off:B].T                                     # [rows][HID]
                z2 = a @ W2 + b2
                v = (np.maximum(z2, np.float32(0.1) * z2) @ W3 + b3)[:, 0]
                want = r_applied[s, n, :nrows] + np.float32(gamma) * v if with_r else v
                rel_close(y[s, n, :nrows], want, 3e-6, "value on cached activations")
    return out


def check_actor_step(bk, S, N, B, in_dim, steps=2, lr=0.002):
    rng = np.random.default_rng(S + N + B + in_dim)
    A = 5
    P, _ = geom(in_dim, A)
    ldp, ldb = pad64(P), pad64(B)
    params = random_params(rng, S, N, in_dim, A)
    theta = pack_rows(params, ldp)
    x = rng.normal(size=(S, B, in_dim)).astype(np.float32)
    act = rng.integers(0, A, size=(S, N, ldb)).astype(np.float32)
    delta = rng.normal(size=(S, N, ldb)).astype(np.float32)
    mask = np.ones(N, np.int32)
    mask[N - 1] = 0
    nchunk = (B + 255) // 256
    psz = bk.lib.rcmarl_actor_partial_size(HID, A)
    d_x, d_th, d_act, d_delta, d_mask = bk.dev(x), bk.dev(theta), bk.dev(act), bk.dev(delta), bk.dev(mask)
    d_m, d_v = bk.dev(np.zeros_like(theta)), bk.dev(np.zeros_like(theta))
    d_a = bk.dev(np.zeros((S, N * HID, ldb), np.float32))
    d_part = bk.dev(np.zeros((S, N, nchunk, psz), np.float32))
    d_loss = bk.dev(np.zeros((S, N), np.float32))
    L = bk.lib
    b1, b2, eps = 0.9, 0.999, 1e-7
    losses = []
    for t in range(1, steps + 1):
        alpha = np.float32(lr * np.sqrt(1.0 - b2 ** t) / (1.0 - b1 ** t))
        _layer1(bk, d_x, B * in_dim, d_th, d_a, S, N, B, in_dim, ldp, ldb)
        L.rcmarl_mid_actor(bk.ptr(d_a), bk.ptr(d_th), bk.ptr(d_act), bk.ptr(d_delta), bk.ptr(d_part), S, N, B, in_dim, HID,
                           A, ldp, ldb, bk.stream)
        L.rcmarl_small_adam(bk.ptr(d_part), bk.ptr(d_th), bk.ptr(d_m), bk.ptr(d_v), bk.ptr(d_mask), bk.ptr(d_loss), S, N, B,
                            in_dim, HID, A, ldp, float(alpha), float(np.float32(1 - b1)), float(np.float32(1 - b2)),
                            float(np.float32(eps)), bk.stream)
        L.rcmarl_layer1_backward_adam(bk.ptr(d_x), B * in_dim, bk.ptr(d_a), bk.ptr(d_th), bk.ptr(d_m), bk.ptr(d_v),
                                      bk.ptr(d_mask), S, N, B, in_dim, HID, ldp, ldb, float(alpha),
                                      float(np.float32(1 - b1)), float(np.float32(1 - b2)), float(np.float32(eps)),
                                      bk.stream)
        losses.append(bk.host(d_loss).copy())
        if t == 1:
            m_first = bk.host(d_m).copy()               # after ONE Adam step m = (1 - beta1) g: the gradient itself
    th_new = bk.host(d_th)
    errs = [[] for _ in range(6)]
    g_errs = []
    for s in range(S):
        for n in range(N):
            if not mask[n]:
                np.testing.assert_array_equal(th_new[s, n], theta[s, n])
                continue
            pw = M.copy_params(params[s][n])
            st = M.AdamState(pw, lr)
            for t in range(steps):
                l = M.fit_actor_ce(pw, st, x[s], act[s, n, :B], delta[s, n, :B], epochs=1)[0]
                assert abs(losses[t][s, n] - l) <= 2e-5 * max(1.0, abs(l)), (t, losses[t][s, n], l)
                if t == 0:
                    # deterministic bar (identical inputs): the actor GRADIENT (agents/resilient_CAC_agents.py:99) relative to
                    # its largest entry -- the parameters below can only be judged in units of an Adam step
                    want = np.concatenate([np.asarray(a, np.float32).ravel() for a in st.m])
                    g_errs.append(float(np.abs(m_first[s, n, :want.size] - want).max()) / float(np.abs(want).max()))
            got = unpack_row(th_new[s, n], in_dim, A)
            for k in range(6):
                errs[k].append(np.abs(got[k] - pw[k]).ravel())
    for k in range(6):
        # Adam turns every gradient into a ~+-lr step, so errors are judged in units of lr.  Two legitimate
        # knife edges exist between any two fp32 summation orders: a pre-activation within rounding of 0
        # flips its LeakyReLU slope (moves one unit's gradient column by a few %), and a gradient of
        # magnitude ~eps can land anywhere in [-lr, lr].  Hence: bulk within 2% of a step, a vanishing
        # fraction of outliers, none beyond 2 full steps per update.
        e = np.concatenate(errs[k])
        assert e.max() <= 2.0 * lr * steps + 1e-6, ("actor param", k, e.max())
        assert np.mean(e > 0.02 * lr * steps + 1e-6) <= 2e-3, ("actor param outliers", k, np.mean(e > 0.02 * lr * steps))
    # One knife edge survives identical inputs: a pre-activation within rounding of 0 takes the other LeakyReLU slope in one of
    # the two summation orders and moves one unit's gradient column by that row's whole contribution (~1 % of the column; seen
    # at 256 agents x 1000 rows x 40 units = 10 M pre-activations: agent 160, 5.9e-3).  Bar: every agent within 1e-4 except
    # at most 2 % of them, none beyond 5e-2.
    g = np.asarray(g_errs)
    bulk = float(np.median(g)) if g.size else 0.0
    assert g.size == 0 or (float(np.mean(g > 1e-4)) <= 0.02 and float(g.max()) <= 5e-2), ("actor gradient", float(g.max()), float(np.mean(g > 1e-4)))
    print("[parity] actor gradient (Adam m after one step, identical inputs) S=%d N=%d B=%d in=%d: max|dm| / max|m| median %.2e, worst %.2e, "
          "agents beyond 1e-4: %d of %d" % (S, N, B, in_dim, bulk, float(g.max()) if g.size else 0.0, int(np.sum(g > 1e-4)), g.size))
    return float(g.max()) if g.size else 0.0


# ------------------------------------------------------------------------------------------
def check_reward_helpers(bk, S, N, B):
    rng = np.random.default_rng(S + N + B)
    ldb = pad64(B)
    cap = B + 7
    r = rng.normal(size=(S, cap, N)).astype(np.float32)
    coop = np.ones(N, np.int32)
    coop[N // 2] = 0
    n_coop = int(coop.sum())
    mode = np.zeros(N, np.int32)
    mode[0], mode[N // 2] = 1, 2
    d_r, d_coop, d_mode = bk.dev(r), bk.dev(coop), bk.dev(mode)
    d_rc = bk.dev(np.zeros((S, ldb), np.float32))
    d_out = bk.dev(np.zeros((S, N, ldb), np.float32))
    L = bk.lib
    L.rcmarl_team_reward(bk.ptr(d_r), cap * N, bk.ptr(d_coop), n_coop, bk.ptr(d_rc), S, N, B, ldb, bk.stream)
    L.rcmarl_gather_agent_major(bk.ptr(d_r), cap * N, bk.ptr(d_rc), bk.ptr(d_mode), bk.ptr(d_out), S, N, B, ldb, bk.stream)
    rc, out = bk.host(d_rc), bk.host(d_out)
    for s in range(S):
        want = np.zeros(B, np.float32)
        for n in range(N):
            if coop[n]:
                want += r[s, :B, n] / n_coop                          # train_agents.py:96-98
        np.testing.assert_array_equal(rc[s, :B], want)
        for n in range(N):
            w = r[s, :B, n] if mode[n] == 0 else (want if mode[n] == 1 else -want)
            np.testing.assert_array_equal(out[s, n, :B], w)
    a, b, c = (rng.normal(size=1000).astype(np.float32) for _ in range(3))
    d_o, d_a, d_b, d_c = bk.dev(np.zeros(1000, np.float32)), bk.dev(a), bk.dev(b), bk.dev(c)
    L.rcmarl_td_error(bk.ptr(d_a), bk.ptr(d_b), bk.ptr(d_c), 0.9, bk.ptr(d_o), 1000, bk.stream)
    # r + gamma*nV - V (agents/resilient_CAC_agents.py:98) with every operation rounded to fp32, in that order (the library is built
    # without fp contraction): bits
    want = ((a + (np.float32(0.9) * b).astype(np.float32)).astype(np.float32) - c).astype(np.float32)
    np.testing.assert_array_equal(bk.host(d_o).view(np.uint32), want.view(np.uint32))


# ------------------------------------------------------------------------------------------
def check_rollout(bk, S, N, nrow, ncol, steps=6, mode="device"):
    """Rollout kernels vs the oracle env + agents: policy probabilities, start-state
    values, Philox sampling, transitions, rewards, replay rows, discounted returns."""
    from oracle import philox_np as PX
    rng = np.random.default_rng(S * 7 + N)
    A = 5
    in_a = 2 * N
    Pa, _ = geom(in_a, A)
    Pc, _ = geom(in_a, 1)
    ldpa, ldpc = pad64(Pa), pad64(Pc)
    actors = random_params(rng, S, N, in_a, A, bias_scale=0.3)
    critics = random_params(rng, S, N, in_a, 1)
    th_a, th_c = pack_rows(actors, ldpa), pack_rows(critics, ldpc)
    goal = rng.integers(0, min(5, nrow), size=(S, N, 2)).astype(np.int32)
    seeds = np.array([1000 + 17 * s for s in range(S)], dtype=np.uint64)
    scale = np.array([np.mean(np.arange(nrow)), np.mean(np.arange(ncol)), np.std(np.arange(nrow)), np.std(np.arange(ncol))])
    cap = steps + 3
    gamma, mu, episode = 0.9, 0.1, 5
    L = bk.lib
    d_tha, d_thc, d_goal, d_seeds, d_scale = bk.dev(th_a), bk.dev(th_c), bk.dev(goal), bk.dev(seeds), bk.dev(scale)
    d_pos = [bk.dev(np.zeros((S, N, 2), np.int32)) for _ in range(2)]
    d_xs = [bk.dev(np.zeros((S, 2 * N), np.float32)) for _ in range(2)]
    d_ret = bk.dev(np.zeros((S, N), np.float64))
    rp = {k: bk.dev(np.zeros((S, cap, w * N), np.float32)) for k, w in (("s", 2), ("ns", 2), ("sa", 3), ("a", 1), ("r", 1))}
    d_probs = bk.dev(np.zeros((S, N, A), np.float32))
    d_val = bk.dev(np.zeros((S, N), np.float32))
    d_act = bk.dev(np.zeros((S, N), np.int32))
    L.rcmarl_env_reset(None, bk.ptr(d_seeds), nrow, ncol, bk.ptr(d_scale), episode, bk.ptr(d_pos[0]), bk.ptr(d_xs[0]),
                       bk.ptr(d_ret), S, N, bk.stream)
    envs = []
    for s in range(S):
        env = O.GridWorldOracle(nrow, ncol, N, goal[s], None, True, True, rng_mode="device", seed=int(seeds[s]))
        env.reset(episode=episode)
        envs.append(env)
    np.testing.assert_array_equal(bk.host(d_pos[0]), np.stack([e.state for e in envs]))
    L.rcmarl_value_rows(bk.ptr(d_xs[0]), bk.ptr(d_thc), bk.ptr(d_val), S, N, in_a, HID, ldpc, bk.stream)
    val = bk.host(d_val)
    for s in range(S):
        st, _ = envs[s].get_data()
        np.testing.assert_array_equal(bk.host(d_xs[0])[s], st.astype(np.float32).ravel())
        for i in range(N):
            want = M.forward(critics[s][i], st.astype(np.float32).reshape(1, -1))[0, 0]
            assert abs(val[s, i] - want) <= 3e-6 * max(1.0, abs(want))
    want_ret = np.zeros((S, N))
    cur = 0
    n_flip = 0
    for j in range(steps):
        L.rcmarl_policy_probs(bk.ptr(d_xs[cur]), bk.ptr(d_tha), bk.ptr(d_probs), S, N, in_a, HID, A, ldpa, bk.stream)
        probs = bk.host(d_probs)
        oracle_act = np.zeros((S, N), np.int64)
        for s in range(S):
            st, _ = envs[s].get_data()
            op = np.stack([M.softmax(M.forward(actors[s][i], st.astype(np.float32).reshape(1, -1)))[0] for i in range(N)])
            rel_close(probs[s], op, 3e-6, "policy probs")
            oracle_act[s] = PX.sample_actions(op, int(seeds[s]), episode, j, mu)
        if mode == "device":
            L.rcmarl_rollout_step(bk.ptr(d_xs[cur]), bk.ptr(d_pos[cur]), bk.ptr(d_goal), bk.ptr(d_tha), bk.ptr(d_seeds),
                                  nrow, ncol, bk.ptr(d_scale), bk.ptr(rp["s"]), bk.ptr(rp["ns"]), bk.ptr(rp["sa"]),
                                  bk.ptr(rp["a"]), bk.ptr(rp["r"]), cap, j, bk.ptr(d_pos[1 - cur]), bk.ptr(d_xs[1 - cur]),
                                  bk.ptr(d_ret), float(gamma ** j), episode, j, mu, S, N, HID, A, ldpa, bk.ptr(d_act),
                                  bk.stream)
            act = bk.host(d_act).astype(np.int64)
            n_flip += int((act != oracle_act).sum())     # only possible through last-ulp cdf differences
        else:
            act = oracle_act
            d_a = bk.dev(act.astype(np.int32))
            L.rcmarl_env_apply(bk.ptr(d_pos[cur]), bk.ptr(d_goal), bk.ptr(d_a), nrow, ncol, bk.ptr(d_scale), bk.ptr(rp["s"]),
                               bk.ptr(rp["ns"]), bk.ptr(rp["sa"]), bk.ptr(rp["a"]), bk.ptr(rp["r"]), cap, j,
                               bk.ptr(d_pos[1 - cur]), bk.ptr(d_xs[1 - cur]), bk.ptr(d_ret), float(gamma ** j), S, N,
                               bk.stream)
        cur = 1 - cur
        H = {k: bk.host(v) for k, v in rp.items()}
        for s in range(S):
            st, _ = envs[s].get_data()
            envs[s].step(act[s].astype(np.float64))
            nst, rew = envs[s].get_data()
            want_ret[s] += rew * (gamma ** j)
            np.testing.assert_array_equal(bk.host(d_pos[cur])[s], envs[s].state)
            np.testing.assert_array_equal(H["s"][s, j], st.astype(np.float32).ravel())
            np.testing.assert_array_equal(H["ns"][s, j], nst.astype(np.float32).ravel())
            np.testing.assert_array_equal(H["a"][s, j], act[s].astype(np.float32))
            np.testing.assert_array_equal(H["r"][s, j], rew.astype(np.float32))
            np.testing.assert_array_equal(H["sa"][s, j], np.concatenate([st.astype(np.float32), act[s].astype(np.float32)[:, None]], axis=1).ravel())
    np.testing.assert_array_equal(bk.host(d_ret), want_ret)      # float64, same operation order
    assert n_flip == 0, "%d sampled actions differ from the oracle's Philox stream" % n_flip


# ------------------------------------------------------------------------------------------
def check_minibatch_fit(bk, S, N, B, in_dim, advs, bs=32, epochs=3, lr=0.01, shuffle=True, knife_edge_nets=0):
    """X1: whole mini-batch fit(batch_size, epochs) of the adversaries' critic/TR in one launch
    vs oracle mlp_np.fit_mse with the same permutations.
    knife_edge_nets: that many networks may miss the 2e-5 bar, up to 1e-2.  The fp32 kernel repeats the oracle's fmaf chains bit for
    bit, so it holds 2e-5 on every network (RCMARL_MB_MX=0 tests).  ANY other fp32-accurate arithmetic does not, and cannot: over the
    adversaries' real chain (940 dependent SGD steps at lr 0.01) a pre-activation within rounding of zero takes the other LeakyReLU
    slope and plain SGD amplifies the difference.  Measured on 5120 networks (tools/knife_edge_hist.py,
    profiles/r04m_knife_edge_hist.txt): f16 matrix-core kernel vs fp32 kernel -- 94.6 % of the networks within 2e-5, 96.8 % within
    1e-3, max 1.5e-2; CONTROL, the fp32 kernel vs itself started ONE ULP away in one weight -- 96.1 % within 2e-5, 97.8 % within
    1e-3, max 4.8e-2.  The f16 kernel drifts from the fp32 chain like a second fp32 run does; a bar of "1e-4 for 99.9 %" holds for
    neither.  The short chains of these tests (<= 3 epochs) allow `knife_edge_nets` such networks, bounded at 1e-2."""
    knife = set()
    rng = np.random.default_rng(S * 31 + N * 7 + B + in_dim)
    P, _ = geom(in_dim, 1)
    ldp, ldb = pad64(P), pad64(B)
    params = random_params(rng, S, N, in_dim, 1)
    theta = pack_rows(params, ldp)
    cap = B + 5
    x = rng.normal(size=(S, cap, in_dim)).astype(np.float32)
    y = rng.normal(size=(S, N, ldb)).astype(np.float32)
    advs = np.asarray(advs, np.int32)
    nA = len(advs)
    perm = np.stack([[[rng.permutation(B) for _ in range(epochs)] for _ in range(nA)] for _ in range(S)]).astype(np.int32)
    d_x, d_th, d_y, d_adv, d_perm = bk.dev(x), bk.dev(theta), bk.dev(y), bk.dev(advs), bk.dev(perm)
    d_loss = bk.dev(np.zeros((S, N), np.float32))
    bk.lib.rcmarl_minibatch_fit(bk.ptr(d_x), cap * in_dim, bk.ptr(d_th), bk.ptr(d_adv), nA, bk.ptr(d_y),
                                bk.ptr(d_perm) if shuffle else None, S, N, B, in_dim, HID, ldp, ldb, bs, epochs, lr,
                                bk.ptr(d_loss), bk.ptr(_mb_flags(bk)), bk.stream)
    th_new, loss = bk.host(d_th), bk.host(d_loss)
    for s in range(S):
        for n in range(N):
            if n not in advs:
                np.testing.assert_array_equal(th_new[s, n], theta[s, n])
                continue
            k = list(advs).index(n)
            pw = M.copy_params(params[s][n])
            hist = M.fit_mse(pw, x[s, :B], y[s, n, :B], lr, epochs=epochs, batch_size=bs,
                             perms=perm[s, k] if shuffle else np.tile(np.arange(B), (epochs, 1)))
            got = unpack_row(th_new[s, n], in_dim, 1)
            for q in range(6):
                try:
                    rel_close(got[q], pw[q], 2e-5, "minibatch fit param %d" % q)
                except AssertionError:
                    knife.add((s, n))
                    rel_close(got[q], pw[q], 1e-2, "minibatch fit param %d (knife-edge allowance)" % q)
            assert abs(loss[s, n] - hist[0]) <= 2e-5 * max(1.0, abs(hist[0])), (loss[s, n], hist[0])
    assert len(knife) <= knife_edge_nets, sorted(knife)
    return th_new, loss


def check_minibatch_fit_multi(bk, S=2, N=5, B=96, in_dims=(10, 15, 10), adv_sets=((4,), (3, 4), (3, 4)), bs=32, epochs=2, lr=0.01, blow=None):
    """rcmarl_minibatch_fit_multi: several fits in ONE launch (the Malicious agent's private critic, compromised team-reward net and
    compromised critic of a consensus epoch) leave the bits that one rcmarl_minibatch_fit call per job leaves -- parameters, losses
    and untouched rows alike.  (The single-job entry point is held to the oracle by check_minibatch_fit.)
    blow = (job, position in its adversary list): that network's layer-2 weights are +-100 (2^10 W beyond the f16 range), so the f16
    kernel flags it through THAT job's ovf_flags and the fp32 fix-up launch redoes it -- in both launch forms."""
    from rcmarl_amd import capi
    import pytest
    rng = np.random.default_rng(77)
    ldb, cap = pad64(B), B + 3
    jobs = []
    for jn, (in_dim, advs) in enumerate(zip(in_dims, adv_sets)):
        P, _ = geom(in_dim, 1)
        ldp = pad64(P)
        advs = np.asarray(advs, np.int32)
        params = random_params(rng, S, N, in_dim, 1)
        if blow is not None and blow[0] == jn:
            for s_ in range(S):
                w2 = params[s_][int(advs[blow[1]])][2]
                w2[...] = np.float32(100.0) * rng.choice([-1.0, 1.0], size=w2.shape).astype(np.float32)
        jobs.append(dict(in_dim=in_dim, ldp=ldp, advs=advs, theta=pack_rows(params, ldp),
                         x=rng.normal(size=(S, cap, in_dim)).astype(np.float32), y=rng.normal(size=(S, N, ldb)).astype(np.float32),
                         perm=np.stack([[[rng.permutation(B) for _ in range(epochs)] for _ in advs] for _ in range(S)]).astype(np.int32)))
    results = {}
    for mode in ("single", "multi"):
        dev = []
        for j in jobs:
            dev.append(dict(x=bk.dev(j["x"]), th=bk.dev(j["theta"]), y=bk.dev(j["y"]), adv=bk.dev(j["advs"]), perm=bk.dev(j["perm"]),
                            loss=bk.dev(np.zeros((S, N), np.float32)), flags=bk.dev(np.zeros(S * len(j["advs"]) + 1, np.int32))))
        if mode == "single":
            for j, d in zip(jobs, dev):
                rc = bk.lib.rcmarl_minibatch_fit(bk.ptr(d["x"]), cap * j["in_dim"], bk.ptr(d["th"]), bk.ptr(d["adv"]), len(j["advs"]),
                                                 bk.ptr(d["y"]), bk.ptr(d["perm"]), S, N, B, j["in_dim"], HID, j["ldp"], ldb, bs, epochs, lr,
                                                 bk.ptr(d["loss"]), bk.ptr(d["flags"]), bk.stream)
                assert rc in (0, None)
        else:
            arr = (capi.MbJob * len(jobs))(*[capi.MbJob(bk.ptr(d["x"]), cap * j["in_dim"], bk.ptr(d["th"]), bk.ptr(d["adv"]), len(j["advs"]),
                                                        j["in_dim"], j["ldp"], 0, bk.ptr(d["y"]), bk.ptr(d["perm"]), bk.ptr(d["loss"]),
                                                        bk.ptr(d["flags"])) for j, d in zip(jobs, dev)])
            rc = bk.lib.rcmarl_minibatch_fit_multi(arr, len(jobs), S, N, B, HID, ldb, bs, epochs, lr, bk.stream)
            assert rc in (0, None)
        results[mode] = [(bk.host(d["th"]), bk.host(d["loss"])) for d in dev]
    for j, (a, b) in enumerate(zip(results["single"], results["multi"])):
        np.testing.assert_array_equal(a[0], b[0], err_msg="job %d parameters" % j)
        np.testing.assert_array_equal(a[1], b[1], err_msg="job %d losses" % j)
        assert not np.array_equal(a[0], jobs[j]["theta"])
    # job lists the entry point does not take -> RCMARL_ERR_UNSUPPORTED before anything is launched: mixed input classes (<= 16 and
    # 17..20 inputs need different kernel forms) and more jobs than one launch carries
    d, j = dev[0], jobs[0]
    other = 18 if j["in_dim"] <= 16 else 10
    mk = lambda in_dim: capi.MbJob(bk.ptr(d["x"]), cap * j["in_dim"], bk.ptr(d["th"]), bk.ptr(d["adv"]), len(j["advs"]), in_dim, j["ldp"], 0,
                                   bk.ptr(d["y"]), bk.ptr(d["perm"]), bk.ptr(d["loss"]), bk.ptr(d["flags"]))
    before = bk.host(d["th"]).copy()
    for bad in ([mk(j["in_dim"]), mk(other)], [mk(j["in_dim"])] * 5):
        arr = (capi.MbJob * len(bad))(*bad)
        with pytest.raises(capi.RcmarlError, match="RCMARL_ERR_UNSUPPORTED"):
            bk.lib.rcmarl_minibatch_fit_multi(arr, len(bad), S, N, B, HID, ldb, bs, epochs, lr, bk.stream)
    np.testing.assert_array_equal(bk.host(d["th"]), before)
    return results


def check_shuffle_perms(bk, seeds, calls, epochs, B):
    """rcmarl_shuffle_perms (csrc/shuffle.hip: per permutation a bucket sort of the Philox keys) against the oracle's ShuffleStream
    (argsort of the same keys, ties to the lower row): every entry equal."""
    from oracle.rpbcac_oracle import ShuffleStream
    S, n = len(seeds), len(calls)
    d_seeds = bk.dev(np.asarray(seeds, np.uint64))
    d_calls = bk.dev(np.asarray(calls, np.int32))
    d_perm = bk.dev(np.full((S, n, epochs, B), -1, np.int32))
    assert bk.lib.rcmarl_shuffle_perms(bk.ptr(d_seeds), bk.ptr(d_calls), n, epochs, B, bk.ptr(d_perm), S, bk.stream) in (0, None)
    perm = bk.host(d_perm)
    for si, seed in enumerate(seeds):
        for qi, call in enumerate(calls):
            st = ShuffleStream(seed)
            st.calls = int(call)
            np.testing.assert_array_equal(perm[si, qi], st.perms(epochs, B))


def run_minibatch_fit_with_blown_network(bk, S=1, N=5, B=96, in_dim=10, lr=0.01):
    """One mini-batch fit of two adversaries' networks, the first with layer-2 weights of 100 (2^10 W beyond the f16 range) ->
    (rows of the blown-up network, rows of the healthy one) after the fit."""
    rng = np.random.default_rng(5)
    P, _ = geom(in_dim, 1)
    ldp, ldb = pad64(P), pad64(B)
    params = random_params(rng, S, N, in_dim, 1)
    for s_ in range(S):
        params[s_][1][2] *= np.float32(0) ; params[s_][1][2] += np.float32(100.0) * rng.choice([-1.0, 1.0], size=params[s_][1][2].shape).astype(np.float32)
    theta = pack_rows(params, ldp)
    x = rng.normal(size=(S, B, in_dim)).astype(np.float32)
    y = rng.normal(size=(S, N, ldb)).astype(np.float32)
    advs = np.asarray([1, 3], np.int32)
    perm = np.stack([[[rng.permutation(B) for _ in range(2)] for _ in range(2)] for _ in range(S)]).astype(np.int32)
    d_x, d_th, d_y, d_adv, d_perm = bk.dev(x), bk.dev(theta), bk.dev(y), bk.dev(advs), bk.dev(perm)
    bk.lib.rcmarl_minibatch_fit(bk.ptr(d_x), B * in_dim, bk.ptr(d_th), bk.ptr(d_adv), 2, bk.ptr(d_y), bk.ptr(d_perm), S, N, B, in_dim,
                                HID, ldp, ldb, 32, 2, lr, None, bk.ptr(_mb_flags(bk)), bk.stream)
    th = bk.host(d_th)
    assert not np.array_equal(th[:, 1], theta[:, 1]) and not np.array_equal(th[:, 3], theta[:, 3])      # both networks were fitted
    return th[:, 1].copy(), th[:, 3].copy()


def check_minibatch_actor(bk, S, N, B, in_dim, advs, bs=200, lr=0.002, t0=0, shuffle=True):
    """X1: the adversaries' actor fit(batch_size=200, epochs=1) with Adam vs oracle fit_actor_ce."""
    rng = np.random.default_rng(S * 13 + N * 5 + B + in_dim)
    A = 5
    P, _ = geom(in_dim, A)
    ldp, ldb = pad64(P), pad64(B)
    params = random_params(rng, S, N, in_dim, A)
    theta = pack_rows(params, ldp)
    x = rng.normal(size=(S, B, in_dim)).astype(np.float32)
    act = rng.integers(0, A, size=(S, N, ldb)).astype(np.float32)
    delta = rng.normal(size=(S, N, ldb)).astype(np.float32)
    advs = np.asarray(advs, np.int32)
    nA = len(advs)
    perm = np.stack([[[rng.permutation(B)] for _ in range(nA)] for _ in range(S)]).astype(np.int32)
    m0 = (0.01 * rng.normal(size=theta.shape)).astype(np.float32) if t0 else np.zeros_like(theta)
    v0 = (1e-4 * rng.random(size=theta.shape)).astype(np.float32) if t0 else np.zeros_like(theta)
    d_x, d_th, d_act, d_delta, d_adv, d_perm = bk.dev(x), bk.dev(theta), bk.dev(act), bk.dev(delta), bk.dev(advs), bk.dev(perm)
    d_m, d_v = bk.dev(m0), bk.dev(v0)
    d_loss = bk.dev(np.zeros((S, N), np.float32))
    bk.lib.rcmarl_minibatch_actor(bk.ptr(d_x), B * in_dim, bk.ptr(d_th), bk.ptr(d_m), bk.ptr(d_v), bk.ptr(d_adv), nA,
                                  bk.ptr(d_act), bk.ptr(d_delta), bk.ptr(d_perm) if shuffle else None, S, N, B, in_dim, HID,
                                  A, ldp, ldb, bs, 1, lr, 0.9, 0.999, 1e-7, t0, bk.ptr(d_loss), bk.stream)
    th_new, loss = bk.host(d_th), bk.host(d_loss)
    nsteps = (B + bs - 1) // bs
    for s in range(S):
        for n in range(N):
            if n not in advs:
                np.testing.assert_array_equal(th_new[s, n], theta[s, n])
                continue
            k = list(advs).index(n)
            pw = M.copy_params(params[s][n])
            st = M.AdamState(pw, lr)
            st.t = t0
            st.m = unpack_row(m0[s, n], in_dim, A)
            st.v = unpack_row(v0[s, n], in_dim, A)
            l = M.fit_actor_ce(pw, st, x[s], act[s, n, :B], delta[s, n, :B], epochs=1, batch_size=bs,
                               perms=perm[s, k] if shuffle else None)[0]
            assert abs(loss[s, n] - l) <= 2e-5 * max(1.0, abs(l)), (loss[s, n], l)
            got = unpack_row(th_new[s, n], in_dim, A)
            for q in range(6):
                assert np.abs(got[q] - pw[q]).max() <= 0.02 * lr * nsteps + 1e-6, ("mb actor param", q, np.abs(got[q] - pw[q]).max())


def check_projection(bk, S, N, B, in_dim):
    """K3 alone: projection step toward a caller-supplied aggregate."""
    rng = np.random.default_rng(S + N + B + in_dim)
    P, _ = geom(in_dim, 1)
    ldp, ldb = pad64(P), pad64(B)
    live = random_params(rng, S, N, in_dim, 1)
    theta = pack_rows(live, ldp)
    x = rng.normal(size=(S, B, in_dim)).astype(np.float32)
    agg = rng.normal(size=(S, N, ldb)).astype(np.float32)
    coop = np.ones(N, np.int32)
    coop[N - 1] = 0
    nchunk = (B + 255) // 256
    d_x, d_th, d_agg, d_coop = bk.dev(x), bk.dev(theta), bk.dev(agg), bk.dev(coop)
    d_a = bk.dev(np.zeros((S, N * HID, ldb), np.float32))
    d_part = bk.dev(np.zeros((S, N, nchunk, HID + 1), np.float32))
    L = bk.lib
    _layer1(bk, d_x, B * in_dim, d_th, d_a, S, N, B, in_dim, ldp, ldb)
    L.rcmarl_projection_residual(bk.ptr(d_a), bk.ptr(d_th), bk.ptr(d_agg), bk.ptr(d_coop), bk.ptr(d_part), S, N, B, in_dim,
                                 HID, ldp, ldb, bk.stream)
    L.rcmarl_head_apply(bk.ptr(d_part), bk.ptr(d_th), bk.ptr(d_coop), S, N, B, in_dim, HID, ldp, bk.stream)
    th_new = bk.host(d_th)
    for s in range(S):
        for i in range(N):
            if not coop[i]:
                np.testing.assert_array_equal(th_new[s, i], theta[s, i])
                continue
            ag = O.CoopAgent(M.init_mlp(rng, in_dim, HID, 5), live[s][i], live[s][i], 0.002, 0.01, 0.9, 0)
            ag.projection_step_critic(x[s], agg[s, i, :B, None])
            got = unpack_row(th_new[s, i], in_dim, 1)
            rel_close(got[4], ag.critic[4], 2e-5, "W3 after projection")
            rel_close(got[5], ag.critic[5], 2e-5, "b3 after projection")


# ------------------------------------------------------------------------------------------
# lattice (exact bf16x3) layer-1 path: csrc/lattice_gemm.hip
from rcmarl_amd import lattice as LT  # noqa: E402


def lattice_rows(rng, S, B, n_agents, width, nrow, ncol, scaling=True):
    """Replay rows exactly as the environment produces them (environments/grid_world.py:66-72:
    float64 (pos-mean)/std, cast to fp32 at training/train_agents.py:89-92) + raw action columns."""
    pos = np.stack([rng.integers(0, nrow, size=(S, B, n_agents)), rng.integers(0, ncol, size=(S, B, n_agents))], axis=-1)
    if scaling:
        mean = np.array([np.mean(np.arange(nrow)), np.mean(np.arange(ncol))])
        std = np.array([np.std(np.arange(nrow)), np.std(np.arange(ncol))])
    else:
        mean, std = np.zeros(2), np.ones(2)
    xs = ((pos - mean) / std)
    if width == 3:
        act = rng.integers(0, 5, size=(S, B, n_agents, 1)).astype(np.float64)
        xs = np.concatenate([xs, act], axis=-1)
    x = xs.reshape(S, B, n_agents * width).astype(np.float32)
    return x, LT.column_alpha(n_agents, width, nrow, ncol, scaling)


class LatticeBuffers:
    def __init__(self, bk, S, N, in_dim, cap):
        g = LT.Geometry(N, in_dim, cap)
        self.g, self.S = g, S
        z = lambda rk, pieces: bk.dev(np.full(S * LT.Geometry.nbytes(rk, pieces) // 2, 0x7fc0, np.uint16))   # NaN fill
        self.kp, self.ktp, self.wp, self.dzp = z(g.kp, 1), z(g.ktp, 1), z(g.wp, 3), z(g.dzp, 3)
        self.flag = bk.dev(np.zeros(1, np.int32))


def seed_views(buf_u16, S, rt_kt, pieces):
    """Per-seed 1-D views of a packed buffer: the kernels' seed stride is rt*kt*pieces blocks (the buffers are sized for three
    pieces; the two-piece form uses the first two thirds)."""
    n = LT.Geometry.nbytes(rt_kt, pieces) // 2
    flat = np.asarray(buf_u16).reshape(-1)
    return [flat[s * n:(s + 1) * n] for s in range(S)]


def _encode(bk, lb, d_x, x_stride, d_alpha, S, B, in_dim, with_t=True):
    g = lb.g
    bk.lib.rcmarl_lattice_encode(bk.ptr(d_x), x_stride, bk.ptr(d_alpha), S, B, in_dim, bk.ptr(lb.kp), g.kp[0], g.kp[1],
                                 bk.ptr(lb.ktp) if with_t else None, g.ktp[0], g.ktp[1], bk.ptr(lb.flag), bk.stream)


def _layer1_lattice(bk, lb, d_alpha, d_theta, d_a1t, S, N, B, in_dim, ldp, ldb, split=True):
    g = lb.g
    if split:
        bk.lib.rcmarl_w1_split(bk.ptr(d_theta), bk.ptr(d_alpha), bk.ptr(lb.wp), S, N, in_dim, HID, ldp, g.wp[0], g.wp[1], bk.stream)
    bk.lib.rcmarl_layer1_forward_lattice(bk.ptr(lb.kp), g.kp[0], g.kp[1], bk.ptr(lb.wp), g.wp[0], g.wp[1], bk.ptr(d_theta),
                                         bk.ptr(d_a1t), S, N, B, in_dim, HID, ldp, ldb, bk.stream)


def check_lattice_encode(bk, S, n_agents, B, width, nrow, ncol, scaling=True):
    rng = np.random.default_rng(B * 7 + n_agents + width)
    x, alpha = lattice_rows(rng, S, B, n_agents, width, nrow, ncol, scaling)
    in_dim = n_agents * width
    lb = LatticeBuffers(bk, S, n_agents, in_dim, B)
    d_x, d_al = bk.dev(x), bk.dev(alpha)
    _encode(bk, lb, d_x, B * in_dim, d_al, S, B, in_dim)
    kp, ktp, flag = bk.host(lb.kp).reshape(S, -1), bk.host(lb.ktp).reshape(S, -1), bk.host(lb.flag)
    assert flag[0] == 0
    K = np.rint(x.astype(np.float64) / alpha.astype(np.float64)).astype(np.float32)
    assert np.abs(K).max() <= 256 and np.abs(K).max() > 0
    g = lb.g
    b_pad = (B + 255) // 256 * 256
    mode = bk.lib.rcmarl_lattice_f16_mode()           # bit 0: forward image as f16, bit 1: backward image as f16
    for s in range(S):
        got = LT.pk_unpack(kp[s], b_pad, g.kp[1] * 32, g.kp[1], 1, f16=bool(mode & 1))[0]
        want = np.zeros_like(got)
        want[:B, :in_dim] = K[s]
        np.testing.assert_array_equal(got, want)
        got = LT.pk_unpack(ktp[s], g.ktp[0] * 128, b_pad, g.ktp[1], 1, f16=bool(mode & 2))[0]
        want = np.zeros_like(got)
        want[:in_dim, :B] = K[s].T
        np.testing.assert_array_equal(got, want)
    # a tensor that is NOT on the lattice must raise the flag
    x2 = x.copy()
    x2[S - 1, B // 2, in_dim // 2] += np.float32(0.013)
    _encode(bk, lb, bk.dev(x2), B * in_dim, d_al, S, B, in_dim)
    assert bk.host(lb.flag)[0] == 1


def check_lattice_forward(bk, S, N, B, width, nrow, ncol, scaling=True, w_scale=None, tol=2e-6):
    """w_scale: layer-1 weights multiplied by it and b1 zeroed (a probe of the f16 form's subnormal range: with 1e-6 every piece
    of 2^10 alpha W1 is a f16 subnormal; a matrix core that flushed them would return zeros)."""
    rng = np.random.default_rng(B + N * 3 + width)
    in_dim = N * width
    P, _ = geom(in_dim, 1)
    ldp, ldb = pad64(P), pad64(B)
    params = random_params(rng, S, N, in_dim, 1)
    if w_scale is not None:
        for s_ in range(S):
            for n_ in range(N):
                params[s_][n_][0] *= np.float32(w_scale)
                params[s_][n_][1] *= np.float32(0)
    theta = pack_rows(params, ldp)
    x, alpha = lattice_rows(rng, S, B, N, width, nrow, ncol, scaling)
    lb = LatticeBuffers(bk, S, N, in_dim, B)
    d_x, d_al, d_th = bk.dev(x), bk.dev(alpha), bk.dev(theta)
    d_a = bk.dev(np.full((S, N * HID, ldb), np.nan, np.float32))
    _encode(bk, lb, d_x, B * in_dim, d_al, S, B, in_dim, with_t=False)
    _layer1_lattice(bk, lb, d_al, d_th, d_a, S, N, B, in_dim, ldp, ldb)
    a1t = bk.host(d_a)
    assert bk.host(lb.flag)[0] == 0
    # the three bf16 pieces reproduce alpha*W1 exactly; the two f16 pieces reproduce 2^10 alpha*W1 to one fp32 ulp (exact for
    # most), or to 2^-25 where the residual is a f16 subnormal
    f16 = bool(bk.lib.rcmarl_lattice_f16_mode() & 1)
    wp = seed_views(bk.host(lb.wp), S, lb.g.wp, 2 if f16 else 3)
    for s in range(S):
        w1 = np.stack([params[s][n][0] for n in range(N)], axis=0)                     # [N][in][HID]
        want = (w1 * alpha[None, :, None]).astype(np.float32).transpose(0, 2, 1).reshape(N * HID, in_dim)
        if not f16:
            pieces = LT.pk_unpack(wp[s], N * HID, in_dim, lb.g.wp[1], 3).astype(np.float64)
            np.testing.assert_array_equal((pieces[0] + pieces[1] + pieces[2]).astype(np.float32), want)
        else:
            pieces = LT.pk_unpack(wp[s], N * HID, in_dim, lb.g.wp[1], 2, f16=True).astype(np.float64)
            want = want.astype(np.float64) * LT.F16_W_SCALE
            err = np.abs(pieces[0] + pieces[1] - want)
            assert np.all(err <= np.maximum(np.spacing(np.abs(want).astype(np.float32)).astype(np.float64), 2.0 ** -25)), float(err.max())
            assert w_scale is not None or np.mean(err == 0) > 0.6, float(np.mean(err == 0))
    for s in range(S):
        x64 = x[s].astype(np.float64)
        for n in range(N):
            z = x64 @ params[s][n][0].astype(np.float64) + params[s][n][1].astype(np.float64)
            want = np.where(z > 0, z, 0.1 * z)
            rel_close(a1t[s, n * HID:(n + 1) * HID, :B].T, want, tol, "a1 (lattice)")
    assert np.isnan(a1t[:, :, B:]).all()                                              # nothing written beyond B


def check_lattice_f16_saturation(bk, S=1, N=5, B=70, width=2, nrow=5, ncol=5, lr=0.01, gamma=0.9):
    """The two-piece f16 form beyond its range (RCMARL_LAT_F16=3): one agent's layer-1 weights are 1e8-scale and its TD targets
    1e12-scale (a fit that has blown up but is finite in fp32).  Its pieces saturate (MODE.FP16_OVFL: +-65504 each), so its
    activations equal the float64 model on the CLIPPED weights and its SGD step leaves finite weights; every other agent's
    forward and fit are what they are without the blown-up neighbour."""
    assert bk.lib.rcmarl_lattice_f16_mode() == 3
    rng = np.random.default_rng(77)
    in_dim = N * width
    P, _ = geom(in_dim, 1)
    ldp, ldb = pad64(P), pad64(B)
    params = random_params(rng, S, N, in_dim, 1)
    bad = 2
    for s_ in range(S):
        params[s_][bad][0] *= np.float32(1e9)
    theta = pack_rows(params, ldp)
    x, alpha = lattice_rows(rng, S, B, N, width, nrow, ncol, True)
    lb = LatticeBuffers(bk, S, N, in_dim, B)
    g = lb.g
    d_x, d_al, d_th = bk.dev(x), bk.dev(alpha), bk.dev(theta)
    d_a = bk.dev(np.full((S, N * HID, ldb), np.nan, np.float32))
    _encode(bk, lb, d_x, B * in_dim, d_al, S, B, in_dim)
    _layer1_lattice(bk, lb, d_al, d_th, d_a, S, N, B, in_dim, ldp, ldb)
    a1t = bk.host(d_a).copy()
    assert np.isfinite(a1t[:, :, :B]).all()
    K = np.rint(x.astype(np.float64) / alpha.astype(np.float64))
    for s_ in range(S):
        for n in range(N):
            w = params[s_][n][0]
            if n == bad:
                v = (w * alpha[:, None]).astype(np.float32) * np.float32(LT.F16_W_SCALE)
                with np.errstate(over="ignore"):
                    h = np.clip(v, -65504, 65504).astype(np.float16).astype(np.float32)
                    l = np.clip(v - h, -65504, 65504).astype(np.float16).astype(np.float32)
                assert np.abs(h).max() == 65504 and np.abs(l).max() == 65504          # the case does saturate
                z = K[s_] @ ((h.astype(np.float64) + l.astype(np.float64)) / LT.F16_W_SCALE) + params[s_][n][1].astype(np.float64)
            else:
                z = x[s_].astype(np.float64) @ w.astype(np.float64) + params[s_][n][1].astype(np.float64)
            rel_close(a1t[s_, n * HID:(n + 1) * HID, :B].T, np.where(z > 0, z, 0.1 * z), 2e-6, "a1 (saturated f16 pieces)")
    # one SGD step with 1e12-scale targets for the same agent: dz1 saturates, the weights stay finite; the others fit as usual
    y = rng.normal(size=(S, N, ldb)).astype(np.float32)
    y[:, bad] *= np.float32(1e12)
    nchunk = (B + 255) // 256
    L = bk.lib
    d_y, d_mask = bk.dev(y), bk.dev(np.ones(N, np.int32))
    d_part = bk.dev(np.zeros((S, N, nchunk, L.rcmarl_fit_partial_size(HID)), np.float32))
    # the f16 matrix-core mid kernel flags the agent (its activations / dz2 are beyond the f16 range) and the fix-up launch redoes it
    # with the fp32 kernel: records and packed dz1 rows of THAT agent equal a run of the fp32 kernel alone bit for bit
    import os
    prev = os.environ.get("RCMARL_MIDFIT")
    os.environ["RCMARL_MIDFIT"] = "5"
    d_part5 = bk.dev(np.zeros((S, N, nchunk, L.rcmarl_fit_partial_size(HID)), np.float32))
    lb5 = LatticeBuffers(bk, S, N, in_dim, B)
    L.rcmarl_mid_fit_lattice(bk.ptr(d_a), bk.ptr(d_th), bk.ptr(d_y), bk.ptr(d_part5), bk.ptr(lb5.dzp), g.dzp[0], g.dzp[1], S, N, B,
                             in_dim, HID, ldp, ldb, bk.ptr(_mid_flags(bk, S, N)), bk.stream)
    if prev is None:
        del os.environ["RCMARL_MIDFIT"]
    else:
        os.environ["RCMARL_MIDFIT"] = prev
    L.rcmarl_mid_fit_lattice(bk.ptr(d_a), bk.ptr(d_th), bk.ptr(d_y), bk.ptr(d_part), bk.ptr(lb.dzp), g.dzp[0], g.dzp[1], S, N, B,
                             in_dim, HID, ldp, ldb, bk.ptr(_mid_flags(bk, S, N)), bk.stream)
    part, part5 = bk.host(d_part), bk.host(d_part5)
    np.testing.assert_array_equal(part[:, bad], part5[:, bad])
    dz, dz5 = seed_views(bk.host(lb.dzp), S, g.dzp, 2), seed_views(bk.host(lb5.dzp), S, g.dzp, 2)
    b_pad = (B + 255) // 256 * 256
    for s_ in range(S):
        for pc in range(2):
            idx = LT.pk_element_index(N * HID, b_pad, g.dzp[1], 2, pc)[bad * HID:(bad + 1) * HID]
            np.testing.assert_array_equal(dz[s_][idx], dz5[s_][idx])
    L.rcmarl_small_sgd(bk.ptr(d_part), bk.ptr(d_th), bk.ptr(d_mask), None, S, N, B, in_dim, HID, ldp, lr, bk.stream)
    L.rcmarl_layer1_backward_sgd_lattice(bk.ptr(lb.ktp), g.ktp[0], g.ktp[1], bk.ptr(lb.dzp), g.dzp[0], g.dzp[1], bk.ptr(d_al),
                                         bk.ptr(d_th), bk.ptr(d_mask), S, N, B, in_dim, HID, ldp, lr, bk.ptr(lb.wp), g.wp[0],
                                         g.wp[1], bk.stream)
    th = bk.host(d_th)
    assert np.isfinite(th[:, :, :in_dim * HID]).all()                                     # layer 1 of every agent, the blown-up one included
    for s_ in range(S):
        for n in range(N):
            if n == bad:
                continue
            pw = M.copy_params(params[s_][n])
            M.fit_mse(pw, x[s_], y[s_, n, :B, None], lr, epochs=1)
            got = unpack_row(th[s_, n], in_dim, 1)
            for k in range(6):
                rel_close(got[k], pw[k], 1e-5, "fit param %d beside a saturated agent" % k)


def check_pack_dz_rowsum(bk, S, N, B, hid):
    """rcmarl_lattice_pack_dz_rowsum = rcmarl_lattice_pack_dz (the packed dz image, bit for bit) + the row sums of dz in the same
    pass (gb1 of a wide net: rcmarl_wide_bias_grad), against float64 sums."""
    rng = np.random.default_rng(S * 13 + N + B + hid)
    ldb = pad64(B)
    dz = np.zeros((S, N * hid, ldb), np.float32)
    dz[:, :, :B] = (0.01 * rng.normal(size=(S, N * hid, B))).astype(np.float32)
    dz[:, :, B:] = np.float32(7.0)                               # padding columns must be ignored
    # (the dz image only depends on N * hid rows and B: a geometry for the 20-unit nets is too small for wide ones)
    g = LT.Geometry(N * hid // HID + 1, 64, B)
    z = lambda: bk.dev(np.full(S * LT.Geometry.nbytes(g.dzp, 3) // 2, 0x7fc0, np.uint16))
    p1, p2 = z(), z()
    d_dz = bk.dev(dz)
    gsz = 3 * hid + 1
    sums = bk.dev(np.full((S, N, gsz), np.float32(-5.0)))
    L = bk.lib
    L.rcmarl_lattice_pack_dz(bk.ptr(d_dz), bk.ptr(p1), S, N, B, hid, ldb, g.dzp[0], g.dzp[1], bk.stream)
    L.rcmarl_lattice_pack_dz_rowsum(bk.ptr(d_dz), bk.ptr(p2), bk.ptr(sums), gsz, 2 * hid + 1, S, N, B, hid, ldb, g.dzp[0], g.dzp[1],
                                    bk.stream)
    npc = 2 if L.rcmarl_lattice_f16_mode() & 2 else 3
    a, b = seed_views(bk.host(p1), S, g.dzp, npc), seed_views(bk.host(p2), S, g.dzp, npc)
    for s_ in range(S):
        for pc in range(npc):
            idx = LT.pk_element_index(N * hid, ((B + 31) // 32) * 32, g.dzp[1], npc, pc)       # every k-tile in use, padding included
            np.testing.assert_array_equal(a[s_][idx], b[s_][idx])
    got = bk.host(sums)
    want = dz[:, :, :B].astype(np.float64).sum(axis=2).reshape(S, N, hid)
    scale = float(np.abs(dz[:, :, :B]).astype(np.float64).sum(axis=2).max())
    assert np.abs(got[:, :, 2 * hid + 1:] - want).max() <= 2e-6 * scale
    np.testing.assert_array_equal(got[:, :, :2 * hid + 1], np.float32(-5.0))      # the rest of the record untouched


def check_mid_step_f16_vs_fp32_kernel(bk, S, N, B, in_dim, lr=0.01):
    """rcmarl_mid_fit_lattice + rcmarl_small_sgd on the f16 matrix-core kernel (k_mid_fit_v8, the default) against the same call on
    the fp32 kernel (RCMARL_MIDFIT=5, k_mid_fit_v5) on identical random inputs: the small arrays after the step agree to 2e-6 of
    their largest element and the loss to 1e-6.  Cheap at ANY number of (seed, agent) columns -- the case with >= 2048 of them runs
    the one-workgroup-per-agent form (mid_kernels.hip: midfit_cpw), which the oracle-compared fits (a few hundred networks: their
    worst case over thousands of networks grows with the knife edges of DESIGN.md section 4, Round 4) do not reach."""
    rng = np.random.default_rng(S * 7 + N + B + in_dim)
    P, _ = geom(in_dim, 1)
    ldp, ldb = pad64(P), pad64(B)
    theta = (0.3 * rng.normal(size=(S, N, ldp))).astype(np.float32)
    a1 = rng.normal(size=(S, N * HID, ldb)).astype(np.float32)
    a1 = np.where(a1 > 0, a1, np.float32(0.1) * a1).astype(np.float32)          # post-LeakyReLU activations
    y = rng.normal(size=(S, N, ldb)).astype(np.float32)
    mask = np.ones(N, np.int32)
    nchunk = (B + 255) // 256
    psz = bk.lib.rcmarl_fit_partial_size(HID)
    lb = LatticeBuffers(bk, S, N, in_dim, B)
    g = lb.g
    out = {}
    for form in (None, "5"):
        if form is None:
            os.environ.pop("RCMARL_MIDFIT", None)
        else:
            os.environ["RCMARL_MIDFIT"] = form
        try:
            d_a, d_th, d_y, d_mask = bk.dev(a1), bk.dev(theta.copy()), bk.dev(y), bk.dev(mask)
            d_part = bk.dev(np.zeros((S, N, nchunk, psz), np.float32))
            d_loss = bk.dev(np.zeros((S, N), np.float32))
            bk.lib.rcmarl_mid_fit_lattice(bk.ptr(d_a), bk.ptr(d_th), bk.ptr(d_y), bk.ptr(d_part), bk.ptr(lb.dzp), g.dzp[0], g.dzp[1],
                                          S, N, B, in_dim, HID, ldp, ldb, bk.ptr(_mid_flags(bk, S, N)), bk.stream)
            bk.lib.rcmarl_small_sgd(bk.ptr(d_part), bk.ptr(d_th), bk.ptr(d_mask), bk.ptr(d_loss), S, N, B, in_dim, HID, ldp, lr,
                                    bk.stream)
            out[form] = (bk.host(d_th).copy(), bk.host(d_loss).copy())
        finally:
            os.environ.pop("RCMARL_MIDFIT", None)
    th8, l8 = out[None]
    th5, l5 = out["5"]
    small = slice(in_dim * HID, P)                               # b1 | W2 | b2 | W3 | b3 (layer 1's weights belong to the backward GEMM)
    assert not np.array_equal(th8[..., small], theta[..., small])
    # A LeakyReLU pre-activation within an ulp of zero takes the other branch in the other arithmetic (slope 1 vs 0.1 for that one
    # (row, unit)): among S*N*B*20 of them a few hundred do, each worth up to lr * |dv W3 a1| in one gradient element -- hence a bar
    # for (nearly) all elements and a looser one for the stragglers, like the engine tests at this size
    scale = max(1.0, float(np.abs(th5[..., small]).max()))
    diff = np.abs(th8[..., small] - th5[..., small]) / scale
    frac = float((diff > 2e-6).mean())
    print("[parity] mid step f16 vs fp32 kernel (S=%d N=%d B=%d): max %.2e, fraction beyond 2e-6: %.2e" % (S, N, B, diff.max(), frac))
    assert frac <= 2e-5 and diff.max() <= 5e-5, (float(diff.max()), frac)   # measured: 3.7e-6 of the elements, worst 7.7e-6 (profiles/r04zz_*)
    np.testing.assert_allclose(l8, l5, rtol=1e-6, atol=0)


def check_lattice_sgd_fit(bk, S, N, B, width, nrow, ncol, steps=2, lr=0.01, gamma=0.9, masked_agent=None):
    """check_sgd_fit on the lattice path: encode -> [w1_split -> forward_lattice -> mid_fit_lattice ->
    small_sgd -> backward_sgd_lattice] x steps, against the same oracle fit."""
    rng = np.random.default_rng(S * 1000 + N * 100 + B + width)
    in_dim = N * width
    P, _ = geom(in_dim, 1)
    ldp, ldb = pad64(P), pad64(B)
    params = random_params(rng, S, N, in_dim, 1)
    theta = pack_rows(params, ldp)
    x, alpha = lattice_rows(rng, S, B, N, width, nrow, ncol)
    nx, _ = lattice_rows(rng, S, B, N, width, nrow, ncol)
    r_applied = rng.normal(size=(S, N, ldb)).astype(np.float32)
    mask = np.ones(N, np.int32)
    if masked_agent is not None:
        mask[masked_agent] = 0
    nchunk = (B + 255) // 256
    psz = bk.lib.rcmarl_fit_partial_size(HID)
    lb, lbn = LatticeBuffers(bk, S, N, in_dim, B), LatticeBuffers(bk, S, N, in_dim, B)
    g = lb.g
    d_x, d_nx, d_al, d_th, d_r, d_mask = bk.dev(x), bk.dev(nx), bk.dev(alpha), bk.dev(theta), bk.dev(r_applied), bk.dev(mask)
    d_msg = bk.dev(theta.copy())
    d_a = bk.dev(np.zeros((S, N * HID, ldb), np.float32))
    d_y = bk.dev(np.zeros((S, N, ldb), np.float32))
    d_part = bk.dev(np.zeros((S, N, nchunk, psz), np.float32))
    d_loss = bk.dev(np.zeros((S, N), np.float32))
    L = bk.lib
    _encode(bk, lb, d_x, B * in_dim, d_al, S, B, in_dim)
    _encode(bk, lbn, d_nx, B * in_dim, d_al, S, B, in_dim, with_t=False)
    _layer1_lattice(bk, lbn, d_al, d_th, d_a, S, N, B, in_dim, ldp, ldb)
    L.rcmarl_mid_value(bk.ptr(d_a), bk.ptr(d_th), bk.ptr(d_r), gamma, bk.ptr(d_y), S, N, B, in_dim, HID, ldp, ldb,
                       bk.stream)
    for st in range(steps):
        # from step 1 on the forward operand comes from the previous backward's epilogue (odd steps also re-split,
        # which must give the same bytes)
        _layer1_lattice(bk, lb, d_al, d_msg, d_a, S, N, B, in_dim, ldp, ldb, split=(st == 0))
        a_before = bk.host(d_a).copy() if st == 0 else None
        L.rcmarl_mid_fit_lattice(bk.ptr(d_a), bk.ptr(d_msg), bk.ptr(d_y), bk.ptr(d_part), bk.ptr(lb.dzp), g.dzp[0], g.dzp[1],
                                 S, N, B, in_dim, HID, ldp, ldb, bk.ptr(_mid_flags(bk, S, N)), bk.stream)
        if st == 0:
            np.testing.assert_array_equal(bk.host(d_a), a_before)                    # activations left intact
        L.rcmarl_small_sgd(bk.ptr(d_part), bk.ptr(d_msg), bk.ptr(d_mask), bk.ptr(d_loss) if st == 0 else None, S, N, B,
                           in_dim, HID, ldp, lr, bk.stream)
        L.rcmarl_layer1_backward_sgd_lattice(bk.ptr(lb.ktp), g.ktp[0], g.ktp[1], bk.ptr(lb.dzp), g.dzp[0], g.dzp[1],
                                             bk.ptr(d_al), bk.ptr(d_msg), bk.ptr(d_mask), S, N, B, in_dim, HID, ldp, lr,
                                             bk.ptr(lb.wp), g.wp[0], g.wp[1], bk.stream)
        if st == steps - 1:                                   # fused pieces == what a fresh split of the result gives
            npc = 2 if bk.lib.rcmarl_lattice_f16_mode() & 1 else 3
            fused = bk.host(lb.wp).copy()
            L.rcmarl_w1_split(bk.ptr(d_msg), bk.ptr(d_al), bk.ptr(lb.wp), S, N, in_dim, HID, ldp, g.wp[0], g.wp[1], bk.stream)
            fresh = seed_views(bk.host(lb.wp), S, g.wp, npc)
            fused = seed_views(fused, S, g.wp, npc)
            for s_ in range(S):
                for pc in range(npc):
                    idx = LT.pk_element_index(N * HID, in_dim, g.wp[1], npc, pc)
                    np.testing.assert_array_equal(fused[s_][idx], fresh[s_][idx])
    assert bk.host(lb.flag)[0] == 0 and bk.host(lbn.flag)[0] == 0
    msg, y, loss = bk.host(d_msg), bk.host(d_y), bk.host(d_loss)
    for s in range(S):
        for n in range(N):
            p0 = params[s][n]
            target = r_applied[s, n, :B, None] + np.float32(gamma) * M.forward(p0, nx[s])
            rel_close(y[s, n, :B], target[:, 0], 3e-6, "td target (lattice)")
            if not mask[n]:
                np.testing.assert_array_equal(msg[s, n], theta[s, n])
                continue
            pw = M.copy_params(p0)
            hist = M.fit_mse(pw, x[s], target, lr, epochs=steps)
            got = unpack_row(msg[s, n], in_dim, 1)
            for k in range(6):
                rel_close(got[k], pw[k], 1e-5, "fit param %d (lattice)" % k)
            assert abs(loss[s, n] - hist[0]) <= 1e-5 * max(1.0, abs(hist[0])), (loss[s, n], hist[0])
    np.testing.assert_array_equal(bk.host(d_th), theta)
    return msg, fresh                                  # (variant tests compare these bit for bit)


def check_lattice_form_mismatch(bk, lattice_form):
    from rcmarl_amd.capi import RcmarlError
    import pytest
    S, N, B, width = 1, 5, 70, 2
    rng = np.random.default_rng(3)
    in_dim = N * width
    P, _ = geom(in_dim, 1)
    ldp, ldb = pad64(P), pad64(B)
    theta = pack_rows(random_params(rng, S, N, in_dim, 1), ldp)
    x, alpha = lattice_rows(rng, S, B, N, width, 5, 5)
    lb = LatticeBuffers(bk, S, N, in_dim, B)
    d_x, d_al, d_th = bk.dev(x), bk.dev(alpha), bk.dev(theta)
    d_a = bk.dev(np.zeros((S, N * HID, ldb), np.float32))
    d_mask = bk.dev(np.ones(N, np.int32))
    lattice_form(bk, 3)
    _encode(bk, lb, d_x, B * in_dim, d_al, S, B, in_dim)
    _layer1_lattice(bk, lb, d_al, d_th, d_a, S, N, B, in_dim, ldp, ldb)                    # produced and consumed in form 3: fine
    lattice_form(bk, 0)
    g = lb.g
    with pytest.raises(RcmarlError, match="RCMARL_ERR_ARG"):                                # f16 pieces, bf16 consumer
        bk.lib.rcmarl_layer1_forward_lattice(bk.ptr(lb.kp), g.kp[0], g.kp[1], bk.ptr(lb.wp), g.wp[0], g.wp[1], bk.ptr(d_th),
                                             bk.ptr(d_a), S, N, B, in_dim, HID, ldp, ldb, bk.stream)
    with pytest.raises(RcmarlError, match="RCMARL_ERR_ARG"):
        bk.lib.rcmarl_layer1_backward_sgd_lattice(bk.ptr(lb.ktp), g.ktp[0], g.ktp[1], bk.ptr(lb.dzp), g.dzp[0], g.dzp[1], bk.ptr(d_al),
                                                  bk.ptr(d_th), bk.ptr(d_mask), S, N, B, in_dim, HID, ldp, 0.01, None, 0, 0, bk.stream)
    _encode(bk, lb, d_x, B * in_dim, d_al, S, B, in_dim)                                    # re-produced in form 0: accepted again
    _layer1_lattice(bk, lb, d_al, d_th, d_a, S, N, B, in_dim, ldp, ldb)


def check_lattice_vs_f32(bk, S, N, B, width, nrow, ncol, steps=2, lr=0.01):
    rng = np.random.default_rng(N + B + width)
    in_dim = N * width
    P, _ = geom(in_dim, 1)
    ldp, ldb = pad64(P), pad64(B)
    theta = np.zeros((S, N, ldp), np.float32)
    lim = np.sqrt(6.0 / (in_dim + HID))
    theta[:, :, :in_dim * HID] = rng.uniform(-lim, lim, size=(S, N, in_dim * HID)).astype(np.float32)
    theta[:, :, in_dim * HID:P] = rng.uniform(-0.4, 0.4, size=(S, N, P - in_dim * HID)).astype(np.float32)
    x, alpha = lattice_rows(rng, S, B, N, width, nrow, ncol)
    y = rng.normal(size=(S, N, ldb)).astype(np.float32)
    mask = np.ones(N, np.int32)
    nchunk = (B + 255) // 256
    psz = bk.lib.rcmarl_fit_partial_size(HID)
    L = bk.lib
    res = {}
    for path in ("f32", "lattice"):
        d_x, d_al, d_th, d_y, d_mask = bk.dev(x), bk.dev(alpha), bk.dev(theta.copy()), bk.dev(y), bk.dev(mask)
        d_a = bk.dev(np.zeros((S, N * HID, ldb), np.float32))
        d_part = bk.dev(np.zeros((S, N, nchunk, psz), np.float32))
        if path == "lattice":
            lb = LatticeBuffers(bk, S, N, in_dim, B)
            g = lb.g
            _encode(bk, lb, d_x, B * in_dim, d_al, S, B, in_dim)
        a_first = None
        for st in range(steps):
            if path == "f32":
                _layer1(bk, d_x, B * in_dim, d_th, d_a, S, N, B, in_dim, ldp, ldb)
            else:
                _layer1_lattice(bk, lb, d_al, d_th, d_a, S, N, B, in_dim, ldp, ldb, split=(st == 0))
            if st == 0:
                a_first = bk.host(d_a).copy()
            if path == "f32":
                L.rcmarl_mid_fit(bk.ptr(d_a), bk.ptr(d_th), bk.ptr(d_y), bk.ptr(d_part), S, N, B, in_dim, HID, ldp, ldb, bk.stream)
            else:
                L.rcmarl_mid_fit_lattice(bk.ptr(d_a), bk.ptr(d_th), bk.ptr(d_y), bk.ptr(d_part), bk.ptr(lb.dzp), g.dzp[0],
                                         g.dzp[1], S, N, B, in_dim, HID, ldp, ldb, bk.ptr(_mid_flags(bk, S, N)), bk.stream)
            L.rcmarl_small_sgd(bk.ptr(d_part), bk.ptr(d_th), bk.ptr(d_mask), None, S, N, B, in_dim, HID, ldp, lr, bk.stream)
            if path == "f32":
                L.rcmarl_layer1_backward_sgd(bk.ptr(d_x), B * in_dim, bk.ptr(d_a), bk.ptr(d_th), bk.ptr(d_mask), S, N, B,
                                             in_dim, HID, ldp, ldb, lr, bk.stream)
            else:
                L.rcmarl_layer1_backward_sgd_lattice(bk.ptr(lb.ktp), g.ktp[0], g.ktp[1], bk.ptr(lb.dzp), g.dzp[0], g.dzp[1],
                                                     bk.ptr(d_al), bk.ptr(d_th), bk.ptr(d_mask), S, N, B, in_dim, HID, ldp, lr,
                                                     bk.ptr(lb.wp), g.wp[0], g.wp[1], bk.stream)
        res[path] = (a_first, bk.host(d_th).copy())
        if path == "lattice":
            assert bk.host(lb.flag)[0] == 0
    a_f, th_f = res["f32"]
    a_l, th_l = res["lattice"]
    rel_close(a_l[:, :, :B], a_f[:, :, :B], 2e-6, "a1 lattice vs f32")
    # the update itself is small (lr * gradient): compare the CHANGE of the weights, relative to its own size
    d_f, d_l = th_f - theta, th_l - theta
    assert np.abs(d_f).max() > 0
    err = float(np.abs(d_l - d_f).max())
    assert err <= 2e-4 * float(np.abs(d_f).max()), (err, float(np.abs(d_f).max()))


# ------------------------------------------------------------------------------------------
def check_consensus_on_shipped_weights(bk, golden):
    """K1 and K2 on the `hid/*` fixture -- the messages are the reference's SHIPPED
    weights of its malicious run (simulation_results/raw_data/malicious/H=1/seed=300/pretrained_weights2.npy; agent 4
    is the Malicious one) and `hid/H*/{critic,tr}_after` were produced by executing the reference's own
    resilient_consensus_{critic,TR}_hidden (agents/resilient_CAC_agents.py:142-166) on them
    (tests/golden/make_golden.py).  K1: clip window bit-exact vs the oracle, aggregated rows vs the REFERENCE's output
    to 1e-6 (summation order), general and circulant kernel.  K2: estimate consensus on the same messages."""
    in_nodes = np.asarray(golden["hid/in_nodes"], np.int32)
    N, d = in_nodes.shape
    coop = np.array([1, 1, 1, 1, 0], np.int32)
    for net, key, in_dim in (("critic", "hid/critic_msgs", 2 * N), ("tr", "hid/tr_msgs", 3 * N)):
        msgs = np.asarray(golden[key], np.float32)
        P, P_hid = geom(in_dim, 1)
        assert msgs.shape == (N, P)
        ldp = pad64(P)
        S = 3                                        # the same instance in every seed slot (the kernels batch over seeds)
        msg = np.zeros((S, N, ldp), np.float32)
        msg[:, :, :P] = msgs
        for H in (0, 1):
            after = np.asarray(golden["hid/H%d/%s_after" % (H, net)], np.float32)        # [4][P], reference output
            kernels = ["general"]
            if bk.lib.rcmarl_consensus_params_circulant_supported(N, d, H) == 1 and \
                    all(list(in_nodes[i]) == [(i + k) % N for k in range(d)] for i in range(N)):
                kernels.append("circulant")
            for kern in kernels:
                d_msg, d_theta = bk.dev(msg), bk.dev(msg.copy())       # live net == own message (make_golden.py:79-80)
                d_nbr, d_coop = bk.dev(in_nodes), bk.dev(coop)
                d_lo, d_hi = bk.dev(np.zeros_like(msg)), bk.dev(np.zeros_like(msg))
                if kern == "general":
                    bk.lib.rcmarl_consensus_params(bk.ptr(d_msg), bk.ptr(d_theta), bk.ptr(d_nbr), bk.ptr(d_coop), S, N, ldp,
                                                   P_hid, d, H, bk.ptr(d_lo), bk.ptr(d_hi), bk.stream)
                else:
                    bk.lib.rcmarl_consensus_params_circulant(bk.ptr(d_msg), bk.ptr(d_theta), bk.ptr(d_coop), S, N, ldp, P_hid,
                                                             d, H, bk.ptr(d_lo), bk.ptr(d_hi), bk.stream)
                theta, lo, hi = bk.host(d_theta), bk.host(d_lo), bk.host(d_hi)
                for s in range(S):
                    for i in range(4):
                        wl, wh, _ = O.aggregation_bounds(msgs[in_nodes[i], :P_hid], H)
                        np.testing.assert_array_equal(lo[s, i, :P_hid], wl, err_msg="%s %s H=%d lower" % (net, kern, H))
                        np.testing.assert_array_equal(hi[s, i, :P_hid], wh, err_msg="%s %s H=%d upper" % (net, kern, H))
                        ref = after[i]
                        err = np.abs(theta[s, i, :P_hid] - ref[:P_hid])
                        assert float((err / np.maximum(1.0, np.abs(ref[:P_hid]))).max()) <= 1e-6, (net, kern, H, i, float(err.max()))
                        # aggregated W3,b3 are discarded (agents/resilient_CAC_agents.py:150-153): output layer untouched
                        np.testing.assert_array_equal(theta[s, i, P_hid:P], msgs[i, P_hid:])
                        np.testing.assert_array_equal(ref[P_hid:], msgs[i, P_hid:])
                    np.testing.assert_array_equal(theta[s, 4], msg[s, 4])               # the Malicious agent's row
    # K2 on the critic messages: every cooperative agent evaluates its neighbours' heads on its own (post-K1) features
    H, in_dim = 1, 2 * N
    msgs = np.asarray(golden["hid/critic_msgs"], np.float32)
    after = np.asarray(golden["hid/H1/critic_after"], np.float32)
    P, P_hid = geom(in_dim, 1)
    ldp, B = pad64(P), 300
    ldb = pad64(B)
    rng = np.random.default_rng(5)
    x = ((rng.integers(0, 5, size=(1, B, in_dim)) - 2.0) / np.sqrt(2.0)).astype(np.float32)    # z-scored 5x5 grid states
    theta = np.zeros((1, N, ldp), np.float32)
    theta[0, :4, :P] = after
    theta[0, 4, :P] = msgs[4]
    msg = np.zeros((1, N, ldp), np.float32)
    msg[0, :, :P] = msgs
    nchunk = (B + 255) // 256
    d_x, d_th, d_msg, d_nbr, d_coop = bk.dev(x), bk.dev(theta), bk.dev(msg), bk.dev(in_nodes), bk.dev(coop)
    d_a = bk.dev(np.zeros((1, N * HID, ldb), np.float32))
    d_part = bk.dev(np.zeros((1, N, nchunk, HID + 1), np.float32))
    d_agg = bk.dev(np.zeros((1, N, ldb), np.float32))
    _layer1(bk, d_x, B * in_dim, d_th, d_a, 1, N, B, in_dim, ldp, ldb)
    bk.lib.rcmarl_consensus_head(bk.ptr(d_a), bk.ptr(d_th), bk.ptr(d_msg), bk.ptr(d_nbr), bk.ptr(d_coop), bk.ptr(d_part),
                                 bk.ptr(d_agg), 1, N, B, in_dim, HID, ldp, ldb, d, H, bk.stream)
    agg = bk.host(d_agg)
    for i in range(4):
        live = unpack_row(theta[0, i], in_dim, 1)
        ag = O.CoopAgent(M.init_mlp(rng, in_dim, HID, 5), live, live, 0.002, 0.01, 0.9, H)
        want = ag.consensus_estimates_critic(x[0], [unpack_row(msgs[j], in_dim, 1) for j in in_nodes[i]])
        rel_close(agg[0, i, :B], want[:, 0], 5e-6, "estimate aggregate on shipped weights, agent %d" % i)


# ------------------------------------------------------------------------------------------
SENT = -7           # NaN-free sentinel of the "nothing else written" checks: untouched memory compares EQUAL to it
KNIFE_EDGE = 1.2e-5      # a policy draw this close to a cdf boundary may fall either way: 4 cdf terms x the 3e-6 bar on a probability
KNIFE_EDGE_CAP = 1e-3    # share of a case's draws that may be knife edges (expected: 8 boundaries' sides x 1.2e-5 ~ 1e-4)


def check_rollout_episodes(bk, S, N, nrow, ncol, E, ep_len, episode0, row0, pos_in=False):
    """The episode-parallel rollout (rcmarl_env_reset_episodes, rcmarl_value_rows_episodes, rcmarl_rollout_step_episodes: one lane =
    one episode, episode-minor state) against one oracle environment per (seed, episode): start positions (Philox, or pos_in),
    scaled states, start-state values, every replay row, positions and float64 returns EXACTLY, with every buffer pre-filled with a
    sentinel so that the padding lanes E..EP, the est entries past E and the replay rows outside [row0, row0 + E*ep_len) are shown
    untouched after every launch.  The oracle is stepped with the KERNEL's actions; an action may differ from the oracle's draw only
    where u1 is within KNIFE_EDGE of a cdf boundary (printed), and at most KNIFE_EDGE_CAP of the draws may be that close.  The last
    episode of seed 0 is replayed with the sequential kernels (rcmarl_env_reset + rcmarl_rollout_step) and must leave the same rows,
    positions and returns (skipped, with a note, if that episode holds a knife-edge draw).  Bad arguments are refused before anything
    is written.  -> dict(draws, knife_edges, knife_flips, sequential_compared)"""
    import pytest
    from oracle import philox_np as PX
    from rcmarl_amd import capi
    rng = np.random.default_rng(S * 7 + N + 13 * E)
    A = 5
    in_a = 2 * N
    Pa, _ = geom(in_a, A)
    Pc, _ = geom(in_a, 1)
    ldpa, ldpc = pad64(Pa), pad64(Pc)
    actors = random_params(rng, S, N, in_a, A, bias_scale=0.3)
    critics = random_params(rng, S, N, in_a, 1)
    th_a, th_c = pack_rows(actors, ldpa), pack_rows(critics, ldpc)
    goal = rng.integers(0, min(5, nrow), size=(S, N, 2)).astype(np.int32)
    start = np.stack([rng.integers(0, nrow, size=(S, N)), rng.integers(0, ncol, size=(S, N))], axis=2).astype(np.int32) if pos_in else None
    seeds = np.array([1000 + 17 * s for s in range(S)], dtype=np.uint64)
    mean = np.array([np.mean(np.arange(nrow)), np.mean(np.arange(ncol))])
    std = np.array([np.std(np.arange(nrow)), np.std(np.arange(ncol))])
    scale = np.concatenate([mean, std])
    EP = pad64(E)
    cap = row0 + E * ep_len + 5
    gamma, mu = 0.9, 0.1
    widths = (("s", 2), ("ns", 2), ("sa", 3), ("a", 1), ("r", 1))
    L = bk.lib
    d_tha, d_thc, d_goal, d_seeds, d_scale = bk.dev(th_a), bk.dev(th_c), bk.dev(goal), bk.dev(seeds), bk.dev(scale)
    d_start = bk.dev(start) if pos_in else None
    # what every buffer is expected to hold, kept on the host beside it: compared WHOLE after every launch
    want_rp = {k: np.full((S, cap, w * N), SENT, np.float32) for k, w in widths}
    want_est = np.full((E + 2, S, N), SENT, np.float32)
    want_pos = [np.full((S, N, 2, EP), SENT, np.int32) for _ in range(2)]
    want_xs = [np.full((S, 2 * N, EP), SENT, np.float32) for _ in range(2)]
    want_ret = np.full((S, N, EP), SENT, np.float64)
    rp = {k: bk.dev(v) for k, v in want_rp.items()}
    d_est, d_ret = bk.dev(want_est), bk.dev(want_ret)
    d_pos, d_xs = [bk.dev(v) for v in want_pos], [bk.dev(v) for v in want_xs]

    def reset(E_, EP_):
        return L.rcmarl_env_reset_episodes(bk.ptr(d_start) if pos_in else None, bk.ptr(d_seeds), nrow, ncol, bk.ptr(d_scale), episode0,
                                           bk.ptr(d_pos[0]), bk.ptr(d_xs[0]), bk.ptr(d_ret), S, N, E_, EP_, bk.stream)

    def values(E_, EP_):
        return L.rcmarl_value_rows_episodes(bk.ptr(d_xs[0]), bk.ptr(d_thc), bk.ptr(d_est), S, N, E_, EP_, HID, ldpc, bk.stream)

    def step(cur, j, gpow, E_=E, EP_=EP, cap_=cap):
        return L.rcmarl_rollout_step_episodes(bk.ptr(d_xs[cur]), bk.ptr(d_pos[cur]), bk.ptr(d_goal), bk.ptr(d_tha), bk.ptr(d_seeds), nrow,
                                              ncol, bk.ptr(d_scale), bk.ptr(rp["s"]), bk.ptr(rp["ns"]), bk.ptr(rp["sa"]), bk.ptr(rp["a"]),
                                              bk.ptr(rp["r"]), cap_, row0, ep_len, bk.ptr(d_pos[1 - cur]), bk.ptr(d_xs[1 - cur]),
                                              bk.ptr(d_ret), gpow, episode0, j, mu, S, N, E_, EP_, HID, A, ldpa, bk.stream)

    def assert_state(what):
        for k, _ in widths:
            np.testing.assert_array_equal(bk.host(rp[k]), want_rp[k], err_msg="%s: replay tensor %s" % (what, k))
        np.testing.assert_array_equal(bk.host(d_est), want_est, err_msg="%s: est" % what)
        np.testing.assert_array_equal(bk.host(d_ret), want_ret, err_msg="%s: retT" % what)
        for c in range(2):
            np.testing.assert_array_equal(bk.host(d_pos[c]), want_pos[c], err_msg="%s: posT[%d]" % (what, c))
            np.testing.assert_array_equal(bk.host(d_xs[c]), want_xs[c], err_msg="%s: xsT[%d]" % (what, c))

    # ---- refused argument sets: RCMARL_ERR_ARG, nothing written ---------------------------------------------------------
    bad = [lambda: reset(E, EP - 64), lambda: reset(E, EP + 8), lambda: values(E, EP - 64), lambda: values(E, EP + 8),
           lambda: step(0, 0, 1.0, EP_=EP - 64), lambda: step(0, 0, 1.0, EP_=EP + 8), lambda: step(0, ep_len, 1.0),
           lambda: step(0, 0, 1.0, cap_=row0 + E * ep_len - 1)]
    for call in bad:
        with pytest.raises(capi.RcmarlError, match="RCMARL_ERR_ARG"):
            call()
    assert_state("after the refused calls")

    # ---- reset ------------------------------------------------------------------------------------------------------
    reset(E, EP)
    envs = []
    for s in range(S):
        row = []
        for e in range(E):
            env = O.GridWorldOracle(nrow, ncol, N, goal[s], start[s] if pos_in else None, not pos_in, True, rng_mode="device", seed=int(seeds[s]))
            env.reset(episode=episode0 + e)
            if pos_in:
                np.testing.assert_array_equal(env.state, start[s])
            else:
                np.testing.assert_array_equal(env.state, PX.reset_positions(N, nrow, ncol, int(seeds[s]), episode0 + e))
            row.append(env)
        envs.append(row)

    def scaled(pos_t):
        """int positions [S][N][2][lanes] -> the state vector [S][2N][lanes]: float32 of the float64 (pos - mean) / std"""
        x = (pos_t.astype(np.float64) - mean[None, None, :, None]) / std[None, None, :, None]
        return x.astype(np.float32).reshape(pos_t.shape[0], 2 * N, pos_t.shape[3])

    def states():
        """the environments' positions, episode-minor [S][N][2][E]"""
        return np.stack([np.stack([env.state for env in row], axis=2) for row in envs]).astype(np.int32)

    want_pos[0][...] = 0                                 # the padding lanes: cell 0, its scaled value, return 0 (as documented)
    want_pos[0][:, :, :, :E] = states()
    want_xs[0] = scaled(want_pos[0])
    want_ret[...] = 0.0
    assert_state("after the reset")
    for s in range(S):                                   # (the oracle's own get_data() gives the same float32 vector)
        for e in (0, E - 1):
            np.testing.assert_array_equal(want_xs[0][s, :, e], envs[s][e].get_data()[0].astype(np.float32).ravel())

    # ---- start-state values -----------------------------------------------------------------------------------------
    values(E, EP)
    est = bk.host(d_est)
    for s in range(S):
        X = np.ascontiguousarray(want_xs[0][s, :, :E].T)                       # [E][2N]
        for i in range(N):
            want = M.forward(critics[s][i], X)[:, 0]
            err = np.abs(est[:E, s, i] - want)
            assert np.all(err <= 3e-6 * np.maximum(1.0, np.abs(want))), ("start value", s, i, float(err.max()))
    want_est[:E] = est[:E]
    assert_state("after the start-state values")

    # ---- steps ------------------------------------------------------------------------------------------------------
    ret64 = np.zeros((S, N, E))
    n_draws = n_knife = n_flip_knife = 0
    knife_in_last_episode = False
    cur = 0
    for j in range(ep_len):
        gpow = float(gamma ** j)
        step(cur, j, gpow)
        rows = row0 + np.arange(E) * ep_len + j
        act_k = bk.host(rp["a"])[:, rows, :]                                    # [S][E][N], the kernel's actions
        assert np.all((act_k == np.round(act_k)) & (act_k >= 0) & (act_k < A)), "step %d: actions outside 0..%d" % (j, A - 1)
        act_k = act_k.astype(np.int64)
        for s in range(S):
            X = np.ascontiguousarray(want_xs[cur][s, :, :E].T)                  # [E][2N]: every episode's state, one forward per agent
            op = np.stack([M.softmax(M.forward(actors[s][i], X)) for i in range(N)], axis=1)            # [E][N][A] fp32
            act_o = np.stack([PX.sample_actions(op[e], int(seeds[s]), episode0 + e, j, mu) for e in range(E)])
            knife = PX.action_margins(op, int(seeds[s]), episode0 + np.arange(E)[:, None], j) <= KNIFE_EDGE
            flip = act_k[s] != act_o
            n_draws += flip.size
            n_knife += int(knife.sum())
            n_flip_knife += int((flip & knife).sum())
            if s == 0 and knife[E - 1].any():
                knife_in_last_episode = True
            for e, i in zip(*np.nonzero(flip & knife)):
                print("[rollout episodes] knife-edge draw fell the other way: seed %d episode %d step %d agent %d: kernel %d, oracle %d"
                      % (s, episode0 + e, j, i, act_k[s, e, i], act_o[e, i]))
            assert not (flip & ~knife).any(), ("actions differ from the oracle's Philox draw away from any cdf boundary: step %d, seed %d, "
                                               "(episode, agent) %s" % (j, s, list(zip(*np.nonzero(flip & ~knife)))[:8]))
            for e in range(E):
                env = envs[s][e]
                st = env.get_data()[0].astype(np.float32)
                env.step(act_k[s, e].astype(np.float64))
                nst, rew = env.get_data()
                a32 = act_k[s, e].astype(np.float32)
                ret64[s, :, e] += rew * (gamma ** j)
                want_rp["s"][s, rows[e]] = st.ravel()
                want_rp["ns"][s, rows[e]] = nst.astype(np.float32).ravel()
                want_rp["sa"][s, rows[e]] = np.concatenate([st, a32[:, None]], axis=1).ravel()
                want_rp["a"][s, rows[e]] = a32
                want_rp["r"][s, rows[e]] = rew.astype(np.float32)
        nxt = 1 - cur
        want_pos[nxt][:, :, :, :E] = states()                                   # lanes E..EP keep what they held (the sentinel, or an
        want_xs[nxt][:, :, :E] = scaled(want_pos[nxt][:, :, :, :E])             # earlier step's output of lanes < E only)
        want_ret[:, :, :E] = ret64
        assert_state("after step %d" % j)                                       # incl. the step's INPUT copy of posT / xsT: unchanged
        cur = nxt
    share = n_knife / max(1, n_draws)
    print("[rollout episodes] S=%d N=%d %dx%d E=%d ep_len=%d episode0=%d row0=%d%s: %d draws, %d knife edges (%.4f %%), %d of them fell "
          "the other way" % (S, N, nrow, ncol, E, ep_len, episode0, row0, " pos_in" if pos_in else "", n_draws, n_knife, 100.0 * share,
                             n_flip_knife))
    assert share <= KNIFE_EDGE_CAP, "knife-edge share %.3e of this case's draws: pick another seed for the case" % share

    # ---- the sequential kernels on the last episode of seed 0 -------------------------------------------------------------------
    if knife_in_last_episode:
        print("[rollout episodes] episode %d of seed 0 holds a knife-edge draw: sequential-vs-parallel comparison skipped" % (episode0 + E - 1))
        return dict(draws=n_draws, knife_edges=n_knife, knife_flips=n_flip_knife, sequential_compared=False)
    q_rp = {k: bk.dev(np.full((1, ep_len, w * N), SENT, np.float32)) for k, w in widths}
    q_pos = [bk.dev(np.full((1, N, 2), SENT, np.int32)) for _ in range(2)]
    q_xs = [bk.dev(np.full((1, 2 * N), SENT, np.float32)) for _ in range(2)]
    q_ret = bk.dev(np.full((1, N), SENT, np.float64))
    ep_last = episode0 + E - 1
    L.rcmarl_env_reset(bk.ptr(d_start) if pos_in else None, bk.ptr(d_seeds), nrow, ncol, bk.ptr(d_scale), ep_last, bk.ptr(q_pos[0]),
                       bk.ptr(q_xs[0]), bk.ptr(q_ret), 1, N, bk.stream)
    qc = 0
    for j in range(ep_len):
        L.rcmarl_rollout_step(bk.ptr(q_xs[qc]), bk.ptr(q_pos[qc]), bk.ptr(d_goal), bk.ptr(d_tha), bk.ptr(d_seeds), nrow, ncol,
                              bk.ptr(d_scale), bk.ptr(q_rp["s"]), bk.ptr(q_rp["ns"]), bk.ptr(q_rp["sa"]), bk.ptr(q_rp["a"]),
                              bk.ptr(q_rp["r"]), ep_len, j, bk.ptr(q_pos[1 - qc]), bk.ptr(q_xs[1 - qc]), bk.ptr(q_ret), float(gamma ** j),
                              ep_last, j, mu, 1, N, HID, A, ldpa, None, bk.stream)
        qc = 1 - qc
    first = row0 + (E - 1) * ep_len
    for k, _ in widths:
        np.testing.assert_array_equal(bk.host(q_rp[k])[0], bk.host(rp[k])[0, first:first + ep_len], err_msg="sequential vs episode-parallel: " + k)
    np.testing.assert_array_equal(bk.host(q_pos[qc])[0], bk.host(d_pos[cur])[0, :, :, E - 1])
    np.testing.assert_array_equal(bk.host(q_xs[qc])[0], bk.host(d_xs[cur])[0, :, E - 1])
    np.testing.assert_array_equal(bk.host(q_ret)[0], bk.host(d_ret)[0, :, E - 1])
    return dict(draws=n_draws, knife_edges=n_knife, knife_flips=n_flip_knife, sequential_compared=True)


# ------------------------------------------------------------------------------------------
def check_row_helpers(bk, S, N, B, ep, width):
    """The TD-target shortcut's two helpers (engine._value_next_cached*), every `ep`-th row starting at ep - 1:
    rcmarl_gather_rows on a replay tensor addressed as the engine does (base pointer row0 rows in, seed stride = the whole capacity)
    == the NumPy slice, nothing written behind dst; rcmarl_scatter_values, both forms == v, resp. float32(r + float32(gamma * v)) to
    the BIT, every other entry of out untouched, a last row beyond ldb refused; and the identity the shortcut rests on: the TD target
    rcmarl_mid_value(..., r_applied, gamma) leaves at those rows equals the two-call route -- rcmarl_mid_value(..., NULL) on the
    gathered columns, then rcmarl_scatter_values.  With RCMARL_MIDVALUE_MX=0 both routes run the same fp32 lane code on a row: equal
    bits.  With the matrix-core form (the default) a row's value may depend on its position in the 16-row tile, so there the two
    routes are only held to the existing 3e-6 bar of check_mid_value."""
    import pytest
    from rcmarl_amd import capi
    rng = np.random.default_rng(S * 11 + N * 5 + B + ep + width)
    L = bk.lib
    n_rows, first = B // ep, ep - 1
    assert n_rows >= 1
    # ---- gather ----
    row0 = 3
    cap = row0 + B + 4
    src = rng.normal(size=(S, cap, width)).astype(np.float32)
    dst0 = np.full(S * n_rows * width + 9, SENT, np.float32)
    d_src, d_dst = bk.dev(src), bk.dev(dst0)
    L.rcmarl_gather_rows(_ptr_add(bk.ptr(d_src), 4 * row0 * width), cap * width, first, ep, n_rows, width, bk.ptr(d_dst), S, bk.stream)
    dst = bk.host(d_dst)
    np.testing.assert_array_equal(dst[:S * n_rows * width].reshape(S, n_rows, width), src[:, row0 + first:row0 + B:ep][:, :n_rows])
    np.testing.assert_array_equal(dst[S * n_rows * width:], dst0[S * n_rows * width:])
    np.testing.assert_array_equal(bk.host(d_src), src)
    # ---- scatter ----
    ldb = pad64(B)
    gamma = 0.9
    v = rng.normal(size=(S, N, ldb)).astype(np.float32)
    r_applied = rng.normal(size=(S, N, ldb)).astype(np.float32)
    out0 = rng.normal(size=(S, N, ldb)).astype(np.float32)
    d_v, d_r = bk.dev(v), bk.dev(r_applied)
    cols = first + ep * np.arange(n_rows)
    for with_r in (False, True):
        d_out = bk.dev(out0)
        L.rcmarl_scatter_values(bk.ptr(d_v), bk.ptr(d_r) if with_r else None, gamma, bk.ptr(d_out), first, ep, n_rows, S, N, ldb, bk.stream)
        want = out0.copy()
        if with_r:
            gv = (np.float32(gamma) * v[:, :, :n_rows]).astype(np.float32)          # multiply, round, add, round
            want[:, :, cols] = (r_applied[:, :, cols] + gv).astype(np.float32)
        else:
            want[:, :, cols] = v[:, :, :n_rows]
        np.testing.assert_array_equal(bk.host(d_out).view(np.uint32), want.view(np.uint32), err_msg="scatter_values, r_applied %s" % with_r)
    d_out = bk.dev(out0)
    with pytest.raises(capi.RcmarlError, match="RCMARL_ERR_ARG"):                 # the last row would be column ldb
        L.rcmarl_scatter_values(bk.ptr(d_v), bk.ptr(d_r), gamma, bk.ptr(d_out), ldb - (n_rows - 1) * ep, ep, n_rows, S, N, ldb, bk.stream)
    np.testing.assert_array_equal(bk.host(d_out), out0)
    # ---- the TD target through the shortcut == the TD target of the straight path ----
    in_dim = 2 * N
    P, _ = geom(in_dim, 1)
    ldp = pad64(P)
    theta = np.zeros((S, N, ldp), np.float32)
    theta[:, :, :P] = (0.3 * rng.normal(size=(S, N, P))).astype(np.float32)
    a1 = rng.normal(size=(S, N * HID, ldb)).astype(np.float32)
    a1g = np.zeros_like(a1)
    a1g[:, :, :n_rows] = a1[:, :, cols]
    d_th, d_a, d_ag = bk.dev(theta), bk.dev(a1), bk.dev(a1g)
    d_y, d_vg = bk.dev(np.full((S, N, ldb), SENT, np.float32)), bk.dev(np.full((S, N, ldb), SENT, np.float32))
    d_out = bk.dev(out0)
    L.rcmarl_mid_value(bk.ptr(d_a), bk.ptr(d_th), bk.ptr(d_r), gamma, bk.ptr(d_y), S, N, B, in_dim, HID, ldp, ldb, bk.stream)
    L.rcmarl_mid_value(bk.ptr(d_ag), bk.ptr(d_th), None, gamma, bk.ptr(d_vg), S, N, n_rows, in_dim, HID, ldp, ldb, bk.stream)
    L.rcmarl_scatter_values(bk.ptr(d_vg), bk.ptr(d_r), gamma, bk.ptr(d_out), first, ep, n_rows, S, N, ldb, bk.stream)
    straight, two_call = bk.host(d_y)[:, :, cols], bk.host(d_out)[:, :, cols]
    assert np.all(straight != np.float32(SENT)) and np.all(bk.host(d_vg)[:, :, n_rows:] == np.float32(SENT))
    if os.environ.get("RCMARL_MIDVALUE_MX", "1") == "0" or bk.lib.rcmarl_lattice_f16_mode() == 0:
        np.testing.assert_array_equal(two_call.view(np.uint32), straight.view(np.uint32), err_msg="TD target: shortcut vs straight path, fp32 lane code")
    else:
        rel_close(two_call, straight, 3e-6, "TD target: shortcut vs straight path, matrix-core form")


COPY3D_DEFAULT = dict(batches=5, rows=3, cols=8, ld_src=12, ld_dst=12, pad_src=0, pad_dst=0, src_off=0, dst_off=0, mask="mixed", refused=False)
COPY3D_CASES = {
    # rcmarl_copy3d with more than 65535 batches (AdversaryPath publishes message rows with batches = seeds): the grid's z extent is
    # capped and the kernel strides over the rest; masked rows stay untouched.
    "more_batches_than_a_grid_dimension": dict(batches=70001),
    # the 4-byte form k_copy3d<1>: a column block of the sharded instance that starts or ends at an odd offset
    "odd_cols": dict(cols=7),
    "odd_ld_src": dict(ld_src=13),
    "odd_ld_dst": dict(ld_dst=15),
    "odd_batch_strides": dict(pad_src=1, pad_dst=3),
    "src_one_float_in": dict(src_off=1),
    "dst_one_float_in": dict(dst_off=1),
    "scalar_form_several_column_blocks": dict(cols=1027, ld_src=1030, ld_dst=1027, rows=2, batches=2),
    # the 16-byte form k_copy3d<4>
    "mask_null": dict(mask=None),
    "mask_all_zero": dict(mask="zeros"),
    "vector_form_several_column_blocks": dict(cols=2052, ld_src=2056, ld_dst=2060, rows=2, batches=2),        # blockIdx.x = 0..2, last ragged
    # the early return and the refused shapes
    "no_batches": dict(batches=0),
    "no_rows": dict(rows=0, mask=None),
    "ld_src_below_cols": dict(ld_src=4, refused=True),
    "ld_dst_below_cols": dict(ld_dst=7, refused=True),
}
COPY3D_SMALL = [k for k in COPY3D_CASES if k != "more_batches_than_a_grid_dimension"]


def check_copy3d(bk, case):
    """rcmarl_copy3d (the pack pass of the sharded all-to-all, the adversaries' message rows): dst[b][r][:cols] = src[b][r][:cols] for
    the rows the mask keeps == the NumPy box copy, and every float of dst outside the box keeps its previous contents (dst is random, so
    a stray write shows).  `case` names an entry of COPY3D_CASES."""
    import pytest
    from rcmarl_amd import capi
    c = dict(COPY3D_DEFAULT, **COPY3D_CASES[case])
    rng = np.random.default_rng(9)
    batches, rows, cols, ld_src, ld_dst = c["batches"], c["rows"], c["cols"], c["ld_src"], c["ld_dst"]
    src_batch = max(rows, 1) * max(ld_src, cols) + c["pad_src"]
    dst_batch = max(rows, 1) * max(ld_dst, cols) + c["pad_dst"]
    src = rng.normal(size=c["src_off"] + max(batches, 1) * src_batch + 8).astype(np.float32)
    dst0 = rng.normal(size=c["dst_off"] + max(batches, 1) * dst_batch + 8).astype(np.float32)
    mask = {"mixed": np.array([1, 0, 1] * rows, np.int32)[:rows], "zeros": np.zeros(rows, np.int32), None: None}[c["mask"]]
    d_src, d_dst = bk.dev(src), bk.dev(dst0)
    d_mask = None if mask is None else bk.dev(mask)

    def call():
        return bk.lib.rcmarl_copy3d(_ptr_add(bk.ptr(d_src), 4 * c["src_off"]), src_batch, ld_src, _ptr_add(bk.ptr(d_dst), 4 * c["dst_off"]),
                                    dst_batch, ld_dst, batches, rows, cols, None if mask is None else bk.ptr(d_mask), bk.stream)
    want = dst0.copy()
    if c["refused"]:
        with pytest.raises(capi.RcmarlError, match="RCMARL_ERR_ARG"):
            call()
    else:
        assert call() in (0, None)
        keep = np.arange(rows) if mask is None else np.nonzero(mask)[0]
        b, r, k = np.arange(batches)[:, None, None], keep[None, :, None], np.arange(cols)[None, None, :]
        want[c["dst_off"] + b * dst_batch + r * ld_dst + k] = src[c["src_off"] + b * src_batch + r * ld_src + k]
    np.testing.assert_array_equal(bk.host(d_dst), want)
    np.testing.assert_array_equal(bk.host(d_src), src)
