"""Checks of the tiled home of the fp32 W1 between the SGD steps of a local fit (rcmarl_layer1_backward_sgd_lattice_tiled,
EngineConfig.w1_tiled), shared by the hipemu (CPU), GPU and C-ABI tests.  The yardstick is always the strided entry point,
rcmarl_layer1_backward_sgd_lattice, on copies of the same inputs, and the comparison is word for word."""
import os

import numpy as np

import engine_checks as EC
import kernel_checks as KC
from kernel_checks import HID, LT, geom, pad64

# (S, N, in_dim, B, masked agent).  First: 140 columns -- the second n-tile partial, agent 6 straddles column 128; 300 rows -- a partial
# 256-row tile and a partial 32-row k-tile of Wp; 70 replay rows -- a partial last k-tile of the reduction.  Second: the 128-row form.
SHAPES = [(2, 7, 300, 70, 3), (1, 16, 100, 70, None)]


def roles(steps):
    """(src_tiled, dst_tiled) of every step of one fit; None = the strided entry point (a one-step fit)"""
    if steps == 1:
        return [None]
    return [(int(st > 0), int(st < steps - 1)) for st in range(steps)]


def tiled_index(S, N, in_dim, hid=HID):
    """float index [S][in_dim][N * hid] of W1[s][k][col] in the tiled scratch (include/rcmarl.h)"""
    KT, CT = 8 * ((in_dim + 255) // 256), 4 * ((N * hid + 127) // 128)
    s = np.arange(S)[:, None, None]
    k = np.arange(in_dim)[None, :, None]
    col = np.arange(N * hid)[None, None, :]
    lane = col % 32 + 32 * ((k % 8) // 4)
    q = 4 * ((k % 32) // 8) + k % 4
    return ((s * KT + k // 32) * CT + col // 32) * 1024 + q * 64 + lane, S * KT * CT * 1024


def _inputs(S, N, in_dim, B, masked, steps):
    rng = np.random.default_rng(1000 * S + 100 * N + in_dim + B)
    P, _ = geom(in_dim, 1)
    ldp, ldb = pad64(P), pad64(B)
    theta = rng.uniform(-0.3, 0.3, size=(S, N, ldp)).astype(np.float32)        # W1, the small arrays AND the columns P..ldp
    alpha = rng.uniform(0.2, 1.5, size=in_dim).astype(np.float32)
    K = rng.integers(-31, 32, size=(S, B, in_dim))
    x = (alpha.astype(np.float64) * K).astype(np.float32)                      # replay rows on the integer lattice alpha * K
    dz = np.zeros((steps, S, N * HID, ldb), np.float32)
    dz[..., :B] = (0.02 * rng.normal(size=(steps, S, N * HID, B))).astype(np.float32)      # a distinct dz1 per step
    mask = np.ones(N, np.int32)
    if masked is not None:
        mask[masked] = 0
    return theta, alpha, x, dz, mask, ldp, ldb


def check_tiled_sequence(bk, S, N, in_dim, B, masked, steps=5, lr=0.01):
    """`steps` backward launches of one fit through the tiled roles against `steps` calls of the strided entry point: Wp word for
    word after every step, the whole parameter matrix word for word after the last one."""
    L = bk.lib
    theta, alpha, x, dz, mask, ldp, ldb = _inputs(S, N, in_dim, B, masked, steps)
    lb = KC.LatticeBuffers(bk, S, N, in_dim, B)
    g = lb.g
    d_x, d_al, d_mask = bk.dev(x), bk.dev(alpha), bk.dev(mask)
    KC._encode(bk, lb, d_x, B * in_dim, d_al, S, B, in_dim)
    assert bk.host(lb.flag)[0] == 0
    dzp = []
    for st in range(steps):
        buf = bk.dev(np.full(S * LT.Geometry.nbytes(g.dzp, 3) // 2, 0x7fc0, np.uint16))
        L.rcmarl_lattice_pack_dz(bk.ptr(bk.dev(dz[st])), bk.ptr(buf), S, N, B, HID, ldb, g.dzp[0], g.dzp[1], bk.stream)
        dzp.append(buf)
    nbytes = int(L.rcmarl_lattice_w1_tiled_bytes(S, N, in_dim, HID))
    idx, nfloat = tiled_index(S, N, in_dim)
    assert nbytes == 4 * nfloat
    wp_fill = np.full(S * LT.Geometry.nbytes(g.wp, 3) // 2, 0x7fc0, np.uint16)
    d_th = {"old": bk.dev(theta.copy()), "new": bk.dev(theta.copy())}
    d_wp = {"old": bk.dev(wp_fill), "new": bk.dev(wp_fill)}
    d_wt = bk.dev(np.full(nfloat, np.nan, np.float32))                          # the first step must write every position it later reads
    for st, role in enumerate(roles(steps)):
        last = st == steps - 1
        for which in ("old", "new"):
            args = (bk.ptr(lb.ktp), g.ktp[0], g.ktp[1], bk.ptr(dzp[st]), g.dzp[0], g.dzp[1], bk.ptr(d_al), bk.ptr(d_th[which]),
                    bk.ptr(d_mask), S, N, B, in_dim, HID, ldp, lr, None if last else bk.ptr(d_wp[which]), g.wp[0], g.wp[1])
            if which == "old" or role is None:
                L.rcmarl_layer1_backward_sgd_lattice(*args, bk.stream)
            else:
                L.rcmarl_layer1_backward_sgd_lattice_tiled(*args, bk.ptr(d_wt), nbytes, role[0], role[1], bk.stream)
        wp_old, wp_new = bk.host(d_wp["old"]), bk.host(d_wp["new"])
        np.testing.assert_array_equal(wp_new.view(np.uint16), wp_old.view(np.uint16), err_msg="Wp after step %d" % st)
        if st == 0:
            assert not np.array_equal(wp_old.view(np.uint16), wp_fill)           # the operand of the next forward was written
        if role is not None and role[1]:
            # the documented layout: the scratch holds exactly the strided sequence's W1 (masked agent: its unchanged weights) and
            # zeros everywhere else in the 32-row blocks that hold a real row (the ones whose Wp rows the epilogue writes); blocks
            # further out are zero or, where the running form's tiles do not reach (128-row tiles), untouched
            wt = bk.host(d_wt).copy()
            w1_old = bk.host(d_th["old"])[:, :, :in_dim * HID].reshape(S, N, in_dim, HID).transpose(0, 2, 1, 3).reshape(S, in_dim, N * HID)
            np.testing.assert_array_equal(wt[idx].view(np.uint32), w1_old.view(np.uint32), err_msg="tiled W1 after step %d" % st)
            wt[idx] = 0
            blocks = wt.view(np.uint32).reshape(S, 8 * ((in_dim + 255) // 256), -1)
            used = (in_dim + 31) // 32
            np.testing.assert_array_equal(blocks[:, :used], 0)
            assert np.isin(blocks[:, used:], (0, 0x7fc00000)).all()
    th_old, th_new = bk.host(d_th["old"]), bk.host(d_th["new"])
    np.testing.assert_array_equal(th_new.view(np.uint32), th_old.view(np.uint32))
    w1 = slice(0, in_dim * HID)
    for n in range(N):
        if mask[n]:
            assert not np.array_equal(th_new[:, n, w1], theta[:, n, w1])        # the update did happen
        else:
            np.testing.assert_array_equal(th_new[:, n], theta[:, n])
    np.testing.assert_array_equal(th_new[:, :, in_dim * HID:], theta[:, :, in_dim * HID:])      # small arrays and P..ldp: not this kernel's


# ---- engine ---------------------------------------------------------------------------------------------------------------------
class CountingLib:
    """the library with a count of the layer-1 backward launches by entry point, network width, input width and role"""

    def __init__(self, lib):
        self._lib = lib
        self.calls = []

    def __getattr__(self, name):
        fn = getattr(self._lib, name)
        if name == "rcmarl_layer1_backward_sgd_lattice":
            def counted(*a):
                self.calls.append(("strided", a[13], a[12], None))
                return fn(*a)
            return counted
        if name == "rcmarl_layer1_backward_sgd_lattice_tiled":
            def counted(*a):
                self.calls.append(("tiled", a[13], a[12], (a[21], a[22])))
                return fn(*a)
            return counted
        return fn


def _run(device, lib, labels, w1_tiled, n=16, critic_hid=20, tr_hid=20, lattice=True, seeds=(51,), local_fit_steps=5):
    from rcmarl_amd import capi
    from rcmarl_amd.engine import EngineConfig, RPBCACEngine
    in_nodes = [[i, (i + 1) % n, (i - 1) % n] for i in range(n)]               # a ring, own value first
    args = EC.make_args(labels, H=1, n_episodes=2, max_ep_len=3, n_ep_fixed=2, n_epochs=2, buffer_size=6, seed=seeds[0], in_nodes=in_nodes)
    wrng = np.random.default_rng(5)
    M = EC.M
    W = [[{"actor": M.init_mlp(wrng, 2 * n, 20, 5), "critic": M.init_mlp(wrng, 2 * n, critic_hid, 1), "tr": M.init_mlp(wrng, 3 * n, tr_hid, 1)}
          for _ in range(n)] for _ in seeds]
    goals = np.stack([np.random.default_rng(100 + s).integers(0, 5, size=(n, 2)) for s in range(len(seeds))])
    cfg = EngineConfig(n, labels, in_nodes, H=1, max_ep_len=3, n_ep_fixed=2, n_epochs=2, buffer_size=6, nrow=5, ncol=5,
                       n_seeds=len(seeds), rng_mode="device", lattice=lattice, critic_hid=critic_hid, tr_hid=tr_hid, w1_tiled=w1_tiled,
                       local_fit_steps=local_fit_steps)
    clib = CountingLib(lib if lib is not None else capi.load())
    eng = RPBCACEngine(cfg, seeds=list(seeds), device=device, lib=clib)
    for s in range(len(seeds)):
        for i in range(n):
            for net in ("actor", "critic", "tr"):
                eng.set_weights(s, i, net, W[s][i][net])
    eng.set_goals(goals)
    eng.train(args["n_episodes"])
    eng.sync()
    return eng, clib.calls, {net: eng.theta[net].detach().cpu().numpy().copy() for net in ("actor", "critic", "tr")}


def check_engine_tiled_equals_strided(device, lib, labels):
    """16 agents on a ring, H = 1, 5 x 5 grid, lattice path, one block of two epochs: every network's weights with W1 tiled between the
    steps equal those of the strided path bit for bit, and each five-step fit is 1 strided->tiled + 3 tiled->tiled + 1 tiled->strided."""
    eng_t, calls_t, th_t = _run(device, lib, labels, True)
    eng_f, calls_f, th_f = _run(device, lib, labels, False)
    assert eng_t.lat_enabled and eng_t.lat_active and eng_f.lat_active and eng_t.lat_w1_tiled is not None and eng_f.lat_w1_tiled is None
    for net in ("actor", "critic", "tr"):
        assert np.isfinite(th_t[net]).all()
        np.testing.assert_array_equal(th_t[net].view(np.uint32), th_f[net].view(np.uint32), err_msg=net)
    assert all(c[0] == "strided" for c in calls_f) and len(calls_f) == len(calls_t) and len(calls_t) == 2 * 2 * 5     # 2 epochs x 2 nets
    assert all(c[0] == "tiled" for c in calls_t)
    for f in range(0, len(calls_t), 5):
        assert [c[3] for c in calls_t[f:f + 5]] == [(0, 1), (1, 1), (1, 1), (1, 1), (1, 0)], calls_t[f:f + 5]
        assert len({c[2] for c in calls_t[f:f + 5]}) == 1                       # one fit = one network family


def check_engine_other_paths_stay_strided(device, lib, monkeypatch):
    """w1_tiled=True does not reach the wide nets (their half-wave already covers whole lines), the chain fits, or a one-step fit"""
    n = 16
    _, calls, _ = _run(device, lib, ["Cooperative"] * n, True, critic_hid=40, tr_hid=40)
    assert calls and all(c[0] == "strided" and c[1] == 40 for c in calls), calls
    monkeypatch.setenv("RCMARL_FIT_CHAINS", "1")                               # (chains serve nets of at most 20 inputs, off the lattice path)
    eng, calls, _ = _run(device, lib, ["Cooperative"] * 5, True, n=5, lattice=False)
    assert eng._fit_as_chains("critic", eng.coop) and eng._fit_as_chains("tr", eng.coop) and calls == []
    monkeypatch.delenv("RCMARL_FIT_CHAINS")
    eng, calls, _ = _run(device, lib, ["Cooperative"] * n, True, local_fit_steps=1)
    assert len(calls) == 2 * 2 and all(c[0] == "strided" for c in calls), calls


# ---- no GPU -----------------------------------------------------------------------------------------------------------------------
def check_size_query(lib):
    q = lib.rcmarl_lattice_w1_tiled_bytes
    assert q(16, 256, 768, 20) == 16 * 768 * 5120 * 4                           # the headline shape: 252 MB
    assert q(16, 256, 512, 20) == 16 * 512 * 5120 * 4
    assert q(2, 7, 300, 20) == 2 * 512 * 256 * 4                                # 300 rows -> 512, 140 columns -> 256
    assert q(1, 16, 100, 20) == 256 * 384 * 4                                   # padded to the 256-row tile whatever form runs
    assert q(1, 1, 1, 1) == 256 * 128 * 4
    assert q(0, 5, 10, 20) == -1 and q(1, 0, 10, 20) == -1 and q(1, 5, 0, 20) == -1 and q(1, 5, 10, 0) == -1


def check_arg_errors(lib):
    """bad tiled calls come back as RCMARL_ERR_ARG before the HIP runtime is touched (the pointers below are never dereferenced)"""
    import pytest
    from rcmarl_amd.capi import RcmarlError
    S, N, in_dim, B = 1, 5, 10, 100
    need = int(lib.rcmarl_lattice_w1_tiled_bytes(S, N, in_dim, HID))
    fake = 0x10000
    base = (fake, 2, 8, fake, 1, 8, fake, fake, None, S, N, B, in_dim, HID, 704, 0.01)
    wp = (fake, 1, 1)
    bad = {
        "buffer too small (src)": base + wp + (fake, need - 4, 1, 1, None),
        "buffer too small (dst)": base + wp + (fake, need - 4, 0, 1, None),
        "zero-size buffer": base + (None, 0, 0) + (fake, 0, 1, 0, None),
        "NULL buffer, tiled source": base + (None, 0, 0) + (None, need, 1, 0, None),
        "NULL buffer, tiled destination": base + wp + (None, need, 0, 1, None),
        "dst_tiled without wp_out (first step)": base + (None, 0, 0) + (fake, need, 0, 1, None),
        "dst_tiled without wp_out (middle step)": base + (None, 0, 0) + (fake, need, 1, 1, None),
        "the old checks still hold": (None,) + base[1:] + wp + (fake, need, 1, 1, None),
    }
    for what, args in bad.items():
        with pytest.raises(RcmarlError, match="RCMARL_ERR_ARG"):
            lib.rcmarl_layer1_backward_sgd_lattice_tiled(*args)


def check_exports(lib_path):
    import re
    import subprocess
    from rcmarl_amd import capi
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = subprocess.run(["nm", "-D", "--defined-only", lib_path], capture_output=True, text=True).stdout
    exported = set(re.findall(r"\bT (rcmarl_\w+)", out))
    header = open(os.path.join(root, "include", "rcmarl.h")).read()
    for name in ("rcmarl_layer1_backward_sgd_lattice_tiled", "rcmarl_lattice_w1_tiled_bytes", "rcmarl_layer1_backward_sgd_lattice"):
        assert name in exported and re.search(r"\b%s\s*\(" % name, header), name
    assert "rcmarl_layer1_backward_sgd_lattice_tiled" in capi.SIGNATURES and "rcmarl_lattice_w1_tiled_bytes" in capi.LONG_QUERIES
    # the new launch takes the old one's arguments, then the scratch, its size and the two roles in front of the stream
    old, new = capi.SIGNATURES["rcmarl_layer1_backward_sgd_lattice"], capi.SIGNATURES["rcmarl_layer1_backward_sgd_lattice_tiled"]
    assert new[:len(old) - 1] == old[:-1] and len(new) == len(old) + 4 and new[-1] == old[-1]
    assert re.search(r"long\s+rcmarl_lattice_w1_tiled_bytes\s*\(", header)
