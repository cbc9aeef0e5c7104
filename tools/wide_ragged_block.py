#!/usr/bin/env python
"""The fused ragged head of a wide net (rcmarl_wide_consensus_head_ragged) beside the uniform chain, on the GPU.

    python tools/wide_ragged_block.py head  [--agents 256 --hid 512 --d 18 --H 8 --rows 1000 --repeats 21 --iters 5]
    python tools/wide_ragged_block.py block [--agents 256 --hid 512 --rows 1000 --blocks 4]
    python tools/wide_ragged_block.py all   [--out FILE.json]

head   the head in isolation on a REGULAR graph, handed to the ragged entry as one class: (1) the uniform chain
       (rcmarl_wide_consensus_head: gather, 128 x 128 GEMM tile on d + 1 rows, select, rows) in the library's default form, (2) the
       same in the fp32 form (rcmarl_wide_set_f16_mode(0)), (3) the fused entry.  The three alternate inside every repetition; a
       repetition times `iters` calls between two HIP events after a warm-up; the median, minimum and maximum over the repetitions
       are reported.  Before timing, the aggregates of (2) and (3) are compared bit for bit at the size that is timed.
block  one update block (n_ep_fixed episodes + n_epochs epochs, host clock around eng.train() ending in a device synchronise) of an
       engine with a wide critic on (a) an irregular instance with degrees mixed between 4 and 18, ragged_wide='auto', (b) the regular
       d = 18, H = 8 instance of the same shape on the uniform chain, (c) the regular d = 4, H = 1 instance.  The first block of each
       engine is warm-up.
Prints one JSON line per part; --out also writes them to a file.  The bytes of hmat / hb / est the fused head does not allocate are
computed from the shape."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from rcmarl_amd import capi  # noqa: E402
from rcmarl_amd.engine import EngineConfig, RPBCACEngine  # noqa: E402


def pad64(n):
    return (n + 63) // 64 * 64


def stats(ts):
    ts = sorted(ts)
    return {"median_us": ts[len(ts) // 2], "min_us": ts[0], "max_us": ts[-1], "repeats": len(ts)}


def scratch_bytes(S, N, d, hid, ldb):
    """hmat [S][N][d+1][hid] + hb [S][N][d+1] + est [S][N][d+1][ldb], fp32"""
    return 4 * S * N * (d + 1) * (hid + 1 + ldb)


def head(L, N, hid, d, H, B, repeats, iters, S=1):
    dev = "cuda"
    st = torch.cuda.current_stream().cuda_stream
    in_dim = 2 * N
    P = in_dim * hid + hid + hid * hid + hid + hid + 1
    ldp, ldb = pad64(P), pad64(B)
    g = torch.Generator(device=dev).manual_seed(1)
    rnd = lambda *sh: torch.randn(*sh, device=dev, generator=g)
    theta, msg = rnd(S, N, ldp) * 0.05, rnd(S, N, ldp) * 0.05
    phi = rnd(S, N * hid, ldb).abs()
    i32 = dict(dtype=torch.int32, device=dev)
    rows = [[(i + k) % N for k in range(d)] for i in range(N)]
    nbr = torch.tensor(rows, **i32)
    coop = torch.ones(N, **i32)
    off = torch.tensor(np.arange(N + 1, dtype=np.int32) * d, **i32)
    idx = torch.tensor(np.asarray(rows, np.int32).ravel(), **i32)
    order = torch.arange(N, **i32)
    table = (capi.RaggedClass * 1)(capi.RaggedClass(d, H, 0, N))
    z = lambda *sh: torch.zeros(*sh, device=dev)
    hmat, hb, est = z(S, N, d + 1, hid), z(S, N, d + 1), z(S, N, d + 1, ldb)
    ebuf, grads, agg_u, agg_r = z(S, N, ldb), z(S, N, L.rcmarl_wide_grad_size(hid)), z(S, N, ldb), z(S, N, ldb)
    ebuf_r, grads_r = z(S, N, ldb), z(S, N, L.rcmarl_wide_grad_size(hid))

    def uniform(agg=None):
        L.rcmarl_wide_consensus_head(phi.data_ptr(), theta.data_ptr(), msg.data_ptr(), nbr.data_ptr(), coop.data_ptr(), None,
                                     hmat.data_ptr(), hb.data_ptr(), est.data_ptr(), ebuf.data_ptr(), grads.data_ptr(),
                                     None if agg is None else agg.data_ptr(), S, N, B, in_dim, hid, ldp, ldb, d, H, st)

    def ragged(agg=None):
        L.rcmarl_wide_consensus_head_ragged(phi.data_ptr(), None, 0, theta.data_ptr(), msg.data_ptr(), off.data_ptr(), idx.data_ptr(),
                                            order.data_ptr(), table, 1, ebuf_r.data_ptr(), grads_r.data_ptr(),
                                            None if agg is None else agg.data_ptr(), None, 0, S, N, B, in_dim, hid, ldp, ldb, st)

    def form(mode, fn):
        def run():
            L.rcmarl_wide_set_f16_mode(mode)
            fn()
        return run
    variants = [("uniform_default", form(-1, uniform)), ("uniform_fp32", form(0, uniform)), ("ragged_fused", form(-1, ragged))]
    try:
        # results first: same aggregates, bit for bit, at the size that is timed
        L.rcmarl_wide_set_f16_mode(0)
        uniform(agg_u)
        ragged(agg_r)
        torch.cuda.synchronize()
        same = bool(torch.equal(agg_u[:, :, :B].view(torch.int32), agg_r[:, :, :B].view(torch.int32)))
        e_err = float((ebuf[:, :, :B] - ebuf_r[:, :, :B]).abs().max() / max(1.0, float(ebuf[:, :, :B].abs().max())))
        g_err = float((grads[:, :, :hid + 1] - grads_r[:, :, :hid + 1]).abs().max() / max(1.0, float(grads[:, :, :hid + 1].abs().max())))
        for _, fn in variants:                    # warm-up: code objects, every shape of the timed window
            for _ in range(3):
                fn()
        torch.cuda.synchronize()
        times = {name: [] for name, _ in variants}
        for _ in range(repeats):
            for name, fn in variants:             # alternating: drift of the shared machine hits all three alike
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(iters):
                    fn()
                e1.record()
                torch.cuda.synchronize()
                times[name].append(e0.elapsed_time(e1) / iters * 1e3)
    finally:
        L.rcmarl_wide_set_f16_mode(-1)
    out = {"part": "head", "agents": N, "hid": hid, "d": d, "H": H, "rows": B, "iters_per_repeat": iters,
           "aggregates_bit_equal": same, "ebuf_max_rel_diff": e_err, "grads_max_rel_diff": g_err,
           "phi_bytes": 4 * S * N * hid * ldb, "scratch_bytes_not_allocated": scratch_bytes(S, N, d, hid, ldb)}
    for name in times:
        out[name] = stats(times[name])
    out["ragged_over_uniform_fp32"] = out["ragged_fused"]["median_us"] / out["uniform_fp32"]["median_us"]
    out["ragged_over_uniform_default"] = out["ragged_fused"]["median_us"] / out["uniform_default"]["median_us"]
    return out


def block(L, N, hid, rows, blocks, n_epochs=2):
    max_ep_len = 20
    n_ep_fixed = max(1, rows // max_ep_len)
    rng = np.random.default_rng(3)
    deg = [int(x) for x in rng.integers(4, 19, size=N)]
    instances = {
        "irregular_4_to_18": ([[(i + k) % N for k in range(deg[i])] for i in range(N)], [(dd - 1) // 2 for dd in deg], "auto"),
        "regular_18_8": ([[(i + k) % N for k in range(18)] for i in range(N)], 8, "refuse"),
        "regular_4_1": ([[(i + k) % N for k in range(4)] for i in range(N)], 1, "refuse"),
    }
    out = {"part": "block", "agents": N, "critic_hid": hid, "rows_per_block": n_ep_fixed * max_ep_len, "n_epochs": n_epochs,
           "timed_blocks": blocks - 1}
    for name, (in_nodes, H, switch) in instances.items():
        cfg = EngineConfig(N, ["Cooperative"] * N, in_nodes, H=H, max_ep_len=max_ep_len, n_ep_fixed=n_ep_fixed, n_epochs=n_epochs,
                           buffer_size=n_ep_fixed * max_ep_len, nrow=16, ncol=16, n_seeds=1, rng_mode="device", critic_hid=hid,
                           fast_lr=1e-3, ragged_wide=switch)      # (the reference's fast_lr = 0.01 diverges beyond ~64 agents)
        eng = RPBCACEngine(cfg, seeds=[1], device="cuda", lib=L)
        eng.init_glorot(base_seed=3)
        eng.set_goals(np.random.default_rng(9).integers(0, 16, size=(N, 2)))
        ts = []
        for b in range(blocks):
            eng.sync()
            t0 = time.perf_counter()
            eng.train(n_ep_fixed)
            eng.sync()
            if b:                                 # block 0: warm-up (code objects, buffers, graph capture)
                ts.append((time.perf_counter() - t0) * 1e3)
        ts.sort()
        w = eng.get_all_weights("critic")
        out[name] = {"median_ms": ts[len(ts) // 2], "min_ms": ts[0], "max_ms": ts[-1], "finite": bool(np.isfinite(w).all()),
                     "head_scratch_allocated": eng.w_est is not None,
                     "head_scratch_bytes": 0 if eng.w_est is None else 4 * (eng.w_est.numel() + eng.w_hmat.numel() + eng.w_hb.numel())}
        if eng.w_est is None:
            out[name]["scratch_bytes_not_allocated"] = scratch_bytes(1, N, max(deg), hid, eng.ldb)
        del eng
        torch.cuda.empty_cache()
    out["irregular_over_regular_18_8"] = out["irregular_4_to_18"]["median_ms"] / out["regular_18_8"]["median_ms"]
    return out


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("part", choices=["head", "block", "all"])
    ap.add_argument("--agents", type=int, default=256)
    ap.add_argument("--hid", type=int, default=512)
    ap.add_argument("--d", type=int, default=18)
    ap.add_argument("--H", type=int, default=8)
    ap.add_argument("--rows", type=int, default=1000)
    ap.add_argument("--repeats", type=int, default=21)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--blocks", type=int, default=4)
    ap.add_argument("--out", default=None)
    a = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("wide_ragged_block.py measures on the GPU: no device here, nothing measured")
    if a.repeats < 20:
        raise SystemExit("--repeats: at least 20 (the median of fewer says little on a shared machine)")
    L = capi.load()
    res = []
    if a.part in ("head", "all"):
        res.append(head(L, a.agents, a.hid, a.d, a.H, a.rows, a.repeats, a.iters))
        print(json.dumps(res[-1]), flush=True)
    if a.part in ("block", "all"):
        res.append(block(L, a.agents, a.hid, a.rows, a.blocks))
        print(json.dumps(res[-1]), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            for r in res:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
