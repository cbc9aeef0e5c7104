"""One-agent views over the batched kernels (S = 1, N = 1 or N = d parameter rows).

The reference's agent methods (agents/resilient_CAC_agents.py, agents/
adversarial_CAC_agents.py) operate on ONE agent's Keras models.  The drop-in
classes in ``rcmarl_amd.agents`` keep those methods; each call packs the model
weights into parameter rows, launches the very same C-ABI kernels the batched
engine uses, and unpacks the result.  This is the compatibility path (legacy
per-agent loops keep working); throughput comes from ``train_RPBCAC`` ->
``engine.RPBCACEngine``.

A 20-unit net (main.py:59-82) issues the launches of the engine's 20-unit path.  A net of
any other hidden width goes through the dense fp32 entry points the engine uses for wide nets
(csrc/wide_kernels.hip, csrc/minibatch_wide*.hip, csrc/minibatch_actor_wide.hip) with S = 1;
it never takes the lattice or packed-operand paths.

No CPU fallback: the ops need librcmarl_hip.so and a GPU (tests inject the hipemu
build with ``set_backend``).
"""
import ctypes as C
import math

import numpy as np
import torch

from . import capi

HID = 20
_backend = None


def pad64(n):
    return (int(n) + 63) // 64 * 64


def set_backend(lib, device):
    """Test hook: run the single-agent ops on an explicitly given C-ABI library/device."""
    global _backend
    _backend = RowOps(lib, device)
    return _backend


def get_ops():
    global _backend
    if _backend is None:
        lib = capi.load()                                   # raises when the HIP library is missing
        if not torch.cuda.is_available():
            raise capi.RcmarlError("rcmarl_amd needs a ROCm GPU (torch.cuda.is_available() is False); no CPU fallback")
        _backend = RowOps(lib, "cuda")
    return _backend


def flat(params):
    return np.concatenate([np.asarray(p, dtype=np.float32).ravel() for p in params])


def shapes(in_dim, out_dim, hid=HID):
    return [(in_dim, hid), (hid,), (hid, hid), (hid,), (hid, out_dim), (out_dim,)]


def unflat(vec, in_dim, out_dim, hid=HID):
    out, o = [], 0
    for sh in shapes(in_dim, out_dim, hid):
        n = int(np.prod(sh))
        out.append(np.array(vec[o:o + n], dtype=np.float32).reshape(sh))
        o += n
    return out


def dims_of(params):
    """(in_dim, out_dim, hid) of a Keras-order weight list [W1,b1,W2,b2,W3,b3]: two equally wide hidden layers."""
    W1, W2, W3 = np.asarray(params[0]), np.asarray(params[2]), np.asarray(params[4])
    hid = int(W1.shape[1]) if W1.ndim == 2 else 0
    if len(params) != 6 or hid <= 0 or W2.shape != (hid, hid) or W3.ndim != 2 or W3.shape[0] != hid:
        raise capi.RcmarlError("the kernels support two hidden layers of equal width (got %s)"
                               % ([tuple(np.shape(p)) for p in params],))
    return int(W1.shape[0]), int(W3.shape[1]), hid


def offsets(in_dim, hid):
    """(o_b1, o_W2, o_b2, o_W3) of a parameter row"""
    o_b1 = in_dim * hid
    o_W2 = o_b1 + hid
    o_b2 = o_W2 + hid * hid
    return o_b1, o_W2, o_b2, o_b2 + hid


def as_rows(x):
    """[B, N, k] (or already flat [B, in]) -> contiguous fp32 [B, in] (Keras Flatten)."""
    x = np.asarray(x, dtype=np.float32)
    return np.ascontiguousarray(x.reshape(x.shape[0], -1))


class RowOps:
    def __init__(self, lib, device):
        self.lib = lib
        self.dev = torch.device(device)
        self._mb_flags = torch.zeros(8, dtype=torch.int32, device=self.dev)      # out-of-range flags of rcmarl_minibatch_fit (one network)

    # ---- plumbing ----------------------------------------------------------------------------
    @property
    def stream(self):
        return torch.cuda.current_stream().cuda_stream if self.dev.type == "cuda" else None

    def _t(self, arr):
        return torch.from_numpy(np.ascontiguousarray(arr)).to(self.dev)

    def _zeros(self, *shape, dtype=torch.float32):
        return torch.zeros(*shape, dtype=dtype, device=self.dev)

    def _rows(self, params_list, ldp):
        th = np.zeros((1, len(params_list), ldp), np.float32)
        for n, p in enumerate(params_list):
            v = flat(p)
            th[0, n, :v.size] = v
        return self._t(th)

    def _host(self, t):
        if self.dev.type == "cuda":
            torch.cuda.synchronize()
        return t.detach().cpu().numpy()

    def _layer1(self, x, B, in_dim, theta, a1t, N, ldp, ldb):
        self.lib.rcmarl_layer1_forward(x.data_ptr(), B * in_dim, theta.data_ptr(), a1t.data_ptr(), 1, N, B, in_dim, HID,
                                       ldp, ldb, self.stream)

    # ---- forward passes ----------------------------------------------------------------------
    def value(self, params, x):
        """model(x) for a linear head of width 1 -> [B, 1]   (Keras __call__, agents/...:95-97,114)."""
        in_dim, out_dim, hid = dims_of(params)
        assert out_dim == 1
        x = as_rows(x)
        B = x.shape[0]
        ldp, ldb = pad64(flat(params).size), pad64(B)
        th, xd = self._rows([params], ldp), self._t(x)
        if hid != HID:
            out = self._zeros(1, 1, ldb)
            self._value_wide(xd, th, None, 0.0, out, B, in_dim, hid, ldp, ldb)
            return self._host(out)[0, 0, :B].reshape(B, 1).copy()
        a1t, out = self._zeros(1, HID, ldb), self._zeros(1, 1, ldb)
        self._layer1(xd, B, in_dim, th, a1t, 1, ldp, ldb)
        self.lib.rcmarl_mid_value(a1t.data_ptr(), th.data_ptr(), None, 0.0, out.data_ptr(), 1, 1, B, in_dim, HID, ldp, ldb,
                                  self.stream)
        return self._host(out)[0, 0, :B].reshape(B, 1).copy()

    def policy(self, params, x):
        """actor.predict(x) -> [B, n_actions] softmax probabilities (agents/...:215), row by row."""
        in_dim, A, hid = dims_of(params)
        x = as_rows(x)
        B = x.shape[0]
        ldp = pad64(flat(params).size)
        th = self._rows([params], ldp)
        out = np.zeros((B, A), np.float32)
        probs = self._zeros(1, 1, A)
        kernel = self.lib.rcmarl_policy_probs if hid == HID else self.lib.rcmarl_policy_probs_wide
        for b in range(B):
            xd = self._t(x[b:b + 1])
            kernel(xd.data_ptr(), th.data_ptr(), probs.data_ptr(), 1, 1, in_dim, hid, A, ldp, self.stream)
            out[b] = self._host(probs)[0, 0]
        return out

    # ---- nets of any other hidden width: the dense fp32 entry points of the engine's wide path, S = 1 ------------
    def _forward_wide(self, xd, B, theta, a1, a2, N, in_dim, hid, ldp, ldb):
        """layers 1 and 2 of N parameter rows over the rows of xd (engine._wide_forward's dense branch)"""
        o_b1, o_W2, o_b2, _ = offsets(in_dim, hid)
        L, st = self.lib, self.stream
        L.rcmarl_dense_forward(xd.data_ptr(), B * in_dim, 0, 1, in_dim, theta.data_ptr(), 0, o_b1, a1.data_ptr(), 1, N, B, in_dim,
                               hid, ldp, ldb, st)
        L.rcmarl_dense_forward(a1.data_ptr(), N * hid * ldb, hid * ldb, 0, ldb, theta.data_ptr(), o_W2, o_b2, a2.data_ptr(), 1, N,
                               B, hid, hid, ldp, ldb, st)

    def _value_wide(self, xd, theta, r_applied, gamma, out, B, in_dim, hid, ldp, ldb):
        """out[0][0][b] = model(x_b), or r_applied + gamma * that (engine._value_wide's dense branch)"""
        a1, a2 = self._zeros(1, hid, ldb), self._zeros(1, hid, ldb)
        self._forward_wide(xd, B, theta, a1, a2, 1, in_dim, hid, ldp, ldb)
        self.lib.rcmarl_wide_head_value(a2.data_ptr(), theta.data_ptr(), None if r_applied is None else r_applied.data_ptr(),
                                        float(gamma), out.data_ptr(), 1, 1, B, in_dim, hid, ldp, ldb, self.stream)

    def _sgd_steps_wide(self, msg, xd, y, B, in_dim, hid, ldp, ldb, lr, steps, loss):
        """`steps` full-batch SGD steps on the MSE loss over the B rows of xd, in place on the row `msg`
        (engine._local_fit_wide's dense branch); loss[0][0] = the first step's loss"""
        L, st = self.lib, self.stream
        _, o_W2, _, _ = offsets(in_dim, hid)
        a1, a2, dz1 = self._zeros(1, hid, ldb), self._zeros(1, hid, ldb), self._zeros(1, hid, ldb)
        dz3 = self._zeros(1, 1, ldb)
        grads = self._zeros(1, 1, L.rcmarl_wide_grad_size(hid))
        losspart = self._zeros(1, 1, (B + L.rcmarl_wide_rows_per_chunk() - 1) // L.rcmarl_wide_rows_per_chunk())
        for step in range(steps):
            self._forward_wide(xd, B, msg, a1, a2, 1, in_dim, hid, ldp, ldb)
            L.rcmarl_wide_head_fit(a2.data_ptr(), msg.data_ptr(), y.data_ptr(), dz3.data_ptr(), grads.data_ptr(),
                                   losspart.data_ptr(), 1, 1, B, in_dim, hid, ldp, ldb, st)                   # a2 now holds dz2
            L.rcmarl_dense_backward_data(a2.data_ptr(), msg.data_ptr(), o_W2, a1.data_ptr(), dz1.data_ptr(), 1, 1, B, hid, hid,
                                         ldp, ldb, st)
            L.rcmarl_wide_bias_grad(dz1.data_ptr(), grads.data_ptr(), 1, 1, B, hid, ldb, st)
            # every gradient above came from the pre-step weights; now the updates
            L.rcmarl_dense_backward_sgd(a1.data_ptr(), hid * ldb, hid * ldb, 0, ldb, a2.data_ptr(), msg.data_ptr(), o_W2, None, 1,
                                        1, B, hid, hid, ldp, ldb, float(lr), st)
            L.rcmarl_dense_backward_sgd(xd.data_ptr(), B * in_dim, 0, 1, in_dim, dz1.data_ptr(), msg.data_ptr(), 0, None, 1, 1, B,
                                        in_dim, hid, ldp, ldb, float(lr), st)
            L.rcmarl_wide_small_sgd(grads.data_ptr(), losspart.data_ptr(), msg.data_ptr(), None,
                                    loss.data_ptr() if step == 0 else None, 1, 1, B, in_dim, hid, ldp, float(lr), st)

    def _padded(self, values, B, ldb):
        row = np.zeros((1, 1, ldb), np.float32)
        row[0, 0, :B] = np.asarray(values, dtype=np.float32).reshape(B)
        return self._t(row)

    # ---- A5/A6: 5 full-batch SGD steps on a copy (critic.fit / TR.fit, agents/...:118,136) ----
    def fit_full_batch(self, params, x, r, lr, steps=5, bootstrap_x=None, gamma=0.0):
        """Returns (fitted weight list, first-step loss).  With ``bootstrap_x`` the target is
        r + gamma*model(bootstrap_x) computed once from the pre-fit weights (:114-115)."""
        in_dim, out_dim, hid = dims_of(params)
        assert out_dim == 1
        x = as_rows(x)
        B = x.shape[0]
        ldp, ldb = pad64(flat(params).size), pad64(B)
        L = self.lib
        th, xd = self._rows([params], ldp), self._t(x)
        msg = th.clone()
        if hid != HID:
            y = self._padded(r, B, ldb)
            if bootstrap_x is not None:
                tgt = self._zeros(1, 1, ldb)
                self._value_wide(self._t(as_rows(bootstrap_x)), th, y, gamma, tgt, B, in_dim, hid, ldp, ldb)
                y = tgt
            loss = self._zeros(1, 1)
            self._sgd_steps_wide(msg, xd, y, B, in_dim, hid, ldp, ldb, lr, steps, loss)
            return unflat(self._host(msg)[0, 0], in_dim, 1, hid), float(self._host(loss)[0, 0])
        a1t = self._zeros(1, HID, ldb)
        rr = np.zeros((1, 1, ldb), np.float32)
        rr[0, 0, :B] = np.asarray(r, dtype=np.float32).reshape(B)
        y = self._t(rr)
        if bootstrap_x is not None:
            nx = self._t(as_rows(bootstrap_x))
            self._layer1(nx, B, in_dim, th, a1t, 1, ldp, ldb)
            tgt = self._zeros(1, 1, ldb)
            L.rcmarl_mid_value(a1t.data_ptr(), th.data_ptr(), y.data_ptr(), float(gamma), tgt.data_ptr(), 1, 1, B, in_dim, HID,
                               ldp, ldb, self.stream)
            y = tgt
        nchunk = (B + L.rcmarl_rows_per_chunk() - 1) // L.rcmarl_rows_per_chunk()
        part = self._zeros(nchunk * L.rcmarl_fit_partial_size(HID))
        loss = self._zeros(1, 1)
        for st in range(steps):
            self._layer1(xd, B, in_dim, msg, a1t, 1, ldp, ldb)
            L.rcmarl_mid_fit(a1t.data_ptr(), msg.data_ptr(), y.data_ptr(), part.data_ptr(), 1, 1, B, in_dim, HID, ldp, ldb,
                             self.stream)
            L.rcmarl_small_sgd(part.data_ptr(), msg.data_ptr(), None, loss.data_ptr() if st == 0 else None, 1, 1, B, in_dim,
                               HID, ldp, float(lr), self.stream)
            L.rcmarl_layer1_backward_sgd(xd.data_ptr(), B * in_dim, a1t.data_ptr(), msg.data_ptr(), None, 1, 1, B, in_dim, HID,
                                         ldp, ldb, float(lr), self.stream)
        return unflat(self._host(msg)[0, 0], in_dim, 1), float(self._host(loss)[0, 0])

    # ---- A2: hidden-layer consensus (agents/...:142-166) ---------------------------------------
    def consensus_hidden(self, msgs, H):
        """msgs: list of d weight lists, msgs[0] = own message.  Returns the 4 aggregated hidden arrays."""
        in_dim, out_dim, hid = dims_of(msgs[0])
        d = len(msgs)
        P = flat(msgs[0]).size
        ldp = pad64(P)
        P_hid = P - (hid * out_dim + out_dim)
        msg = self._rows(msgs, ldp)
        theta = self._zeros(1, d, ldp)
        # row 0 = the agent (own message first); rows >= 1 are placeholders and are masked out by `coop`
        nbr = self._t(np.array([[(i + k) % d for k in range(d)] for i in range(d)], np.int32))
        coop = self._t(np.array([1] + [0] * (d - 1), np.int32))
        self.lib.rcmarl_consensus_params(msg.data_ptr(), theta.data_ptr(), nbr.data_ptr(), coop.data_ptr(), 1, d, ldp, P_hid,
                                         d, int(H), None, None, self.stream)
        return unflat(self._host(theta)[0, 0], in_dim, out_dim, hid)[:4]

    # ---- A3 (+A4 residual): consensus over estimates (agents/...:168-206) ----------------------
    def consensus_estimates(self, live, x, msgs, H):
        """live: the agent's current weight list (freshly aggregated hidden layers + own head).
        Returns agg [B, 1]."""
        in_dim, _, hid = dims_of(live)
        x = as_rows(x)
        B = x.shape[0]
        d = len(msgs)
        ldp, ldb = pad64(flat(live).size), pad64(B)
        L = self.lib
        theta = self._rows([live] + [live] * (d - 1), ldp)
        msg = self._rows(msgs, ldp)
        nbr = self._t(np.array([[(i + k) % d for k in range(d)] for i in range(d)], np.int32))
        coop = self._t(np.array([1] + [0] * (d - 1), np.int32))
        xd = self._t(x)
        if hid != HID:                                         # engine._consensus_wide; the head itself is left to projection_step
            a1, a2 = self._zeros(1, d * hid, ldb), self._zeros(1, d * hid, ldb)
            hmat, hb, est = self._zeros(1, d, d + 1, hid), self._zeros(1, d, d + 1), self._zeros(1, d, d + 1, ldb)
            ebuf, grads, agg = self._zeros(1, d, ldb), self._zeros(1, d, L.rcmarl_wide_grad_size(hid)), self._zeros(1, d, ldb)
            self._forward_wide(xd, B, theta, a1, a2, d, in_dim, hid, ldp, ldb)
            L.rcmarl_wide_consensus_head(a2.data_ptr(), theta.data_ptr(), msg.data_ptr(), nbr.data_ptr(), coop.data_ptr(), None,
                                         hmat.data_ptr(), hb.data_ptr(), est.data_ptr(), ebuf.data_ptr(), grads.data_ptr(),
                                         agg.data_ptr(), 1, d, B, in_dim, hid, ldp, ldb, d, int(H), self.stream)
            return self._host(agg)[0, 0, :B].reshape(B, 1).copy()
        a1t = self._zeros(1, d * HID, ldb)
        nchunk = (B + L.rcmarl_rows_per_chunk() - 1) // L.rcmarl_rows_per_chunk()
        part = self._zeros(d * nchunk * (HID + 1))
        agg = self._zeros(1, d, ldb)
        self._layer1(xd, B, in_dim, theta, a1t, d, ldp, ldb)
        L.rcmarl_consensus_head(a1t.data_ptr(), theta.data_ptr(), msg.data_ptr(), nbr.data_ptr(), coop.data_ptr(),
                                part.data_ptr(), agg.data_ptr(), 1, d, B, in_dim, HID, ldp, ldb, d, int(H), self.stream)
        return self._host(agg)[0, 0, :B].reshape(B, 1).copy()

    # ---- A4: projection ("team") update of the output layer (agents/...:60-84) -----------------
    def projection_step(self, live, x, agg):
        """Returns the new (W3, b3)."""
        in_dim, _, hid = dims_of(live)
        x = as_rows(x)
        B = x.shape[0]
        ldp, ldb = pad64(flat(live).size), pad64(B)
        L = self.lib
        theta, xd = self._rows([live], ldp), self._t(x)
        ag = np.zeros((1, 1, ldb), np.float32)
        ag[0, 0, :B] = np.asarray(agg, dtype=np.float32).reshape(B)
        agd = self._t(ag)
        coop = self._t(np.array([1], np.int32))
        if hid != HID:
            a1, a2 = self._zeros(1, hid, ldb), self._zeros(1, hid, ldb)
            ebuf, grads = self._zeros(1, 1, ldb), self._zeros(1, 1, L.rcmarl_wide_grad_size(hid))
            self._forward_wide(xd, B, theta, a1, a2, 1, in_dim, hid, ldp, ldb)
            L.rcmarl_wide_consensus_head(a2.data_ptr(), theta.data_ptr(), None, None, coop.data_ptr(), agd.data_ptr(), None, None,
                                         None, ebuf.data_ptr(), grads.data_ptr(), None, 1, 1, B, in_dim, hid, ldp, ldb, 1, 0,
                                         self.stream)
            L.rcmarl_wide_head_apply(grads.data_ptr(), theta.data_ptr(), coop.data_ptr(), 1, 1, B, in_dim, hid, ldp, self.stream)
            new = unflat(self._host(theta)[0, 0], in_dim, 1, hid)
            return new[4], new[5]
        a1t = self._zeros(1, HID, ldb)
        nchunk = (B + L.rcmarl_rows_per_chunk() - 1) // L.rcmarl_rows_per_chunk()
        part = self._zeros(nchunk * (HID + 1))
        self._layer1(xd, B, in_dim, theta, a1t, 1, ldp, ldb)
        L.rcmarl_projection_residual(a1t.data_ptr(), theta.data_ptr(), agd.data_ptr(), coop.data_ptr(), part.data_ptr(), 1, 1, B,
                                     in_dim, HID, ldp, ldb, self.stream)
        L.rcmarl_head_apply(part.data_ptr(), theta.data_ptr(), coop.data_ptr(), 1, 1, B, in_dim, HID, ldp, self.stream)
        new = unflat(self._host(theta)[0, 0], in_dim, 1)
        return new[4], new[5]

    # ---- A7: one Adam step of the actor (actor.train_on_batch, agents/...:99) -------------------
    def actor_step(self, params, adam, x, labels, weights, lr):
        """adam: dict(m=flat fp32, v=flat fp32, t=int), updated in place.  Returns (new weights, loss)."""
        in_dim, A, hid = dims_of(params)
        x = as_rows(x)
        B = x.shape[0]
        P = flat(params).size
        ldp, ldb = pad64(P), pad64(B)
        L = self.lib
        theta, xd = self._rows([params], ldp), self._t(x)
        mm, vv = np.zeros((1, 1, ldp), np.float32), np.zeros((1, 1, ldp), np.float32)
        mm[0, 0, :P], vv[0, 0, :P] = adam["m"], adam["v"]
        m, v = self._t(mm), self._t(vv)
        lab, wgt = np.zeros((1, 1, ldb), np.float32), np.zeros((1, 1, ldb), np.float32)
        lab[0, 0, :B] = np.asarray(labels, dtype=np.float32).reshape(B)
        wgt[0, 0, :B] = np.asarray(weights, dtype=np.float32).reshape(B)
        labd, wgtd = self._t(lab), self._t(wgt)
        loss = self._zeros(1, 1)
        adam["t"] += 1
        b1, b2, eps = 0.9, 0.999, 1e-7
        alpha = float(np.float32(lr * math.sqrt(1.0 - b2 ** adam["t"]) / (1.0 - b1 ** adam["t"])))
        omb1, omb2, epsf = float(np.float32(1 - b1)), float(np.float32(1 - b2)), float(np.float32(eps))
        if hid != HID:
            self._actor_step_wide(xd, theta, m, v, labd, wgtd, loss, B, in_dim, hid, A, ldp, ldb, (alpha, omb1, omb2, epsf))
            adam["m"], adam["v"] = self._host(m)[0, 0, :P].copy(), self._host(v)[0, 0, :P].copy()
            return unflat(self._host(theta)[0, 0], in_dim, A, hid), float(self._host(loss)[0, 0])
        a1t = self._zeros(1, HID, ldb)
        nchunk = (B + L.rcmarl_rows_per_chunk() - 1) // L.rcmarl_rows_per_chunk()
        part = self._zeros(nchunk * L.rcmarl_actor_partial_size(HID, A))
        self._layer1(xd, B, in_dim, theta, a1t, 1, ldp, ldb)
        L.rcmarl_mid_actor(a1t.data_ptr(), theta.data_ptr(), labd.data_ptr(), wgtd.data_ptr(), part.data_ptr(), 1, 1, B, in_dim,
                           HID, A, ldp, ldb, self.stream)
        L.rcmarl_small_adam(part.data_ptr(), theta.data_ptr(), m.data_ptr(), v.data_ptr(), None, loss.data_ptr(), 1, 1, B,
                            in_dim, HID, A, ldp, alpha, omb1, omb2, epsf, self.stream)
        L.rcmarl_layer1_backward_adam(xd.data_ptr(), B * in_dim, a1t.data_ptr(), theta.data_ptr(), m.data_ptr(), v.data_ptr(),
                                      None, 1, 1, B, in_dim, HID, ldp, ldb, alpha, omb1, omb2, epsf, self.stream)
        adam["m"], adam["v"] = self._host(m)[0, 0, :P].copy(), self._host(v)[0, 0, :P].copy()
        return unflat(self._host(theta)[0, 0], in_dim, A), float(self._host(loss)[0, 0])

    def _actor_step_wide(self, xd, theta, m, v, labd, wgtd, loss, B, in_dim, hid, A, ldp, ldb, adam):
        """the nine launches of engine._actor_step_wide on one parameter row: every gradient from the pre-step weights"""
        L, st = self.lib, self.stream
        o_b1, o_W2, o_b2, o_W3 = offsets(in_dim, hid)
        a1, a2, dz = self._zeros(1, hid, ldb), self._zeros(1, hid, ldb), self._zeros(1, hid, ldb)
        dz3 = self._zeros(1, A, ldb)
        losspart = self._zeros(1, 1, (B + L.rcmarl_wide_rows_per_chunk() - 1) // L.rcmarl_wide_rows_per_chunk())
        th, mp, vp = theta.data_ptr(), m.data_ptr(), v.data_ptr()
        adam = tuple(adam) + (st,)
        self._forward_wide(xd, B, theta, a1, a2, 1, in_dim, hid, ldp, ldb)
        L.rcmarl_wide_actor_head(a2.data_ptr(), th, labd.data_ptr(), wgtd.data_ptr(), ldb, dz3.data_ptr(), losspart.data_ptr(), 1, 1, B,
                                 in_dim, hid, A, ldp, ldb, st)
        L.rcmarl_dense_backward_data(dz3.data_ptr(), th, o_W3, a2.data_ptr(), dz.data_ptr(), 1, 1, B, hid, A, ldp, ldb, st)
        L.rcmarl_dense_backward_adam(a2.data_ptr(), hid * ldb, hid * ldb, 0, ldb, dz3.data_ptr(), th, mp, vp, o_W3, None, 1, 1, B, hid,
                                     A, ldp, ldb, *adam)
        L.rcmarl_dense_backward_data(dz.data_ptr(), th, o_W2, a1.data_ptr(), a2.data_ptr(), 1, 1, B, hid, hid, ldp, ldb, st)
        L.rcmarl_dense_backward_adam(a1.data_ptr(), hid * ldb, hid * ldb, 0, ldb, dz.data_ptr(), th, mp, vp, o_W2, None, 1, 1, B, hid,
                                     hid, ldp, ldb, *adam)
        L.rcmarl_dense_backward_adam(xd.data_ptr(), B * in_dim, 0, 1, in_dim, a2.data_ptr(), th, mp, vp, 0, None, 1, 1, B, in_dim, hid,
                                     ldp, ldb, *adam)
        L.rcmarl_wide_actor_small_adam(a2.data_ptr(), dz.data_ptr(), dz3.data_ptr(), losspart.data_ptr(), th, mp, vp, None,
                                       loss.data_ptr(), 1, 1, B, in_dim, hid, A, ldp, ldb, *adam)

    # ---- X1: the adversaries' mini-batch fits (agents/adversarial_CAC_agents.py) ---------------
    def shuffle_perms(self, seed, call, epochs, B):
        """[epochs][B] int32 permutations of the call-th mini-batch fit (csrc/shuffle.hip)."""
        seeds = self._t(np.asarray([int(seed) & 0xFFFFFFFFFFFFFFFF], dtype=np.uint64).view(np.int64))
        calls = self._t(np.asarray([int(call)], np.int32))
        out = self._zeros(1, 1, int(epochs), int(B), dtype=torch.int32)
        self.lib.rcmarl_shuffle_perms(seeds.data_ptr(), calls.data_ptr(), 1, int(epochs), int(B), out.data_ptr(), 1, self.stream)
        return self._host(out)[0, 0]

    def minibatch_fit(self, params, x, y, lr, batch_size=32, epochs=10, perms=None):
        in_dim, out_dim, hid = dims_of(params)
        assert out_dim == 1
        x = as_rows(x)
        B = x.shape[0]
        ldp, ldb = pad64(flat(params).size), pad64(B)
        theta, xd = self._rows([params], ldp), self._t(x)
        yy = np.zeros((1, 1, ldb), np.float32)
        yy[0, 0, :B] = np.asarray(y, dtype=np.float32).reshape(B)
        yd = self._t(yy)
        agents = self._t(np.array([0], np.int32))
        pd = None if perms is None else self._t(np.asarray(perms, np.int32).reshape(1, 1, epochs, B))
        loss = self._zeros(1, 1)
        if hid != HID:
            L = self.lib
            chain = next((getattr(L, name) for name in ("rcmarl_minibatch_fit_wide", "rcmarl_minibatch_fit_wide2")
                          if getattr(L, name + "_supported")(in_dim, hid, int(batch_size)) == 1), None)
            if chain is not None:                       # the whole fit in one launch, one workgroup
                jobs = (capi.MbJob * 1)(capi.MbJob(xd.data_ptr(), B * in_dim, theta.data_ptr(), agents.data_ptr(), 1, in_dim, ldp, 0,
                                                   yd.data_ptr(), None if pd is None else pd.data_ptr(), loss.data_ptr(), None))
                chain(jobs, (C.c_int * 1)(hid), 1, 1, 1, B, ldb, int(batch_size), int(epochs), float(lr), self.stream)
                return unflat(self._host(theta)[0, 0], in_dim, 1, hid), float(self._host(loss)[0, 0])
            # no kernel holds a mini-batch of this net in LDS: one full-batch-style SGD step per mini-batch on the gathered rows
            yh, bs, tot = yy[0, 0, :B], min(int(batch_size), B), 0.0
            for ep in range(int(epochs)):
                order = np.arange(B) if perms is None else np.asarray(perms, np.int64).reshape(epochs, B)[ep]
                for lo in range(0, B, bs):
                    idx = order[lo:lo + bs]
                    nb = len(idx)
                    self._sgd_steps_wide(theta, self._t(x[idx]), self._padded(yh[idx], nb, pad64(nb)), nb, in_dim, hid, ldp,
                                         pad64(nb), lr, 1, loss)
                    if ep == 0:                         # Keras History: the mean of the batch losses weighted by batch length
                        tot += float(self._host(loss)[0, 0]) * nb
            return unflat(self._host(theta)[0, 0], in_dim, 1, hid), float(np.float32(tot / B))
        self.lib.rcmarl_minibatch_fit(xd.data_ptr(), B * in_dim, theta.data_ptr(), agents.data_ptr(), 1, yd.data_ptr(),
                                      None if pd is None else pd.data_ptr(), 1, 1, B, in_dim, HID, ldp, ldb, int(batch_size),
                                      int(epochs), float(lr), loss.data_ptr(), self._mb_flags.data_ptr(), self.stream)
        return unflat(self._host(theta)[0, 0], in_dim, 1), float(self._host(loss)[0, 0])

    def minibatch_actor(self, params, adam, x, labels, weights, lr, batch_size=200, epochs=1, perms=None):
        in_dim, A, hid = dims_of(params)
        x = as_rows(x)
        B = x.shape[0]
        P = flat(params).size
        ldp, ldb = pad64(P), pad64(B)
        if hid != HID and self.lib.rcmarl_minibatch_actor_wide_supported(in_dim, hid, A, int(batch_size)) != 1:
            # no kernel for this shape: one wide Adam step per mini-batch on the gathered rows
            lab, wgt = np.asarray(labels, np.float32).reshape(B), np.asarray(weights, np.float32).reshape(B)
            bs, tot = min(int(batch_size), B), 0.0
            for ep in range(int(epochs)):
                order = np.arange(B) if perms is None else np.asarray(perms, np.int64).reshape(epochs, B)[ep]
                for lo in range(0, B, bs):
                    idx = order[lo:lo + bs]
                    params, l = self.actor_step(params, adam, x[idx], lab[idx], wgt[idx], lr)
                    if ep == 0:
                        tot += l * len(idx)
            return params, float(np.float32(tot / B))
        theta, xd = self._rows([params], ldp), self._t(x)
        mm, vv = np.zeros((1, 1, ldp), np.float32), np.zeros((1, 1, ldp), np.float32)
        mm[0, 0, :P], vv[0, 0, :P] = adam["m"], adam["v"]
        m, v = self._t(mm), self._t(vv)
        lab, wgt = np.zeros((1, 1, ldb), np.float32), np.zeros((1, 1, ldb), np.float32)
        lab[0, 0, :B] = np.asarray(labels, dtype=np.float32).reshape(B)
        wgt[0, 0, :B] = np.asarray(weights, dtype=np.float32).reshape(B)
        labd, wgtd = self._t(lab), self._t(wgt)
        agents = self._t(np.array([0], np.int32))
        pd = None if perms is None else self._t(np.asarray(perms, np.int32).reshape(1, 1, epochs, B))
        loss = self._zeros(1, 1)
        if hid != HID:                                  # the whole fit in one launch, one workgroup (csrc/minibatch_actor_wide.hip)
            grad = self._zeros(1, 1, ldp)
            self.lib.rcmarl_minibatch_actor_wide(xd.data_ptr(), B * in_dim, theta.data_ptr(), m.data_ptr(), v.data_ptr(),
                                                 grad.data_ptr(), agents.data_ptr(), 1, labd.data_ptr(), wgtd.data_ptr(),
                                                 None if pd is None else pd.data_ptr(), 1, 1, B, in_dim, hid, A, ldp, ldb,
                                                 int(batch_size), int(epochs), float(lr), 0.9, 0.999, 1e-7, int(adam["t"]),
                                                 loss.data_ptr(), self.stream)
            bs = min(int(batch_size), B)
            adam["t"] += epochs * ((B + bs - 1) // bs)
            adam["m"], adam["v"] = self._host(m)[0, 0, :P].copy(), self._host(v)[0, 0, :P].copy()
            return unflat(self._host(theta)[0, 0], in_dim, A, hid), float(self._host(loss)[0, 0])
        self.lib.rcmarl_minibatch_actor(xd.data_ptr(), B * in_dim, theta.data_ptr(), m.data_ptr(), v.data_ptr(),
                                        agents.data_ptr(), 1, labd.data_ptr(), wgtd.data_ptr(),
                                        None if pd is None else pd.data_ptr(), 1, 1, B, in_dim, HID, A, ldp, ldb,
                                        int(batch_size), int(epochs), float(lr), 0.9, 0.999, 1e-7, int(adam["t"]),
                                        loss.data_ptr(), self.stream)
        bs = min(int(batch_size), B)
        adam["t"] += epochs * ((B + bs - 1) // bs)
        adam["m"], adam["v"] = self._host(m)[0, 0, :P].copy(), self._host(v)[0, 0, :P].copy()
        return unflat(self._host(theta)[0, 0], in_dim, A), float(self._host(loss)[0, 0])
