#!/usr/bin/env python
"""The 20-unit rollout and actor-step kernels of two builds of the library on the same inputs, bit for bit (on the GPU):

    python tools/diag_rollout_two_builds.py OTHER/librcmarl_hip.so

OTHER is typically a build of the parent commit.  The draw / transition / replay-append tails of k_rollout_step and k_rollout_step_ep
became device functions shared with the wide-actor kernels, and the Adam arithmetic of rcmarl_small_adam / rcmarl_layer1_backward_adam
became rc_adam_apply (rcmarl_common.h): the existing entry points must give the same bits as before.  Compared: every replay tensor,
position, state vector and float64 return after ep_len steps of rcmarl_rollout_step_episodes (E = 50 and E = 70: two lane blocks, a
ragged one) and of rcmarl_rollout_step; theta, adam_m, adam_v and the loss after two actor steps (rcmarl_mid_actor, rcmarl_small_adam,
rcmarl_layer1_backward_adam).  An older build lacks newer symbols: only the symbols it exports are bound.  Exit status 0 = identical.
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from rcmarl_amd import capi  # noqa: E402
from diag_head_two_builds import load_other  # noqa: E402

HID, A = 20, 5


def pad64(n):
    return (n + 63) // 64 * 64


def rollout_outputs(L, S, N, E, ep_len, nrow=7):
    st = torch.cuda.current_stream().cuda_stream
    g = torch.Generator(device="cpu").manual_seed(S * 100 + N + E)
    in_dim, EP = 2 * N, pad64(E)
    P = in_dim * HID + HID + HID * HID + HID + HID * A + A
    ldp = pad64(P)
    theta = (torch.rand(S, N, ldp, generator=g) - 0.5).cuda()
    goal = torch.randint(0, 5, (S, N, 2), generator=g, dtype=torch.int32).cuda()
    seeds = torch.arange(11, 11 + S, dtype=torch.int64).cuda()
    mean, std = (nrow - 1) / 2.0, float(np.std(np.arange(nrow)))
    scale = torch.tensor([mean, mean, std, std], dtype=torch.float64).cuda()
    cap = E * ep_len + 4
    out = []
    # episode-parallel
    rp = [torch.zeros(S, cap, w * N).cuda() for w in (2, 2, 3, 1, 1)]
    posT = [torch.zeros(S, N, 2, EP, dtype=torch.int32).cuda() for _ in range(2)]
    xsT = [torch.zeros(S, 2 * N, EP).cuda() for _ in range(2)]
    retT = torch.zeros(S, N, EP, dtype=torch.float64).cuda()
    L.rcmarl_env_reset_episodes(None, seeds.data_ptr(), nrow, nrow, scale.data_ptr(), 3, posT[0].data_ptr(), xsT[0].data_ptr(),
                                retT.data_ptr(), S, N, E, EP, st)
    cur = 0
    for j in range(ep_len):
        L.rcmarl_rollout_step_episodes(xsT[cur].data_ptr(), posT[cur].data_ptr(), goal.data_ptr(), theta.data_ptr(), seeds.data_ptr(), nrow,
                                       nrow, scale.data_ptr(), *[t.data_ptr() for t in rp], cap, 2, ep_len, posT[1 - cur].data_ptr(),
                                       xsT[1 - cur].data_ptr(), retT.data_ptr(), 0.9 ** j, 3, j, 0.1, S, N, E, EP, HID, A, ldp, st)
        cur = 1 - cur
    out += rp + posT + xsT + [retT]
    # sequential
    rq = [torch.zeros(S, ep_len, w * N).cuda() for w in (2, 2, 3, 1, 1)]
    pos = [torch.zeros(S, N, 2, dtype=torch.int32).cuda() for _ in range(2)]
    xs = [torch.zeros(S, 2 * N).cuda() for _ in range(2)]
    ret = torch.zeros(S, N, dtype=torch.float64).cuda()
    act = torch.zeros(S, N, dtype=torch.int32).cuda()
    L.rcmarl_env_reset(None, seeds.data_ptr(), nrow, nrow, scale.data_ptr(), 5, pos[0].data_ptr(), xs[0].data_ptr(), ret.data_ptr(), S, N, st)
    cur = 0
    for j in range(ep_len):
        L.rcmarl_rollout_step(xs[cur].data_ptr(), pos[cur].data_ptr(), goal.data_ptr(), theta.data_ptr(), seeds.data_ptr(), nrow, nrow,
                              scale.data_ptr(), *[t.data_ptr() for t in rq], ep_len, j, pos[1 - cur].data_ptr(), xs[1 - cur].data_ptr(),
                              ret.data_ptr(), 0.9 ** j, 5, j, 0.1, S, N, HID, A, ldp, act.data_ptr(), st)
        cur = 1 - cur
    out += rq + pos + xs + [ret, act]
    torch.cuda.synchronize()
    return [t.cpu().numpy() for t in out]


def actor_outputs(L, S, N, B):
    st = torch.cuda.current_stream().cuda_stream
    g = torch.Generator(device="cpu").manual_seed(S + N + B)
    in_dim = 2 * N
    P = in_dim * HID + HID + HID * HID + HID + HID * A + A
    ldp, ldb = pad64(P), pad64(B)
    theta = (torch.rand(S, N, ldp, generator=g) - 0.5).cuda()
    x = torch.randn(S, B, in_dim, generator=g).cuda()
    act = torch.randint(0, A, (S, N, ldb), generator=g).float().cuda()
    delta = torch.randn(S, N, ldb, generator=g).cuda()
    mask = torch.ones(N, dtype=torch.int32).cuda()
    m, v = torch.zeros_like(theta), torch.zeros_like(theta)
    a1 = torch.zeros(S, N * HID, ldb).cuda()
    part = torch.zeros(S * N * ((B + 255) // 256) * L.rcmarl_actor_partial_size(HID, A)).cuda()
    loss = torch.zeros(S, N).cuda()
    for t in (1, 2):
        alpha = float(np.float32(0.002 * np.sqrt(1.0 - 0.999 ** t) / (1.0 - 0.9 ** t)))
        ad = (alpha, float(np.float32(0.1)), float(np.float32(0.001)), float(np.float32(1e-7)), st)
        L.rcmarl_layer1_forward(x.data_ptr(), B * in_dim, theta.data_ptr(), a1.data_ptr(), S, N, B, in_dim, HID, ldp, ldb, st)
        L.rcmarl_mid_actor(a1.data_ptr(), theta.data_ptr(), act.data_ptr(), delta.data_ptr(), part.data_ptr(), S, N, B, in_dim, HID, A,
                           ldp, ldb, st)
        L.rcmarl_small_adam(part.data_ptr(), theta.data_ptr(), m.data_ptr(), v.data_ptr(), mask.data_ptr(), loss.data_ptr(), S, N, B,
                            in_dim, HID, A, ldp, *ad)
        L.rcmarl_layer1_backward_adam(x.data_ptr(), B * in_dim, a1.data_ptr(), theta.data_ptr(), m.data_ptr(), v.data_ptr(),
                                      mask.data_ptr(), S, N, B, in_dim, HID, ldp, ldb, *ad)
    torch.cuda.synchronize()
    return [t.cpu().numpy() for t in (theta, m, v, loss)]


def same_bits(a, b):
    return all(x.shape == y.shape and np.array_equal(x.view(np.uint8), y.view(np.uint8)) for x, y in zip(a, b))


if __name__ == "__main__":
    new, old = capi.load(), load_other(sys.argv[1])
    ok = True
    for S, N, E, ep_len in ((2, 5, 50, 4), (1, 70, 70, 3)):
        same = same_bits(rollout_outputs(new, S, N, E, ep_len), rollout_outputs(old, S, N, E, ep_len))
        ok &= same
        print("rollout S=%d N=%d E=%d ep_len=%d: rcmarl_rollout_step_episodes / rcmarl_rollout_step of the two builds bit-identical: %s"
              % (S, N, E, ep_len, same))
    for S, N, B in ((2, 5, 100), (1, 40, 1000)):          # (the second: in_dim 80 -> the layer-1 backward's fast kernel where it applies)
        same = same_bits(actor_outputs(new, S, N, B), actor_outputs(old, S, N, B))
        ok &= same
        print("actor step S=%d N=%d B=%d: theta, adam_m, adam_v, loss of the two builds bit-identical: %s" % (S, N, B, same))
    print("ROLLOUT_TWO_BUILDS_IDENTICAL" if ok else "ROLLOUT_TWO_BUILDS_DIFFER")
    sys.exit(0 if ok else 1)
