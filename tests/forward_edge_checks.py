"""The last row tile of the layer-1 lattice forward (rcmarl_layer1_forward_lattice): wavefronts whose replay rows all lie beyond B do no
matrix work.  Shared by the hipemu (CPU) and GPU tests.  An output element depends on its own replay row only, so the yardstick is
the same call with B = 256 (no row beyond B in the tile, every wavefront at work) on the same packed inputs: rows < B word for word,
rows >= B untouched."""
import numpy as np

import kernel_checks as KC
from kernel_checks import HID, geom, pad64

S, N, IN_DIM, ROWS = 2, 7, 300, 256
# B = 70: rows 128.. (four-wavefront form: wn = 1) resp. 128.. and 192.. (eight: wn = 2, 3) belong to wavefronts without a live row, and
# the live ones end inside a 32-row block; 200: the last wavefront of either form is live but partial -- nobody may be skipped; 192: the
# boundary itself -- the eight-wavefront form's wn = 3 starts at row 192 == B.
EDGES = (70, 200, 192)
SENTINEL = np.float32(-12345.5)


def check_forward_edge(bk, B):
    assert B < ROWS
    L = bk.lib
    rng = np.random.default_rng(70 + B)
    P, _ = geom(IN_DIM, 1)
    ldp, ldb = pad64(P), pad64(ROWS)
    theta = rng.uniform(-0.3, 0.3, size=(S, N, ldp)).astype(np.float32)
    alpha = rng.uniform(0.2, 1.5, size=IN_DIM).astype(np.float32)
    K = rng.integers(-31, 32, size=(S, ROWS, IN_DIM))
    x = (alpha.astype(np.float64) * K).astype(np.float32)          # ordinary data in EVERY one of the 256 rows, those >= B included
    lb = KC.LatticeBuffers(bk, S, N, IN_DIM, ROWS)
    g = lb.g
    d_th, d_al = bk.dev(theta), bk.dev(alpha)
    KC._encode(bk, lb, bk.dev(x), ROWS * IN_DIM, d_al, S, ROWS, IN_DIM, with_t=False)
    assert bk.host(lb.flag)[0] == 0
    L.rcmarl_w1_split(bk.ptr(d_th), bk.ptr(d_al), bk.ptr(lb.wp), S, N, IN_DIM, HID, ldp, g.wp[0], g.wp[1], bk.stream)
    out = {}
    for b in (B, ROWS):
        d_a1 = bk.dev(np.full((S, N * HID, ldb), SENTINEL, np.float32))
        L.rcmarl_layer1_forward_lattice(bk.ptr(lb.kp), g.kp[0], g.kp[1], bk.ptr(lb.wp), g.wp[0], g.wp[1], bk.ptr(d_th), bk.ptr(d_a1),
                                        S, N, b, IN_DIM, HID, ldp, ldb, bk.stream)
        out[b] = bk.host(d_a1).reshape(S, N * HID, ldb).copy()
    full, part = out[ROWS], out[B]
    assert np.isfinite(full).all() and not (full == SENTINEL).any()             # the yardstick wrote every row
    assert len(np.unique(full[:, :, B:])) > 100                                 # ... with ordinary values beyond B too
    np.testing.assert_array_equal(part[:, :, :B].view(np.uint32), full[:, :, :B].view(np.uint32))
    np.testing.assert_array_equal(part[:, :, B:], SENTINEL)
