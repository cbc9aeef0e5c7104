#!/usr/bin/env python
"""rcmarl_consensus_head of two builds of the library on the same inputs, bit for bit, in both operand forms (on the GPU):

    python tools/diag_head_two_builds.py OTHER/librcmarl_hip.so

OTHER is typically a build of the parent commit: the consensus-head kernels gained an optional agent list and an optional
neighbour-row offset table for irregular graphs, and the existing entry point (which passes null for both) must give the same bits
as before.  An older build lacks newer symbols: only the symbols it exports are bound.  Exit status 0 = identical.
"""
import ctypes
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from rcmarl_amd import capi  # noqa: E402
import ragged_checks as RC  # noqa: E402
from test_kernels_gpu import GpuBackend  # noqa: E402


def load_other(path):
    capi._preload_hip_runtime()
    have = ctypes.CDLL(path)
    full = dict(capi.SIGNATURES)
    try:
        for name in list(capi.SIGNATURES):
            if not hasattr(have, name):
                del capi.SIGNATURES[name]
        return capi.CLib(path)
    finally:
        capi.SIGNATURES.clear()
        capi.SIGNATURES.update(full)


if __name__ == "__main__":
    new, old = GpuBackend(), GpuBackend()
    old.lib = load_other(sys.argv[1])
    ok = True
    for form in (3, 0):
        for bk in (new, old):
            bk.lib.rcmarl_lattice_set_f16_mode(form)
        for k, ((ta, ga), (tb, gb)) in enumerate(zip(RC.uniform_head_outputs(new), RC.uniform_head_outputs(old))):
            same = np.array_equal(ta.view(np.uint32), tb.view(np.uint32)) and np.array_equal(ga.view(np.uint32), gb.view(np.uint32))
            ok &= same
            print("operand form %d, case %d: rcmarl_consensus_head of the two builds bit-identical: %s" % (form, k, same))
    print("HEAD_TWO_BUILDS_IDENTICAL" if ok else "HEAD_TWO_BUILDS_DIFFER")
    sys.exit(0 if ok else 1)
