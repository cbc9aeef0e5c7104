"""The wide actor fit's entry points in the gfx950 build: declared in include/rcmarl.h, bound in capi.py, exported by the library,
answering the query and validating their arguments before they touch the HIP runtime (no GPU needed).  The ABI number stays 4:
additions only."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("rcmarl_minibatch_actor_wide_supported", "rcmarl_minibatch_actor_wide")


def test_wide_actor_fit_entry_points_are_declared_bound_and_exported():
    from rcmarl_amd import build, capi
    path = build.build_hip()
    lib = capi.CLib(path)
    assert lib.rcmarl_abi_version() == 4
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "rcmarl.h")).read(), flags=re.S)
    exported = set(re.findall(r"\bT (rcmarl_\w+)", subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True).stdout))
    for name in NEW:
        assert re.search(r"\bint\s+%s\s*\(" % name, txt), name
        assert name in capi.SIGNATURES and name in exported, name


def test_query_and_argument_validation_in_the_product_library():
    import wide_single_checks as WS
    from rcmarl_amd import build, capi
    lib = capi.CLib(build.build_hip())
    WS.check_query(lib)
    WS.check_argument_validation(lib)


def test_dims_of_reads_the_width_off_the_weights():
    import numpy as np
    import pytest
    from oracle import mlp_np as M
    from rcmarl_amd import capi, single
    rng = np.random.default_rng(0)
    for hid in (20, 24, 600):
        p = M.init_mlp(rng, 10, hid, 5)
        assert single.dims_of(p) == (10, 5, hid)
        assert [a.shape for a in single.unflat(single.flat(p), 10, 5, hid)] == single.shapes(10, 5, hid) == [np.shape(a) for a in p]
    p = M.init_mlp(rng, 10, 24, 1)
    p[2] = np.zeros((24, 32), np.float32)              # two hidden layers of different widths
    with pytest.raises(capi.RcmarlError, match="equal width"):
        single.dims_of(p)
