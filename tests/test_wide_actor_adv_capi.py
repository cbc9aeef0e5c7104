"""The adversaries' actor fit for 385 .. 576 units in the gfx950 build: declared in include/rcmarl.h, bound in capi.py, exported by
the library, answering the query and validating its arguments before it touches the HIP runtime (no GPU needed).  The ABI number
stays 4: additions only."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("rcmarl_minibatch_actor_wide2_supported", "rcmarl_minibatch_actor_wide2")


def test_wide2_actor_fit_entry_points_are_declared_bound_and_exported():
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
    import wide_actor_adv_checks as WAA
    import wide_single_checks as WS
    from rcmarl_amd import build, capi
    lib = capi.CLib(build.build_hip())
    WAA.check_query(lib)
    WAA.check_argument_validation(lib)
    WS.check_query(lib)                                # what the existing entry point serves does not change
    WS.check_argument_validation(lib)
