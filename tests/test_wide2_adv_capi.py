"""The mini-batch fit entry points for 385 .. 576 units in the gfx950 build: declared in include/rcmarl.h, bound in capi.py, exported
by the library, answering the query and validating their arguments before they touch the HIP runtime (no GPU needed).  The ABI
number stays 4: additions only."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("rcmarl_minibatch_fit_wide2_supported", "rcmarl_minibatch_fit_wide2")


def test_wide2_minibatch_fit_entry_points_are_declared_bound_and_exported():
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
    import wide2_adv_checks as W2
    from rcmarl_amd import build, capi
    lib = capi.CLib(build.build_hip())
    W2.check_query(lib)
    W2.check_argument_validation(lib)
