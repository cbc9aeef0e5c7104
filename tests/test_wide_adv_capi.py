"""The wide mini-batch fit entry points in the gfx950 build: declared in include/rcmarl.h, bound in capi.py, exported by the library,
answering the query and validating their arguments before they touch the HIP runtime (no GPU needed).  The ABI number stays 4:
additions only."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("rcmarl_minibatch_fit_wide_supported", "rcmarl_minibatch_fit_wide")


def test_wide_minibatch_fit_entry_points_are_declared_bound_and_exported():
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
    import wide_adv_checks as WA
    from rcmarl_amd import build, capi
    lib = capi.CLib(build.build_hip())
    WA.check_query(lib)
    WA.check_argument_validation(lib)
