"""The C ABI of the small step with a separate source: argument validation and exports.  Host-only calls on the gfx950 build (no GPU)."""
import pytest

import fit_from_live_checks as FL


@pytest.fixture(scope="module")
def lib():
    from rcmarl_amd import build, capi
    return capi.CLib(build.build_hip())


def test_bad_calls_are_argument_errors_before_the_hip_runtime_is_touched(lib):
    FL.check_arg_errors(lib)


def test_exports_and_binding_table(lib):
    FL.check_exports(lib.path)
    assert lib.rcmarl_abi_version() == 4
