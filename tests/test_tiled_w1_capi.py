"""The C ABI of the tiled W1 scratch: size query, argument validation and exports.  Host-only calls on the gfx950 build (no GPU)."""
import pytest

import tiled_w1_checks as TC


@pytest.fixture(scope="module")
def lib():
    from rcmarl_amd import build, capi
    return capi.CLib(build.build_hip())


def test_size_query(lib):
    TC.check_size_query(lib)


def test_bad_tiled_calls_are_argument_errors_before_the_hip_runtime_is_touched(lib):
    TC.check_arg_errors(lib)


def test_exports_and_binding_table(lib):
    TC.check_exports(lib.path)
    assert lib.rcmarl_abi_version() == 4
