"""W1 in accumulator-tile order between the SGD steps of a local fit, on a real MI355X through the product library: the tiled roles
of the layer-1 backward GEMM against the strided entry point, bit for bit, and the engine switch."""
import pytest

import tiled_w1_checks as TC
from test_kernels_gpu import GpuBackend

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def bk():
    return GpuBackend()


@pytest.mark.parametrize("w8", ["0", "1"])
@pytest.mark.parametrize("mode", [3, 0])
@pytest.mark.parametrize("shape", TC.SHAPES)
def test_five_step_fit_through_the_tiled_roles_is_bit_identical(bk, shape, mode, w8, monkeypatch, lattice_form):
    lattice_form(bk, mode)
    monkeypatch.setenv("RCMARL_LAT_W8", w8)
    TC.check_tiled_sequence(bk, *shape, steps=5)


@pytest.mark.parametrize("shape", TC.SHAPES)
def test_two_step_fit_strided_to_tiled_to_strided(bk, shape):
    TC.check_tiled_sequence(bk, *shape, steps=2)


@pytest.mark.parametrize("labels", [["Cooperative"] * 16, ["Cooperative"] * 7 + ["Greedy"] + ["Cooperative"] * 8])
def test_engine_weights_are_bit_identical_with_w1_tiled_on_and_off(labels):
    TC.check_engine_tiled_equals_strided("cuda", None, labels)


def test_engine_wide_chain_and_one_step_fits_stay_on_the_strided_entry_point(monkeypatch):
    TC.check_engine_other_paths_stay_strided("cuda", None, monkeypatch)
