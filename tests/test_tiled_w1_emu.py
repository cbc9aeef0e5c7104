"""W1 in accumulator-tile order between the SGD steps of a local fit, on the hipemu (CPU) build of the kernel sources: the tiled
roles of the layer-1 backward GEMM against the strided entry point, bit for bit, and the engine switch.  Same checks on the GPU:
test_tiled_w1_gpu.py."""
import pytest

import tiled_w1_checks as TC
from emu_util import emu_lib
from test_kernels_emu import EmuBackend


@pytest.fixture(scope="module")
def bk():
    return EmuBackend()


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


def test_engine_weights_are_bit_identical_with_w1_tiled_on_and_off():
    """The engine switch with one Greedy agent (a masked row in every fit).  A 16-agent block costs the emulation the better part of a
    minute, so the all-cooperative run and the wide / chain / one-step routing run on the GPU only (test_tiled_w1_gpu.py): the routing is
    host code, the same on both."""
    TC.check_engine_tiled_equals_strided("cpu", emu_lib(), ["Cooperative"] * 7 + ["Greedy"] + ["Cooperative"] * 8)
