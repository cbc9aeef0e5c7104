"""The local fit that starts from the live net, on the hipemu (CPU) build of the kernel sources: the small step with a separate
source against the in-place one, bit for bit, and the engine switch.  Same checks on the GPU: test_fit_from_live_gpu.py."""
import pytest

import fit_from_live_checks as FL
from emu_util import emu_lib
from test_kernels_emu import EmuBackend


@pytest.fixture(scope="module")
def bk():
    return EmuBackend()


def test_small_step_with_a_separate_source_equals_the_in_place_step(bk):
    FL.check_small_sgd_from(bk)


def test_config_switch():
    FL.check_config_switch()


def test_engine_results_and_launches_with_fit_from_live_on_and_off():
    """The all-cooperative team (the rule holds).  A 16-agent block costs the emulation about a minute, so the runs in which the rule
    does not hold (a Greedy agent, W1 strided between the steps) and the run with the first epoch's TD target as it was are on the GPU
    only (test_fit_from_live_gpu.py): the routing is host code, the same on both."""
    FL.check_engine_live_equals_copy("cpu", emu_lib())
