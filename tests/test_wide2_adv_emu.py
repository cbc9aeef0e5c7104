"""Adversaries beside critic-family nets of 385 .. 576 units on the hipemu (CPU) build of the kernel sources:
rcmarl_minibatch_fit_wide2 against oracle/mlp_np.fit_mse, its determinism, query and refusals.  The same checks run on the MI355X in
test_wide2_adv_gpu.py (tests/wide2_adv_checks.py holds them), and three more run there only, because the emulation takes minutes
per case at these widths: the 576-unit shape with four input chunks, the multi-job form, and the engine against oracle.train with
the routing counted."""
import pytest

import wide2_adv_checks as W2
from emu_util import emu_lib
from test_kernels_emu import EmuBackend


@pytest.fixture(scope="module")
def bk():
    return EmuBackend()


@pytest.mark.parametrize("name", ["first_unserved", "cfg5_width"])
def test_wide2_minibatch_fit_against_the_oracle(bk, name):
    W2.check_fit(bk, name)


def test_wide2_minibatch_fit_in_natural_row_order(bk):
    W2.check_fit(bk, "first_unserved_natural", shuffle=False)


def test_wide2_minibatch_fit_is_deterministic(bk):
    W2.check_determinism(bk)


def test_query_and_argument_validation():
    W2.check_query(emu_lib())
    W2.check_argument_validation(emu_lib())
