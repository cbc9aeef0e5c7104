"""Adversaries beside critic-family nets of 385 .. 576 units on a real MI355X through the product library: the checks of
test_wide2_adv_emu.py (tests/wide2_adv_checks.py), and what the emulation is too slow for: the 576-unit shape with four input chunks,
the multi-job form, and the engine against oracle.train with the routing counted on the forced launch, on the forced loop and
under the crossover constant."""
import pytest

import wide2_adv_checks as W2
from test_kernels_gpu import GpuBackend

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def bk():
    return GpuBackend()


@pytest.mark.parametrize("name", ["first_unserved", "cfg5_width", "widest_chunks"])
def test_wide2_minibatch_fit_against_the_oracle(bk, name):
    W2.check_fit(bk, name)


def test_wide2_minibatch_fit_in_natural_row_order(bk):
    W2.check_fit(bk, "first_unserved_natural", shuffle=False)


def test_wide2_minibatch_fit_is_deterministic(bk):
    W2.check_determinism(bk)


def test_jobs_in_one_launch_equal_single_job_calls(bk):
    W2.check_multi_job(bk)


def test_query_and_argument_validation(bk):
    W2.check_query(bk.lib)
    W2.check_argument_validation(bk.lib)


@pytest.mark.parametrize("on", [False, True], ids=["loop", "launch"])
def test_engine_wide2_critic_beside_a_20_unit_team_reward_net(bk, on):
    W2.check_engine_narrow_tr("cuda", bk.lib, on)


@pytest.mark.parametrize("on", [False, True], ids=["loop", "launch"])
def test_engine_three_wide2_jobs_in_one_call(bk, on):
    W2.check_engine_both_wide2("cuda", bk.lib, on)


@pytest.mark.parametrize("on", [False, True], ids=["loop", "launch"])
def test_engine_one_call_of_each_wide_entry_point(bk, on):
    W2.check_engine_mixed("cuda", bk.lib, on)


def test_engine_crossover_constant_decides_under_auto(bk, monkeypatch):
    W2.check_engine_crossover("cuda", bk.lib, monkeypatch)
