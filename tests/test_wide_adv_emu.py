"""Adversaries beside wide critic-family nets on the hipemu (CPU) build of the kernel sources: rcmarl_minibatch_fit_wide against
oracle/mlp_np.fit_mse, its multi-job form, query and refusals, and the engine against oracle.train with the routing counted and the
launch-per-step fallback kept under test.  The same checks run on the MI355X in test_wide_adv_gpu.py (tests/wide_adv_checks.py holds
them; the 256-unit shape runs there only)."""
import pytest

import wide_adv_checks as WA
from emu_util import emu_lib
from test_kernels_emu import EmuBackend


@pytest.fixture(scope="module")
def bk():
    return EmuBackend()


@pytest.mark.parametrize("name", ["partial_tile", "odd_in_one_batch", "two_chunks", "short_batch"])
def test_wide_minibatch_fit_against_the_oracle(bk, name):
    WA.check_fit(bk, name)


def test_wide_minibatch_fit_in_natural_row_order(bk):
    WA.check_fit(bk, "partial_tile", shuffle=False)


def test_wide_minibatch_fit_is_deterministic(bk):
    WA.check_determinism(bk)


def test_jobs_in_one_launch_equal_single_job_calls(bk):
    WA.check_multi_job(bk)


def test_query_and_argument_validation():
    WA.check_query(emu_lib())
    WA.check_argument_validation(emu_lib())


@pytest.mark.parametrize("labels,critic_hid,tr_hid", WA.ENGINE_CASES)
def test_engine_adversaries_beside_wide_nets_match_the_oracle_in_one_launch_per_epoch(labels, critic_hid, tr_hid):
    WA.check_engine("cpu", emu_lib(), labels, critic_hid, tr_hid)


def test_engine_narrow_critic_beside_a_wide_team_reward_net_three_seeds():
    WA.check_engine_mixed("cpu", emu_lib())


def test_engine_falls_back_to_the_launch_per_step_loop_when_the_query_refuses():
    WA.check_engine_fallback("cpu", emu_lib())
