"""Adversaries beside wide critic-family nets on a real MI355X through the product library: the checks of test_wide_adv_emu.py
(tests/wide_adv_checks.py), and the 256-unit shape -- the largest width the query must serve."""
import pytest

import wide_adv_checks as WA
from test_kernels_gpu import GpuBackend

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def bk():
    return GpuBackend()


@pytest.mark.parametrize("name", ["partial_tile", "odd_in_one_batch", "two_chunks", "short_batch", "widest"])
def test_wide_minibatch_fit_against_the_oracle(bk, name):
    WA.check_fit(bk, name)


def test_wide_minibatch_fit_in_natural_row_order(bk):
    WA.check_fit(bk, "partial_tile", shuffle=False)


def test_wide_minibatch_fit_is_deterministic(bk):
    WA.check_determinism(bk)


def test_jobs_in_one_launch_equal_single_job_calls(bk):
    WA.check_multi_job(bk)


def test_query_and_argument_validation(bk):
    WA.check_query(bk.lib)
    WA.check_argument_validation(bk.lib)


@pytest.mark.parametrize("labels,critic_hid,tr_hid", WA.ENGINE_CASES)
def test_engine_adversaries_beside_wide_nets_match_the_oracle_in_one_launch_per_epoch(bk, labels, critic_hid, tr_hid):
    WA.check_engine("cuda", bk.lib, labels, critic_hid, tr_hid)


def test_engine_narrow_critic_beside_a_wide_team_reward_net_three_seeds(bk):
    WA.check_engine_mixed("cuda", bk.lib)


def test_engine_falls_back_to_the_launch_per_step_loop_when_the_query_refuses(bk):
    WA.check_engine_fallback("cuda", bk.lib)
