"""The local fit that starts from the live net, on a real MI355X through the product library: the small step with a separate source
against the in-place one, bit for bit, and the engine switch with the rule on (all-cooperative team) and off."""
import pytest

import fit_from_live_checks as FL
from test_kernels_gpu import GpuBackend

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def bk():
    return GpuBackend()


def test_small_step_with_a_separate_source_equals_the_in_place_step(bk):
    FL.check_small_sgd_from(bk)


def test_engine_results_and_launches_with_fit_from_live_on_and_off():
    eng = FL.check_engine_live_equals_copy("cuda", None)
    assert eng.graph_replays >= 1          # the second epoch ran as a captured graph: replay needs no change


def test_first_epoch_td_target_from_the_fits_own_forward_pass():
    FL.check_engine_td_from_fit_forward("cuda", None)


def test_engine_with_a_greedy_agent_keeps_the_copy_and_todays_launches():
    FL.check_engine_rule_off("cuda", None, FL.GREEDY16)


def test_engine_with_strided_w1_keeps_the_copy_and_todays_launches():
    FL.check_engine_rule_off("cuda", None, FL.COOP16, w1_tiled=False)
