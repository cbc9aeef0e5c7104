"""Per-agent classes at any hidden width on a real MI355X through the product library: the checks of test_wide_single_emu.py
(tests/wide_single_checks.py), the kernel shapes of the reference's batch (450 rows in mini-batches of 200) and of the widest net the
query serves, and the host-loop mini-batch fit of a 600-unit critic."""
import pytest

import wide_single_checks as WS
from test_kernels_gpu import GpuBackend

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def bk():
    return GpuBackend()


@pytest.mark.parametrize("name", ["partial_tile", "two_unit_tiles", "two_chunks", "one_step", "warm_slots", "natural_order",
                                  "reference_batch", "widest"])
def test_wide_actor_fit_against_the_oracle(bk, name):
    WS.check_kernel(bk, name)


def test_query_and_argument_validation(bk):
    WS.check_query(bk.lib)
    WS.check_argument_validation(bk.lib)


def test_agent_methods_on_wide_models_match_oracle():
    WS.check_agent_methods(B=100)


def test_adversary_methods_on_wide_models_match_oracle():
    WS.check_adversary_methods(B=100)


@pytest.mark.parametrize("B", [100, 450])
def test_adversary_actor_updates_on_wide_models_match_oracle(B):
    WS.check_adversary_actor_updates(B)


def test_keras_compat_views_of_wide_models():
    WS.check_keras_compat_views()


def test_minibatch_fit_of_a_600_unit_critic_takes_the_host_loop():
    WS.check_minibatch_fit_host_loop()


def test_wide_actor_update_is_one_launch_and_narrow_models_keep_their_entry_points():
    WS.check_launch_counts(B=450)
