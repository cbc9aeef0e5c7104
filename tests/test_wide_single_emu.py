"""Per-agent classes at any hidden width on the hipemu (CPU) build of the kernel sources: rcmarl_minibatch_actor_wide against
oracle/mlp_np.fit_actor_ce and the nine-launch composition, its query and refusals, and single.RowOps / keras_compat / the agent
classes on nets of 24, 40 and 32 units against the oracle's agents.  The same checks run on the MI355X in test_wide_single_gpu.py
(tests/wide_single_checks.py holds them; the 64- and 384-unit kernel shapes and the 600-unit host loop run there only)."""
import pytest

import wide_single_checks as WS
from emu_util import emu_lib
from rcmarl_amd import single
from test_kernels_emu import EmuBackend


@pytest.fixture(scope="module")
def bk():
    return EmuBackend()


@pytest.fixture
def emu_backend():
    single.set_backend(emu_lib(), "cpu")
    yield
    single._backend = None


@pytest.mark.parametrize("name", ["partial_tile", "two_unit_tiles", "two_chunks", "one_step", "warm_slots", "natural_order"])
def test_wide_actor_fit_against_the_oracle(bk, name):
    WS.check_kernel(bk, name)


def test_query_and_argument_validation():
    WS.check_query(emu_lib())
    WS.check_argument_validation(emu_lib())


def test_agent_methods_on_wide_models_match_oracle(emu_backend):
    WS.check_agent_methods(B=100)


def test_adversary_methods_on_wide_models_match_oracle(emu_backend):
    WS.check_adversary_methods(B=100)


@pytest.mark.parametrize("B", [100, 450])
def test_adversary_actor_updates_on_wide_models_match_oracle(emu_backend, B):
    WS.check_adversary_actor_updates(B)


def test_keras_compat_views_of_wide_models(emu_backend):
    WS.check_keras_compat_views()


def test_wide_actor_update_is_one_launch_and_narrow_models_keep_their_entry_points(emu_backend):
    WS.check_launch_counts(B=210)
