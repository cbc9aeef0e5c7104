"""Wide actors beside adversaries on the hipemu (CPU) build of the kernel sources: rcmarl_minibatch_actor_wide2 against
oracle/mlp_np.fit_actor_ce and the nine-launch composition, its query and refusals, and the engine with Greedy / Malicious / Faulty
agents beside 32- and 24-unit actors against oracle.train with every phase-III fit's route counted.  The same checks run on the
MI355X in test_wide_actor_adv_gpu.py (tests/wide_actor_adv_checks.py holds them); the 576-unit, the two-chunk and the
warm-slot kernel shapes, the 416-unit actor end to end, the shuffled mini-batches on the loop, the loop in the wide critic's scratch
and the checkpoint resume run there only (each takes the emulation a minute or more)."""
import pytest

import wide_actor_adv_checks as WAA
from emu_util import emu_lib
from test_kernels_emu import EmuBackend


@pytest.fixture(scope="module")
def bk():
    return EmuBackend()


def test_one_step_case_has_a_well_conditioned_loss():
    WAA.check_one_step_loss_is_well_conditioned()


@pytest.mark.parametrize("name", ["partial_unit_tile", "one_step"])
def test_wide2_actor_fit_against_the_oracle(bk, name):
    WAA.check_kernel(bk, name)


def test_query_and_argument_validation():
    WAA.check_query(emu_lib())
    WAA.check_argument_validation(emu_lib())


@pytest.mark.parametrize("adv_actor", ["launch", "loop"])
def test_engine_two_blocks_greedy_and_malicious(adv_actor):
    WAA.check_engine_two_blocks("cpu", emu_lib(), adv_actor)


def test_engine_auto_follows_the_queries_and_the_measured_constant():
    WAA.check_engine_auto("cpu", emu_lib())


def test_engine_shuffled_mini_batches():
    WAA.check_engine_shuffled("cpu", emu_lib(), "launch")


def test_engine_plain_rollout_kernel_beside_faulty_and_malicious():
    WAA.check_engine_plain_rollout("cpu", emu_lib())


def test_engine_wide_critic_beside_the_wide_actor():
    WAA.check_engine_wide_critic("cpu", emu_lib())


def test_cooperative_adam_step_leaves_the_adversaries_rows_alone():
    WAA.check_cooperative_step_leaves_adversaries_alone("cpu", emu_lib())


def test_construction_and_the_20_unit_actor_keeps_its_launches():
    WAA.check_construction("cpu", emu_lib())


def test_dropin_trainer_with_wide_actors_beside_adversaries():
    WAA.check_dropin((emu_lib(), "cpu"))
