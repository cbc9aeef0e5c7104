"""Wide actors beside adversaries on a real MI355X through the product library: the checks of test_wide_actor_adv_emu.py
(tests/wide_actor_adv_checks.py), and what the emulation is too slow for: the two-chunk, the warm-slot and the 576-unit kernel
shapes, a 416-unit actor end to end on rcmarl_minibatch_actor_wide2, the shuffled mini-batches on the loop, the loop in scratch shared
with a wide critic, and the checkpoint resume."""
import pytest

import wide_actor_adv_checks as WAA
from test_kernels_gpu import GpuBackend

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def bk():
    return GpuBackend()


@pytest.mark.parametrize("name", ["partial_unit_tile", "one_step", "two_chunks", "warm_natural", "widest"])
def test_wide2_actor_fit_against_the_oracle(bk, name):
    WAA.check_kernel(bk, name)


def test_query_and_argument_validation(bk):
    WAA.check_query(bk.lib)
    WAA.check_argument_validation(bk.lib)


@pytest.mark.parametrize("adv_actor", ["launch", "loop"])
def test_engine_two_blocks_greedy_and_malicious(bk, adv_actor):
    WAA.check_engine_two_blocks("cuda", bk.lib, adv_actor)


def test_engine_auto_follows_the_queries_and_the_measured_constant(bk):
    WAA.check_engine_auto("cuda", bk.lib)


@pytest.mark.parametrize("adv_actor", ["launch", "loop"])
def test_engine_shuffled_mini_batches(bk, adv_actor):
    WAA.check_engine_shuffled("cuda", bk.lib, adv_actor)


def test_engine_plain_rollout_kernel_beside_faulty_and_malicious(bk):
    WAA.check_engine_plain_rollout("cuda", bk.lib)


def test_engine_wide_critic_beside_the_wide_actor(bk):
    WAA.check_engine_wide_critic("cuda", bk.lib)


def test_engine_loop_in_scratch_shared_with_the_wide_critic(bk):
    WAA.check_engine_wide_critic_aliased("cuda", bk.lib)


def test_engine_416_unit_actor_on_the_two_image_kernel(bk):
    WAA.check_engine_wide2("cuda", bk.lib)


def test_cooperative_adam_step_leaves_the_adversaries_rows_alone(bk):
    WAA.check_cooperative_step_leaves_adversaries_alone("cuda", bk.lib)


def test_checkpoint_resume_is_bit_identical(bk, tmp_path):
    WAA.check_checkpoint("cuda", bk.lib, str(tmp_path / "ck.pt"))


def test_construction_and_the_20_unit_actor_keeps_its_launches(bk):
    WAA.check_construction("cuda", bk.lib)


def test_dropin_trainer_with_wide_actors_beside_adversaries(bk):
    WAA.check_dropin((bk.lib, "cuda"))
