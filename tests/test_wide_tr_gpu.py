"""Wide team-reward nets (EngineConfig.tr_hid != 20) on a real MI355X through the product library: the checks of test_wide_tr_emu.py
(tests/wide_tr_checks.py)."""
import pytest

import wide_tr_checks as WT
from test_kernels_gpu import GpuBackend

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def bk():
    return GpuBackend()


@pytest.mark.parametrize("critic_hid,tr_hid", WT.WIDTH_PAIRS)
def test_engine_two_blocks_against_the_oracle(bk, critic_hid, tr_hid):
    WT.check_engine_vs_oracle("cuda", bk.lib, critic_hid, tr_hid)


def test_engine_both_nets_on_packed_operands_against_the_oracle(bk):
    WT.check_engine_vs_oracle("cuda", bk.lib, *WT.PK_PAIR, lattice=True)


@pytest.mark.parametrize("critic_hid,tr_hid", WT.PK_MIXED_PAIRS)
def test_engine_packed_nets_of_different_widths_against_the_oracle(bk, critic_hid, tr_hid):
    WT.check_engine_vs_oracle("cuda", bk.lib, critic_hid, tr_hid, lattice=True, seeds=(11,))


def test_engine_lattice_layer_1_with_dense_layers_against_the_oracle(bk):
    WT.check_engine_vs_oracle("cuda", bk.lib, *WT.LATTICE_PAIR, lattice=True)


def test_caches_on_and_off_give_the_same_bits(bk):
    WT.check_cache_invariant("cuda", bk.lib, 24, 24)


def test_caches_on_and_off_give_the_same_bits_on_packed_operands(bk):
    WT.check_cache_invariant("cuda", bk.lib, *WT.PK_PAIR, lattice=True)


def test_routing_by_net(bk):
    WT.check_routing("cuda", bk.lib)


@pytest.mark.parametrize("label", ["Greedy", "Malicious"])
def test_adversary_beside_a_wide_team_reward_net(bk, label):
    WT.check_adversary("cuda", bk.lib, label)


@pytest.mark.parametrize("B", [7, 130])
def test_wide_td_error_equals_the_three_launch_form(bk, B):
    WT.check_wide_td_error(bk, B)


def test_wide_td_error_argument_validation(bk):
    WT.check_wide_td_error_arguments(bk.lib)


def test_dropin_trainer_reads_the_team_reward_width_from_the_agents(bk):
    WT.check_dropin((bk.lib, "cuda"))


def test_checkpoints(bk, tmp_path):
    WT.check_checkpoints("cuda", bk.lib, str(tmp_path / "ck.pt"))


def test_validation_and_refusals(bk):
    WT.check_validation("cuda", bk.lib)
