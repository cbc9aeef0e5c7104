"""Wide team-reward nets (EngineConfig.tr_hid != 20) on the hipemu (CPU) build of the kernel sources: the engine against oracle.train
for every combination of widths, the cross-epoch caches, routing, adversaries, rcmarl_wide_td_error, the drop-in trainer, checkpoints
and refusals.  The same checks run on the MI355X in test_wide_tr_gpu.py (tests/wide_tr_checks.py holds them)."""
import pytest

import wide_tr_checks as WT
from emu_util import emu_lib
from test_kernels_emu import EmuBackend


@pytest.fixture(scope="module")
def bk():
    return EmuBackend()


@pytest.mark.parametrize("critic_hid,tr_hid", WT.WIDTH_PAIRS)
def test_engine_two_blocks_against_the_oracle(critic_hid, tr_hid):
    WT.check_engine_vs_oracle("cpu", emu_lib(), critic_hid, tr_hid)


def test_engine_both_nets_on_packed_operands_against_the_oracle():
    WT.check_engine_vs_oracle("cpu", emu_lib(), *WT.PK_PAIR, lattice=True)


@pytest.mark.parametrize("critic_hid,tr_hid", WT.PK_MIXED_PAIRS[:1])         # (the emulated GEMMs are slow: the second pair runs on the GPU)
def test_engine_packed_nets_of_different_widths_against_the_oracle(critic_hid, tr_hid):
    WT.check_engine_vs_oracle("cpu", emu_lib(), critic_hid, tr_hid, lattice=True, seeds=(11,))


def test_engine_lattice_layer_1_with_dense_layers_against_the_oracle():
    WT.check_engine_vs_oracle("cpu", emu_lib(), *WT.LATTICE_PAIR, lattice=True)


def test_caches_on_and_off_give_the_same_bits():
    WT.check_cache_invariant("cpu", emu_lib(), 24, 24)


def test_caches_on_and_off_give_the_same_bits_on_packed_operands():
    WT.check_cache_invariant("cpu", emu_lib(), *WT.PK_PAIR, lattice=True)


def test_routing_by_net():
    WT.check_routing("cpu", emu_lib())


@pytest.mark.parametrize("label", ["Greedy", "Malicious"])
def test_adversary_beside_a_wide_team_reward_net(label):
    WT.check_adversary("cpu", emu_lib(), label)


@pytest.mark.parametrize("B", [7, 130])
def test_wide_td_error_equals_the_three_launch_form(bk, B):
    WT.check_wide_td_error(bk, B)


def test_wide_td_error_argument_validation():
    WT.check_wide_td_error_arguments(emu_lib())


def test_dropin_trainer_reads_the_team_reward_width_from_the_agents():
    WT.check_dropin((emu_lib(), "cpu"))


def test_checkpoints(tmp_path):
    WT.check_checkpoints("cpu", emu_lib(), str(tmp_path / "ck.pt"))


def test_validation_and_refusals():
    WT.check_validation("cpu", emu_lib())
