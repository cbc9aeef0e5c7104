"""Wide actors (EngineConfig.actor_hid != 20) on the hipemu (CPU) build of the kernel sources: the plain and the matrix-core forward
kernel of the rollout against the oracle's network and its Philox draw, the Adam step against the oracle's Keras Adam, the engine
against oracle.train, checkpoints, the drop-in trainer, refusals, routing.  The same checks run on the MI355X in
test_wide_actor_gpu.py (tests/wide_actor_checks.py holds them)."""
import pytest

import wide_actor_checks as WA
from emu_util import emu_lib
from test_kernels_emu import EmuBackend


@pytest.fixture(scope="module")
def bk():
    return EmuBackend()


def test_no_draw_of_the_kernel_cases_is_near_a_cdf_boundary():
    WA.check_seed_has_no_knife_edge()


def test_oracle_trains_a_wide_actor():
    WA.check_oracle_runs_with_a_wide_actor()


@pytest.mark.parametrize("hid", [24, 32])
def test_plain_forward(bk, hid):
    WA.check_forward_plain(bk, hid)


@pytest.mark.parametrize("hid", [32, 96])
def test_matrix_core_forward(bk, hid):
    WA.check_forward_matrix_core(bk, hid)


@pytest.mark.parametrize("which", ["lattice", "wide"])
def test_matrix_core_forward_exact_operand_form(bk, which, lattice_form, wide_form):
    if which == "lattice":
        lattice_form(bk, 0)
    else:
        wide_form(bk, 0)
    WA.check_forward_matrix_core(bk, 96)


def test_matrix_core_forward_weight_beyond_the_f16_range_takes_the_fp32_form(bk):
    WA.check_forward_matrix_core(bk, 32, plant=True)


@pytest.mark.parametrize("B", [7, 130])
@pytest.mark.parametrize("hid", [32, 96])
def test_adam_step(bk, B, hid):
    """(neither row count is a multiple of 4: these run the fp32-input MFMA GEMMs, whose loader takes any shape)"""
    WA.check_adam_step(bk, B, hid)


@pytest.mark.parametrize("f16", [1, 0])
@pytest.mark.parametrize("hid", [32, 96])
def test_adam_step_row_count_a_multiple_of_four(bk, hid, f16, wide_form):
    """B = 132 (crosses a 128-row tile): the vectorised loaders, i.e. the GEMMs a block's 1000 rows take -- on the 16-bit matrix core
    (k_wgemm16 with the Adam epilogue, f16 = 1) and on the fp32-input MFMA (f16 = 0)"""
    wide_form(bk, f16)
    assert bk.lib.rcmarl_wide_f16_mode() == f16
    WA.check_adam_step(bk, 132, hid)


@pytest.mark.parametrize("critic_hid", [20, 32])
def test_engine_two_blocks_against_the_oracle(critic_hid):
    WA.check_engine_vs_oracle("cpu", emu_lib(), critic_hid)


def test_engine_device_rng_is_reproducible():
    WA.check_engine_device_mode("cpu", emu_lib())


def test_checkpoints(tmp_path):
    WA.check_checkpoints("cpu", emu_lib(), str(tmp_path / "ck.pt"))


def test_refused_combinations():
    WA.check_refusals("cpu", emu_lib())


def test_widths_the_matrix_core_kernel_does_not_serve_take_the_plain_kernel():
    WA.check_routing("cpu", emu_lib())


def test_dropin_trainer_reads_the_actor_width_from_the_agents():
    WA.check_dropin((emu_lib(), "cpu"))


def test_argument_validation():
    WA.check_argument_validation(emu_lib())
