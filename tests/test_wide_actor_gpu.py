"""Wide actors (EngineConfig.actor_hid != 20) on a real MI355X through the product library: the checks of test_wide_actor_emu.py
(tests/wide_actor_checks.py)."""
import pytest

import wide_actor_checks as WA
from test_kernels_gpu import GpuBackend

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def bk():
    return GpuBackend()


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


def test_matrix_core_forward_largest_width(bk):
    """512 units: every wavefront owns two tiles, the activations fill the LDS"""
    WA.check_forward_matrix_core(bk, 512)


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
def test_engine_two_blocks_against_the_oracle(bk, critic_hid):
    WA.check_engine_vs_oracle("cuda", bk.lib, critic_hid)


def test_engine_device_rng_is_reproducible(bk):
    WA.check_engine_device_mode("cuda", bk.lib)


def test_checkpoints(bk, tmp_path):
    WA.check_checkpoints("cuda", bk.lib, str(tmp_path / "ck.pt"))


def test_refused_combinations(bk):
    WA.check_refusals("cuda", bk.lib)


def test_widths_the_matrix_core_kernel_does_not_serve_take_the_plain_kernel(bk):
    WA.check_routing("cuda", bk.lib)


def test_dropin_trainer_reads_the_actor_width_from_the_agents(bk):
    WA.check_dropin((bk.lib, "cuda"))


def test_argument_validation(bk):
    WA.check_argument_validation(bk.lib)
