"""Wide nets on irregular communication graphs on the hipemu (CPU) build of the kernel sources: the fused ragged head
(csrc/wide_head_ragged.hip) against the oracle and, bit for bit, against the uniform entry called once per class; the engine with
ragged_wide="auto" against oracle.train.  The smaller half of the shapes of test_wide_ragged_gpu.py, one seed and short runs (the
emulated dense GEMMs are what takes the time; tests/wide_ragged_checks.py holds the checks; checkpoints run in the GPU file)."""
import pytest

import wide_ragged_checks as WR
from emu_util import emu_lib
from test_kernels_emu import EmuBackend


@pytest.fixture(scope="module")
def bk():
    return EmuBackend()


@pytest.mark.parametrize("hid,B,S", [(24, 70, 1), (33, 130, 1), (128, 70, 1)])
def test_head_on_an_irregular_graph(bk, hid, B, S):
    # (per-class uniform calls for a few degrees: the emulated 128 x 128 GEMM tile of every agent is what takes the time here)
    WR.check_kernel(bk, hid, B, S, uniform_classes=(1, 7, 21) if hid == 24 else ((5, 21) if hid == 33 else (5,)))


def test_head_with_estimates_on_both_sides_of_a_head_tile(bk):
    WR.check_kernel(bk, 24, 70, 1, degrees=WR.DEGREES_B, N=36, uniform_classes=(31, 32))


@pytest.mark.parametrize("N,d,H,graph", [(12, 4, 1, "rand"), (12, 4, 1, "circ")])
def test_regular_graph_as_one_class(bk, N, d, H, graph):
    WR.check_regular_as_one_class(bk, N, d, H, graph)


def test_outputs_do_not_depend_on_the_rest_of_the_call(bk):
    WR.check_independence(bk)


def test_more_than_32_classes(bk):
    WR.check_more_than_32_classes(bk, uniform_classes=(3, 19))      # (classes of both launches against the uniform entry)


def test_two_identical_calls_give_identical_bits(bk):
    WR.check_determinism(bk)


@pytest.mark.parametrize("rng_mode", ["device", "numpy"])
def test_engine_six_agents_wide_critic_and_team_reward_net(rng_mode):
    WR.check_engine_vs_oracle("six", rng_mode, "cpu", emu_lib(), critic_hid=32, tr_hid=24, seeds=(11,), n_episodes=2,
                              buffer_size=9)


def test_engine_packed_operand_forward_hands_its_norm_parts_to_the_ragged_head():
    WR.check_engine_vs_oracle("six", "device", "cpu", emu_lib(), critic_hid=128, tr_hid=20, lattice=True, seeds=(11,), n_episodes=2, buffer_size=9)


def test_engine_with_an_agent_that_listens_to_nobody():
    WR.check_engine_vs_oracle("loner", "device", "cpu", emu_lib(), critic_hid=24, tr_hid=24, seeds=(31,), n_episodes=2, buffer_size=9)


def test_engine_adversaries_wide_fits_beside_an_irregular_graph():
    eng = WR.check_engine_vs_oracle("malicious", "device", "cpu", emu_lib(), critic_hid=32, tr_hid=24, seeds=(21,), n_episodes=4,
                                    buffer_size=9)
    assert hasattr(eng, "adv") and eng.classes == [(3, 0, 0, 2), (5, 1, 2, 2)]


def test_engine_wide_actor_on_an_irregular_graph():
    WR.check_engine_wide_actor("six", "cpu", emu_lib(), seeds=(11,))


def test_engine_wide_actor_beside_a_malicious_agent_on_an_irregular_graph():
    WR.check_engine_wide_actor("malicious", "cpu", emu_lib(), adv_actor="auto", seeds=(11,))


def test_clip_report_counts(monkeypatch):
    WR.check_clip_report("cpu", emu_lib(), monkeypatch)


def test_regular_engine_is_unchanged_by_the_switch():
    WR.check_regular_engine_unchanged("cpu", emu_lib(), seeds=(11,), n_episodes=2)


def test_switch_defaults_and_refusals():
    WR.check_switch("cpu", emu_lib(), construction=False)


def test_dropin_trainer_with_wide_models_on_ragged_in_nodes():
    WR.check_dropin((emu_lib(), "cpu"))
