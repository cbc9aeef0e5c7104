"""Irregular communication graphs and per-agent H on the hipemu (CPU) build of the kernel sources: the ragged consensus entry
points against the oracle and against the uniform entry points, the engine against oracle.train, checkpoints, the drop-in
trainer, refusals.  The same checks run on the MI355X in test_ragged_gpu.py (tests/ragged_checks.py holds them)."""
import pytest

import ragged_checks as RC
from emu_util import emu_lib
from test_kernels_emu import EmuBackend


@pytest.fixture(scope="module")
def bk():
    return EmuBackend()


def test_k1_ragged_all_classes_in_one_launch(bk):
    RC.check_k1_ragged(bk)


def test_k1_ragged_more_than_32_classes(bk):
    RC.check_k1_ragged_more_classes_than_one_launch_takes(bk)


@pytest.mark.parametrize("N,d,H,graph", [(12, 4, 1, "rand"), (9, 7, 2, "rand"), (5, 4, 1, "circ"), (30, 23, 5, "rand")])
def test_k1_ragged_equals_the_uniform_entry_on_a_regular_graph(bk, N, d, H, graph):
    RC.check_k1_ragged_on_a_regular_graph(bk, N, d, H, graph=graph)


@pytest.mark.parametrize("form", ["3", "0"])      # f16 operand form (matrix-core head kernel where d + 1 <= 32) | exact form (fp32 lane code)
def test_k2_ragged(bk, form, lattice_form):
    lattice_form(bk, form)
    RC.check_k2_ragged(bk)


def test_k2_ragged_vector_alu_kernels(bk, monkeypatch):
    monkeypatch.setenv("RCMARL_K2_MX", "0")
    RC.check_k2_ragged(bk, B=70, seed=6)


def test_argument_validation_of_the_ragged_entry_points():
    RC.check_argument_validation(emu_lib())


def test_config_describes_the_graph():
    RC.check_config()


@pytest.mark.parametrize("rng_mode", ["device", "numpy"])
def test_engine_six_agents_mixed_degrees_and_H(rng_mode):
    RC.check_engine_vs_oracle("six", rng_mode, "cpu", emu_lib())


def test_engine_larger_H_only_where_the_malicious_agent_is_a_neighbour():
    eng = RC.check_engine_vs_oracle("malicious", "device", "cpu", emu_lib(), seeds=(21, 22), n_episodes=4, buffer_size=9)
    assert hasattr(eng, "adv") and eng.classes == [(3, 0, 0, 2), (5, 1, 2, 2)]


def test_engine_with_an_agent_that_listens_to_nobody():
    RC.check_engine_vs_oracle("loner", "device", "cpu", emu_lib(), seeds=(31,), n_episodes=4, buffer_size=9)


def test_checkpoints(tmp_path):
    RC.check_checkpoints("cpu", emu_lib(), str(tmp_path / "ck.pt"))


def test_dropin_trainer_reads_H_from_the_agents():
    RC.check_dropin((emu_lib(), "cpu"))


def test_main_passes_a_ragged_in_nodes_value_through_unchanged(tmp_path, monkeypatch):
    RC.check_main_in_nodes((emu_lib(), "cpu"), tmp_path, monkeypatch)


def test_refused_combinations():
    RC.check_refusals("cpu", emu_lib())
