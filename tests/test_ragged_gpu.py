"""Irregular communication graphs and per-agent H on a real MI355X through the product library: the checks of
test_ragged_emu.py (tests/ragged_checks.py), plus the captured-epoch replay, which needs the GPU."""
import pytest

import ragged_checks as RC
from test_kernels_gpu import GpuBackend

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def bk():
    return GpuBackend()


def test_k1_ragged_all_classes_in_one_launch(bk):
    RC.check_k1_ragged(bk)
    RC.check_k1_ragged(bk, N=300, S=3, P=700, P_hid=650, seed=3)        # [N][32] tiles: several agents per wavefront


def test_k1_ragged_more_than_32_classes(bk):
    RC.check_k1_ragged_more_classes_than_one_launch_takes(bk)


@pytest.mark.parametrize("N,d,H,graph", [(12, 4, 1, "rand"), (9, 7, 2, "rand"), (5, 4, 1, "circ"), (30, 23, 5, "rand"),
                                         (256, 18, 8, "circ"), (300, 10, 4, "rand")])
def test_k1_ragged_equals_the_uniform_entry_on_a_regular_graph(bk, N, d, H, graph):
    RC.check_k1_ragged_on_a_regular_graph(bk, N, d, H, graph=graph)


@pytest.mark.parametrize("form", ["3", "0"])      # f16 operand form (matrix-core head kernel where d + 1 <= 32) | exact form (fp32 lane code)
def test_k2_ragged(bk, form, lattice_form):
    lattice_form(bk, form)
    RC.check_k2_ragged(bk)
    RC.check_k2_ragged(bk, S=2, N=24, B=1000, in_dim=10, seed=5)


def test_k2_ragged_vector_alu_kernels(bk, monkeypatch):
    monkeypatch.setenv("RCMARL_K2_MX", "0")
    RC.check_k2_ragged(bk, B=70, seed=6)


def test_argument_validation_of_the_ragged_entry_points(bk):
    RC.check_argument_validation(bk.lib)


@pytest.mark.parametrize("rng_mode", ["device", "numpy"])
def test_engine_six_agents_mixed_degrees_and_H(bk, rng_mode):
    RC.check_engine_vs_oracle("six", rng_mode, "cuda", bk.lib)


def test_engine_larger_H_only_where_the_malicious_agent_is_a_neighbour(bk):
    eng = RC.check_engine_vs_oracle("malicious", "device", "cuda", bk.lib, seeds=(21, 22), n_episodes=4, buffer_size=9)
    assert hasattr(eng, "adv") and eng.classes == [(3, 0, 0, 2), (5, 1, 2, 2)]


def test_engine_with_an_agent_that_listens_to_nobody(bk):
    RC.check_engine_vs_oracle("loner", "device", "cuda", bk.lib, seeds=(31,), n_episodes=4, buffer_size=9)


def test_single_instance_replays_its_captured_epochs(bk, monkeypatch):
    RC.check_graph_replay("cuda", bk.lib, monkeypatch)


def test_checkpoints(bk, tmp_path):
    RC.check_checkpoints("cuda", bk.lib, str(tmp_path / "ck.pt"))


def test_dropin_trainer_reads_H_from_the_agents(bk):
    RC.check_dropin((bk.lib, "cuda"))


def test_main_passes_a_ragged_in_nodes_value_through_unchanged(bk, tmp_path, monkeypatch):
    RC.check_main_in_nodes((bk.lib, "cuda"), tmp_path, monkeypatch)


def test_refused_combinations(bk):
    RC.check_refusals("cuda", bk.lib)
