"""Wide nets on irregular communication graphs on a real MI355X through the product library: the fused ragged head
(csrc/wide_head_ragged.hip) against the oracle and, bit for bit, against the uniform entry called once per class; the engine with
ragged_wide="auto" against oracle.train (tests/wide_ragged_checks.py holds the checks)."""
import pytest

import wide_ragged_checks as WR
from test_kernels_gpu import GpuBackend

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def bk():
    return GpuBackend()


# hid: 24 is no multiple of 32, 33 has an odd k tail, 128 is the width the nparts path serves; B: 70 is less than one row chunk and no
# multiple of 4, 130 has a ragged second chunk
@pytest.mark.parametrize("hid", [24, 33, 128])
@pytest.mark.parametrize("B,S", [(70, 2), (130, 1)])
def test_head_on_an_irregular_graph(bk, hid, B, S):
    WR.check_kernel(bk, hid, B, S)


@pytest.mark.parametrize("hid,B,S", [(24, 130, 2), (33, 70, 1)])
def test_head_with_estimates_on_both_sides_of_a_head_tile(bk, hid, B, S):
    WR.check_kernel(bk, hid, B, S, degrees=WR.DEGREES_B, N=36)


@pytest.mark.parametrize("graph", ["rand", "circ"])
@pytest.mark.parametrize("N,d,H", [(12, 4, 1), (30, 23, 5)])
def test_regular_graph_as_one_class(bk, N, d, H, graph):
    WR.check_regular_as_one_class(bk, N, d, H, graph)


def test_outputs_do_not_depend_on_the_rest_of_the_call(bk):
    WR.check_independence(bk)


def test_more_than_32_classes(bk):
    WR.check_more_than_32_classes(bk)


def test_two_identical_calls_give_identical_bits(bk):
    WR.check_determinism(bk)


@pytest.mark.parametrize("rng_mode", ["device", "numpy"])
def test_engine_six_agents_wide_critic_and_team_reward_net(bk, rng_mode):
    WR.check_engine_vs_oracle("six", rng_mode, "cuda", bk.lib, critic_hid=32, tr_hid=24)


def test_engine_packed_operand_forward_hands_its_norm_parts_to_the_ragged_head(bk):
    WR.check_engine_vs_oracle("six", "device", "cuda", bk.lib, critic_hid=128, tr_hid=20, lattice=True)


def test_engine_with_an_agent_that_listens_to_nobody(bk):
    WR.check_engine_vs_oracle("loner", "device", "cuda", bk.lib, critic_hid=24, tr_hid=24, seeds=(31,), n_episodes=4, buffer_size=9)


def test_engine_adversaries_wide_fits_beside_an_irregular_graph(bk):
    eng = WR.check_engine_vs_oracle("malicious", "device", "cuda", bk.lib, critic_hid=32, tr_hid=24, seeds=(21, 22), n_episodes=4,
                                    buffer_size=9)
    assert hasattr(eng, "adv") and eng.classes == [(3, 0, 0, 2), (5, 1, 2, 2)]


def test_engine_wide_actor_on_an_irregular_graph(bk):
    WR.check_engine_wide_actor("six", "cuda", bk.lib)


def test_engine_wide_actor_beside_a_malicious_agent_on_an_irregular_graph(bk):
    WR.check_engine_wide_actor("malicious", "cuda", bk.lib, adv_actor="auto")


def test_clip_report_counts(bk, monkeypatch):
    WR.check_clip_report("cuda", bk.lib, monkeypatch)


def test_regular_engine_is_unchanged_by_the_switch(bk):
    WR.check_regular_engine_unchanged("cuda", bk.lib)


def test_switch_defaults_and_refusals(bk):
    WR.check_switch("cuda", bk.lib)


def test_checkpoints(bk, tmp_path):
    WR.check_checkpoints("cuda", bk.lib, str(tmp_path / "ck.pt"))


def test_dropin_trainer_with_wide_models_on_ragged_in_nodes(bk):
    WR.check_dropin((bk.lib, "cuda"))
