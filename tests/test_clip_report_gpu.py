"""The clip report on a real MI355X through the product library: the checks of test_clip_report_emu.py
(tests/clip_report_checks.py), plus the captured-epoch replay, which needs the GPU."""
import pytest

import clip_report_checks as CC
from test_kernels_gpu import GpuBackend

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def bk():
    return GpuBackend()


@pytest.mark.parametrize("N,d,H,graph,S,P,P_hid", [
    (5, 4, 1, "circ", 2, 215, 150),       # a generated network with a kernel of its own, a partial last tile
    (12, 7, 2, "rand", 2, 215, 150),      # a generated network through the switch of the general kernel
    (30, 23, 5, "rand", 1, 100, 77),      # no generated network: rank counting
    (70, 66, 32, "rand", 1, 100, 70),     # more slots than lanes in a wavefront; several agent groups
    (300, 18, 8, "circ", 1, 100, 70),     # [N][32] tiles: two agents per wavefront
    (256, 18, 8, "circ", 3, 1400, 1330),  # several column ranges of several tiles each, four agent groups
])
def test_counts_equal_the_recount(bk, N, d, H, graph, S, P, P_hid):
    CC.check_regular(bk, N, d, H, graph, S, P, P_hid)


def test_ties_signed_zeros_nans_and_an_extreme_own_value(bk):
    CC.check_ties(bk)


def test_H0_changes_nothing(bk):
    CC.check_H0(bk)


def test_ragged_entry_equals_the_recount_and_the_regular_entry_class_by_class(bk):
    CC.check_ragged(bk)


def test_argument_validation(bk):
    CC.check_argument_validation(bk.lib)


def test_switch_on_changes_no_result_and_off_launches_nothing(bk):
    CC.check_switch_changes_nothing("cuda", bk.lib)


@pytest.mark.parametrize("scenario", ["malicious", "ragged", "wide"])
def test_engine_report_equals_the_recount_of_every_call(bk, scenario, monkeypatch):
    CC.check_engine_recount("cuda", bk.lib, scenario, monkeypatch)


def test_faulty_sender_is_trimmed_everywhere(bk):
    CC.check_faulty_sender("cuda", bk.lib)


def test_report_of_replayed_epochs_equals_the_uncaptured_run(bk, monkeypatch):
    CC.check_graph_replay("cuda", bk.lib, monkeypatch)


def test_checkpoint_round_trip(bk, tmp_path):
    CC.check_checkpoint("cuda", bk.lib, str(tmp_path / "ck.pt"))


def test_shard_agents_is_refused(bk):
    CC.check_shard_refusal("cuda", bk.lib)


def test_dropin_trainer_attaches_the_report(bk):
    CC.check_dropin((bk.lib, "cuda"))


def test_main_writes_the_report(bk, tmp_path, monkeypatch):
    CC.check_main((bk.lib, "cuda"), tmp_path, monkeypatch)
