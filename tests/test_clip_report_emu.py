"""The clip report on the hipemu (CPU) build of the kernel sources: the two count entries against a NumPy recount whose window is
the oracle's, the engine's report against a recount at every call, checkpoints, refusals, the drop-in trainer and main.  The same
checks run on the MI355X in test_clip_report_gpu.py (tests/clip_report_checks.py holds them)."""
import pytest

import clip_report_checks as CC
from emu_util import emu_lib
from test_kernels_emu import EmuBackend


@pytest.fixture(scope="module")
def bk():
    return EmuBackend()


@pytest.mark.parametrize("N,d,H,graph,S,P,P_hid", [
    (5, 4, 1, "circ", 2, 215, 150),       # a generated network with a kernel of its own, a partial last tile, several tiles per range
    (12, 7, 2, "rand", 2, 215, 150),      # a generated network through the switch of the general kernel
    (30, 23, 5, "rand", 1, 100, 77),      # no generated network: rank counting
    (70, 66, 32, "rand", 1, 100, 70),     # more slots than lanes in a wavefront; several agent groups
    (300, 18, 8, "circ", 1, 100, 70),     # [N][32] tiles: two agents per wavefront
])
def test_counts_equal_the_recount(bk, N, d, H, graph, S, P, P_hid):
    CC.check_regular(bk, N, d, H, graph, S, P, P_hid)


def test_ties_signed_zeros_nans_and_an_extreme_own_value(bk):
    CC.check_ties(bk)


def test_H0_changes_nothing(bk):
    CC.check_H0(bk)


def test_ragged_entry_equals_the_recount_and_the_regular_entry_class_by_class(bk):
    CC.check_ragged(bk)


def test_argument_validation():
    CC.check_argument_validation(emu_lib())


def test_switch_on_changes_no_result_and_off_launches_nothing():
    CC.check_switch_changes_nothing("cpu", emu_lib())


@pytest.mark.parametrize("scenario", ["malicious", "ragged", "wide"])
def test_engine_report_equals_the_recount_of_every_call(scenario, monkeypatch):
    CC.check_engine_recount("cpu", emu_lib(), scenario, monkeypatch)


def test_faulty_sender_is_trimmed_everywhere():
    CC.check_faulty_sender("cpu", emu_lib())


def test_checkpoint_round_trip(tmp_path):
    CC.check_checkpoint("cpu", emu_lib(), str(tmp_path / "ck.pt"))


def test_shard_agents_is_refused():
    CC.check_shard_refusal("cpu", emu_lib())


def test_dropin_trainer_attaches_the_report():
    CC.check_dropin((emu_lib(), "cpu"))


def test_main_writes_the_report(tmp_path, monkeypatch):
    CC.check_main((emu_lib(), "cpu"), tmp_path, monkeypatch)
