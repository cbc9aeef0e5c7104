"""The fused ragged head's entry points in the gfx950 build: argument validation and the coverage query come before any HIP call, so
they need no GPU; the ABI number stays 4 (entry points are added without a bump); the engine's switch is plain configuration."""


def _lib():
    from rcmarl_amd import build, capi
    return capi.CLib(build.build_hip())


def test_argument_validation_and_coverage_query_in_the_product_library():
    import wide_ragged_checks as WR
    lib = _lib()
    WR.check_argument_validation(lib)
    assert lib.rcmarl_abi_version() == 4


def test_argument_validation_and_coverage_query_in_the_emulation_build():
    import wide_ragged_checks as WR
    from emu_util import emu_lib
    WR.check_argument_validation(emu_lib())


def test_both_entry_points_are_declared_bound_and_exported():
    import os
    import re
    import subprocess
    from rcmarl_amd import build, capi
    names = {"rcmarl_wide_consensus_head_ragged", "rcmarl_wide_consensus_head_ragged_supported"}
    assert names <= set(capi.SIGNATURES) and "rcmarl_wide_consensus_head_ragged_supported" in capi.UNCHECKED
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(root, "include", "rcmarl.h")).read(), flags=re.S)
    assert names <= set(re.findall(r"\bint\s+(rcmarl_\w+)\s*\(", txt))
    out = subprocess.run(["nm", "-D", "--defined-only", build.build_hip()], capture_output=True, text=True).stdout
    assert names <= set(re.findall(r"\bT (rcmarl_\w+)", out))


def test_the_switch_is_configuration():
    """EngineConfig alone (no library): the default refuses with a hint naming the switch, 'auto' lifts the three refusals, any other
    value raises"""
    import pytest
    import ragged_checks as RC
    from rcmarl_amd.engine import EngineConfig
    sc = RC.SCENARIOS["six"]
    mk = lambda **kw: EngineConfig(6, sc["labels"], sc["in_nodes"], H=sc["H"], **kw)
    for kw in (dict(critic_hid=512), dict(tr_hid=24), dict(actor_hid=32)):
        with pytest.raises(ValueError, match="irregular.*ragged_wide='auto'"):
            mk(**kw)
        assert mk(ragged_wide="auto", **kw).ragged_wide == "auto"
    with pytest.raises(ValueError, match="ragged_wide must be"):
        mk(ragged_wide="yes")
