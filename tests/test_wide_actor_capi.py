"""The wide-actor entry points in the gfx950 build: declared in include/rcmarl.h, bound in capi.py, exported by the library, and
validating their arguments before they touch the HIP runtime (no GPU needed).  The ABI number stays 4: additions only."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("rcmarl_policy_probs_wide", "rcmarl_rollout_step_wide", "rcmarl_rollout_wide_supported", "rcmarl_policy_probs_episodes_wide",
       "rcmarl_rollout_step_episodes_wide", "rcmarl_dense_backward_adam", "rcmarl_wide_actor_head", "rcmarl_wide_actor_small_adam")


def test_wide_actor_entry_points_are_declared_bound_and_exported():
    from rcmarl_amd import build, capi
    path = build.build_hip()
    lib = capi.CLib(path)
    assert lib.rcmarl_abi_version() == 4
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "rcmarl.h")).read(), flags=re.S)
    exported = set(re.findall(r"\bT (rcmarl_\w+)", subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True).stdout))
    for name in NEW:
        assert re.search(r"\bint\s+%s\s*\(" % name, txt), name
        assert name in capi.SIGNATURES and name in exported, name
    # the episode-parallel entry takes the argument list of the 20-unit one
    assert capi.SIGNATURES["rcmarl_rollout_step_episodes_wide"] == capi.SIGNATURES["rcmarl_rollout_step_episodes"]
    assert capi.SIGNATURES["rcmarl_rollout_step_wide"] == capi.SIGNATURES["rcmarl_rollout_step"]
    assert capi.SIGNATURES["rcmarl_policy_probs_wide"] == capi.SIGNATURES["rcmarl_policy_probs"]


def test_argument_validation_of_the_wide_actor_entry_points_in_the_product_library():
    import wide_actor_checks as WA
    from rcmarl_amd import build, capi
    WA.check_argument_validation(capi.CLib(build.build_hip()))
