"""Forced playouts and policy target pruning (fpc_search_set_forced, fpc_search_targets) on the wavefront emulator (CPU): the
FORCE instances of select_game in k_select, k_expand_select and their _multi twins, root_targets in k_root_targets,
k_collect_tuples and k_play_ply, driven through the C-ABI, against the plain-Python model (tests/forced_model.py).  The cases
are those of tests/test_forced_gpu.py; everything is compared exactly."""
import pytest

import forced_cases as fc


@pytest.mark.parametrize("fused", [True, False], ids=["fused", "unfused"])
@pytest.mark.parametrize("case", fc.CASES, ids=fc.IDS)
def test_engine_equals_model(case, fused):
    fc.engine_vs_model("emul", case, fused)


@pytest.mark.parametrize("refill", [False, True], ids=["advance", "advance_refill"])
def test_reuse_forces_at_the_new_root(refill):
    fc.reuse("emul", refill)


@pytest.mark.parametrize("case", [fc.CASES[2], fc.CASES[1], fc.CASES[10]], ids=[fc.IDS[2], fc.IDS[1], fc.IDS[10]])
def test_tuples_and_play_take_the_targets(case):
    fc.tuples_and_play("emul", case)


def test_play_with_a_proven_root():
    fc.tuples_and_play("emul", fc.proven_root_case())


def test_selfplay_loop_host_and_device_paths_agree():
    fc.selfplay_loop("emul")


@pytest.mark.parametrize("factor,rules", fc.OFF, ids=["factor%g-rules%d" % c for c in fc.OFF])
def test_off_means_off(factor, rules):
    fc.off_means_off("emul", factor, rules)


def test_refusals():
    fc.refusals("emul")
