"""The MCTS solver (fpc_search_set_solver, fpc_search_proofs) on the wavefront emulator (CPU): the SOLVE instances of
select_game in k_select, k_expand_select and their _multi twins, prove_upward, k_tree_advance's status copy, k_play_ply's pick
rule and k_root_proofs, driven through the C-ABI, against the plain-Python model (tests/solver_model.py).  The cases are those
of tests/test_solver_gpu.py; everything is compared exactly."""
import pytest

import solver_cases as sc


@pytest.mark.parametrize("rules", [sc.TRAINING, sc.SELFPLAY])
def test_by_hand_king_takers_are_proven_by_one_visit(rules):
    sc.by_hand("emul", rules)


def test_conditions_of_the_near_end_cases():
    sc.conditions()


@pytest.mark.parametrize("fused", [True, False], ids=["fused", "unfused"])
@pytest.mark.parametrize("shape,rules,K", sc.CASES2, ids=["%s-rules%d-K%d" % c for c in sc.CASES2])
def test_engine_equals_model_on_near_end_positions(shape, rules, K, fused):
    sc.engine_vs_model("emul", shape, rules, K, fused)


@pytest.mark.parametrize("refill", [False, True], ids=["advance", "advance_refill"])
def test_reuse_carries_the_statuses(refill):
    sc.reuse("emul", refill)


def test_live_rows_and_budgets():
    sc.live_rows_and_budgets("emul")


@pytest.mark.parametrize("rules", [sc.TRAINING, sc.SELFPLAY])
def test_play_follows_the_proofs(rules):
    sc.play("emul", rules)


def test_selfplay_loop_host_and_device_paths_agree():
    sc.selfplay_loop("emul")


def test_off_means_off():
    sc.off_means_off("emul")


def test_refusals():
    sc.refusals("emul")
