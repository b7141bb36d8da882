"""FPC_RULES_VISITS (every node is born with N = 0) and first-play urgency on the wavefront emulator (CPU): the product's
birth counts, select_game's FPU term, k_tree_advance, k_play_ply, k_collect_tuples and k_replay_decode, driven through the
C-ABI, against the plain-Python model (tests/visits_model.py).  The cases are those of tests/test_visits_gpu.py;
everything is compared exactly."""
import pytest

import visits_cases as vc


@pytest.mark.parametrize("copies", [1, 2])
def test_q5_golden_position_closed_form(copies):
    vc.golden("emul", copies)


@pytest.mark.parametrize("rules", [vc.V, vc.V | 1])
@pytest.mark.parametrize("shape", ["8x8", "14x14"])
def test_engine_equals_model_visits_alone_and_with_puct(shape, rules):
    vc.engine_vs_model("emul", shape, rules, 1, fused=rules == vc.V)      # strict through the fused entry point, PUCT step by step


@pytest.mark.parametrize("fused", [True, False], ids=["fused", "unfused"])
@pytest.mark.parametrize("K", [1, 4])
@pytest.mark.parametrize("shape", ["8x8", "14x14"])
def test_engine_equals_model_selfplay_rules(shape, K, fused):
    vc.engine_vs_model("emul", shape, vc.SELFPLAY, K, fused)


def test_engine_equals_model_selfplay_rules_root_noise():
    vc.engine_vs_model("emul", "8x8", vc.SELFPLAY, 4, True, noise=True)


@pytest.mark.parametrize("K", [1, 4])
@pytest.mark.parametrize("reduction", [0.0, 0.25])
@pytest.mark.parametrize("shape", ["8x8", "14x14"])
def test_first_play_urgency(shape, reduction, K):
    vc.fpu_vs_model("emul", shape, reduction, K, fused=K == 4)      # k_select and k_expand_select, k_select_multi and k_expand_select_multi


def test_reuse_refill_and_budgets_over_three_plies():
    vc.reuse_refill_budgets("emul")


def test_play_and_tuples_without_a_visit():
    vc.play_and_tuples("emul")


def test_inert_switches_and_refused_arguments():
    vc.inert("emul")
