"""FPC_RULES_TERMINAL (search past terminal leaves, value by result) on the wavefront emulator (CPU): the product's
select_game terminal branch, driven through the step-wise C-ABI, against the plain-Python model
(tests/terminal_model.py), and the Python surface above it (fpc_ffi.RULES_*, MCTS args["rules"] = "training",
selfplay.play(z_from_result=True)).  The cases are those of tests/test_terminal_gpu.py; everything is compared exactly."""
import pytest

import terminal_cases as tc


@pytest.mark.parametrize("copies", [1, 2])
def test_q5_golden_position_is_searched_to_the_end(copies):
    tc.golden("emul", copies)


@pytest.mark.parametrize("fused", [True, False], ids=["fused", "unfused"])
@pytest.mark.parametrize("K", [1, 3])
@pytest.mark.parametrize("rules", [tc.T, tc.TRAINING])
@pytest.mark.parametrize("shape", ["8x8", "14x14"])
def test_engine_equals_model_on_near_end_positions(shape, rules, K, fused):
    tc.engine_vs_model("emul", shape, rules, K, fused)


def test_leaf_whose_side_to_move_won():
    tc.won_leaf("emul")


def test_budgets():
    tc.budgets("emul")


def test_terminal_root_leaves_the_search():
    tc.terminal_root("emul")


def test_reuse():
    tc.reuse("emul")


def test_selfplay_z_from_result():
    tc.selfplay_z("emul")


def test_set_rules_range():
    tc.rules_range("emul")


def test_mcts_rules_names():
    tc.mcts_rules_names()
