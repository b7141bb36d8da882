"""Per-game simulation budgets (fpc_search_set_budget) on the wavefront emulator (CPU): the product's select_game gate,
driven ply by ply through the step-wise C-ABI, against the plain-Python model (tests/budget_model.py), and the Python
surface above it (mcts.budgets_for, MCTS args["sim_budget"], AlphaZero).  The cases are those of
tests/test_budget_gpu.py; everything is compared exactly."""
import pytest

import budget_cases as bc


@pytest.mark.parametrize("case", ["A", "B", "C"])
def test_engine_equals_model(case):
    bc.engine_vs_model("emul", case)


def test_independence():
    bc.independence("emul")


@pytest.mark.parametrize("K", [1, 2])
def test_null_budgets_are_todays_search(K):
    bc.null_budgets("emul", K)


def test_capacity_per_game():
    bc.capacity_per_game("emul")


def test_capacity_visit_target():
    bc.capacity_visit_target("emul")


def test_errors():
    bc.errors("emul")


def test_budgets_for():
    bc.budgets_for_by_hand()


def test_mcts_search_with_explicit_budgets():
    bc.mcts_explicit_budgets("emul")


def test_alphazero_visit_target():
    bc.alphazero_visit_target("emul")
