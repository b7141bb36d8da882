"""FPC_RULES_TERMINAL (search past terminal leaves, value by result) on the MI355X: the terminal branch of select_game in
k_select, k_expand_select and their _multi twins against the plain-Python model (tests/terminal_model.py) -- the cases of
tests/terminal_cases.py -- and in k_expand_legal_select through fpc_search_run with the legal-only policy head on an
integer network whose float64 reference is the model's evaluator.  Everything is compared exactly."""
import pytest

import search_model as sm
import terminal_cases as tc
from fpc_testlib import roots_of

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("copies", [1, 2])
def test_q5_golden_position_is_searched_to_the_end(copies):
    tc.golden("gpu", copies)


@pytest.mark.parametrize("fused", [True, False], ids=["fused", "unfused"])
@pytest.mark.parametrize("K", [1, 3])
@pytest.mark.parametrize("rules", [tc.T, tc.TRAINING])
@pytest.mark.parametrize("shape", ["8x8", "14x14"])
def test_engine_equals_model_on_near_end_positions(shape, rules, K, fused):
    tc.engine_vs_model("gpu", shape, rules, K, fused)


def test_legal_only_head_through_search_run(monkeypatch):
    """fpc_set_policy_mode(FPC_POLICY_LEGAL) + fpc_search_run under rules 31 == Model(policy_head="legal"), all bits"""
    from test_linear_probe_gpu import _engine_for_search
    monkeypatch.delenv("FPC_DEV_KNOBS", raising=False)
    c, case = tc.LEGAL, tc.legal_case()
    boards = case["boards"]
    eng = _engine_for_search(c["R"], c["hidden"], c["dtype"], c["layout"], case["m"], boards, case["s"], len(boards), c["sims"])
    try:
        roots = roots_of(boards, c["R"])
        eng.set_rules(c["rules"])
        eng.set_policy_mode(True)
        eng.search_begin(roots, 3.0)
        eng.search_run(c["sims"])
        res = eng.search_results(roots=roots)
        sm.compare(eng, res, case["want"], "legal-only head, rules 31")
    finally:
        eng.set_rules(0)
        eng.close()


def test_leaf_whose_side_to_move_won():
    tc.won_leaf("gpu")


def test_budgets():
    tc.budgets("gpu")


def test_terminal_root_leaves_the_search():
    tc.terminal_root("gpu")


def test_reuse():
    tc.reuse("gpu")


def test_set_rules_range():
    tc.rules_range("gpu")
