"""The MCTS solver (fpc_search_set_solver, fpc_search_proofs) on the MI355X: the SOLVE instances of select_game in k_select,
k_expand_select and their _multi twins, prove_upward, k_tree_advance's status copy, k_play_ply's pick rule and k_root_proofs,
driven through the C-ABI, against the plain-Python model (tests/solver_model.py) -- the cases of tests/test_solver_emul.py --
and k_expand_select / k_expand_legal_select through fpc_search_run on an integer network whose float64 reference is the
model's evaluator.  Everything is compared exactly."""
import pytest

import solver_cases as sc
from fpc_testlib import roots_of

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("rules", [sc.TRAINING, sc.SELFPLAY])
def test_by_hand_king_takers_are_proven_by_one_visit(rules):
    sc.by_hand("gpu", rules)


@pytest.mark.parametrize("fused", [True, False], ids=["fused", "unfused"])
@pytest.mark.parametrize("shape,rules,K", sc.CASES2, ids=["%s-rules%d-K%d" % c for c in sc.CASES2])
def test_engine_equals_model_on_near_end_positions(shape, rules, K, fused):
    sc.engine_vs_model("gpu", shape, rules, K, fused)


@pytest.mark.parametrize("refill", [False, True], ids=["advance", "advance_refill"])
def test_reuse_carries_the_statuses(refill):
    sc.reuse("gpu", refill)


def test_live_rows_and_budgets():
    sc.live_rows_and_budgets("gpu")


@pytest.mark.parametrize("rules", [sc.TRAINING, sc.SELFPLAY])
def test_play_follows_the_proofs(rules):
    sc.play("gpu", rules)


def test_selfplay_loop_host_and_device_paths_agree():
    sc.selfplay_loop("gpu")


def test_off_means_off():
    sc.off_means_off("gpu")


def test_refusals():
    sc.refusals("gpu")


@pytest.mark.parametrize("policy_head", ["full", "legal"])
def test_search_run_on_the_internal_network(policy_head, monkeypatch):
    """fpc_search_run under rules 31 with the solver on, the full and the legal-only policy head == the solver model"""
    from test_linear_probe_gpu import _engine_for_search
    monkeypatch.delenv("FPC_DEV_KNOBS", raising=False)
    c = sc.RUN
    m, boards, s, model = sc.run_case(policy_head)
    eng = _engine_for_search(c["R"], c["hidden"], c["dtype"], c["layout"], m, boards, s, len(boards), c["sims"])
    try:
        roots = roots_of(boards, c["R"])
        eng.set_rules(c["rules"])
        eng.set_policy_mode(policy_head == "legal")
        eng.search_begin(roots, 3.0)
        eng.set_solver(True)
        eng.search_run(c["sims"])
        res = eng.search_results(roots=roots)
        sc.compare_all(eng, res, model, ("fpc_search_run", policy_head))
    finally:
        eng.set_policy_mode(False)
        sc._close(eng)
