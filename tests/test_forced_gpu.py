"""Forced playouts and policy target pruning (fpc_search_set_forced, fpc_search_targets) on the MI355X: the FORCE instances of
select_game in k_select, k_expand_select and their _multi twins, root_targets in k_root_targets, k_collect_tuples and
k_play_ply, driven through the C-ABI, against the plain-Python model (tests/forced_model.py) -- the cases of
tests/test_forced_emul.py -- and k_expand_select / k_expand_legal_select through fpc_search_run on an integer network whose
float64 reference is the model's evaluator.  Everything is compared exactly."""
import pytest

import forced_cases as fc
from fpc_testlib import roots_of

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("fused", [True, False], ids=["fused", "unfused"])
@pytest.mark.parametrize("case", fc.CASES, ids=fc.IDS)
def test_engine_equals_model(case, fused):
    fc.engine_vs_model("gpu", case, fused)


@pytest.mark.parametrize("refill", [False, True], ids=["advance", "advance_refill"])
def test_reuse_forces_at_the_new_root(refill):
    fc.reuse("gpu", refill)


@pytest.mark.parametrize("case", [fc.CASES[2], fc.CASES[1], fc.CASES[10]], ids=[fc.IDS[2], fc.IDS[1], fc.IDS[10]])
def test_tuples_and_play_take_the_targets(case):
    fc.tuples_and_play("gpu", case)


def test_play_with_a_proven_root():
    fc.tuples_and_play("gpu", fc.proven_root_case())


def test_selfplay_loop_host_and_device_paths_agree():
    fc.selfplay_loop("gpu")


@pytest.mark.parametrize("factor,rules", fc.OFF, ids=["factor%g-rules%d" % c for c in fc.OFF])
def test_off_means_off(factor, rules):
    fc.off_means_off("gpu", factor, rules)


def test_refusals():
    fc.refusals("gpu")


@pytest.mark.parametrize("policy_head", ["full", "legal"])
def test_search_run_on_the_internal_network(policy_head, monkeypatch):
    """fpc_search_run under rules 63 with root noise, FPU, the solver and forcing on, the full and the legal-only policy
    head == the forced model: trees, proofs and targets"""
    from test_linear_probe_gpu import _engine_for_search
    monkeypatch.delenv("FPC_DEV_KNOBS", raising=False)
    c = fc.RUN
    m, boards, s, gamma, model = fc.run_case(policy_head)
    eng = _engine_for_search(c["R"], c["hidden"], c["dtype"], c["layout"], m, boards, s, len(boards), c["sims"])
    try:
        roots = roots_of(boards, c["R"])
        fc._setup(eng, c["rules"], True, True, fc.FACTOR, gamma)
        eng.set_policy_mode(policy_head == "legal")
        eng.search_begin(roots, fc.C_PUCT)
        eng.search_run(c["sims"])
        res = eng.search_results(roots=roots)
        fc.compare_all(eng, res, model, ("fpc_search_run", policy_head))
    finally:
        eng.set_policy_mode(False)
        fc._close(eng)
