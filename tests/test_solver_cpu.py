"""The solver model (tests/solver_model.py) against itself and against visits_model.Model: no engine.  With the solver not in
effect it IS visits_model.Model; its invariants hold after every step; every proof it holds is confirmed by an exhaustive
negamax over its own tree and, at the leaves, by the oracle's GetGameResult."""
import pytest

import evaluators
import solver_cases as sc
import solver_model as so
import terminal_model as tm
import visits_model as vm
from oracle import orc

CASES = sc.CASES2


def _results_equal(a, b):
    assert len(a) == len(b)
    for x, y in zip(a, b):
        assert x["root_n"] == y["root_n"] and x["children"] == y["children"] and x["sims_done"] == y["sims_done"]
        assert x["terminated"] == y["terminated"] and x["grand"] == y["grand"]
        assert x["priors"].tobytes() == y["priors"].tobytes() and x["w"].tobytes() == y["w"].tobytes()


@pytest.mark.parametrize("shape,rules,K", CASES, ids=["%s-rules%d-K%d" % c for c in CASES])
@pytest.mark.parametrize("solver,mask", [(False, 63), (True, 16 | 32), (True, 15 | 32)], ids=["off", "on-no-puct", "on-no-terminal"])
def test_not_in_effect_is_visits_model(shape, rules, K, solver, mask):
    """solver=False, and solver=True under a rule set without FPC_RULES_PUCT (16) or without FPC_RULES_TERMINAL (15) -- with
    the shape's FPC_RULES_VISITS bit kept: visits_model.Model bit for bit, and no status anywhere"""
    R, G, sims, _ = sc.SHAPES[(shape, rules)]
    rl = rules & mask
    boards = sc.near_end_boards(shape, rules)
    ev = evaluators.make("hash", R)
    a = so.Model([orc.clone(b) for b in boards], R, sc.INV_OF[R], 3.0, ev, rules=rl, vl=1.0, solver=solver)
    b = vm.Model([orc.clone(x) for x in boards], R, sc.INV_OF[R], 3.0, ev, rules=rl, vl=1.0)
    assert not a.in_effect()
    assert a.search(sims, K) == b.search(sims, K)
    _results_equal(a.results(), b.results())
    assert a.steps == b.steps and not a.S
    assert {k: v for k, v in a.counts.items() if k in b.counts} == b.counts


@pytest.mark.parametrize("shape,rules,K", CASES, ids=["%s-rules%d-K%d" % c for c in CASES])
def test_invariants_hold_after_every_step(shape, rules, K):
    """(a) after every step (check_invariants: also what a WIN / LOSS / DRAW node's children must look like); (b) and (c) are
    asserted inside the descent.  Step by step the search is the one-call search."""
    R, G, sims, _ = sc.SHAPES[(shape, rules)]
    boards = sc.near_end_boards(shape, rules)
    model = so.Model([orc.clone(b) for b in boards], R, sc.INV_OF[R], 3.0, evaluators.make("hash", R), rules=rules, vl=1.0, solver=True)
    assert model.in_effect()
    for k in so.sm.schedule(sims, K):
        assert model.search(k, k) == 0
        model.check_invariants()
    _results_equal(model.results(), sc.searched_model(shape, rules, K)[1].results())
    assert model.proofs() == sc.searched_model(shape, rules, K)[1].proofs()


def _nodes(model):
    stack = list(model.roots)
    while stack:
        nd = stack.pop()
        stack.extend(nd.children)
        yield nd


@pytest.mark.parametrize("shape,rules,K", CASES, ids=["%s-rules%d-K%d" % c for c in CASES])
def test_every_proof_is_confirmed_by_negamax(shape, rules, K):
    R, G, sims, _ = sc.SHAPES[(shape, rules)]
    model = sc.searched_model(shape, rules, K)[1]
    seen = 0
    orc.set_rules(rules & 15)
    try:
        for nd in _nodes(model):
            st = model.status(nd)
            if st == so.UNKNOWN:
                assert so.negamax(model, nd) is None or nd.children      # a childless unknown node decides nothing ...
                if nd.children:
                    assert so.negamax(model, nd) is None                 # ... and an unknown interior node is undecided: the proofs are complete
                continue
            seen += 1
            if nd.children:
                assert so.negamax(model, nd) == so.PV[st]
            else:                                                        # a leaf: the oracle's verdict on its state
                res = orc.game_result(orc.clone(nd.state), R, sc.INV_OF[R])
                assert res != 0 and tm.terminal_value(res, nd.state.turn) == so.PV[st]
    finally:
        orc.set_rules(0)
    assert seen == sum(model.counts["proven"].values()) > 0


def test_conditions_of_the_near_end_cases():
    sc.conditions()
