"""The forced-playout model (tests/forced_model.py) without an engine: the pure `targets` function against rows computed by
hand, the model with forcing not in effect against solver_model.Model, and the cap on the inputs of the engine-vs-model
cases (tests/forced_cases.py), asserted for the exact case list."""
import math

import pytest

import forced_cases as fc
import forced_model as fm
import solver_model as so
from oracle import orc

# targets(N_p, N, W, P, C, factor) with W = 0 everywhere (q = 0), C = 1, N_p = 16 (sq = 4) unless said otherwise, so that
# u_k(T) = 4 P_k / T and ub = 4 P_b / (1 + N_b), all exact in binary
HAND = {
    # b = 0 (N = 8, P = 0.5): ub = 2 / 9.  Child 1: N = 2, P = 0.125 -> F = (int)sqrt(2 * 0.125 * 16) = 2, a = 0.5; T = 2: 0.25 >= 2/9
    # stops at once -> 2.  Child 2: N = 3, P = 0.03125 -> F = (int)sqrt(1) = 1, a = 0.125; T = 3: 0.0416.. < 2/9 -> T = 2, F used up -> 2.
    "plain": ((16, [8, 2, 3], [0.0, 0.0, 0.0], [0.5, 0.125, 0.03125], 1.0, 2.0), [8, 2, 2]),
    # a tie for b: the FIRST largest (index 1) keeps its count, the later one (index 3, the same N) is pruned like any other.
    # ub = 4 * 0.25 / 6 = 1/6.  Child 3: N = 5, P = 0.125 -> F = 2, a = 0.5; T = 5: 0.1 < 1/6 -> 4; T = 4: 0.125 < 1/6 -> 3; F used up.
    # Child 0: N = 1, P = 0.5 -> F = 4, a = 2; T = 1: 2 >= 1/6 -> stays 1 (not reduced, so not pruned outright).
    "tie for b": ((16, [1, 5, 0, 5], [0.0] * 4, [0.5, 0.25, 0.125, 0.125], 1.0, 2.0), [1, 5, 0, 3]),
    # a child reduced to 1, then 0: N = 2, P = 0.03125 * 2 = 0.0625 -> F = (int)sqrt(2) = 1, a = 0.25; ub = 4 * 0.5 / 9 = 2/9;
    # T = 2: 0.125 < 2/9 -> T = 1 < N and <= 1 -> 0.  Child 2: N = 1, P = 0.03125 -> F = 1, a = 0.125; T = 1: 0.125 < 2/9 -> 0 -> 0.
    "to one then zero": ((16, [8, 2, 1], [0.0] * 3, [0.5, 0.0625, 0.03125], 1.0, 2.0), [8, 0, 0]),
    # F = 0: P = 0.0078125 -> sqrt(2 * 0.0078125 * 16) = 0.5 -> F = 0: nothing is taken out though u is far below ub
    "F = 0": ((16, [8, 3], [0.0, 0.0], [0.5, 0.0078125], 1.0, 2.0), [8, 3]),
    # all N = 0 (a root expanded and nothing more, under FPC_RULES_VISITS): the counts as they are
    "all zero": ((1, [0, 0, 0], [0.0] * 3, [0.5, 0.25, 0.25], 1.0, 2.0), [0, 0, 0]),
    # q counts: child 1 (N = 4, W = -3: q = +0.75 for the parent) holds all four though 4 * 0.125 / 4 is far below ub = 2/9 ...
    "q holds": ((16, [8, 4], [0.0, -3.0], [0.5, 0.125], 1.0, 2.0), [8, 4]),
    # ... and with W = +3 (q = -0.75) it loses F = 2 of them
    "q prunes": ((16, [8, 4], [0.0, 3.0], [0.5, 0.125], 1.0, 2.0), [8, 2]),
}


@pytest.mark.parametrize("name", list(HAND))
def test_targets_by_hand(name):
    args, want = HAND[name]
    assert fm.targets(*args) == want
    assert sum(fm.targets(*args)) <= sum(args[1]) and fm.targets(*args)[want.index(max(want))] == max(args[1])


def test_targets_of_no_children_and_factor_zero():
    assert fm.targets(5, [], [], [], 3.0, 2.0) == []
    assert fm.targets(16, [8, 2, 1], [0.0] * 3, [0.5, 0.0625, 0.03125], 1.0, 0.0) == [8, 2, 1]      # F = 0 everywhere
    assert int(math.sqrt(2.0 * 0.125 * 16.0)) == 2


def _results_equal(a, b):
    assert len(a) == len(b)
    for x, y in zip(a, b):
        assert x["root_n"] == y["root_n"] and x["children"] == y["children"] and x["sims_done"] == y["sims_done"]
        assert x["terminated"] == y["terminated"] and x["grand"] == y["grand"]
        assert x["priors"].tobytes() == y["priors"].tobytes() and x["w"].tobytes() == y["w"].tobytes()


@pytest.mark.parametrize("K", [1, 3])
@pytest.mark.parametrize("factor,rules", fc.OFF + [(0.0, 47)], ids=["factor%g-rules%d" % c for c in fc.OFF + [(0.0, 47)]])
def test_not_in_effect_is_solver_model(factor, rules, K):
    """factor 0, and factor 2 under a rule set without FPC_RULES_VISITS (31, 15) or without FPC_RULES_PUCT either (0):
    solver_model.Model bit for bit, the targets are the stored visits and the pick is solver_model's"""
    G, sims = 4, 60
    boards = fc.boards_for("near", rules, G)
    gamma = fc.gamma_for(G, 51)
    a = fc._model(fm.Model, boards, rules, True, True, gamma, forced=factor)
    b = fc._model(so.Model, boards, rules, True, True, gamma)
    assert not a.forced_in_effect()
    assert a.search(sims, K) == b.search(sims, K)
    _results_equal(a.results(), b.results())
    assert a.steps == b.steps and a.proofs() == b.proofs()
    assert {k: v for k, v in a.counts.items() if k in b.counts} == b.counts
    assert a.counts["forced_decided"] == a.counts["pruned_visits"] == a.counts["pruned_to_zero"] == 0
    assert a.targets() == [[c.N for c in r.children] for r in b.roots]
    assert [a.pick(g, 1.0, 0.37) for g in range(G)] == [b.pick(g, 1.0, 0.37) for g in range(G)]


def test_in_effect_changes_the_search_and_the_model_targets_are_the_pure_function():
    case = fc.CASES[0]
    boards, gamma, model = fc.searched_model(case)
    plain = fc._model(so.Model, boards, case[1], case[2], case[3], gamma)
    assert plain.search(case[6], case[4]) == 0
    assert [o["children"] for o in plain.results()] != [o["children"] for o in model.results()]
    for r, T in zip(model.roots, model.targets()):
        kids = r.children
        assert T == fm.targets(r.N, [c.N for c in kids], [c.W for c in kids], [c.P for c in kids], fc.C_PUCT, fc.FACTOR)
        if kids:
            b = max(range(len(kids)), key=lambda k: (kids[k].N, -k))
            assert T[b] == kids[b].N and all(0 <= t <= c.N for t, c in zip(T, kids)) and 1 not in [t for t, c in zip(T, kids) if t < c.N]


def test_conditions_of_the_engine_vs_model_cases():
    """every case: forced_decided >= 1 and pruned_visits >= 1; across the list pruned_to_zero >= 1 -- and the play cases
    have a root that is proven WIN or DRAW"""
    assert fc.conditions() >= 1
    assert fc.proven_root_case() in fc.CASES
    assert orc is not None
