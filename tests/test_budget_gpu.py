"""Per-game simulation budgets (fpc_search_set_budget) on the MI355X: the select_game gate in the tree kernels against
the plain-Python model (tests/budget_model.py), the independence, null-budget, capacity, error and Python-surface cases of
tests/budget_cases.py, and the fused fpc_search_run with budgets set after every refilling advance against the step-wise
C-ABI fed by fpc_nn_forward (k_towerc and k_towerw, one leaf and two leaves per step), and under the legal-only head
against the same roots searched alone.  Everything is compared exactly."""
import numpy as np
import pytest

import budget_cases as bc
import fpc_ffi
import search_model as sm
from test_nn_gpu import _positions
from test_tree_reuse_gpu import _net_engine, _room

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("case", ["A", "B", "C"])
def test_engine_equals_model(case):
    bc.engine_vs_model("gpu", case)


def test_independence():
    bc.independence("gpu")


@pytest.mark.parametrize("K", [1, 2])
def test_null_budgets_are_todays_search(K):
    bc.null_budgets("gpu", K)


def test_capacity_per_game():
    bc.capacity_per_game("gpu")


def test_capacity_visit_target():
    bc.capacity_visit_target("gpu")


def test_errors():
    bc.errors("gpu")


def test_mcts_search_with_explicit_budgets():
    bc.mcts_explicit_budgets("gpu")


def test_alphazero_visit_target():
    bc.alphazero_visit_target("gpu")


def _mix(rng, n, K, top, room):
    """a ply's budgets: 0, 1, a value no multiple of K, the maximum, the rest drawn; each within the game's room"""
    mix = [0, 1, 7, top] + [int(x) for x in rng.integers(0, top + 1, size=n - 4)]
    return [min(mix[i], room[g]) for g, i in enumerate(rng.permutation(n))]


@pytest.mark.parametrize("K", [1, 2])
@pytest.mark.parametrize("R,hidden,kernel", [(14, 128, "k_towerc"), (8, 256, "k_towerw")])
def test_fused_equals_stepwise(R, hidden, kernel, K):
    """with budgets set at every ply -- after fpc_search_begin and after every search_advance_refill (three rows refilled
    per advance) -- fpc_search_run(max(b)) == the step-wise loop fed by fpc_nn_forward, bit for bit"""
    import torch
    G, plies, sims = 12, 3, 20
    fused, step = _net_engine(R, hidden, 1, G * K, sims), _net_engine(R, hidden, 1, G * K, sims)

    def ev(enc):
        n = enc.shape[0]
        x = torch.from_numpy(np.ascontiguousarray(enc)).cuda()
        lg = torch.empty(n, step.A, device="cuda")
        va = torch.empty(n, device="cuda")
        torch.cuda.synchronize()
        step.nn_forward(x.data_ptr(), n, lg.data_ptr(), va.data_ptr())
        return lg.cpu().numpy(), va.cpu().numpy()

    try:
        assert fused.L.fpc_nn_kernel(fused.h).decode() == kernel
        boards = _positions(R, G + 3 * (plies - 1))
        pool = boards[G:]
        rng = np.random.default_rng(7 * R + K)
        fused.set_leaves(K)
        fused.search_begin([fpc_ffi.clone_board(b) for b in boards[:G]], 3.0)
        step.search_begin([fpc_ffi.clone_board(b) for b in boards[:G]], 3.0)
        kept, expanded, idle = np.ones(G, np.int32), 0, 0
        for ply in range(plies):
            b = _mix(rng, G, K, _room(fused, kept, sims), [fused.max_sims - (int(k) - 1) for k in kept])
            fused.search_set_budget(b)
            step.search_set_budget(b)
            fused.search_run(max(b))
            sm.run_steps(step, "gpu", max(b), ev, K)
            a, c = fused.search_results(), step.search_results()
            sm.same_results(a, c)
            assert (a["sims_done"] <= np.array(b)).all() and int(a["sims_done"].sum()) > sum(b) // 4      # (K > 1: collisions complete nothing)
            idle += int((a["sims_done"] < max(b)).sum())
            if ply + 1 == plies:
                break
            picked = dict(zip(*sm.pick_rule(a)))
            refilled = [(5 * ply + 4 * j + 1) % G for j in range(3)]        # three distinct rows, other ones every ply
            src = [g if g in picked and g not in refilled else -1 for g in range(G)]
            flats = [picked[g] if s >= 0 else 0 for g, s in enumerate(src)]
            fresh = [None] * G
            for g in range(G):
                if src[g] < 0:
                    fresh[g] = pool[(3 * ply + g) % len(pool)]
            kept, kb = fused.search_advance_refill(flats, src, fresh=fresh), step.search_advance_refill(flats, src, fresh=fresh)
            assert np.array_equal(kept, kb) and all(int(kept[g]) == 1 for g in refilled)
            after = fused.search_results()
            sm.same_results(after, step.search_results())
            expanded += int((after["n_children"] > 0).sum())
        assert expanded > 0 and idle > 0
    finally:
        fused.set_leaves(1)
        fused.close()
        step.close()


def test_legal_head_budgets_are_searches_alone():
    """FPC_POLICY_LEGAL is not bit-comparable with the step-wise full head; what holds exactly is that under
    FPC_RULES_FIXED a game's fused search does not depend on the batch: run with budgets b for max(b) simulations, game g
    has the search of the same root run alone for b[g], through a ply of reuse (k_expand_legal_select's gate; k_towerw)"""
    R, hidden, G, sims = 8, 256, 6, 20
    budgets = [[20, 3, 11, 1, 20, 6], [5, 20, 0, 20, 1, 9]]
    eng = _net_engine(R, hidden, 1, G, sims, rules=fpc_ffi.RULES_FIXED, legal=True)
    try:
        assert eng.L.fpc_nn_kernel(eng.h).decode() == "k_towerw"
        boards = _positions(R, G)

        def plies_of(pods, b_of_ply, use_budget):
            out = []
            eng.search_begin(pods, 3.0)
            for ply, b in enumerate(b_of_ply):
                if use_budget:
                    eng.search_set_budget(b)
                eng.search_run(max(b))
                res = eng.search_results()
                out.append(res)
                if ply + 1 < len(b_of_ply):
                    flats = [int(res["flat"][g, int(np.argmax(res["visits"][g, :res["n_children"][g]]))]) for g in range(len(pods))]
                    eng.search_advance(flats)
            return out

        batch = plies_of([fpc_ffi.clone_board(x) for x in boards], budgets, True)
        for ply, res in enumerate(batch):
            assert (res["sims_done"] <= np.array(budgets[ply])).all() and int(res["sims_done"].sum()) > sum(budgets[ply]) // 2
        for g in range(G):
            alone = plies_of([fpc_ffi.clone_board(boards[g])], [[b[g]] for b in budgets], False)
            for a, c in zip(alone, batch):
                sm.same_results(a, c, [0], [g])
    finally:
        eng.close()
