"""Live-row numbering (fpc_search_set_live_rows) on the MI355X.

First half: the cases of tests/live_rows_cases.py through the step entry points (k_live_rows, the compact encodings,
k_softmax_partials over n_live rows, the expansion's inv[row]) -- the switch on against the switch off and the model.

Second half: the fused fpc_search_run on the internal network -- the tower fed from k_live_rows' c_slot / c_turn, xfc,
value and the softmax records in compact order, the policy Linear's row-tile gate (k_fcw / k_fc16 / k_fc_reduce with
*n_live), k_policy_gemv's inv[r], and every k_expand* reading at inv[row] -- the switch on against the switch off on the
integer network of tests/test_linear_probe_gpu.py.  Dead rows are made by budget zeros; every case asserts the simulations
each game completed.  Everything is compared exactly."""
import pytest

import live_rows_cases as lr
from fpc_testlib import roots_of

pytestmark = pytest.mark.gpu


# ---- the step entry points ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(lr.PATTERNS))
def test_layout(name):
    lr.layout("gpu", name)


@pytest.mark.parametrize("rules", [0, 31], ids=["strict", "training"])
def test_two_leaves_near_end_on_equals_off_equals_model(rules):
    lr.near_end("gpu", rules)


def test_reuse_with_refill():
    lr.reuse("gpu")


def test_state_rules():
    lr.state_rules("gpu")


# ---- fpc_search_run on the internal network --------------------------------------------------------------------------------
_setups = {}


def _setup(R, hidden, dtype, boards):
    """legal_head_cases.search_setup (the integer network and its scale exponent), once per network"""
    from legal_head_cases import search_setup
    key = (R, hidden, dtype)
    if key not in _setups:
        m, boards12, s, _ = search_setup(R, hidden, dtype, boards=boards)
        _setups[key] = (m, boards12, s)
    return _setups[key]


def _engine(R, hidden, dtype, layout, boards, rows, max_sims):
    from test_linear_probe_gpu import _engine_for_search
    m, boards12, s = _setup(R, hidden, dtype, boards)
    return _engine_for_search(R, hidden, dtype, layout, m, boards12, s, rows, max_sims)


def _run(eng, boards, R, on, K, rules, budget, sims, legal=False):
    eng.set_rules(rules)
    eng.set_leaves(K, 1.0)
    eng.set_policy_mode(legal)
    eng.search_begin(roots_of(boards, R), 3.0)
    eng.set_live_rows(on)
    eng.search_set_budget(budget)
    eng.search_run(sims)
    res = eng.search_results()
    return res, lr.grand_of(eng, res), None


def _on_equals_off(eng, boards, R, K, rules, budget, sims, legal=False):
    try:
        off = _run(eng, boards, R, 0, K, rules, budget, sims, legal)
        on = _run(eng, boards, R, 1, K, rules, budget, sims, legal)
        lr.same_search(off, on)
        return on[0]
    finally:
        eng.set_live_rows(0)
        eng.set_leaves(1)
        eng.set_policy_mode(False)
        eng.set_rules(0)


def _check_done(res, budget):
    """the dead rows the case meant to produce: a game without a budget never selects, one with a budget is live in the
    first step at least (its root is in progress) and never passes its budget"""
    done = [int(x) for x in res["sims_done"]]
    assert [d > 0 for d in done] == [b > 0 for b in budget] and all(d <= b for d, b in zip(done, budget))
    return done


def _boards8(n):
    base = lr.mid_boards(70)
    return [base[g % 70] for g in range(n)]


# 6. one row tile: G = 70, every third row dead
@pytest.mark.parametrize("layout,dtype,legal", [(2, 1, False), (1, 1, False), (1, 0, False), (2, 1, True), (1, 0, True)],
                         ids=["layout2-fp16-full", "layout1-fp16-full", "layout1-bf16-full", "layout2-fp16-legal", "layout1-bf16-legal"])
def test_fused_one_tile(layout, dtype, legal, monkeypatch):
    monkeypatch.delenv("FPC_DEV_KNOBS", raising=False)
    R, G, sims = 8, 70, 6
    boards = _boards8(G)
    budget = [0 if g % 3 == 2 else sims for g in range(G)]
    eng = _engine(R, 128, dtype, layout, boards, G, sims)
    try:
        res = _on_equals_off(eng, boards, R, 1, 0, budget, sims, legal)
        _check_done(res, budget)
    finally:
        eng.close()


# 7. two row tiles: G = 260; the second tile of the policy Linear is skipped whole / partly live / full
GATE_G, GATE_SIMS = 260, 4
GATE_ZEROS = {"second-tile-skipped": [g for g in range(GATE_G) if g % 26 == 5],      # 10 games: 250 live rows
              "second-tile-partly-live": [7, 200],                                    # 258 live rows
              "all-live": []}


@pytest.fixture(scope="module", params=[2, 1], ids=["layout2", "layout1"])
def gate_engine(request):
    import os
    knobs = os.environ.pop("FPC_DEV_KNOBS", None)
    eng = _engine(8, 128, 1, request.param, _boards8(GATE_G), GATE_G, GATE_SIMS)
    yield eng
    eng.close()
    if knobs is not None:
        os.environ["FPC_DEV_KNOBS"] = knobs


@pytest.mark.parametrize("zeros", list(GATE_ZEROS))
def test_fused_two_tiles(gate_engine, zeros):
    boards = _boards8(GATE_G)
    budget = [0 if g in GATE_ZEROS[zeros] else GATE_SIMS for g in range(GATE_G)]
    assert {"second-tile-skipped": 250, "second-tile-partly-live": 258, "all-live": 260}[zeros] == sum(b > 0 for b in budget)
    res = _on_equals_off(gate_engine, boards, 8, 1, 0, budget, GATE_SIMS)
    _check_done(res, budget)


# 8. 14x14 through k_towerc: G = 6, two rows dead
@pytest.fixture(scope="module")
def engine14():
    import os
    knobs = os.environ.pop("FPC_DEV_KNOBS", None)
    m, boards, _s = _setup(14, 128, 1, None)
    eng = _engine(14, 128, 1, 2, None, 18, 6)
    assert (eng.L.fpc_nn_kernel(eng.h) or b"").decode() == "k_towerc"
    yield eng, boards[:6]
    eng.close()
    if knobs is not None:
        os.environ["FPC_DEV_KNOBS"] = knobs


@pytest.mark.parametrize("rules", [0, 31], ids=["strict", "training"])
@pytest.mark.parametrize("K", [1, 3])
def test_fused_14x14_towerc(engine14, K, rules):
    eng, boards = engine14
    sims = 6
    budget = [sims, 0, sims, sims, 0, sims]
    res = _on_equals_off(eng, boards, 14, K, rules, budget, sims)
    done = _check_done(res, budget)
    if K == 1 and rules == 31:
        assert done == budget                                         # an alive game completes one simulation per step
