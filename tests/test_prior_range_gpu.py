"""The softmax and prior arithmetic across the whole range of fpc_expf on the device, bit for bit against
sm._priors / orc.search / search_model.Model: child flats, child order, f32 priors, visits and f64 value sums.

* external evaluator (k_softmax_partials in front): the direct rows of tests/prior_cases.py through one simulation by
  fpc_search_expand (k_expand), fpc_search_expand_select (k_expand_select) and with two leaves per step (k_expand_multi,
  k_expand_select_multi), under the strict and the fixed rules, one case with root noise; the evaluator families as
  whole searches, step-wise, fused and with two leaves;
* internal network (k_fc_reduce's records, logit_at on the slabs and on the dense matrix): the single rows as the bias
  of tower_probe's "bias_row" Linear behind a family A integer tower, both operand types and both Linear layouts;
* legal-only head (k_policy_gemv -> k_expand_legal, k_expand_legal_select, the _multi forms) on the same Linear;
* refusals: the engine raises exactly where sm._priors returns 1 and names the first such game.

tests/test_prior_range_cpu.py holds the coverage of every case and proves with single faults that the cases can fail."""
import numpy as np
import pytest

import prior_cases as pc
import search_model as sm
import tower_probe as tp
from fpc_testlib import make_engine, roots_of

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("way", list(pc.WAYS))
@pytest.mark.parametrize("name", list(pc.DIRECT_CASES))
def test_direct_rows_on_the_device(name, way):
    """one crafted row per game: subnormal p_i, subnormal T, subnormal quotients, children flushed one f32 step below -86
    and kept at it, overflowing differences, the row maximum in every kind of place -- the device's bits are the model's"""
    case = pc.direct_case(name)
    rc, model = pc.model_of(case, way)
    assert rc == 0
    eng, res = pc.engine_run("gpu", case, way)
    try:
        sm.compare(eng, res, model, (name, way))
    finally:
        eng.close()


@pytest.mark.parametrize("name", list(pc.REFUSAL_CASES))
def test_refusals_on_the_device_name_the_game(name):
    """+inf at an illegal index, NaN at a legal index, at index A - 1 alone, at an illegal index, every legal move
    flushed, an all -inf row: the first refusing game of the batch is named, the rows in front of it are fine"""
    case = pc.direct_case(name)
    assert pc.first_refusal(case) == case["first"]
    for way in ("expand", "expand_select", "select_multi"):
        with pytest.raises(RuntimeError, match=r"game %d: legal policy mass" % case["first"]):
            eng, _ = pc.engine_run("gpu", case, way)
            eng.close()


@pytest.mark.parametrize("kind,R,G,sims,seed", pc.FAMILY_CASES, ids=["%s-%dx%d" % (c[0], c[1], c[1]) for c in pc.FAMILY_CASES])
def test_evaluator_families_on_the_device(kind, R, G, sims, seed):
    """whole searches whose rows differ leaf by leaf: step-wise, fused and with two leaves per step against the oracle
    and the model"""
    pc.family_engine_runs("gpu", kind, R, G, sims, seed)


# ---------------------------------------------------------------------------------------------------------------------
# the internal network: the rows as the bias of an all-zero policy Linear
# ---------------------------------------------------------------------------------------------------------------------
R8 = 8
# (operand type, fc_layout, dense logits knob): both operand types on both layouts (k_fc16 / k_fcw in front of k_fc_reduce),
# and logit_at's second source, the dense matrix (FPC_DENSE_LOGITS under FPC_DEV_KNOBS)
FULL_CONFIGS = [(1, 2, False), (0, 1, False), (1, 1, False), (0, 2, False), (1, 2, True)]
LEGAL_CONFIGS = [(1, 2, False), (0, 1, False)]
_model_cache = {}


def _config_id(c):
    return "%s-layout%d%s" % (tp.FMT[c[0]]["name"], c[1], "-dense" if c[2] else "")


def _single_model(entry, head, run):
    key = (head, entry[0], run)
    if key not in _model_cache:
        _model_cache[key] = pc.single_model(entry, head, run)
    return _model_cache[key]


def _run_single_rows(config, head, monkeypatch):
    dtype, layout, dense = config
    monkeypatch.delenv("FPC_DEV_KNOBS", raising=False)
    monkeypatch.delenv("FPC_DENSE_LOGITS", raising=False)
    if dense:
        monkeypatch.setenv("FPC_DEV_KNOBS", "1")
        monkeypatch.setenv("FPC_DENSE_LOGITS", "1")
    net = tp.integer_net(R8, 2, 128, 100 * R8 + 2)
    base = tp.tail(R8, dtype, layout, "bias_row")
    blob0 = tp.splice(net, base)
    front = blob0[:len(blob0) - len(base.bytes)]
    del blob0
    G = pc.SINGLE_G
    rows = pc.single_rows(head)
    eng = make_engine("gpu", R8, pc.INV_OF[R8], max_games=2 * G, max_sims=16, nn_dtype=dtype)
    try:
        eng.set_policy_mode(head == "legal")
        for entry in rows["run"] + rows["refuse"]:
            name, board, row, _geo = entry
            eng.load_weights(front + base.with_bias(row).bytes)
            refuse = entry in rows["refuse"]
            for run in (["run1"] if refuse else pc.single_runs(head, name)):
                K, sims = pc.SINGLE_RUNS[run]
                tag = (_config_id(config), head, name, run)
                roots = roots_of([board] * G, R8)
                eng.set_leaves(K)
                eng.search_begin(roots, 3.0)
                if refuse:
                    assert _single_model(entry, head, run)[0] == -3, tag
                    with pytest.raises(RuntimeError, match="game 0: legal policy mass"):
                        eng.search_run(sims)
                        eng.search_results(roots=roots)
                    continue
                rc, model = _single_model(entry, head, run)
                assert rc == 0, tag
                eng.search_run(sims)
                res = eng.search_results(roots=roots)
                sm.compare(eng, res, model, tag)
        eng.set_leaves(1)
    finally:
        eng.close()


@pytest.mark.parametrize("config", FULL_CONFIGS, ids=_config_id)
def test_single_rows_through_the_internal_network(config, monkeypatch):
    """fpc_search_run with the row at every leaf: one simulation for every row (k_expand behind k_fc_reduce), 16
    simulations (k_expand_select) and two leaves per step (the _multi kernels) for the rows that can be searched deeper;
    -inf, NaN and 3e38 travel through the bias, the slabs hold exact zeros"""
    _run_single_rows(config, "full", monkeypatch)


@pytest.mark.parametrize("config", LEGAL_CONFIGS, ids=_config_id)
def test_single_rows_through_the_legal_only_head(config, monkeypatch):
    """the same Linear with fpc_set_policy_mode(FPC_POLICY_LEGAL) against Model(policy_head="legal"): the maximum over the
    legal moves alone, no 1/S; subnormal p / T at the many-moves root, -inf on some legal logits, NaN at every illegal
    index (not read), and the documented divergence from the full head"""
    _run_single_rows(config, "legal", monkeypatch)
