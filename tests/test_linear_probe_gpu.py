"""The policy Linear (k_fcw / k_fc16 + k_fc_reduce, csrc/fpc_fc.h) EVERY ELEMENT, bit for bit, through a dense integer
Linear (tests/tower_probe.py): a family A integer network's policy-conv outputs are integers, the Linear's
weights are random integers in {-3..3} and its bias in {-5..5}, so every partial sum of a logit is an integer far below
2^24 and fp32 accumulation is exact IN ANY ORDER -- whatever the K-split, the slab order or the tile shape, the engine
must give the float64 reference's bits.  No tolerance anywhere.  tests/test_tower_probe_cpu.py holds that no fragment
product of these inputs is dead and that faults of the Linear's own decomposition are flagged.

Second half: the same Linear scaled by a power of two makes the internal network's logits reproducible on the CPU, so
the fused search (fpc_search_run: k_fc_reduce's softmax records, the slab reader logit_at) meets the oracle directly --
and the opt-in legal-only head (k_fc_unfrag, k_policy_gemv, k_expand_legal(_select)(_multi)) the search model with
policy_head="legal" (tests/legal_head_cases.py; tests/test_legal_head_cpu.py proves those cases able to fail)."""
import time

import numpy as np
import pytest

import legal_head_cases as lc
import search_model as sm
import tower_probe as tp
from fpc_testlib import make_engine, roots_of
from legal_head_cases import G, INV_OF, SIMS, search_setup
from oracle import orc

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("case", tp.LINEAR_CASES, ids=tp.linear_case_id)
def test_dense_integer_linear_every_element(case, monkeypatch):
    """logits == flat @ W.T + bias of the float64 reference, all bits, for the case's row counts one after the other on
    ONE engine (largest first: nothing of the larger call may show in the smaller).  Every forward writes into n + 1 rows
    of NaN: row n must still be NaN afterwards (k_fc_reduce's m >= n_rows)."""
    import torch
    R, dtype, layout, seq = case
    monkeypatch.delenv("FPC_DEV_KNOBS", raising=False)
    rows_max = max(seq)
    p = tp.prepare(tp.linear_case(R, dtype, rows_max))
    want = tp.dense_reference(p, R)                              # asserts linear_conditions
    blob = tp.splice(p["net"], tp.tail(R, dtype, layout, "dense_int"))
    eng = make_engine("gpu", R, INV_OF[R], max_games=rows_max, max_sims=4, nn_dtype=dtype)
    try:
        eng.load_weights(blob)
        del blob
        assert (eng.L.fpc_nn_kernel(eng.h) or b"").decode() == ("k_towerc" if R == 14 else "k_towerw")
        for n in seq:
            sel = tp.linear_rows(rows_max, n)
            x_dev = torch.from_numpy(np.ascontiguousarray(p["x"][sel])).cuda()
            lg = torch.full((n + 1, eng.A), float("nan"), device="cuda")
            va = torch.full((n + 1,), float("nan"), device="cuda")
            eng.nn_forward(x_dev.data_ptr(), n, lg.data_ptr(), va.data_ptr())
            torch.cuda.synchronize()
            lg, va = lg.cpu().numpy(), va.cpu().numpy()
            what = "%s, %d rows" % (tp.linear_case_id(case), n)
            assert np.isnan(lg[n]).all() and np.isnan(va[n]), (what, "the row behind the last was written")
            assert np.isfinite(lg[:n]).all() and np.isfinite(va[:n]).all(), what
            tp.check_exact(lg[:n], want[sel], what)
    finally:
        eng.close()


# ---------------------------------------------------------------------------------------------------------------------
# the fused search on the internal network against the oracle
# ---------------------------------------------------------------------------------------------------------------------
# (R, hidden, operand type, layout, s): s is the power of two that brings the reference's largest |logit| over the 12
# root positions into [8, 16) -- computed from the reference in the test and held against this record
SEARCH_CASES = [(8, 128, 1, 2, 9), (8, 128, 0, 1, 9), (10, 128, 1, 1, 9), (14, 128, 1, 2, 10), (8, 256, 1, 2, 9)]


def _engine_for_search(R, hidden, dtype, layout, m, boards, s, rows, max_sims=SIMS):
    import torch
    eng = make_engine("gpu", R, INV_OF[R], max_games=rows, max_sims=max_sims, nn_dtype=dtype)
    eng.load_weights(tp.splice(m, tp.tail(R, dtype, layout, "dense_scaled", s=s)))
    # the value Linear is all zero: the engine's value is tanh(0), exactly
    x = torch.from_numpy(orc.encode(boards[:G], R)).cuda()
    lg = torch.full((G, eng.A), float("nan"), device="cuda")
    va = torch.full((G,), float("nan"), device="cuda")
    eng.nn_forward(x.data_ptr(), G, lg.data_ptr(), va.data_ptr())
    torch.cuda.synchronize()
    assert not va.cpu().numpy().view(np.uint32).any(), "tanh(0) must be +0.0"
    return eng


@pytest.mark.parametrize("R,hidden,dtype,layout,s_rec", SEARCH_CASES,
                         ids=["%dx%d-h%d-%s-layout%d" % (c[0], c[0], c[1], tp.FMT[c[2]]["name"], c[3]) for c in SEARCH_CASES])
def test_fused_search_on_the_internal_network_meets_the_oracle(R, hidden, dtype, layout, s_rec, monkeypatch):
    """search_begin / search_run / search_results with the integer network + "dense_scaled" Linear loaded, against
    orc.search fed by the float64 reference of the same network: root N, children, visits, f32 priors, f64 value sums and
    the roots' list orders, all bits."""
    from engine_cases import _compare_search
    monkeypatch.delenv("FPC_DEV_KNOBS", raising=False)
    m, boards, s, ev = search_setup(R, hidden, dtype)
    assert s == s_rec, (s, s_rec)
    rc, oref = orc.search([orc.clone(b) for b in boards], R, INV_OF[R], SIMS, 3.0, ev)
    assert rc == 0
    eng = _engine_for_search(R, hidden, dtype, layout, m, boards, s, G)
    try:
        roots = roots_of(boards, R)
        eng.search_begin(roots, 3.0)
        eng.search_run(SIMS)
        res = eng.search_results(roots=roots)
        assert int(res["sims_done"].sum()) > G * SIMS // 2
        _compare_search(res, oref, ("internal network", R, hidden, dtype, layout))
    finally:
        eng.close()


def test_fused_leaf_parallel_search_on_the_internal_network_meets_the_model(monkeypatch):
    """the same with K = 2 leaves per game and step (fpc_search_set_leaves) against the plain-Python search model"""
    R, hidden, dtype, layout, s_rec = SEARCH_CASES[0]
    K = 2
    monkeypatch.delenv("FPC_DEV_KNOBS", raising=False)
    m, boards, s, ev = search_setup(R, hidden, dtype)
    assert s == s_rec
    rc, model, _counts = sm.search([orc.clone(b) for b in boards], R, INV_OF[R], SIMS, 3.0, ev, K)
    assert rc == 0
    eng = _engine_for_search(R, hidden, dtype, layout, m, boards, s, G * K)
    try:
        roots = roots_of(boards, R)
        eng.set_leaves(K)
        eng.search_begin(roots, 3.0)
        eng.search_run(SIMS)
        res = eng.search_results(roots=roots)
        sm.compare(eng, res, model, ("internal network, 2 leaves", R), grand_every=3)
        eng.set_leaves(1)
    finally:
        eng.close()


# ---------------------------------------------------------------------------------------------------------------------
# the legal-only policy head against the search model with the legal head's prior arithmetic
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(lc.LEGAL_CASES))
def test_legal_only_head_meets_the_model_bit_for_bit(name, monkeypatch):
    """fpc_set_policy_mode(FPC_POLICY_LEGAL) + fpc_search_run on the integer network + "dense_scaled" Linear against
    search_model with policy_head="legal" fed by the float64 reference: every partial sum of a logit is an integer times
    2^-s below 2^24 (linear_conditions, asserted on every evaluator call), so k_policy_gemv's logits must be the
    reference's in every bit whatever the order of its v_dot2 accumulators and its butterfly, and the priors are the
    spec of DESIGN.md 5.  Root N, children, visits, f32 priors, f64 value sums, list orders and, for every third game,
    the grandchildren: all bits, no tolerance.  The case's coverage conditions are asserted from the model first."""
    c = lc.LEGAL_CASES[name]
    R, K = c["R"], c["K"]
    monkeypatch.delenv("FPC_DEV_KNOBS", raising=False)
    case = lc.legal_case(name)
    print(name, lc.check_coverage(name, case), "model: %.1f s of host time" % case["seconds"])
    boards = case["boards"]
    t0 = time.time()
    eng = _engine_for_search(R, c["hidden"], c["dtype"], c["layout"], case["m"], boards, case["s"], len(boards) * K, c["sims"])
    try:
        assert (eng.L.fpc_nn_kernel(eng.h) or b"").decode() == ("k_towerc" if R == 14 else "k_towerw")
        roots = roots_of(boards, R)
        eng.set_rules(c["rules"])
        eng.set_policy_mode(True)
        eng.set_leaves(K)
        eng.search_begin(roots, 3.0)
        eng.search_run(c["sims"])
        res = eng.search_results(roots=roots)
        sm.compare(eng, res, case["model"], ("legal-only head", name), grand_every=3)
        eng.set_leaves(1)
    finally:
        eng.close()
    print(name, "engine and comparison: %.1f s" % (time.time() - t0))


def test_legal_only_head_refuses_more_than_2048_games(monkeypatch):
    """GEMV_MAXG: k_policy_gemv's pair offsets live in 2049 ints of LDS.  An engine of 2049 games (max_sims 1: 97 nodes
    and 3 boards per game) refuses the legal head in fpc_search_run with FPC_EINVAL and goes on with the full head: the
    same 12 roots then meet the oracle bit for bit."""
    from engine_cases import _compare_search
    R, hidden, dtype, layout, s_rec = SEARCH_CASES[0]
    monkeypatch.delenv("FPC_DEV_KNOBS", raising=False)
    m, boards, s, ev = search_setup(R, hidden, dtype)
    assert s == s_rec
    rc, oref = orc.search([orc.clone(b) for b in boards], R, INV_OF[R], 1, 3.0, ev)
    assert rc == 0
    eng = _engine_for_search(R, hidden, dtype, layout, m, boards, s, 2049, max_sims=1)
    try:
        eng.set_policy_mode(True)
        eng.search_begin(roots_of(boards, R), 3.0)
        assert eng.L.fpc_search_run(eng.h, 1) == -1                  # FPC_EINVAL
        assert "at most 2048 games" in (eng.L.fpc_last_error(eng.h) or b"").decode()
        eng.set_policy_mode(False)
        roots = roots_of(boards, R)
        eng.search_begin(roots, 3.0)
        eng.search_run(1)
        res = eng.search_results(roots=roots)
        _compare_search(res, oref, ("full head after the refusal", R))
    finally:
        eng.close()
