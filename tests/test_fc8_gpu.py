"""The opt-in int8 policy Linear on the MI355X (k_fcw8 + k_fc_reduce, k_fc_unfrag8 + k_policy_gemv's scaled variant,
k_fc_rowmax + k_pack_fc8).

First half, bit for bit: a family A integer network in front of a Tail8 whose scales are powers of two -- every partial
sum is exact in any order on either side of the scale (fc8_cases.conditions8, asserted), so the engine must give the
float64 reference's bits at every element, through the dense forward, the fused search, the legal-only head and the
live-row gate.  tests/test_fc8_cpu.py proves these cases able to fail.

Second half: the device pack against the host export, and the reference's fixture networks quantised, against a float64
forward of the same quantised network under the bound tests/test_net_gpu.py holds the 16-bit path to."""
import copy

import numpy as np
import pytest

import fc8_cases as f8
import tower_probe as tp
import weights
import weights_cases as wc
from fpc_testlib import make_engine, roots_of
from legal_head_cases import G, INV_OF, SIMS, search_setup

pytestmark = pytest.mark.gpu


def _forward_rows(eng, x, n):
    """fpc_nn_forward of n rows into n + 1 rows of NaN"""
    import torch
    x_dev = torch.from_numpy(np.ascontiguousarray(x)).cuda()
    lg = torch.full((n + 1, eng.A), float("nan"), device="cuda")
    va = torch.full((n + 1,), float("nan"), device="cuda")
    eng.nn_forward(x_dev.data_ptr(), n, lg.data_ptr(), va.data_ptr())
    torch.cuda.synchronize()
    return lg.cpu().numpy(), va.cpu().numpy()


def _every_element(R, seq, lo, hi, monkeypatch):
    monkeypatch.delenv("FPC_DEV_KNOBS", raising=False)
    rows_max = max(seq)
    p = tp.prepare(tp.linear_case(R, 1, rows_max))
    policy = p["ref"]["policy"]
    flat = policy.reshape(policy.shape[0], -1)
    # the exactness condition decides the range: the case's own range where it holds, else the widest that does
    reach = float(np.abs(flat).sum(axis=1).max())
    allowed = int((2.0 ** 24 - 40.0 - 1.0) // reach)
    print("R=%d rows=%d: max_row sum|x| = %.0f allows max|q| = %d" % (R, rows_max, reach, allowed))
    if allowed < max(-lo, hi):
        lo, hi = -allowed, allowed
    q, scale, bias = f8.dense_case(R, lo, hi)
    f8.conditions8(flat, q, scale, bias)
    want = f8.expected8(policy, q, scale, bias)
    blob = f8.splice8(p["net"], f8.Tail8(R, q, scale, bias))
    eng = make_engine("gpu", R, INV_OF[R], max_games=rows_max, max_sims=4, nn_dtype=1)
    try:
        eng.load_weights(blob)
        del blob
        assert eng.nn_fc_kernel() == "k_fcw8"
        assert (eng.L.fpc_nn_kernel(eng.h) or b"").decode() == ("k_towerc" if R == 14 else "k_towerw")
        for n in seq:
            # tower_probe's windows into 256 prepared rows; of fewer rows a window that does not start at row 0 either
            sel = tp.linear_rows(rows_max, n) if rows_max >= 256 or n == rows_max else slice(rows_max // 2, rows_max // 2 + n)
            assert p["x"][sel].shape[0] == n
            lg, va = _forward_rows(eng, p["x"][sel], n)
            what = "int8 %dx%d, %d rows" % (R, R, n)
            assert np.isnan(lg[n]).all() and np.isnan(va[n]), (what, "the row behind the last was written")
            assert np.isfinite(lg[:n]).all() and np.isfinite(va[:n]).all(), what
            tp.check_exact(lg[:n], want[sel], what)
    finally:
        eng.close()


# 6. every element, bit for bit: q over the whole int8 range (-128 included), scales 2^-(n mod 4)
@pytest.mark.parametrize("R,seq", [(8, (256, 37, 1)), (8, (300,)), (9, (256, 37))], ids=["8x8-256-37-1", "8x8-300", "9x9-256-37"])
def test_int8_linear_every_element(R, seq, monkeypatch):
    _every_element(R, seq, -128, 127, monkeypatch)


# 7. the headline K-split: 14x14 is the only shape with sk = 4 and an even stage count
def test_int8_linear_every_element_14x14(monkeypatch):
    assert weights.fcw_split(14) == 4 and weights.fcw_split(8) == 8 and weights.fcw_split(9) == 8
    _every_element(14, (37, 1), -90, 90, monkeypatch)


# ---------------------------------------------------------------------------------------------------------------------
# the fused search, the legal-only head, live rows
# ---------------------------------------------------------------------------------------------------------------------
_search = {}


def _search8(boards=None, key="default"):
    """legal_head_cases.search_setup's 8x8 hidden-128 fp16 network; its Linear as a Tail8 of tower_probe.dense_weights
    (q in -3..3) with per-column scales 2^-(s + n mod 2) and bias * scale; the float64 evaluator for the same scales"""
    if key not in _search:
        R = 8
        m, boards, s, ev = search_setup(R, 128, 1, boards=boards)
        W, bias = tp.dense_weights(R)
        scale = np.exp2(-(s + np.arange(W.shape[0]) % 2)).astype(np.float32)
        tail = f8.Tail8(R, W, scale, bias.astype(np.float64) * scale, value_zero=True)

        def ev8(enc):
            lg = ev.logits_of(np.asarray(enc, np.float64)) * scale.astype(np.float64)[None, :]
            return lg.astype(np.float32), np.zeros(enc.shape[0], np.float32)

        _search[key] = (m, boards, f8.splice8(m, tail), ev8)
    return _search[key]


def _search_engine(blob, rows, max_sims=SIMS):
    eng = make_engine("gpu", 8, INV_OF[8], max_games=rows, max_sims=max_sims, nn_dtype=1)
    eng.load_weights(blob)
    assert eng.nn_fc_kernel() == "k_fcw8"
    return eng


# 8.
def test_fused_search_with_int8_weights_meets_the_oracle(monkeypatch):
    from engine_cases import _compare_search
    from oracle import orc
    monkeypatch.delenv("FPC_DEV_KNOBS", raising=False)
    R = 8
    m, boards, blob, ev8 = _search8()
    rc, oref = orc.search([orc.clone(b) for b in boards], R, INV_OF[R], SIMS, 3.0, ev8)
    assert rc == 0
    eng = _search_engine(blob, G)
    try:
        roots = roots_of(boards, R)
        eng.search_begin(roots, 3.0)
        eng.search_run(SIMS)
        res = eng.search_results(roots=roots)
        assert int(res["sims_done"].sum()) > G * SIMS // 2
        _compare_search(res, oref, ("internal network, int8 Linear", R))
    finally:
        eng.close()


# 9.
def test_legal_only_head_with_int8_weights_meets_the_model(monkeypatch):
    import search_model as sm
    from oracle import orc
    monkeypatch.delenv("FPC_DEV_KNOBS", raising=False)
    R = 8
    m, boards, blob, ev8 = _search8()
    rc, model, _counts = sm.search([orc.clone(b) for b in boards], R, INV_OF[R], SIMS, 3.0, ev8, 1, policy_head="legal")
    assert rc == 0
    eng = _search_engine(blob, G)
    try:
        roots = roots_of(boards, R)
        eng.set_policy_mode(True)
        eng.search_begin(roots, 3.0)
        eng.search_run(SIMS)
        res = eng.search_results(roots=roots)
        sm.compare(eng, res, model, ("legal-only head, int8 Linear", R), grand_every=3)
    finally:
        eng.set_policy_mode(False)
        eng.close()


# 10.
def test_live_rows_with_int8_weights_on_equals_off(monkeypatch):
    """300 slots (two row tiles of the Linear), near-end roots under the training rules: games end during the search and
    their rows die; every result array of the switched-on search equals the switched-off one's"""
    import live_rows_cases as lr
    import search_model as sm
    import terminal_cases as tc
    monkeypatch.delenv("FPC_DEV_KNOBS", raising=False)
    R, slots, sims, rules = 8, 300, 6, 31
    Rr, G8, _, _, seed = tc.SHAPES[("8x8", rules)]
    assert Rr == R
    base = sm.positions(R, G8, seed=seed, near_end=True, rules=rules & 15)
    boards = [base[g % G8] for g in range(slots)]
    m, _b, blob, _ev = _search8()
    eng = _search_engine(blob, slots, sims)
    try:
        # every seventh game without a budget (a dead row from the first step on), odd games cut short
        budget = [0 if g % 7 == 3 else 3 if g % 2 else sims for g in range(slots)]
        runs = []
        for on in (0, 1):
            eng.set_rules(rules)
            eng.search_begin(roots_of(boards, R), 3.0)
            eng.set_live_rows(on)
            eng.search_set_budget(budget)
            eng.search_run(sims)
            res = eng.search_results()
            runs.append((res, lr.grand_of(eng, res), None))
        lr.same_search(runs[0], runs[1])
        done = [int(x) for x in runs[1][0]["sims_done"]]
        assert all(d <= b for d, b in zip(done, budget)) and max(done) == sims and done.count(0) >= slots // 7
    finally:
        eng.set_live_rows(0)
        eng.set_rules(0)
        eng.close()


# ---------------------------------------------------------------------------------------------------------------------
# 11. the device load
# ---------------------------------------------------------------------------------------------------------------------
def test_device_load_int8():
    import torch
    R, hidden = 8, 128
    mods = {"A": wc.model(R, 1, hidden), "B": wc.model(R, 1, hidden, seed=1)}
    x = wc.encodings(R)
    want8, want16 = {}, {}
    for k, m in mods.items():
        e = make_engine("gpu", R, wc.INV_OF[R], max_games=4, max_sims=16, nn_dtype=1)
        e.load_weights(weights.export_weights(m, 1, fc_weights="int8"))
        assert e.nn_fc_kernel() == "k_fcw8"
        want8[k] = wc.forward(e, x)
        e.load_weights(weights.export_weights(m, 1))
        assert e.nn_fc_kernel() == "k_fcw"
        want16[k] = wc.forward(e, x)
        e.close()
    assert not np.array_equal(want8["A"][0], want8["B"][0]) and not np.array_equal(want8["A"][0], want16["A"][0])
    gpu = {k: copy.deepcopy(m).cuda() for k, m in mods.items()}
    eng = make_engine("gpu", R, wc.INV_OF[R], max_games=4, max_sims=16, nn_dtype=1)
    try:
        eng.load_weights_device(gpu["A"], fc_weights="int8")             # a first load: allocates
        assert eng.nn_fc_kernel() == "k_fcw8"
        wc.assert_same_forward(wc.forward(eng, x), want8["A"], "device load A, int8")
        free = []
        for k in ("B", "A", "B"):                                        # refreshes with changed parameters: in place
            eng.load_weights_device(gpu[k])
            torch.cuda.synchronize()
            free.append(torch.cuda.mem_get_info()[0])
            wc.assert_same_forward(wc.forward(eng, x), want8[k], "device refresh " + k)
        assert free[0] == free[1] == free[2], free
        # w16 -> int8 -> w16: the type is part of the geometry, and the 16-bit forward is what it was
        eng.load_weights_device(gpu["A"], fc_weights="w16")
        assert eng.nn_fc_kernel() == "k_fcw"
        wc.assert_same_forward(wc.forward(eng, x), want16["A"], "w16 after int8")
        eng.load_weights_device(gpu["A"], fc_weights="int8")
        wc.assert_same_forward(wc.forward(eng, x), want8["A"], "int8 again")
        eng.load_weights_device(gpu["A"], fc_weights="w16")
        wc.assert_same_forward(wc.forward(eng, x), want16["A"], "w16 again")
        # a planted NaN refuses the int8 load and leaves the 16-bit network in use
        bad = copy.deepcopy(gpu["A"])
        with torch.no_grad():
            bad.policyHead[4].weight[7, 9] = float("nan")
        with pytest.raises(RuntimeError, match="policy Linear"):
            eng.load_weights_device(bad, fc_weights="int8")
        wc.assert_same_forward(wc.forward(eng, x), want16["A"], "after the refusal")
    finally:
        eng.close()


# ---------------------------------------------------------------------------------------------------------------------
# 12. the reference's fixture networks, quantised
# ---------------------------------------------------------------------------------------------------------------------
TOL = 1e-3          # tests/test_net_gpu.py's bound for these fixtures with fp16 operands (north_star), not tuned


@pytest.mark.parametrize("R,blocks,hidden", [(8, 10, 128), (14, 10, 128)])
def test_fixture_network_int8_against_float64_of_the_quantised_network(R, blocks, hidden):
    """The engine with fc_weights="int8" against a float64 CPU forward of the SAME network with the policy Linear's
    weights replaced by q * s: the arithmetic differs from the fp16 path only by weights that are exact in fp16 and one
    f32 multiply per slab element, so the fp16 path's bound applies unchanged."""
    import torch
    import net_cases as nc
    fx = nc.load_net_fixture(R, blocks, hidden)
    model = nc.fixture_model(fx)
    boards = nc.fixture_boards(fx)
    n = len(boards)
    eng = make_engine("gpu", R, nc.INV_OF[R], max_games=n, max_sims=4, nn_dtype=1)
    try:
        eng.load_weights(weights.export_weights(model, 1, fc_weights="int8"))
        assert eng.nn_fc_kernel() == "k_fcw8"
        enc = np.concatenate([eng.encode([b]) for b in boards])
        lg, va = _forward_rows(eng, enc, n)
    finally:
        eng.close()
    fc = model.policyHead[4]
    q, s = weights.quantize_fc(fc.weight)
    bias = fc.bias.detach().double()
    model.policyHead[4] = torch.nn.Identity()
    del fc
    model.double()
    with torch.no_grad():
        flat, value = model(torch.from_numpy(enc).double())
        ref = torch.empty(n, q.shape[0], dtype=torch.float64)
        for c in range(0, q.shape[0], 1024):
            ref[:, c:c + 1024] = flat @ (q[c:c + 1024].double() * s[c:c + 1024].double()[:, None]).t()
        ref += bias[None, :]
    el = float(np.abs(lg[:n] - ref.numpy()).max())
    ev = float(np.abs(va[:n] - value.numpy().reshape(-1)).max())
    print("fixture R=%d ResNet(%d,%d) int8 Linear: max|dlogit| = %.3e over all %d x %d logits, max|dvalue| = %.3e" % (
        R, blocks, hidden, el, n, q.shape[0], ev))
    assert el < TOL and ev < TOL, (el, ev)
