"""The legal-only policy head's bit-for-bit tests (tests/test_linear_probe_gpu.py) proven able to fail,
without a GPU: the legal head's prior arithmetic in the search model (policy_head="legal") agrees with the full head's
within f32 rounding and is not the same arithmetic; single faults of the reference logits in k_policy_gemv's own
decomposition each change a prior's bits in the model's first expansion; every GPU case's coverage conditions hold for
the model alone; k_fc_unfrag's index formula, undone with numpy, gives the zero-padded row-major weights."""
import numpy as np
import pytest

import fpc_testlib  # noqa: F401  (the package path)
import legal_head_cases as lc
import search_model as sm
import tower_probe as tp
from oracle import orc


@pytest.mark.parametrize("name", list(lc.LEGAL_CASES))
def test_coverage_conditions_hold_for_the_model_alone(name):
    """what each GPU case exists for, asserted from Model.steps / Model.results(): the recorded scale exponent, roots of
    mixed turns, more than 64 children at the many-moves root, and for the pair-dealing case more than 4 x 4 x 768 pairs
    in a step, a dead row between two live rows, G > 128"""
    case = lc.legal_case(name)
    print(name, lc.check_coverage(name, case), "model: %.1f s" % case["seconds"])


def _root_logits(name):
    c, case = lc.LEGAL_CASES[name], lc.case_setup(name)
    boards = case["boards"][:lc.G]
    orc.set_rules(c["rules"])
    try:
        enc = orc.encode(boards, c["R"])
    finally:
        orc.set_rules(0)
    return c, boards, case["ev"](enc)[0]


def test_legal_spec_agrees_with_the_full_head_within_f32_rounding():
    """On the (first 12) root logits of every case: priors of orc_policy_priors_legal against orc_policy_priors.
    Measured: the largest difference is 3.6e-7 (six units in the last place of a prior near 0.5: the full head
    multiplies by a rounded 1/S before it divides by the legal mass), 831 of the 1250 priors differ in bits -- the switch
    is alive, and the difference is far below the 2e-5 the GPU suite's legal-against-full tests allow."""
    worst, differ, total = 0.0, 0, 0
    for name in lc.LEGAL_CASES:
        c, boards, logits = _root_logits(name)
        R = c["R"]
        for g, b in enumerate(boards):
            rot = b.turn if c["rules"] & sm.RULES_ROTATION else boards[0].turn
            legal = lc.legal_of(b, R, c["rules"])
            rf, full = sm._priors(logits[g], R, rot, legal, "full")
            rl, leg = sm._priors(logits[g], R, rot, legal, "legal")
            assert rf == 0 and rl == 0
            assert abs(float(leg.astype(np.float64).sum()) - 1.0) < 1e-5
            worst = max(worst, float(np.abs(full.astype(np.float64) - leg.astype(np.float64)).max()))
            differ += int((full.view(np.uint32) != leg.view(np.uint32)).sum())
            total += len(legal)
    print("largest difference %.3e; %d of %d priors differ in bits" % (worst, differ, total))
    assert worst < 2e-5
    assert differ > 0


def test_legal_spec_edges():
    """every legal logit -inf, a NaN among the legal logits: policy error; a NaN elsewhere in the row is not read; legal
    logits more than 86 below the global maximum keep their children (the full head flushes them: policy error)"""
    R = 8
    b = lc.case_boards("select-8x8-fp16")[0]
    legal = lc.legal_of(b, R, 0)
    src = [lc.source_index(R, b.turn, fl) for fl in legal]
    row = np.zeros((8 * R + 8) * R * R, np.float32)
    assert sm._priors(row, R, b.turn, legal, "legal")[0] == 0
    bad = row.copy(); bad[src] = -np.inf
    assert sm._priors(bad, R, b.turn, legal, "legal")[0] == 1
    bad = row.copy(); bad[src[1]] = np.nan
    assert sm._priors(bad, R, b.turn, legal, "legal")[0] == 1
    other = row.copy(); other[:] = np.nan; other[src] = 0.0
    rc, pri = sm._priors(other, R, b.turn, legal, "legal")
    assert rc == 0 and np.array_equal(pri, np.full(len(legal), np.float32(1) / np.float32(len(legal)), np.float32))
    one = row.copy(); one[src[0]] = -np.inf
    rc, pri = sm._priors(one, R, b.turn, legal, "legal")
    assert rc == 0 and pri[0] == 0.0 and pri[1] > 0
    # by design not the full head: legal logits more than 86 below the row's global maximum
    far = row.copy(); far[[i for i in range(len(row)) if i not in src][0]] = 100.0
    assert sm._priors(far, R, b.turn, legal, "full")[0] == 1
    rc, pri = sm._priors(far, R, b.turn, legal, "legal")
    assert rc == 0 and pri.min() > 0


def _first_expansion(name, ev=None):
    """the roots' priors after the model's first expansion (1 simulation) with the legal head"""
    c, case = lc.LEGAL_CASES[name], lc.case_setup(name)
    boards = [orc.clone(b) for b in case["boards"][:lc.G]]
    rc, res, _ = sm.search(boards, c["R"], lc.INV_OF[c["R"]], 1, 3.0, ev or case["ev"], 1, rules=c["rules"], policy_head="legal")
    assert rc == 0
    return [o["priors"] for o in res]


def _differ(a, b):
    return any(x.shape != y.shape or (x.view(np.uint32) != y.view(np.uint32)).any() for x, y in zip(a, b))


def test_single_faults_of_the_logits_change_a_priors_bits(monkeypatch):
    """one product dropped from one legal move's logit, one 8-wide chunk of a weight row taken from the next row, the
    bias of one legal column dropped, the rotation taken from turn0 where the row's own turn differs, legal move 64 of
    the many-moves root given move 0's logit: each changes at least one prior's bits in the model's first expansion"""
    name = "select-8x8-fp16"
    c, case = lc.LEGAL_CASES[name], lc.case_setup(name)
    R, boards = c["R"], case["boards"]
    base = _first_expansion(name)
    assert not _differ(base, _first_expansion(name))                 # the comparison itself: the same run, the same bits
    row = 0                                                          # game 0 is the batch's first live row: rot = its turn
    legal = lc.legal_of(boards[row], R, c["rules"])
    _, bias = tp.dense_weights(R)
    cols = [lc.source_index(R, boards[0].turn, fl) for fl in legal]
    col = next(x for x in cols[1:] if bias[x] != 0)
    for fault in lc.LOGIT_FAULTS:
        assert _differ(base, _first_expansion(name, lc.faulty(case["ev"], R, fault, row, col))), fault

    name = "many-moves-8x8-h256"
    c, case = lc.LEGAL_CASES[name], lc.case_setup(name)
    R, boards = c["R"], case["boards"]
    legal = lc.legal_of(boards[0], R, c["rules"])
    assert len(legal) > 64
    ev = lc.faulty(case["ev"], R, "copy", 0, lc.source_index(R, boards[0].turn, legal[64]), lc.source_index(R, boards[0].turn, legal[0]))
    base = _first_expansion(name)
    got = _first_expansion(name, ev)
    assert _differ(base[:1], got[:1]) and not _differ(base[1:], got[1:])

    name = "rotation-8x8-bf16"
    c, case = lc.LEGAL_CASES[name], lc.case_setup(name)
    assert c["rules"] & sm.RULES_ROTATION
    base = _first_expansion(name)
    real, seen = sm._priors, []

    def turn0_once(logits_row, R, rot, legal, policy_head="full"):
        seen.append(rot)
        if rot != seen[0] and "done" not in seen:                    # the first row whose own turn is not the batch's
            seen.append("done")
            rot = seen[0]
        return real(logits_row, R, rot, legal, policy_head)

    monkeypatch.setattr(sm, "_priors", turn0_once)
    got = _first_expansion(name)
    monkeypatch.setattr(sm, "_priors", real)
    assert "done" in seen and _differ(base, got)


@pytest.mark.parametrize("R", [8, 9])
def test_row_major_copy_of_the_policy_weights(R):
    """k_fc_unfrag's index formula (csrc/fpc_nn.h) restated with numpy on the exported "dense_int" blobs: chunk (n, k8) of
    the row-major copy comes from ((k8 >> 2) * (Np / 16) + (n >> 4)) * 64 + (k8 & 3) * 16 + (n & 15) of the fragment
    order, in units of 8 values.  The result is W in the engine's K order, zero-padded to [Np][Kp], byte for byte -- the
    rows k_policy_gemv streams (9x9 pads both Np and Kp)."""
    W, _ = tp.dense_weights(R)
    A = W.shape[0]
    for dtype in (1, 0):
        for layout in (2, 1):                                        # layouts 1 and 2: one fragment order
            t = tp.tail(R, dtype, layout, "dense_int")
            Np, Kp = t.Np, t.Kp
            frag = np.frombuffer(t.bytes, np.uint16, Np * Kp).reshape(-1, 8)
            n, k8 = np.arange(Np)[:, None], np.arange(Kp // 8)[None, :]
            src = ((k8 >> 2) * (Np // 16) + (n >> 4)) * 64 + (k8 & 3) * 16 + (n & 15)
            assert len(np.unique(src)) == src.size == frag.shape[0]  # a permutation of the chunks
            got = frag[src].reshape(Np, Kp)
            w = tp.engine_order(W, R).astype(np.float32)
            bits = w.astype(np.float16).view(np.uint16) if dtype == 1 else (w.view(np.uint32) >> 16).astype(np.uint16)
            want = np.zeros((Np, Kp), np.uint16)
            want[:A, :A] = bits
            assert got.tobytes() == want.tobytes()


def test_scaled_weights_are_normal_numbers_of_both_operand_types():
    """ "dense_scaled": W * 2^-s with |W| <= 3 and s <= 10 -- every nonzero weight of the exported blob has a nonzero
    exponent field in fp16 (smallest normal 2^-14) and bf16: a kernel that flushes denormal operands changes nothing"""
    for s in sorted(set(c["s"] for c in lc.LEGAL_CASES.values())):
        assert 2.0 ** -s >= 2.0 ** -14
    R, s = 8, 9
    for dtype, expo in ((1, 0x7c00), (0, 0x7f80)):
        t = tp.tail(R, dtype, 2, "dense_scaled", s=s)
        raw = np.frombuffer(t.bytes, np.uint16, t.Np * t.Kp)
        nz = raw[(raw & 0x7fff) != 0]
        assert nz.size > 0 and ((nz & expo) != 0).all()
