"""The softmax and prior arithmetic across the whole range of fpc_expf, everything that needs no GPU:
the coverage of tests/prior_cases.py asserted from float64 alone; the external-path cases on the wavefront emulator
against the search model and the oracle, bit for bit; the oracle against a plain float64 softmax; the two ends of
fpc_expf's domain; and the proof that the cases can fail -- single faults of the oracle's prior arithmetic
(orc.set_prior_fault) each change a prior's bits or a child set over the direct rows, while the `hash` evaluator's roots,
all the suite had before, do not see a flush threshold of -87."""
import numpy as np
import pytest

import evaluators
import fpc_testlib  # noqa: F401  (the package path)
import prior_cases as pc
import search_model as sm
from engine_cases import _compare_search
from oracle import orc

# the oracle's largest relative deviation from the float64 model over every row of the case set, measured on the CPU
# (test_oracle_against_plain_float64 prints the figure of the run: 9.607e-07, at the 14x14 many-moves root, whose legal
# mass is a sequential f32 sum of 135 equal terms; the rows of ordinary positions stay below 2.4e-7); asserted at twice this
MEASURED_REL = 9.7e-7


# ---------------------------------------------------------------------------------------------------------------------
# coverage, from the float64 model alone
# ---------------------------------------------------------------------------------------------------------------------
def test_direct_rows_cover_every_regime():
    """each of a-e and g is hit by at least 8 priors, each position of the row maximum (f) and the -86 straddle by at
    least 2 rows, over the run-to-the-end direct cases; no such case holds a refusal row"""
    for name in pc.DIRECT_CASES:
        print(name, pc.coverage([name]))
    tot = pc.coverage()
    print("direct rows, total:", tot)
    for k in "abcdeg":
        assert tot[k] >= pc.PRIOR_CAP, (k, tot)
    for k in ("f_legal", "f_illegal", "f_tail", "f_otherchunk", "f_chunk0_far", "f_chunk0_inf", "straddle"):
        assert tot[k] >= pc.ROW_CAP, (k, tot)
    assert set(c["R"] for c in pc.DIRECT_CASES.values()) == {8, 10, 14}
    big = pc.direct_case("rows-8x8-70games")
    assert big["G"] == 70 and big["n_term"] == 64 and all(c["G"] <= 16 for n, c in ((n, pc.direct_case(n)) for n in pc.DIRECT_CASES)
                                                          if n != "rows-8x8-70games")
    for name in pc.DIRECT_CASES:                       # more than 64 legal moves at the queens roots
        case = pc.direct_case(name)
        for g, nm in enumerate(case["names"]):
            assert not nm.startswith("queens:") or len(case["geo"][g][0]) > 64


def test_refusal_rows_refuse_and_only_they():
    """h: every kind of refusal on two rows of a batch of its own; sm._priors returns 1 on exactly those rows, the first
    of them is the recorded row, and the rows in front of it are fine"""
    kinds = set()
    for name in pc.REFUSAL_CASES:
        case = pc.direct_case(name)
        bad = [g for g in range(case["G"]) if sm._priors(case["rows"][g], case["R"], case["geo"][g][3], case["geo"][g][0])[0]]
        assert bad == [g for g, nm in enumerate(case["names"]) if nm.startswith("x_")], (name, bad)
        assert len(bad) >= pc.ROW_CAP and bad[0] == case["first"] == pc.first_refusal(case) and case["first"] > 0
        assert pc.model_of(case, "expand")[0] == -3
        kinds.add(case["names"][bad[0]])
        print(name, case["names"], "first refusal: row", bad[0])
    assert kinds == set(pc.REFUSE_FULL)


def test_single_rows_cover_the_legal_head():
    """i: the legal-only head's regimes over its single rows -- deep, flushed with the straddle, subnormal p / T with a
    large T (also at a root of more than 64 moves), overflow, -inf on some legal logits, the documented divergence (the
    full head refuses the row, the legal head keeps every child) -- and its refusals; the full head's single rows"""
    tot = pc.legal_coverage()
    print("legal-only head, single rows:", tot)
    for k in "acdg":
        assert tot[k] >= pc.PRIOR_CAP, (k, tot)
    for k in ("straddle", "ninf_legal", "diverge"):
        assert tot[k] >= pc.ROW_CAP, (k, tot)
    assert tot["many_moves"] >= 1
    for head in ("full", "legal"):
        rows = pc.single_rows(head)
        for name, b, row, g in rows["run"]:
            assert sm._priors(row, 8, g[3], g[0], head)[0] == 0, (head, name)
        for name, b, row, g in rows["refuse"]:
            assert sm._priors(row, 8, g[3], g[0], head)[0] == 1, (head, name)
        n = {}
        for name, *_ in rows["refuse"]:
            n[name.split("-")[0]] = n.get(name.split("-")[0], 0) + 1
        print(head, "refusal rows:", n)
    # the divergence: the same rows on the full head
    for name, b, row, g in pc.single_rows("legal")["run"]:
        if name.startswith("l_diverge"):
            assert sm._priors(row, 8, g[3], g[0], "full")[0] == 1
            rc, pri = sm._priors(row, 8, g[3], g[0], "legal")
            assert rc == 0 and (pri > 0).all()
    # every run of every single row ends on the model: what the GPU tests compare with exists
    for head in ("full", "legal"):
        for e in pc.single_rows(head)["run"]:
            for run in pc.single_runs(head, e[0]):
                assert pc.single_model(e, head, run)[0] == 0, (head, e[0], run)
    assert sum(len(pc.single_runs("full", e[0])) > 1 for e in pc.single_rows("full")["run"]) >= 2


def test_bias_row_linear_is_the_plain_export_with_that_bias():
    """tower_probe's "bias_row" Tail with a row patched in (with_bias) equals, byte for byte, the export of a Linear whose
    weights are zero and whose bias is the row -- -inf, NaN and 3e38 included: the exporter carries the bias as f32"""
    import tower_probe as tp
    rows = pc.single_rows("full")
    row = np.array(rows["run"][-1][2])                               # queens:huge
    row[7] = -np.inf; row[11] = np.nan
    for dtype, layout in ((1, 2), (0, 1)):
        t = tp.tail(8, dtype, layout, "bias_row")
        plain = tp.Tail(8, dtype, layout, "bias_row", bias_row=row)
        assert t.with_bias(row).bytes == plain.bytes and t.bytes != plain.bytes
        assert not np.frombuffer(t.bytes, np.uint16, t.Np * t.Kp).any()


# ---------------------------------------------------------------------------------------------------------------------
# the emulator (the product's tree-kernel source) against the search model and the oracle
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("way", list(pc.WAYS))
@pytest.mark.parametrize("name", list(pc.DIRECT_CASES))
def test_direct_rows_on_the_emulator(name, way):
    """one crafted row per game through fpc_search_expand / fpc_search_expand_select / two leaves per step, under the
    case's rules and root noise: children, their order, f32 priors, visits and f64 value sums equal the model's bits"""
    case = pc.direct_case(name)
    rc, model = pc.model_of(case, way)
    assert rc == 0
    eng, res = pc.engine_run("emul", case, way)
    try:
        sm.compare(eng, res, model, (name, way))
    finally:
        eng.close()
    # the oracle's own search says the same (it hands the evaluator the live rows alone: not with finished games in front)
    if way == "expand" and case["gamma"] is None and not case["n_term"]:
        rc, oref = orc_search_of(case)
        assert rc == 0
        _compare_search(res, oref, (name, "orc.search"))


def orc_search_of(case):
    orc.set_rules(case["rules"])
    try:
        return orc.search([orc.clone(b) for b in case["boards"]], case["R"], pc.INV_OF[case["R"]], 1, 3.0,
                          pc.row_evaluator(case["rows"]))
    finally:
        orc.set_rules(0)


@pytest.mark.parametrize("name", list(pc.REFUSAL_CASES))
def test_refusals_on_the_emulator_name_the_game(name):
    """the engine raises exactly where sm._priors returns 1, and names the first such game"""
    case = pc.direct_case(name)
    for way in ("expand", "multi"):
        with pytest.raises(RuntimeError, match=r"game %d: legal policy mass" % case["first"]):
            eng, _ = pc.engine_run("emul", case, way)
            eng.close()


# what a family's leaves BELOW the roots must hit (prior_cases.regimes over the model's expansions)
FAMILY_HITS = {"spread": "bc", "plateau": "bcd", "cliff": "abc", "spike": "a", "spikes8": "a", "huge": "cg", "infchunks": "c"}


@pytest.mark.parametrize("kind,R,G,sims,seed", pc.FAMILY_CASES, ids=["%s-%dx%d" % (c[0], c[1], c[1]) for c in pc.FAMILY_CASES])
def test_evaluator_families_on_the_emulator(kind, R, G, sims, seed):
    """whole searches with wide-range rows that differ leaf by leaf: rc == 0 on the oracle, the descent expands leaves
    below the roots in the family's regimes, and the emulator equals the oracle and the model"""
    c = pc.family_engine_runs("emul", kind, R, G, sims, seed, stepwise=R == 8)
    print(kind, R, "expansions below the roots:", c["n_below"], c["below"])
    assert c["n_below"] > G
    for k in FAMILY_HITS[kind]:
        assert c["below"][k] > 0, (kind, k, c["below"])


def test_families_reach_subnormal_and_flushed_leaves_below_the_roots():
    tot = dict.fromkeys("abcdeg", 0)
    for fc in pc.FAMILY_CASES:
        for k, v in pc.family_case(*fc)["below"].items():
            tot[k] += v
    print("families, below the roots:", tot)
    assert tot["b"] >= pc.PRIOR_CAP and tot["c"] >= pc.PRIOR_CAP


# ---------------------------------------------------------------------------------------------------------------------
# the oracle against plain float64
# ---------------------------------------------------------------------------------------------------------------------
def _all_rows():
    """(tag, R, row, legal, src, rot, head) of every run-to-the-end row: the direct cases and the single rows"""
    for name in pc.DIRECT_CASES:
        case = pc.direct_case(name)
        for g in range(case["n_term"], case["G"]):
            legal, src, _ill, rot = case["geo"][g]
            yield (name, g, case["names"][g]), case["R"], case["rows"][g], legal, src, rot, "full"
    for head in ("full", "legal"):
        for nm, _b, row, (legal, src, _ill, rot) in pc.single_rows(head)["run"]:
            yield ("single", head, nm), 8, row, legal, src, rot, head


def test_oracle_against_plain_float64():
    """Every run-to-the-end row: the oracle's child set equals the float64 model's (softmax in float64 with the rule
    "l - m < -86 contributes 0", masked, renormalised), and each prior lies within
        2 * MEASURED_REL * prior  +  prior * n_sub * h / T  +  [p_i subnormal] h / T  +  [prior subnormal] h,
    h = 2^-150 half a subnormal step, n_sub the legal moves whose p_i is subnormal: a subnormal p_i is off by up to h, so
    is a subnormal quotient, and the legal mass T -- whose f32 sum over subnormals is exact -- by up to n_sub * h.  The
    relative figure is measured here (printed) and recorded in MEASURED_REL and DESIGN.md 5; the oracle is deterministic,
    the factor two covers the platform's float64 exp."""
    worst, where, n, ok = 0.0, None, 0, True
    h = pc.HALF_STEP
    for tag, R, row, legal, src, rot, head in _all_rows():
        f = pc.f64_priors(row, src, head)
        rc, pri = sm._priors(row, R, rot, legal, head)
        assert rc == 0 and f is not None, tag
        assert np.array_equal(pri != 0, f["d"] >= -86), (tag, "child sets differ")
        alive = f["d"] >= -86
        sub_p = alive & (f["p"] < pc.TINY) if head == "full" else np.zeros(len(src), bool)
        absb = np.where(sub_p, h / f["T"], 0.0) + np.where(f["prior"] < pc.TINY, h, 0.0) + f["prior"] * (sub_p.sum() * h / f["T"])
        dev = np.abs(pri.astype(np.float64) - f["prior"])
        rel = np.maximum(dev - absb, 0.0)[alive] / f["prior"][alive]
        ok = ok and bool((dev <= 2 * MEASURED_REL * f["prior"] + absb).all())
        n += int(alive.sum())
        if rel.max() > worst:
            worst, where = float(rel.max()), tag
    print("oracle against float64 over %d priors: largest relative deviation %.3e at %s (recorded %.1e, asserted at twice that)"
          % (n, worst, where, MEASURED_REL))
    assert ok and worst <= 2 * MEASURED_REL
    assert worst > MEASURED_REL / 4, "the recorded figure is stale: measure again"


def test_expf_at_the_two_ends_of_its_domain():
    """test_expf_accuracy's grid (tests/test_oracle_golden.py) carried to the ends: [-86, -85.9] at the same 2.5e-7, the
    first f32 below -86 gives 0 and -86 itself does not; every result of the domain is a normal f32"""
    L = orc.lib()
    xs = np.concatenate([np.linspace(-86.0, -85.9, 4001), [-86.0, float(pc.ABOVE86)]]).astype(np.float32)
    got = np.array([L.orc_expf(float(x)) for x in xs], dtype=np.float32)
    ref = np.exp(xs.astype(np.float64))
    assert (np.abs(got.astype(np.float64) - ref) / ref).max() < 2.5e-7
    assert got.min() >= pc.TINY
    assert L.orc_expf(float(pc.BELOW86)) == 0.0 and L.orc_expf(-86.0) > 0.0
    assert L.orc_expf(-3e38) == 0.0 and L.orc_expf(float("-inf")) == 0.0 and np.isnan(L.orc_expf(float("nan")))


# ---------------------------------------------------------------------------------------------------------------------
# proof that the cases can fail
# ---------------------------------------------------------------------------------------------------------------------
def _priors_of_all_rows():
    return [(tag, sm._priors(row, R, rot, legal, head)) for tag, R, row, legal, src, rot, head in _all_rows()]


def _changed(base, got):
    """rows whose return code, child set or prior bits differ"""
    return [tag for (tag, (rc0, p0)), (_t, (rc1, p1)) in zip(base, got)
            if rc0 != rc1 or (rc0 == 0 and not np.array_equal(p0.view(np.uint32), p1.view(np.uint32)))]


def _hash_root_priors():
    """the roots of the suite's seeded `hash` searches (case_search_random_vs_oracle's evaluator), 8x8 and 14x14"""
    out = []
    for R, seed in ((8, 3), (14, 3)):
        boards = sm.positions(R, 12, seed=seed)
        logits = evaluators.make("hash", R)(orc.encode(boards, R))[0]
        for g, b in enumerate(boards):
            legal, _src, _ill, rot = pc.geometry(b, R, 0, boards[0].turn)
            out.append(((R, g), sm._priors(logits[g], R, rot, legal)))
    return out


def test_single_faults_of_the_oracle_change_bits_over_the_direct_rows():
    """orc.set_prior_fault: each single fault of the prior arithmetic changes at least one prior's bits, one child set or
    one refusal over the run-to-the-end rows -- the cases can fail -- and a flush threshold of -87 (fault 3) changes nothing
    on the `hash` evaluator's roots: the gap that was there"""
    base = _priors_of_all_rows()
    assert not _changed(base, _priors_of_all_rows())                 # the comparison itself
    hash_base = _hash_root_priors()
    try:
        for fault, what in orc.PRIOR_FAULTS.items():
            orc.set_prior_fault(fault)
            seen = _changed(base, _priors_of_all_rows())
            print("fault %d (%s): %d of %d rows change, first %s" % (fault, what, len(seen), len(base), seen[:1]))
            assert seen, (fault, what)
            if fault == 3:
                assert not _changed(hash_base, _hash_root_priors())
    finally:
        orc.set_prior_fault(0)
    assert not _changed(base, _priors_of_all_rows())                 # the switch is off again
