"""Pins the CPU oracle (oracle/fpc_oracle.cpp) against golden vectors produced by the REAL
reference (oracle/gen_golden.py -> tests/golden/ref_r{8,14}.json.gz).  CPU-only."""
import gzip
import json
import os

import numpy as np
import pytest

from oracle import orc
import evaluators

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def load(R):
    with gzip.open(os.path.join(GOLD, "ref_r%d.json.gz" % R), "rt") as f:
        return json.load(f)


@pytest.fixture(scope="module", params=[8, 14])
def gold(request):
    return load(request.param)


def test_static_dims(gold):
    R = gold["R"]
    L = orc.lib()
    assert L.orc_action_channels(R) == gold["A_ch"]
    assert L.orc_action_size(R) == gold["A"]
    assert gold["state_space_size"] == 24 * R * R
    assert gold["num_queen_moves"] == 8 * (R - 1) and gold["num_knight_moves"] == 8
    for r in range(R):
        for c in range(R):
            assert L.orc_is_legal_location(R, gold["INV"], r, c) == gold["legal_loc"][r][c]


def test_constructor_order(gold):
    """engine/board.cpp:1172-1248: unordered_map iteration + std::sort order of piece_list_."""
    R = gold["R"]
    st = gold["start"]
    b = orc.board_from_dict(R, st["turn"], st["dict"])
    assert orc.lists_of(b) == st["after_ctor"]["pl"]
    assert b.turn == st["after_ctor"]["turn"]


def test_codec(gold):
    """move.cpp:39-61 Move(flat) -> (from,to); missing `to` reads back as row R*R//R, col 0."""
    import ctypes as C
    R = gold["R"]
    L = orc.lib()
    for flat, frm, to in gold["codec_flat_to_move"]:
        f, t = C.c_int(), C.c_int()
        L.orc_flat_to_move(R, flat, C.byref(f), C.byref(t))
        assert f.value == frm
        if flat // (R * R) >= 8 * (R - 1) + 8:
            continue   # unaddressable planes (quirk Q11): reference indexes past knight_move_offsets (UB)
        if t.value == orc.NO_SQ:
            # BoardLocation() has loc_=R*R: GetRow()=R, GetCol()=0 -> R*R
            assert to == R * R
        else:
            assert t.value == to
            assert L.orc_move_flat(R, frm, to) == flat


def test_playouts(gold):
    """Replays every recorded reference call sequence: GetGameResult -> GetLegalMoves -> encode ->
    TakeAction, comparing results AND the piece-list order after every mutating call."""
    R, INV = gold["R"], gold["INV"]
    n_pos = n_children = n_term = 0
    for game in gold["playouts"]:
        b = orc.board_from_lists(R, game[0]["before"]["turn"], game[0]["before"]["pl"])
        for rec in game:
            assert b.turn == rec["before"]["turn"]
            assert orc.lists_of(b) == rec["before"]["pl"]
            res = orc.game_result(b, R, INV)
            assert res == rec["result"]
            assert orc.lists_of(b) == rec["after_result"]
            n_pos += 1
            if res != 0:
                n_term += 1
                break
            lm = orc.legal_moves(b, R, INV)
            assert lm == rec["legal"]
            assert orc.lists_of(b) == rec["after_legal"]
            if "enc" in rec:
                e = orc.encode([b], R)
                assert np.nonzero(e.flatten())[0].tolist() == rec["enc"]
            if "children" in rec:
                for fl, snap in rec["children"]:
                    nb, rc = orc.take_action(b, R, fl)
                    assert rc == 0
                    assert nb.turn == snap["turn"] and orc.lists_of(nb) == snap["pl"]
                    n_children += 1
            b, rc = orc.take_action(b, R, rec["pick"])
            assert rc == 0
    assert n_pos > 1000
    print("positions", n_pos, "children", n_children, "terminal", n_term)


def test_batch_encode_mixed_turns(gold):
    """board.cpp:354-355: whole batch rotated by states[0]'s turn (quirk Q6)."""
    R = gold["R"]
    be = gold["batch_encode"]
    boards = [orc.board_from_lists(R, s["turn"], s["pl"]) for s in be["states"]]
    e = orc.encode(boards, R)
    assert list(e.shape) == be["shape"]
    assert np.nonzero(e.flatten())[0].tolist() == be["enc"]


def _run_search(gold, rec):
    R, INV = gold["R"], gold["INV"]
    boards = [orc.board_from_lists(R, s["turn"], s["pl"]) for s in rec["before"]]
    kind = rec["kind"]
    ev = kind if kind in ("zero", "ramp") else evaluators.make(kind, R)
    rc, res = orc.search(boards, R, INV, rec["sims"], rec["C"], ev)
    return rc, res


def test_search_visit_counts(gold):
    """MCTS.search root + second-level visit counts, and the root state's piece-list order after
    the search, for every recorded (evaluator, sims, batch) case."""
    mism = []
    for si, rec in enumerate(gold["searches"]):
        rc, res = _run_search(gold, rec)
        assert rc == 0
        for g, (r, ref) in enumerate(zip(res, rec["roots"])):
            tag = (si, rec["kind"], rec["sims"], g)
            assert r["root_n"] == ref["root_n"], tag
            got = r["children"]
            exp = [[c[0], c[1]] for c in ref["children"]]
            if rec["kind"] in ("zero", "hashinf"):
                assert got == exp, tag     # exactly representable policies: must be bit-exact
            elif got != exp:
                mism.append(tag)
            assert [c[0] for c in got] == [c[0] for c in exp], tag
            assert orc.lists_of(r["board"]) == ref["after"], tag
    # ramp/hash go through torch.softmax (vendor exp, platform-dependent summation order) on the
    # reference side and through the deterministic fpc_expf spec on ours: report, don't hide.
    print("non-exact evaluator mismatches:", mism)
    assert len(mism) == 0, mism


def test_survey_kats():
    """Known-answer tests recorded in SURVEY.md section 4 (probe of the real reference)."""
    g8 = load(8)
    st = g8["start"]
    b = orc.board_from_dict(8, st["turn"], st["dict"])
    lm = orc.legal_moves(b, 8, 2)
    assert sorted(x[2] for x in lm) == [50, 51, 52, 61, 114, 115, 116, 125, 189, 253, 317, 956, 2746, 3196]
    b = orc.board_from_dict(8, st["turn"], st["dict"])
    rc, res = orc.search([b], 8, 2, 100, 3.0, "zero")
    assert res[0]["root_n"] == 101
    assert res[0]["children"][0] == [50, 9] and all(c[1] == 8 for c in res[0]["children"][1:])
    b = orc.board_from_dict(8, st["turn"], st["dict"])
    rc, res = orc.search([b], 8, 2, 100, 3.0, "ramp")
    assert res[0]["children"] == [[50, 2], [51, 2], [52, 2], [61, 2], [114, 2], [115, 5], [116, 5], [125, 7],
                                  [189, 20], [253, 6], [317, 2], [956, 45], [2746, 7], [3196, 6]]
    g14 = load(14)
    st = g14["start"]
    b = orc.board_from_dict(14, st["turn"], st["dict"])
    lm = orc.legal_moves(b, 14, 3)
    assert sorted(x[2] for x in lm) == list(range(171, 179)) + list(range(367, 375)) + [20962, 20967, 21354, 21359]
    b = orc.board_from_dict(14, st["turn"], st["dict"])
    rc, res = orc.search([b], 14, 3, 100, 3.0, "zero")
    assert res[0]["root_n"] == 101
    assert [c[1] for c in res[0]["children"]] == [6] * 19 + [5]
    # knight at (4,4) on 8x8: exactly 4 moves (quirk Q8)
    kb = orc.board_from_lists(8, 0, [[[4 * 8 + 4, 1], [7 * 8 + 4, 5]], [], [], []])
    lm = orc.legal_moves(kb, 8, 2)
    kn = sorted(x[1] for x in lm if x[0] == 36)
    assert kn == [3 * 8 + 2, 3 * 8 + 6, 5 * 8 + 2, 5 * 8 + 6]


def test_expf_accuracy():
    L = orc.lib()
    # the last tenth in front of the flush threshold has a grid of its own: -86 itself is still in the domain
    xs = np.concatenate([np.linspace(-85.9, 0, 20001), -np.logspace(-8, 1.9, 2000), np.linspace(-86.0, -85.9, 2001)]).astype(np.float32)
    got = np.array([L.orc_expf(float(x)) for x in xs], dtype=np.float32)
    ref = np.exp(xs.astype(np.float64))
    rel = np.abs(got.astype(np.float64) - ref) / ref
    assert rel.max() < 2.5e-7          # <= ~2 ulp
    assert L.orc_expf(0.0) == 1.0 and L.orc_expf(float("-inf")) == 0.0 and L.orc_expf(-90.0) == 0.0
    # the first f32 below -86 is flushed, -86 is not
    assert L.orc_expf(float(np.nextafter(np.float32(-86), np.float32(-np.inf)))) == 0.0 and L.orc_expf(-86.0) > 0.0


@pytest.mark.parametrize("R", [8, 14])
def test_attacked_square_queries_vs_reference(R):
    """wrapper.cpp:201-206 (GetAttackedSquaresPlayers / GetAttackedSquaresTeams / IsAttackedByPlayer / GetSimpleState):
    the oracle's restatement against tests/golden/ref_attack_r{R}.json.gz, dumped from the real reference build
    (oracle/gen_attack_golden.py) -- per colour / team the reported squares IN THE REFERENCE'S ORDER (row-major; a
    colour or team without an attacked square has no entry), and the single-square query for every (square, colour)."""
    import gzip
    import json
    import os
    import numpy as np
    INV = {8: 2, 14: 3}[R]
    with gzip.open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ref_attack_r%d.json.gz" % R), "rt") as f:
        g = json.load(f)
    assert g["R"] == R and len(g["cases"]) >= 300
    n_single = 0
    for case in g["cases"]:
        b = orc.board_from_lists(R, case["turn"], case["pl"])
        maps = orc.attack_maps(b, R, INV)
        for colour in range(4):
            want = case["players"].get(str(colour), [])
            assert [int(x) for x in np.nonzero(maps[colour])[0]] == want, (case["pos"], colour)
        for team in range(2):
            want = case["teams"].get(str(team), [])
            assert [int(x) for x in np.nonzero(maps[4 + team])[0]] == want, (case["pos"], team)
        if "by_player" in case:
            n_single += 1
            for colour in range(4):
                got = [1 if orc.is_attacked_by_player(b, R, sq, colour) else 0 for sq in range(R * R)]
                assert got == case["by_player"][colour], (case["pos"], colour)
            assert case["simple"]["turn"] == case["turn"] and case["simple"]["attacked"] == case["players"]
            # (the generator rebuilt the position through the reference's constructor, which orders the piece lists its own way)
            assert [sorted(col) for col in case["simple"]["pieces"]] == [sorted(col) for col in case["pl"]]
    assert n_single >= 30
