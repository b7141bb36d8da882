"""Device-side move choice (fpc_search_play / k_play_ply): the cases that run both on the wavefront emulator
(tests/test_play_emul.py) and on the GPU (tests/test_play_gpu.py).  The model of the draw is selfplay.sample_move, the
model of the move is today's sequence fpc_search_results -> fpc_boards_take_action -> fpc_boards_game_result.
Everything is compared exactly; there is no tolerance in this file."""
import math

import numpy as np
import pytest

import evaluators
import fpc_ffi
import search_model as sm
import selfplay
from fpc_testlib import make_engine, roots_of

INV_OF = {8: 2, 14: 3}
TEMPS = (1.0, 1.1, 0.5, 0.0)

#        R  G(gpu) sims rules                 seed near_end
CASES = {1: (8, 24, 40, 0, 305, False),
         2: (14, 12, 30, fpc_ffi.RULES_FIXED, 303, False),
         3: (8, 12, 30, 0, 310, True),
         4: (8, 12, 30, fpc_ffi.RULES_FIXED, 311, True)}
USEED = {1: 43, 2: 42, 3: 43, 4: 44}          # seeds of the uniforms (chosen with the positions' so that the cases' conditions hold)

# kings on their home squares and queens of the side to move (red) on an otherwise empty board: more than 64 legal moves
# at the root, no king attacked by the other team
QUEENS = {8: ([60, 32, 3, 31], [5, 19, 20, 46, 61]),
          14: ([189, 98, 6, 97], [17, 43, 120, 131, 145])}


def _searched(backend, R, roots, sims, rules=0, max_sims=None, **kw):
    """an engine with a finished search of `roots` (engine PODs) and its full results"""
    ev = evaluators.make("hash", R)
    eng = make_engine(backend, R, INV_OF[R], max_games=len(roots), max_sims=max_sims or sims, **kw)
    eng.set_rules(rules)
    eng.search_begin(roots, 3.0)
    sm.run_steps(eng, backend, sims, ev)
    return eng, ev, eng.search_results()


def _case(backend, case, G=None):
    R, G0, sims, rules, seed, near_end = CASES[case]
    boards = sm.positions(R, G or G0, seed=seed, near_end=near_end, rules=rules)
    return _searched(backend, R, roots_of(boards, R), sims, rules=rules)


def _children(res, g):
    n = int(res["n_children"][g])
    return res["flat"][g, :n], res["visits"][g, :n]


def _model(res, T, u):
    return [selfplay.sample_move(*_children(res, g), T, u[g]) if int(res["n_children"][g]) else -1
            for g in range(len(u))]


def _sums(visits, T):
    """the spec's prefix sums c_k (f64, left to right) of one game"""
    c, out = 0.0, []
    for v in visits:
        c = c + math.pow(float(int(v)), 1.0 / T)
        out.append(c)
    return out


def _today(eng, res, flats):
    """(results, next PODs) of fpc_boards_take_action + fpc_boards_game_result on the search's root states"""
    roots = [res["boards"][g] for g in range(len(flats))]
    nxt = eng.take_action(roots, [int(f) for f in flats])
    return eng.game_result(nxt), nxt            # game_result rewrites nxt (piece-list order)


def _check_moves(eng, res, flats, results, pods, tag):
    want_r, want_b = _today(eng, res, flats)
    assert [int(x) for x in results] == [int(x) for x in want_r], tag
    for g, b in enumerate(want_b):
        assert pods[g].tobytes() == bytes(b), (tag, g)


def picks_and_moves(backend, case, G=None):
    """1 + 4: flat_out == sample_move for four temperatures; result_out / next_out == today's calls, all 288 bytes"""
    R, _, _, rules, _, near_end = CASES[case]
    eng, _, res = _case(backend, case, G)
    n = len(res["root_n"])
    rng = np.random.default_rng(USEED[case])
    stats = {"unvisited": 0, "visited": 0, "tied_max": 0, "ended": 0}
    try:
        assert int(res["n_children"].min()) > 0
        for T in TEMPS:
            u = rng.random(n)
            flats, results, pods = eng.search_play(T, u)
            assert [int(f) for f in flats] == _model(res, T, u), (case, T)
            _check_moves(eng, res, flats, results, pods, (case, T))
            again = eng.search_play(T, u)                      # idempotent
            assert np.array_equal(again[0], flats) and np.array_equal(again[1], results) and np.array_equal(again[2], pods)
            for g in range(n):
                f, v = _children(res, g)
                k = int(np.nonzero(f == flats[g])[0][0])
                stats["unvisited" if v[k] == 1 else "visited"] += 1
                if T == 0.0:
                    stats["tied_max"] += int((v == v.max()).sum() > 1)
                    assert k == int(np.argmax(v))              # numpy's argmax is the first maximum too
            stats["ended"] += int((results != 0).sum())
            assert set(int(r) for r in results) <= {0, 1, 2, 3}
    finally:
        eng.close()
    # conditions of the case, not results: if a seed misses them, change the seed
    assert stats["unvisited"] > 0 and stats["visited"] > 0, stats
    if not near_end:
        assert stats["tied_max"] > 0, stats
    else:
        assert stats["ended"] > 0, stats
    return stats


def boundaries(backend, G=None):
    """2: uniforms one ulp below, on and one ulp above two inner boundaries c_k / S of every game, u = 0 and the largest u"""
    eng, _, res = _case(backend, 1, G)
    n = len(res["root_n"])
    try:
        for T in (1.0, 1.1, 0.5):
            sums = [_sums(_children(res, g)[1], T) for g in range(n)]
            assert sum(len(c) >= 3 for c in sums) >= 2         # condition: games with two inner boundaries
            for which in (0, 1):
                # boundary k lies between child k and child k + 1; a root with two children has one, with one child none
                ks = [min((len(c) - 1) // 3 if which == 0 else (2 * (len(c) - 1)) // 3, max(len(c) - 2, 0)) for c in sums]
                u0 = np.array([c[k] / c[-1] if len(c) > 1 else 0.5 for c, k in zip(sums, ks)])
                assert (u0 > 0).all() and (u0 < 1).all()
                for u in (np.nextafter(u0, 0.0), u0, np.nextafter(u0, 1.0)):
                    flats, _, _ = eng.search_play(T, u, want_boards=False)
                    assert [int(f) for f in flats] == _model(res, T, u), (T, which)
                    if T == 1.0:                               # exact arithmetic: c_k > u * S decides on integers
                        for g in range(n):
                            f, _ = _children(res, g)
                            x = float(u[g]) * sums[g][-1]
                            if len(f) > 1:
                                assert int(flats[g]) == int(f[ks[g] if sums[g][ks[g]] > x else ks[g] + 1]), (which, g)
            for u in (np.zeros(n), np.full(n, np.nextafter(1.0, 0.0))):
                flats, _, _ = eng.search_play(T, u, want_boards=False)
                assert [int(f) for f in flats] == _model(res, T, u), T
                if T == 1.0:
                    for g in range(n):
                        f, _ = _children(res, g)
                        assert int(flats[g]) == int(f[0] if u[0] == 0.0 else f[-1]), g
    finally:
        eng.close()


def many_children(backend, R, rules=0):
    """3 (+ 4): a root with more than 64 children; the picks fall in every 64-wide pass, the last child included"""
    L = None
    if backend == "emul":
        from fpc_testlib import emul_lib
        L = emul_lib()
    kings, queens = QUEENS[R]
    root = fpc_ffi.board_from_dict(R, 0, [(k, c, 5) for c, k in enumerate(kings)] + [(q, 0, 4) for q in queens], _lib=L)
    G, sims = 4, 40
    eng, _, res = _searched(backend, R, [fpc_ffi.clone_board(root) for _ in range(G)], sims, rules=rules)
    try:
        nc = int(res["n_children"][0])
        assert nc > 64 and (res["n_children"] == nc).all()
        assert len(set(int(v) for v in _children(res, 0)[1])) > 1          # visits differ
        targets = [5, 64, 64 + (nc - 65) // 2 if nc <= 128 else 128 + (nc - 129) // 2, nc - 1]
        for T in (1.0, 0.5):
            u = []
            for g, k in enumerate(targets):
                c = _sums(_children(res, g)[1], T)
                u.append(((c[k - 1] if k else 0.0) + c[k]) / 2 / c[-1])
            flats, results, pods = eng.search_play(T, u)
            assert [int(f) for f in flats] == _model(res, T, u), (R, T)
            picked = [int(np.nonzero(_children(res, g)[0] == flats[g])[0][0]) for g in range(G)]
            assert picked == targets, (R, T, picked)
            assert set(k // 64 for k in picked) == set(range((nc + 63) // 64))
            _check_moves(eng, res, flats, results, pods, (R, T))
        flats, results, pods = eng.search_play(0.0, [0.5] * G)
        assert [int(f) for f in flats] == _model(res, 0.0, [0.5] * G)
        _check_moves(eng, res, flats, results, pods, (R, 0.0))
    finally:
        eng.close()


def tree_untouched(backend, G=None):
    """5: the results (second level included) are the same before and after search_play, and an advance on the picked
    moves gives what it gives on a twin engine that never played"""
    eng, _, res = _case(backend, 1, G)
    twin, _, res_t = _case(backend, 1, G)
    n = len(res["root_n"])
    try:
        sm.same_results(res, res_t)
        heavy = [int(np.argmax(_children(res, g)[1])) for g in range(n)]
        grand = [[eng.grandchildren(g, k) for k in (heavy[g], 0)] for g in range(n)]
        assert any(len(x[0]) > 0 for x in grand)
        u = np.random.default_rng(7).random(n)
        flats, results, _ = eng.search_play(1.0, u)
        eng.search_play(0.5, u)
        eng.search_play(0.0, u)
        sm.same_results(eng.search_results(), res)
        assert [[eng.grandchildren(g, k) for k in (heavy[g], 0)] for g in range(n)] == grand
        assert np.array_equal(eng.search_play(1.0, u)[0], flats)          # results may be read in between
        keep = [g for g in range(n) if results[g] == 0]
        assert len(keep) > 1
        pa, pb = (np.zeros((len(keep), fpc_ffi.BOARD_BYTES), np.uint8) for _ in range(2))
        ka = eng.search_advance(flats[keep], keep, roots_np=pa)
        kb = twin.search_advance(flats[keep], keep, roots_np=pb)
        assert np.array_equal(ka, kb) and np.array_equal(pa, pb)
        sm.same_results(eng.search_results(), twin.search_results())
    finally:
        eng.close()
        twin.close()


def dead_games(backend, G=None):
    """6: a root that is already terminal, and a game a failed advance killed, next to live games: -1, -1 and the root
    state for them, the live games as ever, return code 0"""
    R = 8
    eng, _, res = _case(backend, 3, G)
    try:
        terminal = None
        for g in range(len(res["root_n"])):                    # a root child that ends the game: its state is a terminal root
            f, _ = _children(res, g)
            nxt = eng.take_action([res["boards"][g]] * len(f), [int(x) for x in f])
            ended = [k for k, r in enumerate(eng.game_result(nxt)) if r != 0]
            if ended:
                terminal = nxt[ended[0]]
                break
        assert terminal is not None
        live = [res["boards"][0], res["boards"][1]]
    finally:
        eng.close()
    roots = [live[0], terminal, live[1]]
    eng, ev, res = _searched(backend, R, roots, 20, max_sims=40)
    try:
        assert [int(x) for x in res["n_children"] > 0] == [1, 0, 1]
        u = [0.3, 0.9, 0.6]
        for T in (1.0, 0.0):
            flats, results, pods = eng.search_play(T, u)
            assert int(flats[1]) == -1 and int(results[1]) == -1 and pods[1].tobytes() == bytes(res["boards"][1])
            assert [int(f) for f in flats] == _model(res, T, u)
            idx = [0, 2]
            want_r, want_b = _today(eng, {"boards": [res["boards"][g] for g in idx]}, flats[idx])
            assert [int(results[g]) for g in idx] == [int(x) for x in want_r]
            assert [pods[g].tobytes() for g in idx] == [bytes(b) for b in want_b]
        # a game whose advance failed carries an error: it is not played either
        good = [int(flats[0]), int(flats[2])]
        taken = set(int(f) for f in _children(res, 2)[0])
        wrong = next(f for f in range(eng.A) if f not in taken)
        with pytest.raises(RuntimeError, match="game 1: piece missing for move"):
            eng.search_advance([good[0], wrong], [0, 2])
        rc, after = sm.results_raw(eng)
        assert rc == -7
        flats, results, pods = eng.search_play(1.0, [0.5, 0.5])
        assert int(flats[1]) == -1 and int(results[1]) == -1 and pods[1].tobytes() == bytes(after["boards"][1])
        if int(after["n_children"][0]):
            assert int(flats[0]) == _model(after, 1.0, [0.5, 0.5])[0]
        else:
            assert int(flats[0]) == -1
    finally:
        eng.close()


def errors(backend):
    """7: call sequence and argument errors; a refused call changes nothing"""
    R, G, sims = 8, 3, 12
    boards = sm.positions(R, G, seed=31)
    fresh = make_engine(backend, R, INV_OF[R], max_games=G, max_sims=sims)
    try:
        with pytest.raises(RuntimeError, match="needs a finished search"):
            fresh.search_play(1.0, [])
        fresh.search_begin(roots_of(boards, R), 3.0)
        sm.run_steps(fresh, backend, 3, evaluators.make("hash", R))
        with pytest.raises(RuntimeError, match="needs a finished search"):
            fresh.search_play(1.0, [0.5] * G)
        fresh.search_finish()                                  # fpc_search_results with every array NULL is enough
        flats, _, _ = fresh.search_play(0.0, [0.5] * G)
        assert [int(f) for f in flats] == _model(fresh.search_results(), 0.0, [0.5] * G)
    finally:
        fresh.close()
    eng, _, res = _searched(backend, R, roots_of(boards, R), sims, max_sims=2000, avg_children=8)
    try:
        u = [0.25, 0.5, 0.75]
        good = eng.search_play(1.1, u)

        def same_as_before():
            again = eng.search_play(1.1, u)
            assert all(np.array_equal(a, b) for a, b in zip(again, good))

        for bad in (1.0, -0.25, float("nan"), np.nextafter(0.0, -1.0), 2.0):
            with pytest.raises(RuntimeError, match=r"uniform\[1\]"):
                eng.search_play(1.1, [0.25, bad, 0.75])
            same_as_before()
        for T in (-1.0, float("nan"), float("inf")):
            with pytest.raises(RuntimeError, match="temperature must be finite"):
                eng.search_play(T, u)
            same_as_before()
        with pytest.raises(RuntimeError, match="use temperature 0 for argmax"):
            eng.search_play(0.01, u)
        same_as_before()
        rc = eng.L.fpc_search_play(eng.h, 1.0, None, None, None, None)
        assert rc == -1
        same_as_before()
        assert [int(f) for f in good[0]] == _model(res, 1.1, u)
        assert [int(f) for f in eng.search_play(-0.0, u)[0]] == _model(res, 0.0, u)      # -0.0 is 0: argmax
    finally:
        eng.close()


def _same_episodes(a, b):
    assert len(a) == len(b)
    for x, y in zip(a, b):
        assert x.moves == y.moves and x.z == y.z and x.result == y.result and x.length == y.length, x.gid
        assert len(x.entries) == len(y.entries)
        for (bx, fx, vx), (by, fy, vy) in zip(x.entries, y.entries):
            assert bytes(bx) == bytes(by) and np.array_equal(fx, fy) and np.array_equal(vx, vy), x.gid


def selfplay_loop(backend, reuse, monkeypatch, G=6):
    """8: selfplay.play(device_play=True) == the host loop drawing with sample_move, episode for episode"""
    from treereuse_cases import _episode_fns
    R, sims, L = 8, 20, 12
    boards = sm.positions(R, G, seed=91, near_end=True)
    ev = evaluators.make("hash", R)
    args = {"temperature": 1.1, "max_game_length": L, "heuristic_weight": 0.5}
    uniforms = np.random.default_rng(17).random((L, G)).tolist()
    eng = make_engine(backend, R, INV_OF[R], max_games=G, max_sims=2 * sims)
    try:
        search_fn, continue_fn = _episode_fns(eng, backend, ev, sims)
        cont = continue_fn if reuse else None
        dev = selfplay.play(search_fn, eng, roots_of(boards, R), args, uniforms, continue_fn=cont, device_play=True)
        monkeypatch.setattr(selfplay, "sample_action", selfplay.sample_move)
        host = selfplay.play(search_fn, eng, roots_of(boards, R), args, uniforms, continue_fn=cont)
        _same_episodes(dev, host)
        # conditions: a game ends inside the horizon, another one runs on for several plies
        assert any(e.result != 0 for e in dev) and max(e.length for e in dev) > 2, [(e.result, e.length) for e in dev]
    finally:
        eng.close()


def alphazero_device_play(backend, monkeypatch):
    """8: AlphaZero with device_play + device_replay + reuse_tree fills the rings with what the run without device_play
    (drawing with sample_move) fills them with, byte for byte"""
    import torch

    import dropin_cases
    from replay_cases import _ring_bytes
    R = 8
    dropin_cases.setup(backend, R)
    import alphazero_cpp as az
    from alphazero import AlphaZero
    from fen_parser import parse_board_args_from_fen
    from four_player_chess_board import FourPlayerChess
    args = {"C": 3.0, "num_searches": 8, "num_parallel_games": 3, "temperature": 1.0, "heuristic_weight": 0.02,
            "max_game_length": 6, "replay_buffer_capacity": 40, "validation_buffer_capacity": 10, "reuse_tree": True,
            "device_replay": True}
    init = parse_board_args_from_fen(FourPlayerChess.start_fen, R)
    model = torch.nn.Linear(1, 1)
    opt = torch.optim.SGD(model.parameters(), lr=0.1)
    monkeypatch.setattr(selfplay, "sample_action", selfplay.sample_move)
    rings, moves = {}, {}
    for dev in (False, True):
        a = AlphaZero(model, opt, FourPlayerChess, dict(args, device_play=dev), init, evaluator=dropin_cases.Eval("hash", R), seed=11)
        eps = a.play() + a.play()
        moves[dev] = [e.moves for e in eps]
        rings[dev] = [_ring_bytes(az.engine(), ring) for ring in (0, 1)]
    assert moves[True] == moves[False]
    assert rings[True] == rings[False] and len(rings[True][0]) + len(rings[True][1]) == 36
