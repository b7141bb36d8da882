"""Subtree reuse (fpc_search_advance): the cases that run both on the wavefront emulator (tests/test_tree_reuse_emul.py)
and on the GPU (tests/test_tree_reuse_gpu.py).  Everything is compared exactly; there is no tolerance in this file."""
import numpy as np
import pytest

import evaluators
import fpc_ffi
import search_model as sm
from fpc_testlib import make_engine, roots_of
from oracle import orc

INV_OF = {8: 2, 14: 3}

#                R   G  plies sims K  evaluator  rules  root noise
CASES = {1: (8, 24, 4, 40, 1, "hash", 0, False),
         2: (8, 16, 3, 30, 2, "ramp", 0, False),
         3: (14, 12, 3, 30, 1, "hash", fpc_ffi.RULES_FIXED, True)}


def engine_vs_model(backend, case, G=None, drop_first=False):
    """engine == model after every ply and right after every advance; both kinds of pick and an expanded kept root occur.
    drop_first: the first advance also drops game 0, so that every game moves to another region."""
    R, G0, plies, sims, K, kind, rules, noise = CASES[case]
    G = G or G0
    INV = INV_OF[R]
    boards = sm.positions(R, G, seed=300 + case, rules=rules)
    ev = evaluators.make(kind, R)
    model = sm.Model([orc.clone(b) for b in boards], R, INV, 3.0, ev, rules=rules, noise_eps=0.25)
    eng = make_engine(backend, R, INV, max_games=G * K, max_sims=2 * sims)
    rng = np.random.default_rng(case)
    stats = {"visited": 0, "unvisited": 0, "expanded_roots": 0, "dropped": drop_first, "sims": []}

    def set_noise(n):
        if noise:
            gamma = rng.standard_gamma(0.3, size=(n, fpc_ffi.MAX_MOVES)).astype(np.float32)
            eng.set_root_noise(gamma, 0.25)
            model.set_noise(gamma)

    def pick(res):
        src, flats = sm.pick_rule(res, stats)
        if stats["dropped"]:
            src, flats, stats["dropped"] = src[1:], flats[1:], False
        set_noise(len(flats))
        return src, flats

    try:
        eng.set_rules(rules)
        set_noise(G)
        for ply, info in enumerate(sm.run_plies(eng, backend, roots_of(boards, R), [(sims, pick)] * plies, ev, K)):
            if ply > 0:
                kept = model.advance(info["src"], info["flats"])
                assert [int(x) for x in info["kept"]] == kept, (case, ply, "kept visits")
                sm.compare(eng, info["after"], model.results(), (case, ply, "after the advance"), grand_every=0)
                for g, root in enumerate(model.roots):
                    assert sm.same_state(fpc_ffi.board_of(info["roots"][g]), root.state), (case, ply, g, "roots_out")
                stats["expanded_roots"] += int((info["after"]["n_children"] > 0).sum())
            assert model.search(info["sims"], K) == 0
            sm.compare(eng, info["res"], model.results(), (case, ply), grand_every=5)
            stats["sims"].append(info["sims"])
    finally:
        eng.close()
    # conditions of the case, not results: if a seed misses them, change the seed or the simulation count
    if not drop_first:
        assert stats["visited"] > 0 and stats["unvisited"] > 0 and stats["expanded_roots"] > 0, stats
    return stats


def _first_ply(backend, R, G, sims, rules=0, seed=11, K=1, max_sims=None):
    INV = INV_OF[R]
    boards = sm.positions(R, G, seed=seed, rules=rules)
    ev = evaluators.make("hash", R)
    eng = make_engine(backend, R, INV, max_games=G * K, max_sims=max_sims or 2 * sims)
    eng.set_rules(rules)
    eng.set_leaves(K)
    eng.search_begin(roots_of(boards, R), 3.0)
    sm.run_steps(eng, backend, sims, ev, K)
    return eng, ev, eng.search_results()


def structure(backend):
    """right after an advance, with no model: the new root is the old child, its children the old grandchildren"""
    R, G, sims = 8, 7, 30
    eng, _, res0 = _first_ply(backend, R, G, sims)
    try:
        stats = {"visited": 0, "unvisited": 0}
        src, flats = sm.pick_rule(res0, stats)
        assert stats["visited"] > 0 and stats["unvisited"] > 0
        kidx = [int(np.nonzero(res0["flat"][g, :res0["n_children"][g]] == f)[0][0]) for g, f in zip(src, flats)]
        grand = [eng.grandchildren(g, k) for g, k in zip(src, kidx)]
        made = eng.take_action([res0["boards"][g] for g in src], flats)
        pods = np.zeros((len(src), fpc_ffi.BOARD_BYTES), np.uint8)
        kept = eng.search_advance(flats, src, roots_np=pods)
        after = eng.search_results()
        assert len(after["root_n"]) == len(src)
        for i, (g, k) in enumerate(zip(src, kidx)):
            assert int(after["root_n"][i]) == int(res0["visits"][g, k]) == int(kept[i]), i
            n = int(after["n_children"][i])
            assert [[int(after["flat"][i, j]), int(after["visits"][i, j])] for j in range(n)] == grand[i], i
            assert int(after["sims_done"][i]) == 0
            b = fpc_ffi.board_of(pods[i])
            assert bytes(b.sq) == bytes(made[i].sq) and b.turn == made[i].turn, i
            assert bytes(after["boards"][i]) == bytes(b), i
    finally:
        eng.close()


def dropping(backend):
    """FPC_RULES_FIXED rotates every row by its own side to move, so a game's search does not depend on the batch:
    advancing a strict subsequence of the games gives each survivor the search it has when all are advanced, bit for
    bit, through a further ply -- any mix-up of the games' regions shows here"""
    R, G, sims, rules = 8, 6, 14, fpc_ffi.RULES_FIXED
    sub = [1, 3, 4]

    used = []                                 # simulations per ply: what max_sims leaves room for when all games go on

    def run(only):
        eng, ev, res = _first_ply(backend, R, G, sims, rules=rules, seed=23)
        try:
            src, flats = sm.pick_rule(res)
            assert src == list(range(G))
            out = []
            for ply in range(2):
                if only is not None:
                    src, flats, only = [src[i] for i in only], [flats[i] for i in only], None
                kept = eng.search_advance(flats, src)
                if len(used) == ply:
                    used.append(min(sims, eng.max_sims - (int(kept.max()) - 1)))
                sm.run_steps(eng, backend, used[ply], ev)
                res = eng.search_results()
                out.append(res)
                n = len(res["root_n"])
                assert int(res["n_children"].min()) > 0
                src = list(range(n))
                flats = [int(res["flat"][g, int(np.argmax(res["visits"][g, :res["n_children"][g]]))]) for g in range(n)]
            return out
        finally:
            eng.close()

    everyone, survivors = run(None), run(sub)
    for a, b in zip(everyone, survivors):
        sm.same_results(a, b, sub, None)
        assert int(b["sims_done"].sum()) > 0


def budget(backend):
    """kept + new simulations up to max_sims are admitted, one more is FPC_ECAPACITY"""
    R, G, sims = 8, 4, 16
    eng, ev, res = _first_ply(backend, R, G, sims)
    try:
        flats = [int(res["flat"][g, int(np.argmax(res["visits"][g, :res["n_children"][g]]))]) for g in range(G)]
        kept = eng.search_advance(flats)
        assert int(kept.max()) > 1
        sm.run_steps(eng, backend, 2 * sims - (int(kept.max()) - 1), ev)
        with pytest.raises(RuntimeError, match="max_sims"):
            eng.search_select()
        res = eng.search_results()
        assert (res["root_n"] == kept + res["sims_done"]).all()
        assert int(res["root_n"].max()) <= 2 * sims + 1          # a fresh root after max_sims simulations
    finally:
        eng.close()


def errors(backend):
    R, G, sims = 8, 5, 12
    INV = INV_OF[R]
    eng, ev, res0 = _first_ply(backend, R, G, sims, seed=31)
    ref, _, _ = _first_ply(backend, R, G, sims, seed=31)
    try:
        flats = [int(res0["flat"][g, int(np.argmax(res0["visits"][g, :res0["n_children"][g]]))]) for g in range(G)]
        # the argument checks leave the finished search as it is
        for bad in ([1, 0, 2, 3, 4], [0, 1, 2, 3, G], [0, 1, 1, 3, 4], [-1, 1, 2, 3, 4]):
            with pytest.raises(RuntimeError, match="strictly ascending"):
                eng.search_advance(flats, bad)
        with pytest.raises(RuntimeError, match="n_games"):
            eng.search_advance(flats + [flats[0]])
        eng.set_root_noise(np.ones((G - 1, fpc_ffi.MAX_MOVES), np.float32), 0.25)
        with pytest.raises(RuntimeError, match="root noise was uploaded for %d games" % (G - 1)):
            eng.search_advance(flats)
        eng.set_root_noise(None, 0.0)
        eng.set_leaves(2)
        with pytest.raises(RuntimeError, match="max_games"):
            eng.search_advance(flats)
        eng.set_leaves(1)
        # a move that is no root child: that game is killed, the others are advanced
        wrong = list(flats)
        taken = set(int(f) for f in res0["flat"][2, :res0["n_children"][2]])
        wrong[2] = next(f for f in range(eng.A) if f not in taken)
        with pytest.raises(RuntimeError, match="game 2: piece missing for move"):
            eng.search_advance(wrong)
        rc, got = sm.results_raw(eng)
        assert rc == -7
        ref.search_advance(flats)
        want = ref.search_results()
        others = [0, 1, 3, 4]
        sm.same_results(got, want, others, others)
        assert int(got["n_children"][2]) == 0 and int(got["root_n"][2]) == 1
        sm.run_steps(eng, backend, sims, ev)                     # the killed game stays out of the search
        sm.run_steps(ref, backend, sims, ev)
        rc, got = sm.results_raw(eng)
        assert rc == -7 and int(got["sims_done"][2]) == 0
        sm.same_results(got, ref.search_results(), [0, 1], [0, 1])      # strict rules: rows before the dead one see the same batch rotation
        # call sequence: only a search whose results have been read can be advanced
        eng.search_begin(roots_of(sm.positions(R, 2, seed=3), R), 3.0)
        with pytest.raises(RuntimeError, match="fpc_search_results has not been read"):
            eng.search_advance([0, 0])
        fresh = make_engine(backend, R, INV, max_games=2, max_sims=4)
        with pytest.raises(RuntimeError, match="fpc_search_results has not been read"):
            fresh.search_advance([0, 0])
        fresh.close()
    finally:
        eng.close()
        ref.close()


def _episode_fns(eng, backend, ev, sims):
    def search_fn(pods):
        eng.search_begin(pods, 3.0)
        sm.run_steps(eng, backend, sims, ev)
        return eng.search_results(roots=pods)

    def continue_fn(keep_idx, picks, pods):
        kept = eng.search_advance(picks, keep_idx, roots=pods)
        sm.run_steps(eng, backend, min(sims, eng.max_sims - (int(kept.max()) - 1)), ev)
        return eng.search_results(roots=pods)

    return search_fn, continue_fn


def _same_episodes(a, b):
    assert len(a) == len(b)
    for x, y in zip(a, b):
        assert x.moves == y.moves and x.z == y.z and x.result == y.result and x.length == y.length, x.gid
        for (bx, fx, vx), (by, fy, vy) in zip(x.entries, y.entries):
            assert bytes(bx) == bytes(by) and np.array_equal(fx, fy) and np.array_equal(vx, vy), x.gid


def selfplay_loop(backend):
    """selfplay.play(continue_fn=...) for five plies == the model's episode (moves, pi, z); with continue_fn=None the
    episodes of an engine that has advanced before are those of an engine that never did"""
    import selfplay
    R, INV, G, sims, L = 8, 2, 6, 16, 5
    boards = sm.positions(R, G, seed=71)
    ev = evaluators.make("hash", R)
    args = {"temperature": 1.0, "max_game_length": L, "heuristic_weight": 0.5}
    uniforms = np.random.default_rng(5).random((L, G)).tolist()
    eng = make_engine(backend, R, INV, max_games=G, max_sims=2 * sims)
    fresh = make_engine(backend, R, INV, max_games=G, max_sims=2 * sims)
    try:
        search_fn, continue_fn = _episode_fns(eng, backend, ev, sims)
        eps = selfplay.play(search_fn, eng, roots_of(boards, R), args, uniforms, continue_fn=continue_fn)
        # ---- the model's episode
        model = sm.Model([orc.clone(b) for b in boards], R, INV, 3.0, ev)
        ids = list(range(G))
        moves, pis, zs, turns = {g: [] for g in ids}, {g: [] for g in ids}, {}, {g: [] for g in ids}
        keep_pos, keep_picks, last = [], [], {}
        for ply in range(L):
            if not ids:
                break
            if ply == 0:
                assert model.search(sims) == 0
            else:
                kept = model.advance(keep_pos, keep_picks)
                assert model.search(min(sims, 2 * sims - (max(kept) - 1))) == 0
            res = model.results()
            nxt_ids, keep_pos, keep_picks = [], [], []
            for i, g in enumerate(ids):
                flats = np.array([c[0] for c in res[i]["children"]], np.int32)
                visits = np.array([c[1] for c in res[i]["children"]], np.int32)
                pick = selfplay.sample_action(flats, visits, 1.0, uniforms[ply][g])
                state = model.roots[i].state
                moves[g].append(pick); pis[g].append((flats, visits)); turns[g].append(state.turn)
                nxt, mrc = orc.take_action(state, R, pick)
                assert mrc == 0
                if orc.game_result(nxt, R, INV) != 0:
                    losing = state.turn & 1
                    zs[g] = [1.0 if (t & 1) != losing else -1.0 for t in turns[g]]
                else:
                    nxt_ids.append(g); keep_pos.append(i); keep_picks.append(pick); last[g] = nxt
            ids = nxt_ids
        for g in ids:
            b = last[g]
            fb = fpc_ffi.board_from_lists(R, b.turn, orc.lists_of(b))
            h = eng.L.fpc_board_heuristic(fb, b.turn & 1) * 0.5
            zs[g] = [h if (t & 1) == (b.turn & 1) else -h for t in turns[g]]
        assert len(eps) == G
        for e in eps:
            assert e.moves == moves[e.gid], e.gid
            assert e.z == zs[e.gid], e.gid
            assert len(e.entries) == len(pis[e.gid])
            for (_, f, v), (mf, mv) in zip(e.entries, pis[e.gid]):
                assert np.array_equal(f, mf) and np.array_equal(v, mv), e.gid
        assert max(len(e.moves) for e in eps) == L
        # ---- continue_fn=None: today's loop, also on an engine that has advanced before
        a = selfplay.play(search_fn, eng, roots_of(boards, R), args, uniforms)
        b = selfplay.play(_episode_fns(fresh, backend, ev, sims)[0], fresh, roots_of(boards, R), args, uniforms)
        _same_episodes(a, b)
        assert any(x.moves != y.moves or [list(v) for _, _, v in x.entries] != [list(v) for _, _, v in y.entries]
                   for x, y in zip(a, eps))                   # and reuse does change the searches
    finally:
        eng.close()
        fresh.close()


def alphazero_reuse_tree(backend):
    """args["reuse_tree"] with an external evaluator: AlphaZero.play() goes through MCTS.continue_search and plays the
    episodes of selfplay.play(continue_fn=...) driven directly through the C-ABI (which selfplay_loop holds against
    the model); without the flag it plays those of the fresh-tree loop"""
    import torch

    import dropin_cases
    import selfplay
    R, G, sims, L, seed = 8, 4, 10, 4, 3
    az = dropin_cases.setup(backend, R)
    from alphazero import AlphaZero
    from fen_parser import parse_board_args_from_fen
    from four_player_chess_board import FourPlayerChess
    args = {"C": 3.0, "num_searches": sims, "num_parallel_games": G, "temperature": 1.0, "heuristic_weight": 0.02,
            "max_game_length": L, "replay_buffer_capacity": 100, "validation_buffer_capacity": 20}
    init = parse_board_args_from_fen(FourPlayerChess.start_fen, R)
    model = torch.nn.Linear(1, 1)
    opt = torch.optim.SGD(model.parameters(), lr=0.1)
    got = {}
    for reuse in (True, False):
        a = AlphaZero(model, opt, FourPlayerChess, dict(args, reuse_tree=reuse), init, evaluator=dropin_cases.Eval("hash", R), seed=seed)
        got[reuse] = a.play()
    uniforms = torch.rand(L, G, generator=torch.Generator().manual_seed(seed), dtype=torch.float64).tolist()
    start = [FourPlayerChess(*init)._b for _ in range(G)]
    eng = make_engine(backend, R, INV_OF[R], max_games=G, max_sims=az.engine().max_sims)
    try:
        search_fn, continue_fn = _episode_fns(eng, backend, evaluators.make("hash", R), sims)
        _same_episodes(got[True], selfplay.play(search_fn, eng, start, args, uniforms, continue_fn=continue_fn))
        _same_episodes(got[False], selfplay.play(search_fn, eng, start, args, uniforms))
    finally:
        eng.close()
