"""Refill (fpc_search_advance_refill): the cases that run both on the wavefront emulator (tests/test_refill_emul.py) and
on the GPU (tests/test_refill_gpu.py).  Everything is compared exactly; there is no tolerance in this file."""
import numpy as np
import pytest

import evaluators
import fpc_ffi
import refill_model as rm
import search_model as sm
from fpc_testlib import make_engine, roots_of
from oracle import orc
from treereuse_cases import INV_OF, _episode_fns, _first_ply, _same_episodes

#               R   G  K  rules                evaluator sims plies noise near-end half  max_games  seed
CASES = {"A": (8, 8, 1, 0, "hash", 24, 4, False, True, 8, 400),
         "B": (8, 6, 2, 0, "ramp", 20, 3, False, False, 16, 410),
         "C": (14, 6, 1, fpc_ffi.RULES_FIXED, "hash", 20, 3, True, False, 6, 420)}


def _pod(board_o, R):
    return roots_of([board_o], R)[0]


def _argmax_flats(res):
    return [int(res["flat"][g, int(np.argmax(res["visits"][g, :res["n_children"][g]]))]) for g in range(len(res["root_n"]))]


# ---- 1. engine == model --------------------------------------------------------------------------------------------
def engine_vs_model(backend, case):
    """engine == model after every advance (results, roots_out, kept visits) and after every ply.  Refilled: every row
    whose game is over or whose picked move (sm.pick_rule) ends it, plus row (3 * ply + 1) % n regardless; case B also
    grows from 6 to 8 rows at the second advance, one fresh row in the middle and one appended."""
    R, G, K, rules, kind, sims, plies, noise, near_half, max_games, seed = CASES[case]
    INV = INV_OF[R]
    if near_half:
        a, b = sm.positions(R, G // 2, seed=seed, rules=rules), sm.positions(R, G - G // 2, seed=seed + 1, near_end=True, rules=rules)
        boards = [x for pair in zip(a, b) for x in pair]
    else:
        boards = sm.positions(R, G, seed=seed, rules=rules)
    pool = sm.positions(R, (plies - 1) * (G + 2), seed=seed + 50, rules=rules)       # fresh boards: another seed
    ev = evaluators.make(kind, R)
    model = rm.Model([orc.clone(b) for b in boards], R, INV, 3.0, ev, rules=rules, noise_eps=0.25)
    eng = make_engine(backend, R, INV, max_games=max_games, max_sims=2 * sims)
    rng = np.random.default_rng(seed)
    cond = {"mixed": 0, "fresh_below_kept": 0, "expanded_kept_beside_fresh": 0, "fresh_then_kept": 0, "visited": 0,
            "unvisited": 0, "to_higher_index": 0}

    def set_noise(n):
        if noise:
            gamma = rng.standard_gamma(0.3, size=(n, fpc_ffi.MAX_MOVES)).astype(np.float32)
            eng.set_root_noise(gamma, 0.25)
            model.set_noise(gamma)

    try:
        eng.set_rules(rules)
        eng.set_leaves(K)
        set_noise(G)
        eng.search_begin(roots_of(boards, R), 3.0)
        n_sims, was_fresh = sims, set()
        for ply in range(plies):
            sm.run_steps(eng, backend, n_sims, ev, K)
            res = eng.search_results()
            assert model.search(n_sims, K) == 0
            sm.compare(eng, res, model.results(), (case, ply), grand_every=5)
            if ply + 1 == plies:
                break
            # ---- what the next advance does with every row
            n = len(res["root_n"])
            picked = dict(zip(*sm.pick_rule(res)))
            src, flats = [], []
            for g in range(n):
                over = g not in picked
                if not over:
                    orc.set_rules(rules)
                    try:
                        nxt, mrc = orc.take_action(orc.clone(model.roots[g].state), R, picked[g])
                        assert mrc == 0
                        over = orc.game_result(nxt, R, INV) != 0
                    finally:
                        orc.set_rules(0)
                if over or g == (3 * ply + 1) % n:
                    src.append(-1); flats.append(0)
                else:
                    src.append(g); flats.append(picked[g])
                    k = int(np.nonzero(res["flat"][g, :res["n_children"][g]] == picked[g])[0][0])
                    cond["unvisited" if res["visits"][g, k] == 1 else "visited"] += 1
                    cond["fresh_then_kept"] += g in was_fresh
            if case == "B" and ply == 1:                     # 6 -> 8 rows: a fresh row in the middle, one appended
                src[3:3] = [-1]; flats[3:3] = [0]
                src.append(-1); flats.append(0)
            fresh_o = [pool.pop() if s < 0 else None for s in src]
            set_noise(len(src))
            pods = np.zeros((len(src), fpc_ffi.BOARD_BYTES), np.uint8)
            kept = eng.search_advance_refill(flats, src, fresh=[None if b is None else _pod(b, R) for b in fresh_o], roots_np=pods)
            assert [int(x) for x in kept] == model.advance_refill(src, flats, fresh_o), (case, ply, "kept visits")
            after = eng.search_results()
            sm.compare(eng, after, model.results(), (case, ply, "after the advance"), grand_every=0)
            for g, root in enumerate(model.roots):
                assert sm.same_state(fpc_ffi.board_of(pods[g]), root.state), (case, ply, g, "roots_out")
            fresh_rows = [i for i, s in enumerate(src) if s < 0]
            kept_rows = [i for i, s in enumerate(src) if s >= 0]
            assert all(int(kept[i]) == 1 and int(after["n_children"][i]) == 0 for i in fresh_rows)
            cond["mixed"] += bool(fresh_rows and kept_rows)
            cond["fresh_below_kept"] += bool(fresh_rows and kept_rows and fresh_rows[0] < kept_rows[-1])
            cond["expanded_kept_beside_fresh"] += bool(fresh_rows) and any(int(after["n_children"][i]) > 0 for i in kept_rows)
            cond["to_higher_index"] += any(src[i] < i for i in kept_rows)
            was_fresh = set(fresh_rows)
            n_sims = min(sims, eng.max_sims - (int(kept.max()) - 1))
    finally:
        eng.close()
    # conditions of the case, not results: if a seed misses one, change the seed (on the emulator)
    need = ["mixed", "fresh_below_kept", "expanded_kept_beside_fresh", "fresh_then_kept", "visited", "unvisited"]
    assert all(cond[k] > 0 for k in need + (["to_higher_index"] if case == "B" else [])), cond
    return cond


# ---- 2. all rows fresh == fpc_search_begin ---------------------------------------------------------------------------
def all_fresh(backend):
    R, G, sims = 8, 5, 12
    eng, ev, _ = _first_ply(backend, R, G, sims, seed=41, max_sims=sims)
    other = make_engine(backend, R, INV_OF[R], max_games=G, max_sims=sims)
    try:
        boards = sm.positions(R, G, seed=42)
        pods = np.zeros((G, fpc_ffi.BOARD_BYTES), np.uint8)
        kept = eng.search_advance_refill([0] * G, [-1] * G, fresh=roots_of(boards, R), roots_np=pods)
        assert [int(k) for k in kept] == [1] * G
        for g, b in enumerate(roots_of(boards, R)):
            assert bytes(pods[g]) == bytes(b), g
        sm.run_steps(eng, backend, sims, ev)                   # a fresh root counts 0 simulations as issued: all of max_sims is there
        other.search_begin(roots_of(boards, R), 3.0)
        sm.run_steps(other, backend, sims, ev)
        a, b = eng.search_results(), other.search_results()
        sm.same_results(a, b)
        assert int(a["sims_done"].min()) > 0
    finally:
        eng.close()
        other.close()


# ---- 3. independence -----------------------------------------------------------------------------------------------
def independence(backend):
    """treereuse_cases.dropping's argument: under FPC_RULES_FIXED a search does not depend on the batch.  Through two
    plies after the advance the kept games have, bit for bit, the searches plain fpc_search_advance gives them, and
    every fresh row the search of the same board begun alone on another engine."""
    R, G, sims, rules = 8, 6, 14, fpc_ffi.RULES_FIXED
    fresh_at = [1, 4]
    kept_at = [g for g in range(G) if g not in fresh_at]
    fresh_o = sm.positions(R, len(fresh_at), seed=29, rules=rules)

    def plies_of(eng, ev, advance):
        out = []
        for ply in range(2):
            kept = advance(ply)
            assert eng.max_sims - (int(kept.max()) - 1) >= sims          # the batch-wide budget does not bind
            sm.run_steps(eng, backend, sims, ev)
            res = eng.search_results()
            assert int(res["n_children"].min()) > 0
            out.append(res)
        return out

    def batch(refill):
        eng, ev, res = _first_ply(backend, R, G, sims, rules=rules, seed=23, max_sims=4 * sims)
        try:
            src, flats = sm.pick_rule(res)
            assert src == list(range(G))

            def advance(ply):
                if ply == 0 and refill:
                    fr = [None] * G
                    for g, b in zip(fresh_at, fresh_o):
                        fr[g] = _pod(b, R)
                    return eng.search_advance_refill(flats, [-1 if g in fresh_at else g for g in range(G)], fresh=fr)
                if ply == 0:
                    return eng.search_advance(flats)
                return eng.search_advance(_argmax_flats(eng.search_results()))

            return plies_of(eng, ev, advance)
        finally:
            eng.close()

    def alone(board_o):
        eng = make_engine(backend, R, INV_OF[R], max_games=1, max_sims=4 * sims)
        ev = evaluators.make("hash", R)
        try:
            eng.set_rules(rules)

            def advance(ply):
                if ply == 0:
                    eng.search_begin([_pod(board_o, R)], 3.0)
                    return np.ones(1, np.int32)
                return eng.search_advance(_argmax_flats(eng.search_results()))

            return plies_of(eng, ev, advance)
        finally:
            eng.close()

    plain, mixed = batch(False), batch(True)
    for a, b in zip(plain, mixed):
        sm.same_results(a, b, kept_at, kept_at)
        assert int(b["sims_done"].sum()) > 0
    for g, board_o in zip(fresh_at, fresh_o):
        for a, b in zip(alone(board_o), mixed):
            sm.same_results(a, b, [0], [g])


# ---- 4. errors -----------------------------------------------------------------------------------------------------
def errors(backend):
    """every FPC_EINVAL / FPC_ESTATE case: after each refused call the finished search reads back as it was, and after all
    of them it advances to what an untouched twin engine gives (an advance consumes the search, so the twin is met once);
    a wrong move on a kept row kills that game alone"""
    R, G, sims = 8, 5, 12
    INV = INV_OF[R]
    eng, ev, res0 = _first_ply(backend, R, G, sims, seed=31, max_sims=2 * sims)
    twin, _, _ = _first_ply(backend, R, G, sims, seed=31, max_sims=2 * sims)
    big = make_engine(backend, R, INV, max_games=G + 2, max_sims=2 * sims)
    try:
        flats = _argmax_flats(res0)
        fresh_o = sm.positions(R, G + 1, seed=33)
        fresh = roots_of(fresh_o, R)

        def refused(match, *a, **kw):
            with pytest.raises(RuntimeError, match=match):
                eng.search_advance_refill(*a, **kw)
            assert eng.G == G
            sm.same_results(eng.search_results(), res0)      # the finished search stays as it was

        # the kept entries are not strictly ascending among themselves; an entry < -1 or >= G
        for bad in ([1, 0, 2, 3, 4], [0, 1, 1, 3, 4], [2, -1, 1, 3, 4], [0, -1, -1, 3, 3], [-2, 1, 2, 3, 4], [0, 1, 2, 3, G]):
            refused("strictly ascending", flats, bad, fresh=fresh[:G])
        refused("fresh is NULL", flats, [0, -1, 2, 3, 4])
        refused("n_games", flats + [flats[0]], None)          # identity is fpc_search_advance: no more games than there are
        broken = [fpc_ffi.clone_board(b) for b in fresh[:G]]
        turn1, broken[1].turn = broken[1].turn, 7
        refused(r"fresh\[1\]", flats, [0, -1, 2, 3, 4], fresh=broken)
        broken[1].turn, broken[3].castle[2] = turn1, 9         # at a kept position: not read
        refused("n_games must be positive", [], [], fresh=[])
        refused("max_games", flats + [0], [0, 1, 2, 3, 4, -1], fresh=fresh)      # 6 rows > max_games 5
        eng.set_leaves(2)
        refused("max_games", flats, [0, -1, 2, 3, 4], fresh=fresh[:G])
        eng.set_leaves(1)
        eng.set_root_noise(np.ones((G - 1, fpc_ffi.MAX_MOVES), np.float32), 0.25)
        refused("root noise was uploaded for %d games" % (G - 1), flats, [0, -1, 2, 3, 4], fresh=fresh[:G])
        eng.set_root_noise(None, 0.0)
        # after all of that the search advances to what the untouched twin gives; the board at the kept position 3 is not read
        src = [0, -1, 2, 3, 4]
        ka, kb = eng.search_advance_refill(flats, src, fresh=broken), twin.search_advance_refill(flats, src, fresh=fresh[:G])
        assert np.array_equal(ka, kb) and int(ka[1]) == 1
        sm.same_results(eng.search_results(), twin.search_results())
        # FPC_ESTATE: no search at all, and a search whose results have not been read
        sm.run_steps(eng, backend, sims, ev)
        sm.run_steps(twin, backend, sims, ev)
        res1 = eng.search_results()
        sm.same_results(res1, twin.search_results())
        with pytest.raises(RuntimeError, match="fpc_search_results has not been read"):
            big.search_advance_refill([0], [-1], fresh=fresh[:1])
        big.search_begin(roots_of(fresh_o[:2], R), 3.0)
        with pytest.raises(RuntimeError, match="fpc_search_results has not been read"):
            big.search_advance_refill([0, 0], [-1, -1], fresh=fresh[:2])
        # a move that is no root child on a kept row kills that game alone; fresh and kept rows beside it are as on the twin
        flats1 = _argmax_flats(res1)
        wrong = list(flats1)
        taken = set(int(f) for f in res1["flat"][2, :res1["n_children"][2]])
        wrong[2] = next(f for f in range(eng.A) if f not in taken)
        src = [0, 1, 2, -1, 4]
        with pytest.raises(RuntimeError, match="game 2: piece missing for move"):
            eng.search_advance_refill(wrong, src, fresh=fresh[:G])
        rc, got = sm.results_raw(eng)
        assert rc == -7
        twin.search_advance_refill(flats1, src, fresh=fresh[:G])
        others = [0, 1, 3, 4]
        sm.same_results(got, twin.search_results(), others, others)
        assert int(got["n_children"][2]) == 0 and int(got["root_n"][2]) == 1
        # more rows than the finished search had, up to max_games / leaves
        sm.run_steps(big, backend, sims, ev)
        resb = big.search_results()
        n = G + 2
        srcb = [-1, 0, -1, -1, 1, -1, -1]
        frb = [None if s >= 0 else fresh[i % G] for i, s in enumerate(srcb)]
        fb = _argmax_flats(resb)
        kept = big.search_advance_refill([0, fb[0], 0, 0, fb[1], 0, 0], srcb, fresh=frb)
        assert big.G == n and [int(k) for k in kept] == [1, int(resb["visits"][0].max()), 1, 1, int(resb["visits"][1].max()), 1, 1]
        sm.run_steps(big, backend, 2 * sims - (int(kept.max()) - 1), ev)
        res = big.search_results()
        assert (res["root_n"] == kept + res["sims_done"]).all() and int(res["sims_done"].min()) > 0
    finally:
        eng.close()
        twin.close()
        big.close()


# ---- 5. the loop ---------------------------------------------------------------------------------------------------
LOOP = dict(R=8, slots=3, games=8, sims=10, L=5)


def _loop_boards(seed):
    R, M = LOOP["R"], LOOP["games"]
    a, b = sm.positions(R, M // 2, seed=seed), sm.positions(R, M - M // 2, seed=seed + 1, near_end=True)
    return [x for pair in zip(b, a) for x in pair]


def selfplay_loop(backend, reuse):
    """selfplay.play(refill=...) with 3 slots gives, game for game, the episodes of all 8 boards played as one plain
    batch with the same uniforms (fixed rules: a search does not depend on the batch) -- with search_fn alone, and with
    continue_fn at a max_sims that never binds"""
    import selfplay
    R, S, M, sims, L = LOOP["R"], LOOP["slots"], LOOP["games"], LOOP["sims"], LOOP["L"]
    boards = roots_of(_loop_boards(seed=85), R)
    ev = evaluators.make("hash", R)
    args = {"temperature": 1.0, "max_game_length": L, "heuristic_weight": 0.5}
    uniforms = np.random.default_rng(9).random((L, M)).tolist()
    max_sims = (L + 1) * sims
    eng = make_engine(backend, R, INV_OF[R], max_games=M, max_sims=max_sims)
    try:
        eng.set_rules(fpc_ffi.RULES_FIXED)
        search_fn, _ = _episode_fns(eng, backend, ev, sims)
        bound = []

        def continue_fn(keep_idx, picks, pods):
            if any(k < 0 for k in keep_idx):
                kept = eng.search_advance_refill(picks, keep_idx, fresh=pods, roots=pods)
            else:
                kept = eng.search_advance(picks, keep_idx, roots=pods)
            bound.append(eng.max_sims - (int(kept.max()) - 1) < sims)
            sm.run_steps(eng, backend, sims, ev)
            return eng.search_results(roots=pods)

        cont = continue_fn if reuse else None
        plain = selfplay.play(search_fn, eng, boards, args, uniforms, continue_fn=cont)
        got = selfplay.play(search_fn, eng, boards[:S], args, uniforms, continue_fn=cont, refill=boards[S:])
        assert not any(bound) and len(bound) > 0 if reuse else not bound
        assert [e.gid for e in got] == list(range(M)) and all(e.start == 0 for e in plain)
        _same_episodes(got, plain)
        # conditions: games end on the board at different steps, one by its own max_game_length, and slots were refilled
        ended = sorted(set(e.start + e.length - 1 for e in got if e.result != 0))
        assert len(ended) >= 2 and any(e.result == 0 and e.length == L for e in got), [(e.start, e.length, e.result) for e in got]
        assert max(e.start for e in got) > 0 and all(e.start == 0 for e in got[:S])
    finally:
        eng.close()


def loop_positions(backend):
    """strict rules, through on_searched: a new game takes the finished game's position, and positions are deleted once
    `refill` is empty"""
    import selfplay
    R, S, M, sims, L = LOOP["R"], LOOP["slots"], LOOP["games"], LOOP["sims"], LOOP["L"]
    boards = roots_of(_loop_boards(seed=85), R)
    ev = evaluators.make("hash", R)
    args = {"temperature": 1.0, "max_game_length": L, "heuristic_weight": 0.5}
    uniforms = np.random.default_rng(9).random((L, M)).tolist()
    eng = make_engine(backend, R, INV_OF[R], max_games=S, max_sims=sims)
    seen = []
    try:
        search_fn, _ = _episode_fns(eng, backend, ev, sims)
        eps = selfplay.play(search_fn, eng, boards[:S], args, uniforms, refill=boards[S:],
                            on_searched=lambda ids, step: seen.append((step, list(ids))))
    finally:
        eng.close()
    assert [s for s, _ in seen] == list(range(len(seen))) and seen[0][1] == list(range(S))
    last = {e.gid: e.start + e.length - 1 for e in eps}          # the step of every game's last search
    nxt, took_over, deleted = S, 0, 0
    for (step, ids), (_, after) in zip(seen, seen[1:] + [(None, [])]):
        want = []
        for g in ids:
            if last[g] != step:
                want.append(g)
            elif nxt < M:                                        # the finished game's position goes to the next new game
                want.append(nxt); nxt += 1; took_over += 1
            else:
                deleted += 1
        assert after == want, (step, ids, after, want)
    assert nxt == M and took_over == M - S and deleted == S
    first = {}
    for step, ids in seen:
        for g in ids:
            first.setdefault(g, step)
    assert all(e.start == first[e.gid] for e in eps)


# ---- 6. AlphaZero with args["refill"] ------------------------------------------------------------------------------
def _alphazero_setup(backend):
    import torch

    import dropin_cases
    R = 8
    az = dropin_cases.setup(backend, R)
    from fen_parser import parse_board_args_from_fen
    from four_player_chess_board import FourPlayerChess
    init = parse_board_args_from_fen(FourPlayerChess.start_fen, R)
    model = torch.nn.Linear(1, 1)
    return az, R, FourPlayerChess, init, model, torch.optim.SGD(model.parameters(), lr=0.1)


AZ_ARGS = {"C": 3.0, "num_searches": 10, "num_parallel_games": 3, "temperature": 1.0, "heuristic_weight": 0.02,
           "max_game_length": 4, "replay_buffer_capacity": 100, "validation_buffer_capacity": 20, "refill": True}


def alphazero_refill(backend):
    """AlphaZero.play(total_games=7) with 3 slots and an external evaluator plays the episodes of
    selfplay.play(refill=...) driven directly through the C-ABI, with and without reuse_tree; learn() with the flag set
    makes that one call per iteration"""
    import torch

    import dropin_cases
    import selfplay
    az, R, FourPlayerChess, init, model, opt = _alphazero_setup(backend)
    from alphazero import AlphaZero
    G, total, sims, L, seed = AZ_ARGS["num_parallel_games"], 7, AZ_ARGS["num_searches"], AZ_ARGS["max_game_length"], 3
    got = {}
    for reuse in (True, False):
        a = AlphaZero(model, opt, FourPlayerChess, dict(AZ_ARGS, reuse_tree=reuse), init, evaluator=dropin_cases.Eval("hash", R), seed=seed)
        got[reuse] = a.play(total_games=total)
        assert len(got[reuse]) == total and max(e.start for e in got[reuse]) > 0
    uniforms = torch.rand(L, total, generator=torch.Generator().manual_seed(seed), dtype=torch.float64).tolist()
    start = [FourPlayerChess(*init)._b for _ in range(total)]
    eng = make_engine(backend, R, INV_OF[R], max_games=G, max_sims=az.engine().max_sims)
    try:
        search_fn, _ = _episode_fns(eng, backend, evaluators.make("hash", R), sims)

        def continue_fn(keep_idx, picks, pods):
            kept = eng.search_advance_refill(picks, keep_idx, fresh=pods, roots=pods)
            sm.run_steps(eng, backend, min(sims, eng.max_sims - (int(kept.max()) - 1)), evaluators.make("hash", R))
            return eng.search_results(roots=pods)

        _same_episodes(got[True], selfplay.play(search_fn, eng, start[:G], AZ_ARGS, uniforms, continue_fn=continue_fn, refill=start[G:]))
        _same_episodes(got[False], selfplay.play(search_fn, eng, start[:G], AZ_ARGS, uniforms, refill=start[G:]))
    finally:
        eng.close()
    # learn(): one play(total_games=num_games) per iteration instead of num_games // num_parallel_games plain ones
    calls = []
    a = AlphaZero(model, opt, FourPlayerChess, dict(AZ_ARGS, num_iterations=1, num_games=total, batch_size=10 ** 6), init,
                  evaluator=dropin_cases.Eval("hash", R), seed=seed)
    a.play = lambda total_games=None: calls.append(total_games)
    a.learn()
    assert calls == [total, None]                                # the iteration's games, then learn()'s validation run


def alphazero_refill_device(backend):
    """with device_replay + device_play + reuse_tree both rings hold, entry for entry, what the host buffers of a second
    object with the same seed hold"""
    import dropin_cases
    import selfplay
    import tuples
    az, R, FourPlayerChess, init, model, opt = _alphazero_setup(backend)
    from alphazero import AlphaZero
    total = 7
    args = dict(AZ_ARGS, reuse_tree=True, device_play=True)
    sample_action = selfplay.sample_action
    selfplay.sample_action = selfplay.sample_move                # the host object draws as the device does
    try:
        made = {}
        for dev in (False, True):
            a = AlphaZero(model, opt, FourPlayerChess, dict(args, device_replay=dev, device_play=dev), init,
                          evaluator=dropin_cases.Eval("hash", R), seed=13)
            made[dev] = (a, a.play(total_games=total))
    finally:
        selfplay.sample_action = sample_action
    (host, eps_h), (devc, eps_d) = made[False], made[True]
    _same_episodes(eps_h, eps_d)
    eng = az.engine()
    assert len(host.experience_buffer) + len(host.validation_buffer) == sum(e.length for e in eps_h) > total
    for ring, (hb, db) in enumerate(((host.experience_buffer, devc.experience_buffer), (host.validation_buffer, devc.validation_buffer))):
        assert len(db) == len(hb) == eng.replay_size(ring) and len(hb) > 0
        arr, n = eng.replay_read(ring)
        for r, (pod, flats, visits, z) in zip(tuples.records_of(arr, n, R), hb._items):
            assert r["mailbox"].tobytes() == bytes(pod.sq)[:R * R] and r["turn"] == pod.turn
            assert r["flat"].tolist() == list(flats) and r["visits"].tolist() == list(visits)
            assert np.float32(r["z"]) == np.float32(z)
