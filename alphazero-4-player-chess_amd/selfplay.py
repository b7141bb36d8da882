"""Batched self-play episodes -- the engine-side counterpart of AlphaZero.play()
(/root/reference/src/py/alphazero.py:81-178) and handle_terminal_state (:53-78).

Semantics kept from the reference:
  * one MCTS.search per ply over the still-running games, in list order (finished games are deleted
    from the list, so the batch -- and with it the Q6 batch-wide rotation -- shrinks exactly as there);
  * pi[flat] = child visit count / sum (f32), temperature pow(pi, 1/T) renormalised (f32) (:104-116);
  * the move is drawn from those probabilities (:118).  The reference uses an unseeded
    torch.multinomial; here the draw is an explicit inverse-CDF over ascending flat index driven by a
    caller-supplied uniform, so that traces are reproducible (`sample_action`);
  * TakeAction(Move(flat)) -> GetGameResult (:119-123);
  * terminal: the team that just MOVED is `losing_team`, every stored tuple of that game gets
    z = +1 if its side-to-move team != losing_team else -1 (:128-137, quirk Q12);
  * games alive after max_game_length plies are scored by the material heuristic of the side to move
    times heuristic_weight, sign by team (:161-175).
Beyond the reference (opt-in): `refill` keeps the batch full by starting a new game in a finished game's position.
Returned tuples are compact: (root position POD, flat[], visits[], z); dense tensors are rebuilt with
tuples.dense_pi / engine.encode when the trainer needs them.
"""
import math

import numpy as np

import fpc_ffi


def sample_action(flats, visits, temperature, u):
    """alphazero.py:104-119 with an explicit uniform u in [0,1)."""
    p = np.asarray(visits, dtype=np.float32)
    p = p / p.sum(dtype=np.float32)
    t = np.power(p, np.float32(1.0 / temperature), dtype=np.float32)
    t = t / t.sum(dtype=np.float32)
    c = np.cumsum(t.astype(np.float64))
    k = int(np.searchsorted(c, u * c[-1], side="right"))
    return int(flats[min(k, len(flats) - 1)])


def proven_pick(root_proof, child_proof):
    """The solver's pick rule (include/fpc_engine.h fpc_search_set_solver): the index of the child a proven root plays -- the
    first child with status LOSS under a root proven WIN, the first child with status DRAW under a root proven DRAW, at
    every temperature -- or None where the draw decides (a root proven LOSS or unknown)."""
    want = {fpc_ffi.PROOF_WIN: fpc_ffi.PROOF_LOSS, fpc_ffi.PROOF_DRAW: fpc_ffi.PROOF_DRAW}.get(int(root_proof))
    if want is None or child_proof is None:
        return None
    for k, st in enumerate(child_proof):
        if int(st) == want:
            return k
    return None


def sample_move(flats, visits, temperature, u, root_proof=0, child_proof=None):
    """The draw of the device path (include/fpc_engine.h fpc_search_play) in plain Python -- the readable
    statement of that spec and the model the tests hold k_play_ply against.  Children in the tree's order:
      temperature > 0:  w_k = pow(N_k, 1 / temperature) (libm, f64); c_k = c_{k-1} + w_k strictly left to right;
                        x = u * S with S the last sum; the pick is the first k with c_k > x, else the last child;
      temperature == 0: the first child with the largest N.
      S == 0 (no child has a visit: fpc_ffi.RULES_VISITS only): child min(n - 1, int(u * n)).
    root_proof / child_proof (the solver in effect: the statuses fpc_search_proofs reports for this root and its children):
    a proven win or draw is played whatever the draw would say (proven_pick).
    Differs from sample_action only in rounding (f64 sums of unnormalised weights against f32 probabilities
    renormalised twice): the two pick the same child unless u * S lies within about 1e-5 * S of a c_k."""
    n = len(flats)
    forced = proven_pick(root_proof, None if child_proof is None else child_proof[:n])
    if forced is not None:
        return int(flats[forced])
    if temperature == 0:
        best = 0
        for k in range(1, n):
            if int(visits[k]) > int(visits[best]):
                best = k
        return int(flats[best])
    inv = 1.0 / float(temperature)
    w = [math.pow(float(int(v)), inv) for v in visits]
    total = 0.0
    for x in w:
        total = total + x
    if total == 0.0:
        return int(flats[min(n - 1, int(float(u) * n))])
    x = float(u) * total
    c = 0.0
    for k in range(n):
        c = c + w[k]
        if c > x:
            return int(flats[k])
    return int(flats[n - 1])


class Episode:
    def __init__(self, gid, start=0):
        self.gid = gid
        self.start = start      # the loop step of the game's first search (0 unless the game came in through `refill`)
        self.entries = []       # (board POD snapshot, flats, visits)
        self.fast = []          # per entry: the ply's search was a fast one (play(playout_cap=...)); all False without the cap
        self.moves = []
        self.z = []             # per entry
        self.result = 0
        self.length = 0


def play(search_fn, eng, start_boards, args, uniforms, continue_fn=None, on_searched=None, device_play=False, refill=None,
         z_from_result=False, solver=False, targets=False, playout_cap=None, cap_uniforms=None):
    """search_fn(list_of_PODs) -> search_results dict (fpc_ffi.Engine.search_results layout) and
    leaves the PODs with the piece-list order the search produced.  uniforms[ply][gid] in [0,1): the draw of game gid at
    its OWN ply.
    continue_fn (opt-in subtree reuse, not reference semantics; None: every ply is search_fn, as in the reference):
    from the second ply on the loop calls continue_fn(keep_idx, picks_of_kept, states) instead -- keep_idx: the
    indices, within the last batch, of the games that go on (ascending), picks_of_kept: the moves they played; it
    re-roots the last search on those moves (fpc_search_advance), searches, overwrites `states` with the trees' root
    PODs and returns the same dict.  Terminal detection stays here, on this loop's own copies of the states.
    on_searched (optional): called as on_searched(ids, step) right after each step's search has returned, ids = the game
    ids of that search in batch order (AlphaZero's device replay collects the step's tuples on the device there).
    device_play (opt-in, default False): the ply's moves are chosen, made and judged on the device by ONE
    eng.search_play(temperature, uniforms of the ply) on the search search_fn / continue_fn left finished, instead of
    the per-game sample_action loop, eng.take_action and eng.game_result.  The draw is sample_move's (the same child
    as sample_action's except within rounding of a boundary); everything else in this loop is as it is.
    refill (opt-in, not reference semantics; None: the loop is the reference's, call for call): a list of further start
    PODs.  A game that ends -- on the board, or after max_game_length plies of its OWN (z from the heuristic on the
    state after its last move) -- hands its batch POSITION to the next board of `refill`, which becomes game
    len(start_boards), + 1, ...; once `refill` is used up positions are deleted as before, and the loop runs until no
    game is left.  continue_fn then gets keep_idx[i] = picks[i] = -1 at the refilled positions, with states[i] the new
    game's start board there (fpc_search_advance_refill).  Episode.start is the step of a game's first search.
    z_from_result (opt-in, not reference semantics; default False: Q12): a game that ends on the board with result r
    labels its entries by r, as FPC_RULES_TERMINAL values a terminal leaf -- 0.0 for a stalemate, else +1.0 where the
    entry's side-to-move team is the winner (WIN_RY: team 0, WIN_BG: team 1) and -1.0 where it is not.  The
    max_game_length branch is untouched.
    solver (opt-in, default False; the engine's solver must be in effect -- fpc_search_set_solver under RULES_PUCT |
    RULES_TERMINAL): the host loop plays a root proven WIN or DRAW by proven_pick from eng.search_proofs(); a root proven
    LOSS or unknown keeps sample_action's draw.  The device path needs no flag: fpc_search_play applies the same rule.
    targets (opt-in, default False; the engine's forced playouts must be in effect -- fpc_search_set_forced under RULES_PUCT
    | RULES_VISITS): Episode.entries hold the pruned visit counts of eng.search_targets() instead of the raw visits, and the
    host loop draws its move from them.  The device path's draw needs no flag: fpc_search_play draws from the same counts.
    playout_cap (opt-in, default None: the calls above, argument for argument) = {"full_prob": p, "fast_searches": n}, with
    cap_uniforms[ply][gid] in [0,1): playout cap randomization.  Game gid's search at its OWN ply is a fast search iff
    cap_uniforms[ply][gid] >= p; the loop calls search_fn(states, fast=[...]) / continue_fn(keep_idx, picks, states,
    fast=[...]) with one bool per game of the batch (mcts.MCTS.search / continue_search give those games n simulations, no
    noise and no forcing) and records the flag in Episode.fast, parallel to Episode.entries.  Under targets=True a fast
    game's entry holds its raw visits, which is what eng.search_targets() reports for it.
    Returns the list of finished Episodes (all games, in game-id order)."""
    if playout_cap is not None:
        full_prob = float(playout_cap["full_prob"])
        if not 0 < full_prob <= 1:
            raise ValueError("playout_cap: full_prob must lie in (0, 1], not %r" % (playout_cap["full_prob"],))
        if cap_uniforms is None:
            raise ValueError("playout_cap needs cap_uniforms")
        n_all = len(start_boards) + (len(refill) if refill else 0)
        if len(cap_uniforms) < int(args["max_game_length"]) or any(len(row) < n_all for row in cap_uniforms):
            raise ValueError("cap_uniforms must be [max_game_length = %d][games = %d]" % (int(args["max_game_length"]), n_all))
    states = [fpc_ffi.clone_board(b) for b in start_boards]
    ids = list(range(len(states)))
    eps = {g: Episode(g) for g in ids}
    queue = [fpc_ffi.clone_board(b) for b in refill] if refill else []
    T, L, hw = float(args["temperature"]), int(args["max_game_length"]), float(args["heuristic_weight"])
    step = 0
    while states and L > 0:
        plies = [eps[g].length for g in ids]                     # each game's own ply
        if playout_cap is None:
            fast = [False] * len(ids)
            res = search_fn(states) if continue_fn is None or step == 0 else continue_fn(keep_pos, keep_picks, states)
        else:
            fast = [bool(cap_uniforms[p][g] >= full_prob) for p, g in zip(plies, ids)]
            res = search_fn(states, fast=fast) if continue_fn is None or step == 0 else continue_fn(keep_pos, keep_picks, states, fast=fast)
        if on_searched is not None:
            on_searched(list(ids), step)
        picks = []
        proofs = eng.search_proofs() if solver and not device_play else None
        counts = eng.search_targets(res["visits"].shape[1]) if targets else res["visits"]
        for i in range(len(states)):
            n = int(res["n_children"][i])
            flats, visits = res["flat"][i, :n].copy(), counts[i, :n].copy()
            eps[ids[i]].entries.append((fpc_ffi.clone_board(states[i]), flats, visits))
            eps[ids[i]].fast.append(fast[i])
            if not device_play:
                forced = None if proofs is None else proven_pick(proofs[0][i], proofs[1][i, :n])
                picks.append(int(flats[forced]) if forced is not None else sample_action(flats, visits, T, uniforms[plies[i]][ids[i]]))
        if device_play:
            fl, results, pods = eng.search_play(T, [uniforms[p][g] for p, g in zip(plies, ids)])
            if int(fl.min()) < 0:
                raise RuntimeError("device_play: game %d has no move to play" % ids[int(fl.argmin())])
            picks = [int(f) for f in fl]
            nxt = [fpc_ffi.board_of(pods[i]) for i in range(len(states))]
        else:
            nxt = eng.take_action(states, picks)
            results = eng.game_result(nxt)
        keep_s, keep_i, keep_pos, keep_picks = [], [], [], []
        for i in range(len(states)):
            e = eps[ids[i]]
            e.moves.append(picks[i])
            e.length += 1
            if results[i] != 0:
                e.result = int(results[i])
                if z_from_result and e.result == 3:            # FPC_STALEMATE
                    e.z = [0.0 for _ in e.entries]
                elif z_from_result:
                    winner = 0 if e.result == 1 else 1         # FPC_WIN_RY: team 0, FPC_WIN_BG: team 1
                    e.z = [1.0 if (b.turn & 1) == winner else -1.0 for b, _, _ in e.entries]
                else:
                    losing_team = states[i].turn & 1           # team of the player who just moved (Q12)
                    e.z = [1.0 if (b.turn & 1) != losing_team else -1.0 for b, _, _ in e.entries]
            elif e.length == L:                                  # max_game_length reached (:161-175)
                curr_team = nxt[i].turn & 1
                h = eng.L.fpc_board_heuristic(nxt[i], curr_team) * hw
                e.z = [h if (b.turn & 1) == curr_team else -h for b, _, _ in e.entries]
            else:
                keep_s.append(nxt[i]); keep_i.append(ids[i]); keep_pos.append(i); keep_picks.append(picks[i])
                continue
            if queue:                                            # the finished game's position goes to a new game
                g = len(eps)
                eps[g] = Episode(g, start=step + 1)
                keep_s.append(queue.pop(0)); keep_i.append(g); keep_pos.append(-1); keep_picks.append(-1)
        states, ids = keep_s, keep_i
        step += 1
    return [eps[g] for g in sorted(eps)]
