#!/usr/bin/env python3
"""Refill (fpc_search_advance_refill, selfplay.play(refill=...)): does a batch that stays full finish games faster?

    python3 tools/refill_bench.py --out DIR [--games 768] [--slots 256] [--sims 400] [--length 12] [--repeats 3]

Plays the same M start positions twice with the same network (ResNet(blocks, hidden), seeded random weights, fp16),
rules, simulations per ply and max_game_length L:
    plain   ceil(M / G) runs of selfplay.play over G positions each -- a run shrinks as its games end and lasts as long
            as its longest game (the loop as it is without this feature);
    refill  one run of G slots in which a finished game's position goes to the next start position.
Both with a fresh tree every ply (fpc_search_begin) and with the played move's subtree kept (fpc_search_advance /
fpc_search_advance_refill; max_sims = 2 x sims), the four arms alternating, `repeats` times, in one process after an
untimed warm-up of every path.  Start positions: seeded uniformly random playouts from the start position through the
engine's own board entry points, each cut a random 1 .. 4 plies before its end (--oversample playouts per position,
because most do not end within --playout plies; a shortage is filled from those at a random ply), so that some games
end within a few plies, at different ones, and others run on.
Per arm and repeat: wall seconds (host clock; every step ends in a device synchronise), finished games per second,
plies per second, searches (steps), mean live rows per step, and the histogram of game lengths.  If more than 90 % of
the games of an arm have one length the workload says nothing about refill and the record says so.
DIR/refill_bench.json holds one JSON record (also printed)."""
import argparse
import json
import os
import sys
import time

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(HERE, "alphazero-4-player-chess_amd"), HERE]
import numpy as np
import torch

import fpc_ffi
import net
import positions
import selfplay
import weights
from bench import Spec

MOVE_DT = np.dtype([("frm", "u1"), ("to", "u1"), ("capture", "u1"), ("promo", "u1"), ("flat", "<u2"), ("pad", "<u2")])


def start_positions(eng, M, max_plies, oversample, seed):
    """M positions still in progress from oversample * M seeded random playouts: first those of playouts that ended, cut
    1 .. 4 plies before the end; if they are fewer than M, positions at a random ply of playouts that did not end.
    Shuffled, so that every plain batch gets the same mix."""
    import ctypes as C
    N = oversample * M
    turn, entries = positions.start_entries(eng.R)
    pods = fpc_ffi.pods_of([fpc_ffi.board_from_dict(eng.R, turn, entries)] * N)
    rng = np.random.default_rng(seed)
    back, mid_at = rng.integers(1, 5, size=N), rng.integers(0, max_plies, size=N)
    ring = np.zeros((5, N, fpc_ffi.BOARD_BYTES), np.uint8)   # the last five plies of every playout (back <= 4)
    near, mid = np.zeros_like(pods), np.zeros_like(pods)
    ended_at = np.full(N, -1, np.int64)                      # the ply at which the game was found over
    live = np.arange(N)
    mv = np.zeros((N, fpc_ffi.MAX_MOVES), MOVE_DT)
    cnt = np.zeros(N, np.int32)
    for ply in range(max_plies + 1):
        cur = np.ascontiguousarray(pods[live])
        over = eng.game_result_np(cur) != 0                  # rewrites the piece lists as the reference's GetGameResult does
        done = live[over]
        ended_at[done] = ply
        near[done] = ring[(np.maximum(ply - back[done], 0)) % 5, done]
        live, cur = live[~over], np.ascontiguousarray(cur[~over])
        ring[ply % 5, live] = cur
        here = mid_at[live] == ply
        mid[live[here]] = cur[here]
        if live.size == 0 or ply == max_plies:
            break
        n = live.size
        eng._chk(eng.L.fpc_boards_legal_moves(eng.h, fpc_ffi._bp(cur), n, C.cast(mv.ctypes.data, C.POINTER(fpc_ffi.Move)),
                                              C.cast(cnt.ctypes.data, C.POINTER(C.c_int))))
        assert int(cnt[:n].min()) > 0
        pick = np.minimum((rng.random(n) * cnt[:n]).astype(np.int64), cnt[:n] - 1)
        pods[live] = eng.take_action_np(cur, mv["flat"][np.arange(n), pick].astype(np.int32))
    ended = np.nonzero(ended_at > 0)[0][:M]
    rest = np.nonzero(ended_at < 0)[0][:M - ended.size]
    assert ended.size + rest.size == M, "too few playouts: raise --oversample"
    out = np.concatenate([near[ended], mid[rest]])[rng.permutation(M)]
    assert (eng.game_result_np(out.copy()) == 0).all()
    return np.ascontiguousarray(out), {"playouts": N, "playouts_ended": int((ended_at >= 0).sum()), "near_end_positions": int(ended.size),
                                       "mid_game_positions": int(rest.size), "playout_length_mean": float(ended_at[ended_at >= 0].mean())}


def episode_fns(eng, sims, rows):
    def search_fn(pods):
        eng.search_begin(pods, 3.0)
        eng.search_run(sims)
        return eng.search_results(roots=pods)

    def continue_fn(keep_idx, picks, pods):
        if any(k < 0 for k in keep_idx):
            kept = eng.search_advance_refill(picks, keep_idx, fresh=pods, roots=pods)
        else:
            kept = eng.search_advance(picks, keep_idx, roots=pods)
        eng.search_run(min(sims, eng.max_sims - (int(kept.max()) - 1)))
        return eng.search_results(roots=pods)

    def on_searched(ids, step):
        rows.append(len(ids))

    return search_fn, continue_fn, on_searched


def run_arm(eng, boards, G, sims, args, uniforms, refill, reuse):
    rows = []
    search_fn, continue_fn, on_searched = episode_fns(eng, sims, rows)
    cont = continue_fn if reuse else None
    M = len(boards)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    if refill:
        eps = selfplay.play(search_fn, eng, boards[:G], args, uniforms, continue_fn=cont, on_searched=on_searched, refill=boards[G:])
    else:
        eps = []
        for lo in range(0, M, G):
            u = [row[lo:lo + G] for row in uniforms]
            eps += selfplay.play(search_fn, eng, boards[lo:lo + G], args, u, continue_fn=cont, on_searched=on_searched)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    lengths = np.array([e.length for e in eps])
    hist = {str(k): int(v) for k, v in zip(*np.unique(lengths, return_counts=True))}
    return {"refill": refill, "reuse_tree": reuse, "seconds": dt, "games": len(eps), "games_per_s": len(eps) / dt,
            "plies": int(lengths.sum()), "plies_per_s": float(lengths.sum()) / dt, "steps": len(rows),
            "mean_live_rows_per_step": float(np.mean(rows)), "ended_on_board": int(sum(e.result != 0 for e in eps)),
            "length_histogram": hist, "one_length_share": float(max(hist.values())) / len(eps)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", required=True)
    ap.add_argument("--games", type=int, default=768)
    ap.add_argument("--slots", type=int, default=256)
    ap.add_argument("--sims", type=int, default=400)
    ap.add_argument("--length", type=int, default=12)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--board", type=int, default=14)
    ap.add_argument("--blocks", type=int, default=10)
    ap.add_argument("--hidden", type=int, default=128)
    ap.add_argument("--playout", type=int, default=800)
    ap.add_argument("--oversample", type=int, default=5, help="playouts per start position (about a quarter of the 14x14 playouts end within 800 plies)")
    ap.add_argument("--seed", type=int, default=7)
    a = ap.parse_args()
    os.makedirs(a.out, exist_ok=True)
    R, G, M, L = a.board, a.slots, a.games, a.length
    INV = {8: 2, 14: 3}[R]
    torch.manual_seed(0)
    model = net.ResNet(Spec(R), a.blocks, a.hidden, "cpu").eval()
    eng = fpc_ffi.Engine(R, INV, max_games=G, max_sims=2 * a.sims, nn_dtype=1)
    eng.load_weights(weights.export_weights(model, 1))
    pods, gen = start_positions(eng, M, a.playout, a.oversample, a.seed)
    boards = [fpc_ffi.board_of(pods[i]) for i in range(M)]
    args = {"temperature": 1.0, "max_game_length": L, "heuristic_weight": 0.02}
    uniforms = np.random.default_rng(a.seed + 1).random((L, M)).tolist()
    arms = [(False, False), (True, False), (False, True), (True, True)]
    warm = min(M, G + 8)
    for refill, reuse in arms:                               # untimed: first launches, allocations, every path once
        run_arm(eng, boards[:warm], G, a.sims, dict(args, max_game_length=2), uniforms, refill, reuse)
    runs = []
    for rep in range(a.repeats):
        for refill, reuse in arms:
            rec = run_arm(eng, boards, G, a.sims, args, uniforms, refill, reuse)
            rec["repeat"] = rep
            runs.append(rec)
            print(json.dumps(rec), file=sys.stderr, flush=True)
        if all(r["one_length_share"] > 0.9 for r in runs):   # the workload says nothing about refill: no point in repeating it
            break
    summary = {}
    for refill, reuse in arms:
        mine = [r for r in runs if r["refill"] == refill and r["reuse_tree"] == reuse]
        gps = [r["games_per_s"] for r in mine]
        summary["%s%s" % ("refill" if refill else "plain", "+reuse_tree" if reuse else "")] = {
            "games_per_s": gps, "games_per_s_median": float(np.median(gps)), "games_per_s_min": min(gps), "games_per_s_max": max(gps),
            "plies_per_s_median": float(np.median([r["plies_per_s"] for r in mine])),
            "mean_live_rows_per_step": mine[0]["mean_live_rows_per_step"], "steps": mine[0]["steps"],
            "length_histogram": mine[0]["length_histogram"], "one_length_share": mine[0]["one_length_share"],
            "says_nothing_about_refill": mine[0]["one_length_share"] > 0.9}
    out = {"tool": "refill_bench", "board": R, "blocks": a.blocks, "hidden": a.hidden, "slots": G, "games": M, "sims": a.sims,
           "max_game_length": L, "repeats": 1 + max(r["repeat"] for r in runs), "rules": "strict", "kernel": eng.L.fpc_nn_kernel(eng.h).decode(),
           "start_positions": gen, "summary": summary, "runs": runs}
    eng.close()
    line = json.dumps(out)
    print(line, flush=True)
    with open(os.path.join(a.out, "refill_bench.json"), "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
