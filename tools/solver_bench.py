#!/usr/bin/env python3
"""The MCTS solver (fpc_search_set_solver, args["solver"] = True): what does proving wins, losses and draws in the tree change
in one ply of search -- on positions near the end of a game, where there is something to prove, and from the start
position, where there is nothing and only the extra status loads can show?

    python3 tools/solver_bench.py --out DIR [--slots 256] [--sims 400] [--repeats 3]

Both sets of G positions (tools/refill_bench.py's near-end positions; the start position G times) are searched with the
same network (ResNet(blocks, hidden), seeded random weights, fp16) for one ply of `sims` simulations under
FPC_RULES_SELFPLAY (63) with the live-row numbering on, the solver off and on alternating on ONE engine, `repeats` times,
after an untimed warm-up of every path.  Per position set and arm:
  * timed: fpc_search_begin, then fpc_search_run(sims) between device synchronisations -- the time per simulation step --
    and, in a further run with fpc_set_timing on, the fpc_stats stage times per step;
  * untimed, once: the same search through the step entry points fed by fpc_nn_forward, which report the live rows of
    every step: their sum over the ply is the number of network evaluations paid for.  Simulations completed without an
    expansion (sum of sims_done minus that sum) are the terminal backups -- and, with the solver on, the backups from
    proven nodes, which the host cannot tell apart from them; rows in which a game selected nothing (steps * G minus the
    simulations completed) are, with the solver on, the rows of games idling on a proven root;
  * the roots proven by kind (fpc_search_proofs), and the share of games in which the pick rule of fpc_search_play
    overrode the temperature-1 draw (the same uniforms with the solver off on the same finished trees).
DIR/solver_bench.json holds one JSON record (also printed)."""
import argparse
import json
import os
import sys
import time

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(HERE, "alphazero-4-player-chess_amd"), HERE, os.path.join(HERE, "tools")]
import numpy as np
import torch

import fpc_ffi
import net
import positions
import weights
from bench import Spec
from refill_bench import start_positions

ARMS = (("off", 0), ("on", 1))
RULES = fpc_ffi.RULES_SELFPLAY


def begin(eng, pods, solver):
    eng.set_rule_bits(RULES)
    eng.search_begin_np(pods, 3.0)
    eng.set_live_rows(True)                  # between begin and the first selection
    eng.set_solver(solver)


def timed_ply(eng, pods, sims, solver, stages=False):
    begin(eng, pods, solver)
    if stages:
        eng.stats_reset()
        eng.set_timing(True)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    eng.search_run(sims)
    res = eng.search_results()
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    st = None
    if stages:
        eng.set_timing(False)
        s = eng.stats()
        st = {k: float(s[k]) / sims for k in ("ms_select", "ms_tower", "ms_fc", "ms_expand")}
    return dt, res, st


def stepwise_ply(eng, pods, sims, solver):
    """the same ply through fpc_search_select / fpc_nn_forward / fpc_search_expand_select: the live rows of every step (live-row
    numbering: the network sees rows 0 .. n_live - 1)"""
    G = pods.shape[0]
    begin(eng, pods, solver)
    lg = torch.empty(G, eng.A, device="cuda")
    va = torch.empty(G, device="cuda")
    torch.cuda.synchronize()
    live = []
    n_live, enc = eng.search_select()
    for s in range(sims):
        live.append(n_live)
        last = s + 1 == sims
        if n_live == 0:
            if not last:
                n_live, enc = eng.search_select()
            continue
        eng.nn_forward(enc, n_live, lg.data_ptr(), va.data_ptr())
        if last:
            eng.search_expand(lg.data_ptr(), va.data_ptr())
        else:
            n_live, enc = eng.search_expand_select(lg.data_ptr(), va.data_ptr())
    res = eng.search_results()
    torch.cuda.synchronize()
    return np.array(live), res


def proofs_and_picks(eng, G, seed):
    """on the finished search of the solver-on arm: roots by status, and how often the pick rule overrides the draw"""
    root, _ = eng.search_proofs()
    u = np.random.default_rng(seed).random(G)
    eng.set_solver(True)
    on, _, _ = eng.search_play(1.0, u, want_boards=False)
    eng.set_solver(False)
    off, _, _ = eng.search_play(1.0, u, want_boards=False)
    return ({"unknown": int((root == 0).sum()), "win": int((root == 1).sum()), "loss": int((root == 2).sum()),
             "draw": int((root == 3).sum())}, float((on != off).mean()))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", required=True)
    ap.add_argument("--slots", type=int, default=256)
    ap.add_argument("--sims", type=int, default=400)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--board", type=int, default=14)
    ap.add_argument("--blocks", type=int, default=10)
    ap.add_argument("--hidden", type=int, default=128)
    ap.add_argument("--playout", type=int, default=800)
    ap.add_argument("--oversample", type=int, default=5)
    ap.add_argument("--seed", type=int, default=7)
    a = ap.parse_args()
    os.makedirs(a.out, exist_ok=True)
    R, G, sims = a.board, a.slots, a.sims
    INV = {8: 2, 14: 3}[R]
    torch.manual_seed(0)
    model = net.ResNet(Spec(R), a.blocks, a.hidden, "cpu").eval()
    eng = fpc_ffi.Engine(R, INV, max_games=G, max_sims=sims, nn_dtype=1)
    eng.load_weights(weights.export_weights(model, 1))
    near, gen = start_positions(eng, G, a.playout, a.oversample, a.seed)
    turn, entries = positions.start_entries(R)
    start = fpc_ffi.pods_of([fpc_ffi.board_from_dict(R, turn, entries)] * G)
    sets = (("near_end", near), ("start", start))
    for _, pods in sets:                                     # untimed: first launches, allocations, every path once
        for _, solver in ARMS:
            timed_ply(eng, pods, min(sims, 16), solver, stages=True)
            stepwise_ply(eng, pods, min(sims, 4), solver)
    runs, summary = [], {}
    for sname, pods in sets:
        for rep in range(a.repeats):
            for name, solver in ARMS:
                dt, res, _ = timed_ply(eng, pods, sims, solver)
                rec = {"positions": sname, "arm": name, "repeat": rep, "search_s": dt, "ms_per_step": 1e3 * dt / sims,
                       "sims_done": int(res["sims_done"].sum())}
                runs.append(rec)
                print(json.dumps(rec), file=sys.stderr, flush=True)
        summary[sname] = {}
        for name, solver in ARMS:
            mine = [r for r in runs if r["arm"] == name and r["positions"] == sname]
            _, _, stages = timed_ply(eng, pods, sims, solver, stages=True)
            live, res = stepwise_ply(eng, pods, sims, solver)
            done = int(res["sims_done"].sum())
            rec = {"ms_per_step": [r["ms_per_step"] for r in mine],
                   "ms_per_step_median": float(np.median([r["ms_per_step"] for r in mine])),
                   "stage_ms_per_step": stages,
                   "live_rows_summed": int(live.sum()), "steps": int(live.size), "sims_done": done,
                   "stepwise_pass_matches_timed_sims_done": bool(done == mine[0]["sims_done"]),
                   "backups_without_expansion": done - int(live.sum()),
                   "rows_without_a_selection": sims * G - done}
            if solver:
                rec["roots_proven"], rec["pick_rule_overrode_draw_share"] = proofs_and_picks(eng, G, a.seed)
            summary[sname][name] = rec
    out = {"tool": "solver_bench", "board": R, "blocks": a.blocks, "hidden": a.hidden, "slots": G, "sims": sims, "rules": RULES,
           "live_rows": True, "repeats": a.repeats, "kernel": eng.L.fpc_nn_kernel(eng.h).decode(), "near_end_positions": gen,
           "summary": summary, "runs": runs}
    eng.set_solver(False)
    eng.set_live_rows(False)
    eng.close()
    line = json.dumps(out)
    print(line, flush=True)
    with open(os.path.join(a.out, "solver_bench.json"), "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
