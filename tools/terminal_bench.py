#!/usr/bin/env python3
"""FPC_RULES_TERMINAL (fpc_set_rules bit 16, args["rules"] = "training"): what does searching past terminal leaves change
in one ply of search on positions near the end of a game?

    python3 tools/terminal_bench.py --out DIR [--slots 256] [--sims 400] [--repeats 3]

Searches the same G start positions (tools/refill_bench.py's: seeded random playouts cut a few plies before their end)
with the same network (ResNet(blocks, hidden), seeded random weights, fp16) for one ply of `sims` simulations under
FPC_RULES_FIXED (15) and under FPC_RULES_TRAINING (31), the two arms alternating, `repeats` times, in one process after
an untimed warm-up of every path.  Per arm:
  * timed: fpc_search_begin, then fpc_search_run(sims) between device synchronisations -- the time per simulation step;
    sims_done per game (p10 / median / mean) and the root visits at move time (root N - 1);
  * untimed, once: the same search through the step entry points fed by fpc_nn_forward, which report the live rows of
    every step -- the share of rows dead per step (over the first 10 steps, the last 10 and all of them), and the terminal
    backups as the simulations completed that were no expansion (sum of sims_done - sum of live rows).  The engine keeps
    no counter by kind, so the kinds are counted where the host can see them: a root child whose state is terminal is
    classified with the board entry points (lost: the side to move has no king or is mated; won: its first legal move
    takes a king; stalemate), and every visit of it beyond the one it was born with is one terminal backup of that kind.
    Terminal backups deeper in the tree are reported as one number.
DIR/terminal_bench.json holds one JSON record (also printed)."""
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
import weights
from bench import Spec
from refill_bench import start_positions

ARMS = (("fixed", fpc_ffi.RULES_FIXED), ("training", fpc_ffi.RULES_TRAINING))


def quantiles(x):
    x = np.asarray(x)
    return {"n": int(x.size), "min": int(x.min()), "p10": float(np.percentile(x, 10)), "median": float(np.median(x)),
            "mean": float(x.mean()), "p90": float(np.percentile(x, 90)), "max": int(x.max())}


def timed_ply(eng, rules, pods, sims):
    eng.set_rules(rules)
    eng.search_begin_np(pods, 3.0)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    eng.search_run(sims)
    res = eng.search_results()
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    return dt, res


def stepwise_ply(eng, rules, pods, sims):
    """the same ply through fpc_search_select / fpc_nn_forward / fpc_search_expand_select: the live rows of every step"""
    G = pods.shape[0]
    eng.set_rules(rules)
    eng.search_begin_np(pods, 3.0)
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
        eng.nn_forward(enc, G, lg.data_ptr(), va.data_ptr())
        if last:
            eng.search_expand(lg.data_ptr(), va.data_ptr())
        else:
            n_live, enc = eng.search_expand_select(lg.data_ptr(), va.data_ptr())
    res = eng.search_results()
    torch.cuda.synchronize()
    return np.array(live), res


def root_child_kinds(eng, pods, res):
    """terminal backups through terminal ROOT CHILDREN, by kind: visits - 1 of every root child whose state is terminal"""
    g_of, flats, visits = [], [], []
    for g in range(pods.shape[0]):
        n = int(res["n_children"][g])
        g_of += [g] * n
        flats += res["flat"][g, :n].tolist()
        visits += res["visits"][g, :n].tolist()
    out = {"lost": 0, "won": 0, "stalemate": 0, "terminal_root_children": 0}
    if not g_of:
        return out
    nxt = eng.take_action_np(pods[np.array(g_of)], np.array(flats, np.int32))
    result = eng.game_result_np(nxt)
    turn = nxt[:, fpc_ffi.Board.turn.offset]
    for r, t, v in zip(result.tolist(), turn.tolist(), visits):
        if r == 0:
            continue
        kind = "stalemate" if r == 3 else "won" if (1 if r == 2 else 0) == (t & 1) else "lost"
        out[kind] += int(v) - 1
        out["terminal_root_children"] += 1
    return out


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
    pods, gen = start_positions(eng, G, a.playout, a.oversample, a.seed)
    for _, rules in ARMS:                                    # untimed: first launches, allocations, every path once
        timed_ply(eng, rules, pods, min(sims, 16))
        stepwise_ply(eng, rules, pods, min(sims, 4))
    runs = []
    for rep in range(a.repeats):
        for name, rules in ARMS:
            dt, res = timed_ply(eng, rules, pods, sims)
            rec = {"arm": name, "rules": rules, "repeat": rep, "search_s": dt, "ms_per_step": 1e3 * dt / sims,
                   "sims_per_s": float(res["sims_done"].sum()) / dt,
                   "sims_done": quantiles(res["sims_done"]), "root_visits": quantiles(res["root_n"] - 1),
                   "rows_at_full_count": int((res["sims_done"] == sims).sum())}
            runs.append(rec)
            print(json.dumps(rec), file=sys.stderr, flush=True)
    summary = {}
    for name, rules in ARMS:
        mine = [r for r in runs if r["arm"] == name]
        live, res = stepwise_ply(eng, rules, pods, sims)
        eng.set_rules(rules)
        kinds = root_child_kinds(eng, pods, res)
        done = int(res["sims_done"].sum())
        dead = 1.0 - live / float(G)
        at_root = kinds["lost"] + kinds["won"] + kinds["stalemate"]
        summary[name] = {"rules": rules, "ms_per_step": [r["ms_per_step"] for r in mine],
                         "ms_per_step_median": float(np.median([r["ms_per_step"] for r in mine])),
                         "sims_done": mine[0]["sims_done"], "root_visits": mine[0]["root_visits"],
                         "rows_at_full_count": mine[0]["rows_at_full_count"],
                         "stepwise_pass_matches_timed_sims_done": bool(done == round(mine[0]["sims_done"]["mean"] * G)),
                         "dead_row_share": {"first_10_steps": float(dead[:10].mean()), "last_10_steps": float(dead[-10:].mean()),
                                            "all_steps": float(dead.mean()), "steps": int(live.size)},
                         "terminal_backups": {"total": done - int(live.sum()), "through_terminal_root_children": kinds,
                                              "deeper_in_the_tree": done - int(live.sum()) - at_root}}
    out = {"tool": "terminal_bench", "board": R, "blocks": a.blocks, "hidden": a.hidden, "slots": G, "sims": sims,
           "repeats": a.repeats, "kernel": eng.L.fpc_nn_kernel(eng.h).decode(), "start_positions": gen, "summary": summary, "runs": runs}
    eng.close()
    line = json.dumps(out)
    print(line, flush=True)
    with open(os.path.join(a.out, "terminal_bench.json"), "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
