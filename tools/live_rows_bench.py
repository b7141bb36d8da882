#!/usr/bin/env python3
"""Live-row numbering (fpc_search_set_live_rows, args["live_rows"]): what does evaluating only the live rows of a step buy
in one ply of search on positions near the end of a game, and what does the switch cost where it cannot help?

    python3 tools/live_rows_bench.py --out DIR [--sims 400] [--repeats 3]

Searches near-end start positions (tools/refill_bench.py's: seeded random playouts cut a few plies before their end) with
the same network (ResNet(blocks, hidden), seeded random weights, fp16) for one ply of `sims` simulations under
FPC_RULES_TRAINING in four arms, alternating, `repeats` times, in one process after an untimed warm-up of every path:
  (a) 256 slots, switch off      (b) 256 slots, switch on      (c) 384 slots, off      (d) 384 slots, on
The 256-slot arms search the first 256 of the 384 positions, on an engine of 256 rows (the headline's shape: one row tile
of the policy Linear); the 384-slot arms run on an engine of 384 rows (two row tiles unless the switch skips the second).
Per arm:
  * timed: fpc_search_begin, then fpc_search_run(sims) between device synchronisations with fpc_set_timing on -- ms per
    step, the stage times per step (select / tower / fc / expand; k_live_rows counts towards select), the simulations
    completed per second;
  * untimed, once: the same search through the step entry points fed by fpc_nn_forward, which report the live rows of
    every step: min / p10 / median / p90 / max and the share of steps with more than 256 live rows.  With the switch on
    fpc_nn_forward evaluates n_live rows; the pass must complete the simulations the timed one completed.
DIR/live_rows_bench.json holds one JSON record (also printed)."""
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

ARMS = (("a_256_off", 256, 0), ("b_256_on", 256, 1), ("c_384_off", 384, 0), ("d_384_on", 384, 1))
STAGES = ("ms_select", "ms_tower", "ms_fc", "ms_expand")


def timed_ply(eng, on, pods, sims):
    eng.search_begin_np(pods, 3.0)
    eng.set_live_rows(on)
    eng.stats_reset()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    eng.search_run(sims)
    res = eng.search_results()
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    return dt, res, eng.stats()


def stepwise_ply(eng, on, pods, sims):
    """the same ply through fpc_search_select / fpc_nn_forward / fpc_search_expand_select: the live rows of every step"""
    G = pods.shape[0]
    eng.search_begin_np(pods, 3.0)
    eng.set_live_rows(on)
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
        eng.nn_forward(enc, n_live if on else G, lg.data_ptr(), va.data_ptr())
        if last:
            eng.search_expand(lg.data_ptr(), va.data_ptr())
        else:
            n_live, enc = eng.search_expand_select(lg.data_ptr(), va.data_ptr())
    res = eng.search_results()
    torch.cuda.synchronize()
    return np.array(live), res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", required=True)
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
    R, sims = a.board, a.sims
    INV = {8: 2, 14: 3}[R]
    torch.manual_seed(0)
    model = net.ResNet(Spec(R), a.blocks, a.hidden, "cpu").eval()
    blob = weights.export_weights(model, 1)
    engs = {}
    for slots in sorted(set(s for _, s, _ in ARMS)):
        engs[slots] = fpc_ffi.Engine(R, INV, max_games=slots, max_sims=sims, nn_dtype=1)
        engs[slots].load_weights(blob)
        engs[slots].set_rules(fpc_ffi.RULES_TRAINING)
        engs[slots].set_timing(True)
    del blob
    big = max(engs)
    pods, gen = start_positions(engs[big], big, a.playout, a.oversample, a.seed)
    pods_of = {slots: np.ascontiguousarray(pods[:slots]) for slots in engs}
    for _, slots, on in ARMS:                                # untimed: first launches, allocations, every path once
        timed_ply(engs[slots], on, pods_of[slots], min(sims, 16))
        stepwise_ply(engs[slots], on, pods_of[slots], min(sims, 4))
    runs = []
    for rep in range(a.repeats):
        for name, slots, on in ARMS:
            dt, res, st = timed_ply(engs[slots], on, pods_of[slots], sims)
            rec = {"arm": name, "slots": slots, "live_rows": on, "repeat": rep, "search_s": dt, "ms_per_step": 1e3 * dt / sims,
                   "sims_done": int(res["sims_done"].sum()), "sims_per_s": float(res["sims_done"].sum()) / dt}
            rec.update({k + "_per_step": st[k] / sims for k in STAGES})
            runs.append(rec)
            print(json.dumps(rec), file=sys.stderr, flush=True)
    summary = {}
    for name, slots, on in ARMS:
        mine = [r for r in runs if r["arm"] == name]
        live, res = stepwise_ply(engs[slots], on, pods_of[slots], sims)
        med = lambda k: float(np.median([r[k] for r in mine]))
        summary[name] = {"slots": slots, "live_rows": on, "ms_per_step": [r["ms_per_step"] for r in mine], "ms_per_step_median": med("ms_per_step"),
                         "sims_per_s_median": med("sims_per_s"), "sims_done": mine[0]["sims_done"],
                         "stepwise_pass_matches_timed_sims_done": bool(int(res["sims_done"].sum()) == mine[0]["sims_done"]),
                         "live_rows_per_step": {"steps": int(live.size), "min": int(live.min()), "p10": float(np.percentile(live, 10)),
                                                "median": float(np.median(live)), "p90": float(np.percentile(live, 90)),
                                                "max": int(live.max()), "share_of_steps_above_256": float((live > 256).mean())}}
        summary[name].update({k + "_per_step_median": med(k + "_per_step") for k in STAGES})
    out = {"tool": "live_rows_bench", "board": R, "blocks": a.blocks, "hidden": a.hidden, "sims": sims, "repeats": a.repeats,
           "rules": fpc_ffi.RULES_TRAINING, "kernel": engs[big].L.fpc_nn_kernel(engs[big].h).decode(), "start_positions": gen,
           "summary": summary, "runs": runs}
    for e in engs.values():
        e.close()
    line = json.dumps(out)
    print(line, flush=True)
    with open(os.path.join(a.out, "live_rows_bench.json"), "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
