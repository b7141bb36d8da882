#!/usr/bin/env python3
"""Device-side move choice (fpc_search_play): what the piece of a self-play ply between the finished search and the
advance costs on the host paths and on the device path.

    python3 tools/play_bench.py --out DIR [--sims 100] [--blocks 10] [--hidden 128]

One engine per board (14x14 with 256 games, 8x8 with 100), one finished search from the start position with the
internal network (seeded weights); every arm then works on that same finished search, which none of them changes.
The arms alternate call by call in one process, 5 warm-up rounds + 30 timed ones, wall clock per call (every arm ends
in a stream synchronise of its own):
  a_loop    the path of selfplay.play: full search_results, the per-game sample_action loop, take_action, game_result;
  b_arrays  the same with the picks on whole arrays, as bench.py's step does them (pick_moves, take_action_np,
            game_result_np);
  c_device  search_results with NULL arrays (error words only), then search_play.
In a further 5 + 30 calls with fpc_set_timing on: the wall time of search_play alone, the HIP-event time of k_play_ply
alone in those calls, and their difference (uploads, launch, read-back, synchronise).
Medians with min and max; DIR/play_bench.json holds one JSON record per board (also printed)."""
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
from bench import Spec, pick_moves

T = 1.1


def spread(ms):
    a = np.asarray(ms, np.float64)
    return {"median": float(np.median(a)), "min": float(a.min()), "max": float(a.max()), "repeats": int(a.size)}


def run(R, G, sims, blocks, hidden, warmup=5, repeats=30):
    INV = {8: 2, 14: 3}[R]
    torch.manual_seed(0)
    model = net.ResNet(Spec(R), blocks, hidden, "cpu").eval()
    eng = fpc_ffi.Engine(R, INV, max_games=G, max_sims=sims)
    eng.load_weights(weights.export_weights(model, 0))
    turn, entries = positions.start_entries(R)
    start = fpc_ffi.board_from_dict(R, turn, entries)
    boards = np.repeat(fpc_ffi.pods_of([start]), G, axis=0)
    eng.search_begin_np(boards, 3.0)
    eng.search_run(sims)
    res0 = eng.search_results(roots_np=boards)
    states = [fpc_ffi.board_of(boards[g]) for g in range(G)]
    rng = np.random.default_rng(5)

    def a_loop():
        res = eng.search_results(roots=states)
        u = rng.random(G)
        picks = []
        for i in range(G):
            n = int(res["n_children"][i])
            flats, visits = res["flat"][i, :n].copy(), res["visits"][i, :n].copy()
            picks.append(selfplay.sample_action(flats, visits, T, u[i]))
        nxt = eng.take_action(states, picks)
        return eng.game_result(nxt)

    def b_arrays():
        res = eng.search_results(roots_np=boards)
        flats = pick_moves(res, rng, T)
        nxt = eng.take_action_np(boards, flats)
        return eng.game_result_np(nxt)

    def c_device():
        eng.search_finish()
        return eng.search_play(T, rng.random(G))

    arms = {"a_loop": a_loop, "b_arrays": b_arrays, "c_device": c_device}
    ms = {k: [] for k in arms}
    for it in range(warmup + repeats):
        for name, fn in arms.items():
            t0 = time.perf_counter()
            fn()
            dt = 1e3 * (time.perf_counter() - t0)
            if it >= warmup:
                ms[name].append(dt)
    rec = {"board": R, "games": G, "sims": sims, "net": "ResNet(%d,%d)" % (blocks, hidden), "temperature": T,
           "mean_children": float(res0["n_children"].mean())}
    for name in arms:
        rec[name + "_ms"] = spread(ms[name])
    rec["a_over_c"] = rec["a_loop_ms"]["median"] / rec["c_device_ms"]["median"]
    rec["b_over_c"] = rec["b_arrays_ms"]["median"] / rec["c_device_ms"]["median"]
    eng.set_timing(True)
    call, kern = [], []
    for it in range(warmup + repeats):
        u = rng.random(G)
        t0 = time.perf_counter()
        eng.search_play(T, u)
        dt = 1e3 * (time.perf_counter() - t0)
        if it >= warmup:
            call.append(dt)
            kern.append(eng.search_play_ms())
    eng.set_timing(False)
    rec["play_call_ms"], rec["kernel_ms"] = spread(call), spread(kern)
    rec["call_minus_kernel_ms"] = rec["play_call_ms"]["median"] - rec["kernel_ms"]["median"]
    eng.close()
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", required=True)
    ap.add_argument("--sims", type=int, default=100)
    ap.add_argument("--blocks", type=int, default=10)
    ap.add_argument("--hidden", type=int, default=128)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("play_bench needs the GPU: there is nothing to measure without one")
    os.makedirs(a.out, exist_ok=True)
    with open(os.path.join(a.out, "play_bench.json"), "w") as f:
        for R, G in ((14, 256), (8, 100)):
            line = json.dumps(run(R, G, a.sims, a.blocks, a.hidden))
            print(line, flush=True)
            f.write(line + "\n")
            f.flush()


if __name__ == "__main__":
    main()
