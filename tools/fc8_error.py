#!/usr/bin/env python3
"""What does the opt-in int8 policy Linear (fc_weights="int8", weights.quantize_fc) do to a network's numbers?  CPU only.

    python3 tools/fc8_error.py [--out DIR]

For every network fixture under tests/golden/ that tests/net_cases.py can load (net_r*_b*_h*.npz: the module rebuilt from
its seed and proven equal to the recording by checksum; recnet_r*.npz: the network whose outputs the recorded searches
replay, rebuilt the same way and checked against the recorded logits) the fixture's boards are evaluated in float64
twice: with the module's own policy Linear and with its weights replaced by q * s.  Per fixture:
  max / rms |dlogit| over every logit, max |dprior| over the legal moves, the largest and mean KL(p || p8) over the legal
  moves of a board (p: softmax over the legal moves, the search's priors), and the share of boards whose most probable
  legal move is the same.
Reported, not asserted: this is what a user needs to decide whether to switch the option on.  One JSON line per fixture
and a markdown table on stdout; with --out also DIR/fc8_error.json."""
import argparse
import glob
import json
import os
import re
import sys

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(HERE, "alphazero-4-player-chess_amd"), HERE, os.path.join(HERE, "tests")]
import numpy as np
import torch

import legal_head_cases as lc
import net
import net_cases as nc
import weights
from fpc_testlib import GOLD, gold
from oracle import orc


def both_logits(model, enc):
    """float64 logits [n, A] with the module's Linear and with q * s; the Linear is applied 1024 outputs at a time"""
    fc = model.policyHead[4]
    q, s = weights.quantize_fc(fc.weight)
    w, bias = fc.weight.detach(), fc.bias.detach().double()
    model.policyHead[4] = torch.nn.Identity()
    model.double()
    with torch.no_grad():
        flat, _ = model(torch.from_numpy(enc).double())
        a = torch.empty(flat.shape[0], w.shape[0], dtype=torch.float64)
        b = torch.empty_like(a)
        for c in range(0, w.shape[0], 1024):
            a[:, c:c + 1024] = flat @ w[c:c + 1024].double().t()
            b[:, c:c + 1024] = flat @ (q[c:c + 1024].double() * s[c:c + 1024].double()[:, None]).t()
    return (a + bias[None, :]).numpy(), (b + bias[None, :]).numpy()


def figures(name, R, boards, lg, lg8):
    d = lg8 - lg
    dp, kl, same = [], [], 0
    for g, b in enumerate(boards):
        src = [lc.source_index(R, b.turn, fl) for fl in lc.legal_of(b, R, 0)]

        def soft(row):
            z = row[src] - row[src].max()
            e = np.exp(z)
            return e / e.sum()
        p, p8 = soft(lg[g]), soft(lg8[g])
        dp.append(float(np.abs(p8 - p).max()))
        kl.append(float((p * (np.log(p) - np.log(p8))).sum()))
        same += int(np.argmax(p) == np.argmax(p8))
    return {"fixture": name, "board": R, "boards": len(boards), "logit_sigma": float(lg.std()), "max_dlogit": float(np.abs(d).max()),
            "rms_dlogit": float(np.sqrt((d * d).mean())), "max_dprior_legal": max(dp), "max_kl_legal": max(kl),
            "mean_kl_legal": float(np.mean(kl)), "top1_agreement": same / len(boards)}


def net_fixture(path):
    R, blocks, hidden = (int(x) for x in re.match(r"net_r(\d+)_b(\d+)_h(\d+)\.npz", os.path.basename(path)).groups())
    fx = nc.load_net_fixture(R, blocks, hidden)
    model = nc.fixture_model(fx)
    g = gold(R)
    boards = []
    for gi, pi in fx["pos"]:
        snap = g["playouts"][int(gi)][int(pi)]["before"]
        boards.append(orc.board_from_lists(R, snap["turn"], snap["pl"]))
    enc = np.concatenate([orc.encode([b], R) for b in boards])
    lg, lg8 = both_logits(model, enc)
    assert float(np.abs(lg[:, fx["idx"]] - fx["logits"]).max()) < 1e-4      # the float64 forward IS the recorded network
    return figures("ResNet(%d,%d) %dx%d" % (blocks, hidden, R, R), R, boards, lg, lg8)


def recnet_fixture(path):
    R = int(re.match(r"recnet_r(\d+)\.npz", os.path.basename(path)).group(1))
    rec = nc.load_recnet(R)
    blocks, hidden, seed = (int(x) for x in re.search(r"ResNet\((\d+),(\d+)\), seed (\d+)", rec["meta"]["net"]).groups())
    torch.manual_seed(seed)
    model = net.ResNet(nc.Spec(R), blocks, hidden, "cpu")
    nc.perturb_bn(model, seed)
    model.eval()
    # the recorded calls' first rows: the module rebuilt here is the one that was recorded
    lo, hi = int(rec["enc_off"][0]), int(rec["enc_off"][1])
    x = np.zeros(24 * R * R, np.float32)
    x[rec["enc_idx"][lo:hi]] = 1.0
    with torch.no_grad():
        got = model(torch.from_numpy(x).view(1, 24, R, R))[0][0].numpy()
    assert float(np.abs(got - rec["logits"][0]).max()) < 1e-4
    boards = [orc.board_from_lists(R, s["turn"], s["pl"]) for s in rec["meta"]["before"]]
    enc = np.concatenate([orc.encode([b], R) for b in boards])
    lg, lg8 = both_logits(model, enc)
    return figures("recorded ResNet(%d,%d) %dx%d" % (blocks, hidden, R, R), R, boards, lg, lg8)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    a = ap.parse_args()
    rows = []
    for path in sorted(glob.glob(os.path.join(GOLD, "net_r*_b*_h*.npz"))):
        rows.append(net_fixture(path))
        print(json.dumps(rows[-1]), flush=True)
    for path in sorted(glob.glob(os.path.join(GOLD, "recnet_r*.npz"))):
        rows.append(recnet_fixture(path))
        print(json.dumps(rows[-1]), flush=True)
    print("| network | boards | logit sigma | max dlogit | rms dlogit | max dprior (legal) | max KL | mean KL | top-1 |")
    print("|---|---|---|---|---|---|---|---|---|")
    for r in rows:
        print("| %s | %d | %.3f | %.2e | %.2e | %.2e | %.2e | %.2e | %.3f |" % (
            r["fixture"], r["boards"], r["logit_sigma"], r["max_dlogit"], r["rms_dlogit"], r["max_dprior_legal"], r["max_kl_legal"],
            r["mean_kl_legal"], r["top1_agreement"]))
    if a.out:
        os.makedirs(a.out, exist_ok=True)
        with open(os.path.join(a.out, "fc8_error.json"), "w") as f:
            f.write(json.dumps(rows) + "\n")


if __name__ == "__main__":
    main()
