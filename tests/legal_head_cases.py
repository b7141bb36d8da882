"""The search cases on the internal network (tests/test_linear_probe_gpu.py, second half) and everything of them that
needs no GPU: a family A integer network (tests/tower_probe.py) in front of the "dense_scaled" Linear, whose float64
reference IS the evaluator of the oracle / the plain-Python search model.

LEGAL_CASES are the cases that hold the opt-in legal-only policy head (fpc_set_policy_mode(FPC_POLICY_LEGAL): k_fc_unfrag,
k_policy_gemv, k_expand_legal(_select)(_multi)) bit for bit against search_model.Model(policy_head="legal").  Their
coverage conditions are asserted from the model's step records alone (tests/test_legal_head_cpu.py runs them without a
GPU), and `faulty` builds the single faults of the reference logits that the CPU self-test must see."""
import time

import numpy as np

import search_model as sm
import tower_probe as tp
from oracle import orc

INV_OF = {8: 2, 9: 2, 10: 2, 11: 3, 12: 3, 13: 3, 14: 3}
G, SIMS = 12, 48
GEMV_BLOCKS, GEMV_WAVES = 768, 4                     # k_policy_gemv's launch (csrc/fpc_nn.h forward_legal)


def search_setup(R, hidden, dtype, seed=31, boards=None, rules=0):
    """the network, the root positions (default: 12 seeded random playouts through the oracle), the scale exponent --
    the power of two that brings the reference's largest |logit| over the first 12 roots into [8, 16) -- and the
    evaluator that IS the float64 reference: everything of a search case that needs no GPU.  ev.logits_of(enc) are the
    unscaled integer logits in float64, ev.policy_of(enc) the policy conv's output they are made from."""
    # 3 blocks for both operand types: positions of real games fill 1 % of the input planes (probe_inputs: 25 %), the
    # activations stay below 2^8 -- held by integer_conditions on every call -- and two blocks leave too few distinct values
    blocks = 3
    m = tp.integer_net(R, blocks, hidden, 100 * R + blocks)
    layers = tp.conv_layers(m, dtype)
    W, bias = tp.dense_weights(R)
    if boards is None:
        boards = sm.positions(R, G, seed=seed + R)

    def policy_of(enc):
        assert np.isin(enc, (0.0, 1.0)).all()
        ref = tp.forward(layers, enc, dtype)
        tp.integer_conditions(ref, dtype)
        tp.linear_conditions(ref["policy"].reshape(enc.shape[0], -1), W, bias)
        return ref["policy"]

    def logits_of(enc):
        return tp.expected_logits(policy_of(enc), "dense_int", R)

    orc.set_rules(rules)
    try:
        enc0 = orc.encode(boards[:G], R)
    finally:
        orc.set_rules(0)
    top = float(np.abs(logits_of(enc0)).max())
    s = int(np.floor(np.log2(top))) - 3
    assert 8.0 <= top * 2.0 ** -s < 16.0

    def ev(enc):
        lg = logits_of(np.asarray(enc, np.float64)) * 2.0 ** -s
        return lg.astype(np.float32), np.zeros(enc.shape[0], np.float32)

    ev.policy_of, ev.logits_of, ev.s = policy_of, logits_of, s
    return m, boards, s, ev


# ---------------------------------------------------------------------------------------------------------------------
# the legal-only head's cases.  s: the recorded scale exponent; rules 15: every correction, FPC_RULES_ROTATION among them
# ---------------------------------------------------------------------------------------------------------------------
PAIR_ROOTS = 1300        # 8x8 positions have 9 .. 11 legal moves on average: what the pair count of "pair-dealing" takes
LEGAL_CASES = {
    # k_expand_legal_select; Kp = 4608: 576 chunks, one full group of 8 x 64 and one partial
    "select-8x8-fp16": dict(R=8, hidden=128, dtype=1, layout=2, rules=0, K=1, sims=48, s=9),
    # the bf16 dot2; nsrc by each row's own turn
    "rotation-8x8-bf16": dict(R=8, hidden=128, dtype=0, layout=1, rules=15, K=1, sims=48, s=9),
    # 1152 chunks: two full groups and a quarter; turn0 of the batch (Q6)
    "turn0-10x10-fp16": dict(R=10, hidden=128, dtype=1, layout=1, rules=0, K=1, sims=24, s=9),
    # k_expand_legal(_select)_multi, rows k*G + g; 2944 chunks: five groups and six eighths; k_towerc in front
    "leaves-14x14-fp16": dict(R=14, hidden=128, dtype=1, layout=2, rules=15, K=2, sims=24, s=10),
    # more than 64 legal moves at a root: the second 64-wide pass of the maximum, the p_j loop and the child append
    "many-moves-8x8-h256": dict(R=8, hidden=256, dtype=1, layout=2, rules=0, K=1, sims=16, s=9),
    # k_policy_gemv's pair dealing: several pairs per wave, blocks across game boundaries, cum beyond lane 63
    "pair-dealing-8x8-fp16": dict(R=8, hidden=128, dtype=1, layout=2, rules=15, K=1, sims=3, s=8),
}
N_QUEENS = 4


def queens_root(R):
    """play_cases.QUEENS as an oracle board: red to move with five queens, more than 64 legal moves"""
    from play_cases import QUEENS
    kings, queens = QUEENS[R]
    return orc.board_from_dict(R, 0, [[k, c, 5] for c, k in enumerate(kings)] + [[q, 0, 4] for q in queens])


def case_boards(name):
    c = LEGAL_CASES[name]
    R, rules = c["R"], c["rules"]
    if name == "many-moves-8x8-h256":
        return [queens_root(R) for _ in range(N_QUEENS)] + sm.positions(R, G - N_QUEENS, seed=57, rules=rules)
    if name == "pair-dealing-8x8-fp16":
        # mid-game and near-end roots in turn: a game that meets a terminal leaf has live neighbours
        mid = sm.positions(R, PAIR_ROOTS // 2, seed=71, rules=rules)
        end = sm.positions(R, PAIR_ROOTS // 2, seed=72, near_end=True, rules=rules)
        return [b for pair in zip(mid, end) for b in pair]
    return sm.positions(R, G, seed=31 + R, rules=rules)


_setups, _cases = {}, {}


def case_setup(name):
    """{"m", "boards", "s", "ev"}: search_setup of the case's roots, computed once; the boards are never mutated"""
    if name not in _setups:
        c = LEGAL_CASES[name]
        m, boards, s, ev = search_setup(c["R"], c["hidden"], c["dtype"], boards=case_boards(name), rules=c["rules"])
        _setups[name] = {"m": m, "boards": boards, "s": s, "ev": ev}
    return _setups[name]


def legal_case(name):
    """case_setup and the model's search of it with policy_head="legal", computed once: + {"model" (Model.results()),
    "steps" (Model.steps), "counts", "seconds" (the model's search: the float64 reference of every step and the tree
    work)}"""
    if name not in _cases:
        c, su = LEGAL_CASES[name], case_setup(name)
        t0 = time.time()
        rc, model, counts = sm.search([orc.clone(b) for b in su["boards"]], c["R"], INV_OF[c["R"]], c["sims"], 3.0, su["ev"],
                                      c["K"], rules=c["rules"], policy_head="legal")
        assert rc == 0
        _cases[name] = dict(su, model=model, steps=counts["steps"], counts=counts, seconds=time.time() - t0)
    return _cases[name]


def dead_between_live(step):
    """a row without a leaf lies between two live rows of the step"""
    dead = set(step["dead"])
    live = [r for r in range(step["rows"]) if r not in dead]
    return bool(live) and any(live[0] < r < live[-1] for r in dead)


def check_coverage(name, case):
    """the case's coverage conditions, from the model alone (never from the engine); returns what the summary names"""
    c, steps, model, boards = LEGAL_CASES[name], case["steps"], case["model"], case["boards"]
    assert case["s"] == c["s"], (case["s"], c["s"])
    assert 2.0 ** -case["s"] >= 2.0 ** -14                         # fp16's smallest normal number: no weight is a denormal
    assert len(steps) == len(sm.schedule(c["sims"], c["K"])) and all(st["rows"] == c["K"] * len(boards) for st in steps)
    assert sum(o["sims_done"] for o in model) > len(boards) * c["sims"] // 2
    fig = {"largest step's pairs": max(st["pairs"] for st in steps), "steps with a dead row": sum(1 for st in steps if st["dead"]),
           "steps with a dead row between live rows": sum(1 for st in steps if dead_between_live(st)),
           "most legal moves of a row": max(st["max_legal"] for st in steps), "games": len(boards)}
    root_turns = set(b.turn for b in boards)
    # the rotation: a live row whose own side to move is not the batch's first live row's
    mixed = sum(1 for st in steps if st["turns"] and any(t != st["turns"][0] for t in st["turns"]))
    fig["steps with rows of mixed turns"] = mixed
    if name in ("rotation-8x8-bf16", "turn0-10x10-fp16"):
        assert len(root_turns) > 1, root_turns
        assert mixed > 0
    if name == "leaves-14x14-fp16":
        assert c["K"] == 2 and case["counts"]["collisions"] > 0 and mixed > 0
        # rows k*G + g with k = 1 carry leaves
        assert any(len(boards) + g not in st["dead"] for st in steps for g in range(len(boards)))
    if name == "many-moves-8x8-h256":
        fig["n_children of the many-moves root"] = len(model[0]["children"])
        for g in range(N_QUEENS):
            assert len(model[g]["children"]) > 64, len(model[g]["children"])
            assert len(model[g]["children"]) == len(model[0]["children"])
        assert fig["most legal moves of a row"] > 64
    if name == "pair-dealing-8x8-fp16":
        assert len(boards) > 128
        assert fig["largest step's pairs"] > 4 * GEMV_WAVES * GEMV_BLOCKS, fig    # waves take several pairs, blocks cross games
        assert fig["steps with a dead row between live rows"] > 0, fig
        assert case["counts"]["terminals"] > 0
    return fig


# ---------------------------------------------------------------------------------------------------------------------
# single faults of the reference logits, in k_policy_gemv's own decomposition
# ---------------------------------------------------------------------------------------------------------------------
def source_index(R, rot, flat):
    """where the logit of absolute move `flat` lies in a row evaluated in the frame rotated by `rot`"""
    RR = R * R
    plane, pos = divmod(flat, RR)
    return plane * RR + orc.lib().orc_rot90_src(R, -rot, pos // R, pos % R)


def legal_of(board, R, rules):
    orc.set_rules(rules)
    try:
        return sorted(set(mv[2] for mv in orc.legal_moves(orc.clone(board), R, INV_OF[R])))
    finally:
        orc.set_rules(0)


LOGIT_FAULTS = ("drop_product", "chunk_from_next_row", "drop_bias")


def faulty(ev, R, fault, row, col, src_col=None):
    """the evaluator `ev` with ONE fault in the logit [row, col] of its FIRST call (the model's first expansion):
    "drop_product": one nonzero product x[k] * W[col, k] left out; "chunk_from_next_row": one 8-wide chunk of weight row
    col (16 bytes of k_fc_unfrag's copy, in the engine's K order) read from row col + 1; "drop_bias": the column's bias
    left out; "copy": the logit of src_col instead.  All in float64 on integers times 2^-s: exact."""
    W, bias = tp.dense_weights(R)
    calls = []

    def f(enc):
        lg, v = ev(enc)
        calls.append(1)
        if len(calls) > 1:
            return lg, v
        out = lg.astype(np.float64)
        scale = 2.0 ** -ev.s
        if fault == "copy":
            assert out[row, src_col] != out[row, col]
            out[row, col] = out[row, src_col]
        elif fault == "drop_bias":
            assert bias[col] != 0
            out[row, col] -= float(bias[col]) * scale
        else:
            x = tp.engine_order(ev.policy_of(np.asarray(enc, np.float64))[row].reshape(1, -1), R)[0]
            w = tp.engine_order(W[col:col + 2].astype(np.float64), R)
            if fault == "drop_product":
                k = int(np.flatnonzero(x * w[0])[0])
                out[row, col] -= x[k] * w[0, k] * scale
            elif fault == "chunk_from_next_row":
                d = (x * (w[1] - w[0])).reshape(-1, 8).sum(axis=1)
                ch = int(np.flatnonzero(d)[0])
                out[row, col] += d[ch] * scale
            else:
                raise ValueError(fault)
        assert out[row, col] != lg[row, col]
        got = out.astype(np.float32)
        assert np.array_equal(got.astype(np.float64), out)           # still exact in f32
        return got, v

    return f
