"""The softmax and prior arithmetic across the whole range of fpc_expf: cases that put a logits row of
a chosen regime in front of the expansion kernels, and everything of them that needs no GPU.

DIRECT ROWS: for a list of root positions one crafted logits row per game, as an explicit [G, A] matrix.  The case knows
each game's legal set and rotation, so it writes chosen values at the SOURCE indices of the legal moves
(legal_head_cases.source_index) and at chosen illegal indices: a regime is hit on purpose.  Every value is an f32, and
wherever a difference l - m matters (it is not flushed) it is exact in f32, so that a plain float64 softmax sees the
same differences.  `regimes` computes from the row and the legal set alone, in float64, which regimes a row hits:

  a  deep but normal: l - m in [-86, -40], p_i normal          b  subnormal p_i = exp(l - m) / S
  c  flushed child: l - m < -86 while siblings survive         d  subnormal final prior p / T, child present
  e  subnormal T: every legal p_i subnormal, quotients normal  g  l - m overflows to -inf on finite logits
  f  where the row maximum lies (legal / illegal index, tail chunk, a chunk without a legal move, chunk 0 with every
     other chunk more than 86 below or entirely -inf)           h  refusals        i  the legal-only head's regimes

EVALUATOR FAMILIES: wide-range logits built on the `hash` evaluator's per-position hash (tests/evaluators.py, which
stays what the golden generator mirrors), so that rows differ leaf by leaf below the root; searched to the end.

The same rows serve the internal network through tower_probe's "bias_row" Linear (weights zero, bias = the row)."""
import numpy as np

import legal_head_cases as lc
import search_model as sm
from oracle import orc

F32 = np.float32
NINF = F32(-np.inf)
TINY = 2.0 ** -126                                   # the smallest normal f32
HALF_STEP = 2.0 ** -150                              # half the spacing of the subnormal f32
BELOW86 = np.nextafter(F32(-86), F32(-np.inf))       # the first f32 below -86: flushed
ABOVE86 = np.nextafter(F32(-86), F32(0))
INV_OF = lc.INV_OF
CHUNK = 1024


def action_size(R):
    return (8 * R + 8) * R * R


def _spread(lo, hi, n):
    """n f32 values from hi down to lo on the grid of 1/64 (both ends included for n > 1)"""
    return (np.round(np.linspace(hi, lo, n) * 64) / 64).astype(F32)


def _chunk_of(idx):
    return np.asarray(idx) // CHUNK


# ---------------------------------------------------------------------------------------------------------------------
# row recipes: f(A, src, ill) -> f32 row.  src: source indices of the legal moves (ascending flat order), ill: every
# other index, ascending.  need(A, src, ill): whether the position can carry the recipe.
# ---------------------------------------------------------------------------------------------------------------------
def r_plateau_sub(A, src, ill):
    """the whole row a plateau of maxima (S = A, 4.6e3 .. 2.4e4); half of the legal moves normal, half subnormal p_i"""
    row = np.zeros(A, F32)
    n = len(src); h = n // 2
    row[src[:h]] = _spread(-70, -40, h)
    row[src[h:]] = _spread(-86, -79.5, n - h)
    return row


def r_all_sub(A, src, ill):
    """every legal p_i subnormal: T subnormal, the quotients normal"""
    row = np.zeros(A, F32)
    row[src] = _spread(-86, -80, len(src))
    return row


def r_deep(A, src, ill):
    """S about 1, the maximum at a legal index, the other legal moves down to exactly -86: deep but normal"""
    row = np.full(A, -200, F32)
    row[src[0]] = 0
    row[src[1:]] = _spread(-86, -40, len(src) - 1)
    return row


def r_sub_final(A, src, ill):
    """k >= 6 legal moves at the maximum, the others within [-86, -85.7]: exp(l - m) / k is a subnormal final prior"""
    row = np.full(A, -200, F32)
    n = len(src); nlow = max(2, n // 4)
    row[src[:n - nlow]] = 0
    row[src[n - nlow:]] = _spread(-86, -85.7, nlow)
    return row


STRADDLE = [0, -86, BELOW86, ABOVE86, -np.inf, -87, -100, -1e4, -1, -10, -39.5, -85]


def r_straddle(A, src, ill):
    """-86 (kept), one f32 step below (flushed) and above it, deeper flushes, a -inf: dropped children beside survivors"""
    row = np.full(A, -5, F32)
    row[src] = np.array([STRADDLE[i % len(STRADDLE)] for i in range(len(src))], F32)
    return row


def _r_chunk0(other):
    def f(A, src, ill):
        row = np.full(A, other, F32)
        row[:CHUNK] = -30
        row[ill[0]] = 0
        c0 = src[src < CHUNK]
        row[c0] = _spread(-86, -40, len(c0))
        return row
    return f


def _need_chunk0(A, src, ill):
    return ill[0] < CHUNK and (src < CHUNK).sum() >= 2 and (src >= CHUNK).sum() >= 1


r_chunk0_far = _r_chunk0(-100)                       # the maximum in chunk 0, every other chunk more than 86 below: term = 0
r_chunk0_inf = _r_chunk0(-np.inf)                    # ... every other chunk entirely -inf


def r_tailmax(A, src, ill):
    """the row maximum at an illegal index of the partial tail chunk"""
    row = np.full(A, -20, F32)
    row[ill[ill >= A // CHUNK * CHUNK][0]] = 0
    row[src] = _spread(-60, -1, len(src))
    return row


def r_tail_plateau(A, src, ill):
    """the tail chunk a plateau of maxima except at legal moves: its record dominates S; legal moves down to subnormal p_i"""
    row = np.full(A, -8, F32)
    row[A // CHUNK * CHUNK:] = 0
    row[src] = _spread(-86, -1, len(src))
    return row


def _free_chunk(A, src):
    used = set(_chunk_of(src).tolist())
    return [c for c in range((A + CHUNK - 1) // CHUNK) if c not in used]


def r_otherchunk(A, src, ill):
    """the row maximum in a chunk that holds no legal move"""
    row = np.full(A, -10, F32)
    row[_free_chunk(A, src)[0] * CHUNK + 5] = 0
    row[src] = _spread(-50, -2, len(src))
    return row


HUGE = [3e38, 1e30, -3e38, -1e30, 3e38, -3e38, 0, 1e30]


def r_huge(A, src, ill):
    """+-3e38 and 1e30 mixed: l - m overflows to -inf in f32 on finite logits; the maximum at a legal index"""
    row = np.full(A, -3e38, F32)
    row[ill[::7]] = 1e30
    row[src] = np.array([HUGE[i % len(HUGE)] for i in range(len(src))], F32)
    return row


def r_huge_illegal(A, src, ill):
    """the same with the maximum 3e38 at an illegal index as well (a legal move survives only AT the maximum: one f32
    step below 3e38 is 2e31 below it)"""
    row = r_huge(A, src, ill)
    row[ill[1]] = 3e38
    return row


# ---- refusals: sm._priors returns 1
def x_inf_illegal(A, src, ill):
    row = np.zeros(A, F32); row[ill[len(ill) // 2]] = np.inf
    return row


def x_nan_legal(A, src, ill):
    row = np.zeros(A, F32); row[src[len(src) // 2]] = np.nan
    return row


def x_nan_last(A, src, ill):
    """a NaN at index A - 1 alone: the last lane's last element of the partial tail chunk"""
    row = r_tailmax(A, src, ill); row[A - 1] = np.nan
    return row


def x_nan_illegal(A, src, ill):
    row = r_deep(A, src, ill); row[ill[len(ill) // 3]] = np.nan
    return row


def x_all_flushed(A, src, ill):
    row = np.zeros(A, F32)
    row[src] = np.array([[BELOW86, -87, -1e4, -np.inf][i % 4] for i in range(len(src))], F32)
    return row


def x_all_ninf(A, src, ill):
    return np.full(A, NINF, F32)


# ---- the legal-only head: the maximum is taken over the legal moves, there is no 1/S
def l_deep(A, src, ill):
    row = r_deep(A, src, ill); row[ill] = 50
    return row


def l_sub_final(A, src, ill):
    """subnormal p / T with a large T; an illegal global maximum 100 above: the full head refuses this row"""
    row = r_sub_final(A, src, ill); row[ill] = 100
    return row


def l_diverge(A, src, ill):
    """the documented divergence: every legal logit more than 86 below an illegal global maximum"""
    row = np.full(A, -3, F32)
    row[ill[len(ill) // 2]] = 100
    row[src] = _spread(-5, 0, len(src))
    return row


def l_nan_elsewhere(A, src, ill):
    """NaN at every illegal index: the legal head reads none of them"""
    row = np.full(A, np.nan, F32)
    row[src] = _spread(-86, 0, len(src))
    return row


def l_x_all_ninf(A, src, ill):
    row = np.zeros(A, F32); row[src] = NINF
    return row


def _need(n):
    return lambda A, src, ill: len(src) >= n


RECIPES = {
    # name: (recipe, need, refusal of the full head, refusal of the legal head)
    "plateau_sub": (r_plateau_sub, _need(4)), "all_sub": (r_all_sub, _need(3)), "deep": (r_deep, _need(4)),
    "sub_final": (r_sub_final, _need(8)), "straddle": (r_straddle, _need(6)),
    "chunk0_far": (r_chunk0_far, _need_chunk0), "chunk0_inf": (r_chunk0_inf, _need_chunk0),
    "tailmax": (r_tailmax, _need(3)), "tail_plateau": (r_tail_plateau, _need(4)),
    "otherchunk": (r_otherchunk, lambda A, src, ill: len(src) >= 3 and bool(_free_chunk(A, src))),
    "huge": (r_huge, _need(6)), "huge_illegal": (r_huge_illegal, _need(6)),
    "x_inf_illegal": (x_inf_illegal, _need(2)), "x_nan_legal": (x_nan_legal, _need(2)), "x_nan_last": (x_nan_last, _need(3)),
    "x_nan_illegal": (x_nan_illegal, _need(4)), "x_all_flushed": (x_all_flushed, _need(2)), "x_all_ninf": (x_all_ninf, _need(1)),
    "l_deep": (l_deep, _need(4)), "l_sub_final": (l_sub_final, _need(8)), "l_diverge": (l_diverge, _need(3)),
    "l_nan_elsewhere": (l_nan_elsewhere, _need(3)), "l_x_all_ninf": (l_x_all_ninf, _need(2)),
}
RUN_FULL = ["plateau_sub", "all_sub", "deep", "sub_final", "straddle", "chunk0_far", "chunk0_inf", "tailmax", "tail_plateau",
            "otherchunk", "huge", "huge_illegal"]
REFUSE_FULL = ["x_inf_illegal", "x_nan_legal", "x_nan_last", "x_nan_illegal", "x_all_flushed", "x_all_ninf"]
# the legal head: rows it runs (straddle and huge serve it as they are; l_sub_final, l_diverge refuse on the full head)
RUN_LEGAL = ["l_deep", "straddle", "l_sub_final", "l_diverge", "huge", "l_nan_elsewhere", "x_nan_illegal"]
REFUSE_LEGAL = ["x_nan_legal", "l_x_all_ninf", "x_all_ninf"]

# ---------------------------------------------------------------------------------------------------------------------
# the direct cases
# ---------------------------------------------------------------------------------------------------------------------
# queens: rows on lc.queens_root (more than 64 legal moves); terminal: that many finished games in FRONT of the crafted
# ones (no leaf: with more than 64 of them the expansion finds the batch's first live leaf through first_leaf_turn)
DIRECT_CASES = {
    "rows-8x8-strict": dict(R=8, rules=0, seed=3, rows=RUN_FULL + ["plateau_sub", "deep"], queens=["sub_final", "huge"]),
    "rows-8x8-fixed": dict(R=8, rules=15, seed=4, rows=RUN_FULL + ["straddle", "all_sub"], queens=["sub_final", "huge"]),
    "rows-8x8-noise": dict(R=8, rules=15, seed=5, rows=["plateau_sub", "all_sub", "sub_final", "straddle", "deep", "huge"],
                           queens=["sub_final"], noise=True),
    "rows-10x10-strict": dict(R=10, rules=0, seed=6, rows=["plateau_sub", "all_sub", "deep", "straddle", "chunk0_far", "tailmax",
                                                           "tail_plateau", "huge"], queens=[]),
    "rows-14x14-strict": dict(R=14, rules=0, seed=7, rows=["plateau_sub", "all_sub", "deep", "sub_final", "straddle", "chunk0_inf",
                                                           "tailmax", "tail_plateau"], queens=["sub_final", "huge"]),
    "rows-14x14-fixed": dict(R=14, rules=15, seed=8, rows=["plateau_sub", "all_sub", "straddle", "chunk0_far", "tailmax", "otherchunk",
                                                          "huge_illegal"], queens=["sub_final"]),
    "rows-8x8-70games": dict(R=8, rules=0, seed=9, rows=["plateau_sub", "straddle", "all_sub", "tailmax", "deep", "huge"], queens=[],
                             terminal=64),
}
# refusals: batches of their own; the first refusal row is row `first`, the rows in front of it are fine
REFUSAL_CASES = {"refuse-%s-%s" % (name[2:], "strict" if rules == 0 else "fixed"):
                 dict(R=8, rules=rules, seed=20 + i, rows=["plateau_sub", "deep", "tailmax"][:first] + [name, "deep", name], queens=[],
                      first=first)
                 for i, (name, rules, first) in enumerate(zip(REFUSE_FULL, [0, 15, 0, 15, 0, 15], [1, 2, 3, 1, 2, 3]))}
WAYS = {"expand": (1, 1, False), "expand_select": (1, 2, True), "multi": (2, 2, False), "select_multi": (2, 4, True)}

_pools, _direct = {}, {}


def terminal_root(R, seed=1):
    """a finished game: the last position of a seeded random playout through the oracle"""
    import random
    import positions as pos
    INV = INV_OF[R]
    turn, entries = pos.start_entries(R)
    rng = random.Random(seed)
    while True:
        b = orc.board_from_dict(R, turn, [list(e) for e in entries])
        for _ply in range(800):
            if orc.game_result(orc.clone(b), R, INV) != 0:
                return b
            flats = sorted(set(x[2] for x in orc.legal_moves(b, R, INV)))
            b, rc = orc.take_action(b, R, flats[rng.randrange(len(flats))])
            assert rc == 0


def geometry(board, R, rules, turn0):
    """(legal flats ascending, their source indices in the evaluated row, every other index, rot)"""
    rot = board.turn if rules & sm.RULES_ROTATION else turn0
    legal = lc.legal_of(board, R, rules)
    src = np.array([lc.source_index(R, rot, fl) for fl in legal], np.int64)
    assert len(set(src.tolist())) == len(src)
    return legal, src, np.setdiff1d(np.arange(action_size(R)), src), rot


def _build(c):
    R, rules = c["R"], c["rules"]
    A = action_size(R)
    key = (R, rules, c["seed"])
    if key not in _pools:
        _pools[key] = sm.positions(R, 48, seed=100 + c["seed"], rules=rules)
    pool = list(_pools[key])
    n_term = c.get("terminal", 0)
    boards, names = [], []
    if n_term:
        t = terminal_root(R)
        boards += [orc.clone(t) for _ in range(n_term)]
        names += ["terminal"] * n_term
    # the batch's first live row is the first crafted game: its side to move is the strict rules' rotation of all
    first = next(k for k, b in enumerate(pool) if RECIPES[c["rows"][0]][1](A, *geometry(b, R, rules, b.turn)[1:3]))
    pool.insert(0, pool.pop(first))
    turn0 = pool[0].turn
    rows, geo = [], []
    for name in c["rows"] + ["queens:" + q for q in c["queens"]]:
        queens = name.startswith("queens:")
        name = name.split(":")[-1]
        recipe, need = RECIPES[name]
        if queens:
            b = lc.queens_root(R)
            g = geometry(b, R, rules, turn0)
            assert len(g[0]) > 64
        else:
            for k, b in enumerate(pool if rows else pool[:1]):   # the first crafted game is the pool's first position
                g = geometry(b, R, rules, turn0)
                if need(A, g[1], g[2]):
                    pool.pop(k)
                    break
            else:
                raise AssertionError("no position of the pool carries %s" % name)
        row = recipe(A, g[1], g[2])
        assert row.dtype == F32 and row.shape == (A,)
        boards.append(b); names.append(("queens:" if queens else "") + name); rows.append(row); geo.append(g)
    G = len(boards)
    mat = np.zeros((G, A), F32)
    mat[n_term:] = np.stack(rows)
    gamma = None
    if c.get("noise"):
        import fpc_ffi
        gamma = np.random.default_rng(c["seed"]).standard_gamma(0.3, size=(G, fpc_ffi.MAX_MOVES)).astype(F32)
    return dict(c, boards=boards, names=names, rows=mat, geo=[None] * n_term + geo, G=G, A=A, n_term=n_term, gamma=gamma)


def direct_case(name):
    """the case's boards (never mutated: clone them), row names, [G, A] rows and per-game geometry, built once"""
    if name not in _direct:
        _direct[name] = _build(DIRECT_CASES[name] if name in DIRECT_CASES else REFUSAL_CASES[name])
    return _direct[name]


def row_evaluator(rows, value=True):
    """numpy evaluator: the first call answers with `rows` for the first len(rows) rows of the step, every later call
    (the leaves below the roots) and every other row with logits of zero; the value of row r is ((r % 5) - 2) / 4"""
    calls = []
    G, A = rows.shape

    def ev(enc):
        n = enc.shape[0]
        lg = np.zeros((n, A), F32)
        if not calls:
            lg[:G] = rows
        calls.append(n)
        v = ((np.arange(n) % 5) - 2).astype(F32) / F32(4) if value else np.zeros(n, F32)
        return lg, v

    return ev


def tiled_evaluator(row):
    """the internal network with the "bias_row" Linear: every leaf's logits are the row, every value tanh(0)"""
    def ev(enc):
        n = enc.shape[0]
        return np.tile(row, (n, 1)), np.zeros(n, F32)
    return ev


def model_of(case, way, policy_head="full"):
    """(rc, Model.results() or None) of the search model on the case's rows, driven the `way` the engine is"""
    K, sims, _ = WAYS[way]
    R = case["R"]
    return sm.search([orc.clone(b) for b in case["boards"]], R, INV_OF[R], sims, 3.0, row_evaluator(case["rows"]), K,
                     rules=case["rules"], noise=case["gamma"], noise_eps=0.25 if case["gamma"] is not None else 0.0,
                     policy_head=policy_head)[:2]


def engine_run(backend, case, way):
    """the engine's results of the same run through the step-wise C-ABI; returns (eng, res) -- close eng"""
    from fpc_testlib import make_engine, roots_of
    K, sims, fused = WAYS[way]
    R = case["R"]
    # the node pool holds 1 + 96 * max_sims nodes per game: room for a many-moves root's children after one simulation
    eng = make_engine(backend, R, INV_OF[R], max_games=case["G"] * K, max_sims=sims + 3)
    try:
        eng.set_rules(case["rules"])
        if case["gamma"] is not None:
            eng.set_root_noise(case["gamma"], 0.25)
        roots = roots_of(case["boards"], R)
        return eng, sm.run_stepwise(eng, backend, roots, sims, 3.0, row_evaluator(case["rows"]), K, fused=fused)
    except BaseException:
        eng.close()
        raise


def first_refusal(case, policy_head="full"):
    """the first row on which sm._priors returns 1 (None: no row refuses)"""
    for g in range(case["n_term"], case["G"]):
        legal, _src, _ill, rot = case["geo"][g]
        if sm._priors(case["rows"][g], case["R"], rot, legal, policy_head)[0]:
            return g
    return None


# ---------------------------------------------------------------------------------------------------------------------
# the float64 model of a row and its regimes
# ---------------------------------------------------------------------------------------------------------------------
def f64_priors(row, src, policy_head="full"):
    """plain float64 softmax with the documented rule "l - m < -86 contributes 0", mask, renormalise.  Returns None on a
    refusal (NaN, +inf, no legal mass), else {"d": l - m at the legal moves, "p", "S", "T", "prior", "m", "exact": every
    difference that is not flushed is the f32 difference}"""
    x = row.astype(np.float64)
    sel = x[src] if policy_head == "legal" else x
    if np.isnan(sel).any() or np.isposinf(sel).any():
        return None
    m = sel.max()
    if np.isneginf(m):
        return None
    with np.errstate(over="ignore", invalid="ignore"):
        d = sel - m
        e = np.where(d < -86, 0.0, np.exp(np.maximum(d, -800.0)))
        d32 = (sel.astype(F32) - F32(m)).astype(np.float64)
    S = e.sum() if policy_head == "full" else 1.0
    dl = x[src] - m
    p = np.where(dl < -86, 0.0, np.exp(np.maximum(dl, -800.0))) / S
    T = p.sum()
    if not T > 0:
        return None
    keep = d >= -87
    with np.errstate(over="ignore"):
        overflow = np.isneginf(x[src].astype(F32) - F32(m)) & np.isfinite(x[src])
    return {"d": dl, "p": p, "S": S, "T": T, "prior": p / T, "m": m, "exact": bool(np.array_equal(d[keep], d32[keep])),
            "overflow": overflow}


def regimes(row, src, A, policy_head="full"):
    """per-regime counts of PRIORS (a, b, c, d, e, g) and 0/1 flags of the ROW (f_*, straddle), float64 alone"""
    out = dict.fromkeys(["a", "b", "c", "d", "e", "g", "f_legal", "f_illegal", "f_tail", "f_otherchunk", "f_chunk0_far",
                         "f_chunk0_inf", "straddle", "ninf_legal", "diverge"], 0)
    f = f64_priors(row, src, policy_head)
    if f is None:
        return None
    assert f["exact"], "a difference l - m that is not flushed is not exact in f32"
    d, p, prior = f["d"], f["p"], f["prior"]
    alive = d >= -86
    out["a"] = int((alive & (d <= -40) & (p >= TINY)).sum())
    out["b"] = int((alive & (p < TINY)).sum())
    out["c"] = int((~alive).sum()) if alive.any() else 0
    out["d"] = int((alive & (prior < TINY)).sum())
    if alive.any() and (p[alive] < TINY).all() and (prior[alive] >= TINY).all():
        out["e"] = int(alive.sum())
    out["g"] = int(f["overflow"].sum())
    out["straddle"] = int((d == -86).any() and (d == float(BELOW86)).any())
    out["ninf_legal"] = int(np.isneginf(row[src]).any() and alive.any())
    x = row.astype(np.float64)
    if policy_head == "full":
        at = np.flatnonzero(x == f["m"])
        legal_at = np.isin(at, src)
        out["f_legal"] = int(legal_at.any())
        out["f_illegal"] = int(not legal_at.any())
        out["f_tail"] = int((at >= A // CHUNK * CHUNK).any())
        out["f_otherchunk"] = int(not np.isin(_chunk_of(at), _chunk_of(src)).any())
        rest = x[CHUNK:]
        if (at < CHUNK).all():
            out["f_chunk0_inf"] = int(np.isneginf(rest).all())
            out["f_chunk0_far"] = int((rest < f["m"] - 86).all() and not out["f_chunk0_inf"])
    else:
        out["diverge"] = int(f64_priors(row, src, "full") is None and np.nanmax(x) > x[src].max() + 86)
    return out


# the caps (ISSUE): each of a-e and g by at least 8 priors over the case set, each item of f, h and i by at least 2 rows
PRIOR_CAP, ROW_CAP = 8, 2


def coverage(names=None):
    """the regime totals over the direct cases (full head), the refusal rows by kind, and the legal head's items over
    every crafted position of the direct cases"""
    tot = dict.fromkeys(["a", "b", "c", "d", "e", "g", "f_legal", "f_illegal", "f_tail", "f_otherchunk", "f_chunk0_far",
                         "f_chunk0_inf", "straddle"], 0)
    for name in names or DIRECT_CASES:
        case = direct_case(name)
        for g in range(case["n_term"], case["G"]):
            r = regimes(case["rows"][g], case["geo"][g][1], case["A"])
            assert r is not None, (name, g, case["names"][g], "a run-to-the-end case holds a refusal row")
            for k in tot:
                tot[k] += r[k]
    return tot


# ---------------------------------------------------------------------------------------------------------------------
# single rows: the internal network with the "bias_row" Linear gives EVERY leaf the same row, so each row is searched in
# a batch of SINGLE_G copies of its own position (the rotation is that position's side to move under both rule sets)
# ---------------------------------------------------------------------------------------------------------------------
SINGLE_G = 3
SINGLE = {"full": dict(run=RUN_FULL, refuse=REFUSE_FULL, per=1, queens=("sub_final", "huge"), seed=12),
          "legal": dict(run=RUN_LEGAL, refuse=REFUSE_LEGAL, per=2, queens=("l_sub_final", "huge", "straddle"), seed=11)}
# rows whose background keeps every leaf below the root expandable: searched deeper (16 simulations; K = 2)
DEEP = {"full": ("plateau_sub", "tailmax"), "legal": ("straddle", "l_deep")}
SINGLE_RUNS = {"run1": (1, 1), "run16": (1, 16), "leaves2": (2, 4)}      # (leaves per step, simulations) of fpc_search_run


def single_rows(head, R=8, rules=0):
    """{"run": [(name, board, row, geometry)], "refuse": [...]}: each recipe of the head on `per` positions, and the
    queens recipes on the many-moves root (more than 64 legal moves)"""
    key = ("single", head, R, rules)
    if key not in _direct:
        c = SINGLE[head]
        A = action_size(R)
        pool = sm.positions(R, 96, seed=100 + c["seed"], rules=rules)
        out = {"run": [], "refuse": []}
        for kind in ("run", "refuse"):
            for name in c[kind]:
                recipe, need = RECIPES[name]
                got = 0
                for b in pool:
                    g = geometry(b, R, rules, b.turn)
                    if need(A, g[1], g[2]):
                        out[kind].append((name if got == 0 else "%s-%d" % (name, got), b, recipe(A, g[1], g[2]), g))
                        got += 1
                        if got == c["per"]:
                            break
                assert got == c["per"], name
        for name in c["queens"]:
            b = lc.queens_root(R)
            g = geometry(b, R, rules, b.turn)
            out["run"].append(("queens:" + name, b, RECIPES[name][0](A, g[1], g[2]), g))
        _direct[key] = out
    return _direct[key]


def single_runs(head, name):
    return list(SINGLE_RUNS) if name.split(":")[-1].split("-")[0] in DEEP[head] and "queens" not in name else ["run1"]


def single_model(entry, head, run, R=8, rules=0):
    """(rc, Model.results() or None) of SINGLE_G copies of the row's position searched with the row at every leaf"""
    _name, b, row, _g = entry
    K, sims = SINGLE_RUNS[run]
    return sm.search([orc.clone(b) for _ in range(SINGLE_G)], R, INV_OF[R], sims, 3.0, tiled_evaluator(row), K, rules=rules,
                     policy_head=head)[:2]


def legal_coverage(rows=None):
    tot = dict.fromkeys(["a", "c", "d", "g", "straddle", "ninf_legal", "diverge", "many_moves"], 0)
    for name, _b, row, g in (rows or single_rows("legal")["run"]):
        r = regimes(row, g[1], len(row), "legal")
        assert r is not None, name
        for k in tot:
            tot[k] += r.get(k, 0)
        tot["many_moves"] += int(len(g[0]) > 64 and r["d"] > 0)
    return tot


# ---------------------------------------------------------------------------------------------------------------------
# evaluator families on the hash evaluator's per-position hash
# ---------------------------------------------------------------------------------------------------------------------
FAMILIES = ("spread", "plateau", "spike", "spikes8", "cliff", "huge", "infchunks")


def family(kind, R):
    """evaluator(enc) -> (logits, value): u = the `hash` evaluator's 16-bit draw per (position, index), h its position hash.
    spread: -u / 720 on the grid of 1/512, (-91.1, 0]: a row's own maximum near 0, 5 % of it flushed, p_i subnormal below;
    plateau: 7 of 8 logits 0 (S about A), the others in (-88, -76]: subnormal p_i and flushes side by side;
    cliff: half of the row in (-2, 0], half in (-87, -75]; spike: one maximum of +70 over hash logits, every other logit 66 ..
    74 below; spikes8: eight maxima of +60 .. +67 over hash logits, so that
    every other logit is 56 .. 71 below; huge: 1 in 32 at -3e38, 1 in 32 at 1e30, 1 in 32 a hash logit,
    the rest 3e38 -- l - m overflows; infchunks: hash logits with whole chunks of -inf behind chunk 0 chosen by the position's hash"""
    RR = R * R
    A = (8 * R + 8) * RR
    widx = ((np.arange(24 * RR, dtype=np.uint64) * np.uint64(2654435761)) % np.uint64(1 << 32)).reshape(1, 24, R, R)
    i = np.arange(A, dtype=np.uint64).reshape(1, A)
    iterm = (i * np.uint64(40503) + ((i * i) % np.uint64(8191)) * np.uint64(69069))
    nch = (A + CHUNK - 1) // CHUNK
    assert kind in FAMILIES

    def ev(enc):
        B = enc.shape[0]
        h = (enc.astype(np.uint64) * widx).sum(axis=(1, 2, 3)) % np.uint64(1 << 32)
        u = (((h.reshape(B, 1) * np.uint64(2246822519) + iterm) % np.uint64(1 << 32)) >> np.uint64(16)).astype(np.int64)
        base = u.astype(F32) / F32(8192.0) - F32(4.0)                    # the hash evaluator's logits, [-4, 4)
        if kind == "spread":
            lg = -(np.floor(u * (512.0 / 720.0)) / 512.0)
        elif kind == "plateau":
            lg = np.where(u % 8 == 0, -76.0 - (u // 8 % 6144) / 512.0, 0.0)
        elif kind == "cliff":
            lg = np.where(u % 2 == 0, -(u // 2 % 1024) / 512.0, -75.0 - (u // 2 % 6144) / 512.0)
        elif kind == "spike":
            lg = base.astype(np.float64)
            lg[np.arange(B), (h % np.uint64(A)).astype(np.int64)] = 70.0
        elif kind == "spikes8":
            lg = base.astype(np.float64)
            for b in range(B):
                at = (int(h[b]) * np.arange(1, 9) * 7919) % A
                lg[b, at] = 60.0 + np.arange(8)
        elif kind == "huge":
            lg = np.where(u % 32 == 1, -3e38, np.where(u % 32 == 2, 1e30, np.where(u % 32 == 3, base, 3e38)))
        else:
            lg = base.astype(np.float64)
            for b in range(B):
                dead = [c for c in range(1, nch) if (int(h[b]) >> (2 * c)) & 3 == 3 or (R > 8 and (int(h[b]) >> c) & 1)]
                for c in dead:
                    lg[b, c * CHUNK:(c + 1) * CHUNK] = -np.inf
        v = ((h % np.uint64(9)).astype(F32) - 4) / 4
        return lg.astype(F32), v.astype(F32)

    return ev


# (family, R, games, sims, seed of the roots): at most 6 x 25 at 8x8 and 4 x 15 at 14x14
# the seeds are those of the first roots on which the oracle's search AND the model's with two leaves per step run to the
# end (a leaf with one or two legal moves, all of them flushed, is a policy error: that belongs to the refusal cases)
FAMILY_CASES = ([(k, 8, 6, 25, {"spread": 2, "huge": 3, "infchunks": 5}.get(k, 1)) for k in FAMILIES] +
                [(k, 14, 4, 15, 2 if k == "infchunks" else 1) for k in ("spread", "plateau", "huge", "infchunks")])
_family = {}


def family_case(kind, R, G, sims, seed):
    """roots, evaluator, orc.search's reference (rc asserted 0) and the regimes of the expansions below the roots, from
    the search model's run with its expansion hook"""
    key = (kind, R, G, sims, seed)
    if key not in _family:
        boards = sm.positions(R, G, seed=200 + seed)
        ev = family(kind, R)
        rc, oref = orc.search([orc.clone(b) for b in boards], R, INV_OF[R], sims, 3.0, ev)
        assert rc == 0, (key, "the search must run to the end on the oracle", rc)
        model = sm.Model([orc.clone(b) for b in boards], R, INV_OF[R], 3.0, ev)
        model.expansions = []
        assert model.search(sims, 1) == 0
        below = dict.fromkeys(["a", "b", "c", "d", "e", "g"], 0)
        n_below = 0
        for is_root, row, rot, legal in model.expansions:
            if is_root:
                continue
            n_below += 1
            src = np.array([lc.source_index(R, rot, fl) for fl in legal], np.int64)
            r = regimes(row, src, len(row))
            for k in below:
                below[k] += r[k]
        rc, model2, _ = sm.search([orc.clone(b) for b in boards], R, INV_OF[R], sims, 3.0, ev, 2)
        assert rc == 0, (key, "the search with two leaves per step must run to the end on the model", rc)
        _family[key] = dict(boards=boards, ev=ev, oref=oref, below=below, n_below=n_below, model=model.results(), model2=model2)
    return _family[key]


def family_engine_runs(backend, kind, R, G, sims, seed, stepwise=True):
    """the family's search on the engine three ways -- step-wise (not with stepwise=False: the emulator spends four
    seconds on a 14x14 search), fused, two leaves per step -- against the oracle and the search model, bit for bit"""
    from engine_cases import _compare_search
    from fpc_testlib import make_engine, roots_of, run_external_search
    c = family_case(kind, R, G, sims, seed)
    INV = INV_OF[R]
    for fused in ((False, True) if stepwise else (True,)):
        eng = make_engine(backend, R, INV, max_games=G, max_sims=sims)
        try:
            roots = roots_of(c["boards"], R)
            res = run_external_search(eng, backend, roots, sims, 3.0, c["ev"], fused=fused)
            _compare_search(res, c["oref"], (kind, R, "fused" if fused else "stepwise"))
            sm.compare(eng, res, c["model"], (kind, R, "model"), grand_every=2)
        finally:
            eng.close()
    eng = make_engine(backend, R, INV, max_games=2 * G, max_sims=sims)
    try:
        res = sm.run_stepwise(eng, backend, roots_of(c["boards"], R), sims, 3.0, c["ev"], 2, fused=True)
        sm.compare(eng, res, c["model2"], (kind, R, "two leaves"), grand_every=2)
    finally:
        eng.close()
    return c
