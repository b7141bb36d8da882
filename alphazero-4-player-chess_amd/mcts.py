"""`MCTS` -- drop-in for the reference's src/py/mcts.py:8-89.

Same constructor and `search(games) -> root nodes` contract; the body (per-simulation Python loop
over ChooseLeaf / GetEncodedStates / softmax / mask / BackpropagateNodes / ExpandNodes) is replaced
by the engine:

* `neural_net` is a ResNet (net.py here, or any module with the reference's parameter names):
  its BN-folded weights are exported once per parameter version and the whole search runs on the
  GPU (`fpc_search_run`: select -> encode -> MFMA ResNet -> expand, no host round trips).
* `neural_net` is any other callable with a `.device` attribute (the reference's evaluator seam,
  mcts.py:65-66; synthetic / recorded evaluators in tests): the engine is driven step-wise and the
  callable sees the encoded leaves `[G,24,R,R]` and returns `(logits [G,A], value [G,1])`.
  Difference from the reference: the batch always has one slot per game (finished games are
  all-zero rows whose outputs are ignored) instead of only the live leaves.

Leaf-parallel search (opt-in, not reference semantics; include/fpc_engine.h fpc_search_set_leaves):
args["leaves_per_step"] = K > 1 selects up to K leaves per game per simulation step, kept apart by
args["virtual_loss"] (default 1.0); the engine then has K*G rows and the evaluator sees [K*G,24,R,R]
(row k*G + g = the k-th leaf of game g), num_searches leaves in ceil(num_searches / K) steps.

Per-game simulation budgets (opt-in, not reference semantics; include/fpc_engine.h fpc_search_set_budget):
args["sim_budget"] = "per_game" | "visit_target" makes continue_search give every game its own simulation count
(budgets_for) instead of the batch-wide one; search(games, budgets=...) / continue_search(..., budgets=...) take an
explicit per-game list.  Absent / None: no budget is ever set.

MCTS solver (opt-in; include/fpc_engine.h fpc_search_set_solver): args["solver"] = True proves wins, losses and draws in
the tree under args["rules"] = "training" / "selfplay" -- a proven child is backed up without a board, a move that loses is
left out of the selection, a proven root idles -- and fpc_search_play / selfplay.play(solver=True) play a proven win or draw.

Forced playouts and policy target pruning (opt-in; include/fpc_engine.h fpc_search_set_forced): args["forced_playouts"] =
None (default) | float, usually 2.0 -- with args["root_noise"] under args["rules"] = "selfplay" a visited root child is
guaranteed sqrt(k * P * N) simulations, and the policy target (fpc_collect_tuples, fpc_search_play, fpc_search_targets /
selfplay.play(targets=True)) leaves out the visits that only the forcing put there.

Playout cap randomization (opt-in; include/fpc_engine.h fpc_search_set_fast_rows): args["playout_cap"] = None (default) |
{"full_prob": p, "fast_searches": n}, 0 < p <= 1, 1 <= n <= num_searches -- search / continue_search take fast=[bool per
game]: a fast game is searched with n simulations, an all-zero noise row and no forcing, and its target is not pruned;
selfplay.play(playout_cap=...) draws which plies are fast, and the trainer leaves their policy targets out.

Live-row numbering (opt-in; include/fpc_engine.h fpc_search_set_live_rows): args["live_rows"] = True makes every step work
on its live leaves only -- the same trees; the fused search's policy Linear computes ceil(live / 256) row tiles, and an
external evaluator sees [n_live,24,R,R] (the live leaves in ascending row order) and returns n_live rows.
"""
import math

import numpy as np
import torch

import alphazero_cpp as az


def _param_version(model):
    return (id(model), sum(int(p._version) for p in model.parameters()), sum(int(b._version) for b in model.buffers()),
            bool(model.training))


class _DevPtr:
    def __init__(self, ptr, shape):
        self.__cuda_array_interface__ = {"shape": tuple(shape), "typestr": "<f4", "data": (int(ptr), False), "version": 2}


def _is_resnet(m):
    return isinstance(m, torch.nn.Module) and all(hasattr(m, k) for k in ("startBlock", "backBone", "policyHead", "valueHead"))


def _on_engine_device(m, eng):
    """every parameter and buffer of the module lies on the engine's GPU"""
    import itertools
    return all(t.device.type == "cuda" and t.device.index == eng.device for t in itertools.chain(m.parameters(), m.buffers()))


SIM_BUDGET_MODES = (None, "per_game", "visit_target")


def parse_playout_cap(cap, num_searches):
    """args["playout_cap"] checked: None, or (full_prob, fast_searches) of {"full_prob": p, "fast_searches": n} with
    0 < p <= 1 and 1 <= n <= num_searches (further keys, such as alphazero's "record_fast", are the caller's)"""
    if cap is None:
        return None
    try:
        p, n = cap["full_prob"], cap["fast_searches"]
    except (TypeError, KeyError, IndexError):
        raise ValueError("playout_cap must be None or {\"full_prob\": p, \"fast_searches\": n}, not %r" % (cap,))
    if isinstance(p, bool) or not isinstance(p, (int, float)) or not 0 < p <= 1:
        raise ValueError("playout_cap: full_prob must lie in (0, 1], not %r" % (p,))
    if isinstance(n, bool) or not isinstance(n, (int, np.integer)) or not 1 <= n <= int(num_searches):
        raise ValueError("playout_cap: fast_searches must be an int in 1..num_searches = %d, not %r" % (int(num_searches), n))
    return float(p), int(n)


def budgets_for(kept, num_searches, max_sims, mode, born=1, fast=None, fast_searches=None):
    """Per-game simulation budgets of one ply (fpc_search_set_budget) from the roots' kept visit counts (1 for a fresh
    root, so kept - 1 simulations have gone through a root already); None for mode None.  born: the visit count a node is
    born with -- 1, or 0 under fpc_ffi.RULES_VISITS, where `kept` itself is the simulations through the root and stands
    in place of kept - 1 below.
    "per_game":     min(num_searches, max_sims - (kept - 1)): every game gets num_searches unless ITS OWN kept visits
                    leave less room in the handle -- a fresh row gets its full count beside any kept root.
    "visit_target": max(0, num_searches - (kept - 1)): every root is searched until num_searches simulations have gone
                    through it (kept + new <= num_searches, so a handle of num_searches simulations is enough).
    fast (optional, one bool per game; playout cap randomization): a fast game's budget is the same expression with
    fast_searches in place of num_searches.  Without it the result is what it was."""
    if mode not in SIM_BUDGET_MODES:
        raise ValueError("sim_budget must be one of %r, not %r" % (SIM_BUDGET_MODES, mode))
    if mode is None:
        return None
    M = int(max_sims)
    S = [int(num_searches)] * len(kept)
    if fast is not None:
        if len(fast) != len(kept):
            raise ValueError("budgets_for: %d fast flags for %d games" % (len(fast), len(kept)))
        if fast_searches is None:
            raise ValueError("budgets_for: fast rows need fast_searches")
        S = [int(fast_searches) if f else s for f, s in zip(fast, S)]
    if mode == "per_game":
        return [max(0, min(s, M - (int(k) - born))) for k, s in zip(kept, S)]
    return [max(0, s - (int(k) - born)) for k, s in zip(kept, S)]


class MCTS:
    def __init__(self, gameType, neural_net, args):
        self.gameType = gameType
        self.args = args
        self.neural_net = neural_net
        self.nn_dtype = int(args.get("nn_dtype", 0)) if hasattr(args, "get") else 0
        # "full" (default): whole policy Linear + full softmax, the reference's arithmetic op for op;
        # "legal": opt-in legal-moves-only policy head (same priors up to f32 rounding, ~1.6x the
        # simulations/s at 14x14; include/fpc_engine.h fpc_set_policy_mode)
        self.policy_head = str(args.get("policy_head", "full")) if hasattr(args, "get") else "full"
        self._native = _is_resnet(neural_net)
        # N4 (explicitly NOT part of parity with the reference): args["rules"] = "strict"
        # (default: every quirk of the reference, bit-exact) or "fixed" (AlphaZero PUCT with the child's value
        # negated, per-sample rotation, un-shifted input planes, full moves in the tree), "training" ("fixed" plus
        # fpc_ffi.RULES_TERMINAL: a terminal leaf is valued by its result and no longer takes the root out of the
        # search), or an int of fpc_ffi.RULES_* bits; args["root_noise"] = True applies Dirichlet(dirichlet_alpha) noise with weight
        # dirichlet_epsilon to the root priors inside the fused search loop, seeded by args["noise_seed"].
        rules = args.get("rules", "strict") if hasattr(args, "get") else "strict"
        self.rules = {"strict": 0, "fixed": 15, "training": 31, "selfplay": 63}.get(rules, rules)
        # args["rules"] = "selfplay" (63): "training" plus fpc_ffi.RULES_VISITS -- every node is born with N = 0, so visit
        # counts, the policy target and Q hold real visits only.  args["fpu"] = None (default) | float: first-play urgency,
        # an unvisited child's q is the parent's Q minus that reduction (fpc_search_set_fpu; no effect without RULES_VISITS)
        self.born = 0 if int(self.rules) & 32 else 1
        fpu = args.get("fpu", None) if hasattr(args, "get") else None
        self.fpu = None if fpu is None else float(fpu)
        # args["solver"] = True (opt-in): the MCTS solver (fpc_search_set_solver) -- terminal results are proven up the tree;
        # in effect only where the rule set holds RULES_PUCT and RULES_TERMINAL ("training", "selfplay"), inert elsewhere
        self.solver = bool(args.get("solver", False)) if hasattr(args, "get") else False
        # args["forced_playouts"] = None (default) | float, usually 2.0 (opt-in): forced playouts and policy target pruning at
        # the root (fpc_search_set_forced); in effect only where the rule set holds RULES_PUCT and RULES_VISITS ("selfplay")
        forced = args.get("forced_playouts", None) if hasattr(args, "get") else None
        self.forced = 0.0 if forced is None else float(forced)
        self.root_noise = bool(args.get("root_noise", False)) if hasattr(args, "get") else False
        self._noise_rng = np.random.default_rng(int(args.get("noise_seed", 0))) if self.root_noise else None
        self.leaves = int(args.get("leaves_per_step", 1)) if hasattr(args, "get") else 1
        self.virtual_loss = float(args.get("virtual_loss", 1.0)) if hasattr(args, "get") else 1.0
        # args["device_weights"] = True (opt-in): a module that lies on the engine's GPU is packed into the engine there
        # (fpc_load_weights_device: no host copy, in place); any other module takes the host path as before
        self.device_weights = bool(args.get("device_weights", False)) if hasattr(args, "get") else False
        # args["fc_weights"] = "int8" (opt-in; default "w16"): the policy Linear's weights as int8 with one f32 scale per output
        # (weights.quantize_fc, k_fcw8: half the weight stream and half the engine's largest allocation; it changes the
        # network's numbers -- tools/fc8_error.py says by how much).  fp16 operands only.
        self.fc_weights = str(args.get("fc_weights", "w16")) if hasattr(args, "get") else "w16"
        if self.fc_weights not in ("w16", "int8"):
            raise ValueError("fc_weights must be \"w16\" or \"int8\", not %r" % (self.fc_weights,))
        if self.fc_weights == "int8" and self._native and self.nn_dtype != 1:
            raise ValueError("fc_weights=\"int8\" needs fp16 operands: set args[\"nn_dtype\"] = 1 (bf16 engines have no int8 policy Linear)")
        # args["sim_budget"] (opt-in): None | "per_game" | "visit_target" -- continue_search's per-game budgets (budgets_for)
        self.sim_budget = args.get("sim_budget", None) if hasattr(args, "get") else None
        if self.sim_budget not in SIM_BUDGET_MODES:
            raise ValueError("sim_budget must be one of %r, not %r" % (SIM_BUDGET_MODES, self.sim_budget))
        # args["live_rows"] = True (opt-in): only the live leaves of a step are evaluated (fpc_search_set_live_rows)
        self.live_rows = bool(args.get("live_rows", False)) if hasattr(args, "get") else False
        # args["playout_cap"] = None (default) | {"full_prob": p, "fast_searches": n} (opt-in): playout cap randomization
        # (fpc_search_set_fast_rows) -- search / continue_search accept fast=[...]; who is fast is selfplay.play's draw
        cap = args.get("playout_cap", None) if hasattr(args, "get") else None
        self.playout_cap = None if cap is None else parse_playout_cap(cap, args["num_searches"])

    def _fast_rows(self, fast, G):
        """the fast= argument of search / continue_search as a list of G bools (None: none given)"""
        if fast is None:
            return None
        if self.playout_cap is None:
            raise ValueError("fast= needs args[\"playout_cap\"]")
        fast = [bool(f) for f in fast]
        if len(fast) != G:
            raise ValueError("%d fast flags for %d games" % (len(fast), G))
        return fast

    def _fast_budgets(self, kept, fast, max_sims):
        """the budgets of a ply with fast rows: budgets_for with fast_searches for them; no sim_budget counts as "per_game\""""
        return budgets_for(kept, int(self.args["num_searches"]), max_sims, self.sim_budget or "per_game", self.born, fast=fast,
                           fast_searches=self.playout_cap[1])

    def solver_in_effect(self):
        return self.solver and (int(self.rules) & 17) == 17       # RULES_PUCT | RULES_TERMINAL

    def forced_in_effect(self):
        return self.forced > 0 and (int(self.rules) & 33) == 33   # RULES_PUCT | RULES_VISITS

    def _set_fpu(self, eng):
        if self.fpu is None:
            eng.set_fpu(0, 0.0)
        else:
            eng.set_fpu(1, self.fpu)

    def engine_rows(self, G):
        """rows of the engine handle a search of G games needs (G * leaves_per_step)"""
        return G * self.leaves

    def sync_weights(self, eng):
        """(re-)export the network into the engine when its parameters changed (optimizer.step)."""
        import weights
        ver = _param_version(self.neural_net)
        if getattr(eng, "weights_version", None) != ver:
            if self.device_weights and _on_engine_device(self.neural_net, eng):
                eng.load_weights_device(self.neural_net, fc_weights=self.fc_weights)
            else:
                eng.load_weights(weights.export_weights(self.neural_net, self.nn_dtype, fc_weights=self.fc_weights))   # the module stays where it is
            eng.weights_version = _param_version(self.neural_net)

    def add_dirichlet_noise(self, policy, device):
        """Counterpart of the reference's MCTS.add_dirichlet_noise (mcts.py:45-56): blends every row of
        a [B, A] policy with one Dirichlet(alpha) sample over the whole action space,
        (1 - eps) * policy + eps * noise, alpha/eps from args["dirichlet_alpha"/"dirichlet_epsilon"].
        As in the reference it is provided but never called by search()."""
        alpha, eps = float(self.args["dirichlet_alpha"]), float(self.args["dirichlet_epsilon"])
        n_actions = int(self.gameType.action_space_size)
        draw = np.random.dirichlet(np.full(n_actions, alpha), size=int(policy.shape[0]))
        noise = torch.as_tensor(draw, dtype=torch.float32, device=device)
        return policy * (1.0 - eps) + noise * eps

    @torch.no_grad()
    def search(self, games, budgets=None, fast=None):
        """budgets (optional): per-game simulation counts of this search (fpc_search_set_budget), each at most
        num_searches -- game g completes budgets[g] simulations while the batch runs max(budgets) steps' worth.
        fast (optional, one bool per game; needs args["playout_cap"]): the fast games get an all-zero noise row, the
        fast-row mask (fpc_search_set_fast_rows) and, unless `budgets` is given, fast_searches simulations."""
        G = len(games)
        fast = self._fast_rows(fast, G)
        sims = int(self.args["num_searches"])
        eng = az.engine(self.engine_rows(G), sims, self.nn_dtype if self._native else None)
        pods = [g._b for g in games]
        eng.set_rule_bits(int(self.rules))                 # all six bits; set_rules keeps its range 0..31
        eng.set_leaves(self.leaves, self.virtual_loss)     # the handle is process-wide: set on every search
        self._set_fpu(eng)
        if self.root_noise:
            import fpc_ffi
            gamma = self._noise_rng.standard_gamma(float(self.args["dirichlet_alpha"]), size=(G, fpc_ffi.MAX_MOVES)).astype(np.float32)
            if fast is not None:
                gamma[np.asarray(fast, bool)] = 0.0        # a row whose sum is not positive keeps its priors un-noised
            eng.set_root_noise(gamma, float(self.args["dirichlet_epsilon"]))
        else:
            eng.set_root_noise(None, 0.0)
        eng.search_begin(pods, float(self.args["C"]))
        if fast is not None:
            eng.search_set_fast_rows(fast)
            if budgets is None:
                budgets = self._fast_budgets([self.born] * G, fast, eng.max_sims)
        eng.set_live_rows(self.live_rows)                  # as set_leaves; here, where no selection can be pending
        eng.set_solver(self.solver)                        # the same; begin has cleared the statuses
        eng.set_forced(self.forced)
        if budgets is not None:
            budgets = [int(b) for b in budgets]
            eng.search_set_budget(budgets)
            sims = max(budgets)
        if self._native:
            self.sync_weights(eng)
            eng.set_policy_mode(self.policy_head == "legal")
            eng.search_run(sims)
        else:
            self._search_external(eng, G, sims)
        res = eng.search_results(roots=pods)          # root states keep the piece-list order the search left
        # the roots are views of the result arrays: child objects are made when GetChildren() is first called on a
        # root, TakeAction / GetGameResult of a root child come from one batched prefetch (alphazero_cpp._SearchBatch)
        batch = az._SearchBatch(eng, res, self.args["C"])
        roots = []
        for g, game in enumerate(games):
            root = az.Node(self.args["C"], game, visit_count=int(res["root_n"][g]))
            root._batch, root._g = batch, g
            game.SetRootNode(root)
            roots.append(root)
        assert int(res["n_children"].min()) > 0         # mcts.py:40-41
        return roots

    @torch.no_grad()
    def continue_search(self, pods, keep_idx, flats, budgets=None, fast=None):
        """Opt-in subtree reuse (not reference semantics; include/fpc_engine.h fpc_search_advance), for callers that know
        the moves played -- selfplay.play(continue_fn=...); the drop-in search(games) carries no move history and always
        starts fresh trees.  Re-roots the search this object ran last: new game i continues game keep_idx[i] of it from
        the root child flats[i], then runs num_searches simulations on the kept subtrees -- fewer where kept + new would
        pass the engine's max_sims (create the engine with 2 * num_searches, as AlphaZero.play does).  `pods` (list of
        fpc_ffi.Board) receive the new root states.  keep_idx[i] == -1 (selfplay.play(refill=...)) starts a new game in
        row i instead, on the start board pods[i] (fpc_search_advance_refill; flats[i] is ignored); it shares the
        batch-wide simulation count.
        With args["sim_budget"] set, or an explicit `budgets` list (which overrides the mode), every game gets its own
        simulation count instead (budgets_for / fpc_search_set_budget) and the batch runs max(budget) steps' worth.
        fast (optional, one bool per game; needs args["playout_cap"]): as in search(); the noise row of a fast game is
        zeroed before the advance blends it.
        Returns the fpc_ffi.Engine.search_results dict."""
        G = len(flats)
        fast = self._fast_rows(fast, G)
        eng = az.engine()
        eng.set_rule_bits(int(self.rules))                 # all six bits; set_rules keeps its range 0..31
        eng.set_leaves(self.leaves, self.virtual_loss)
        self._set_fpu(eng)
        if self.root_noise:
            import fpc_ffi
            gamma = self._noise_rng.standard_gamma(float(self.args["dirichlet_alpha"]), size=(G, fpc_ffi.MAX_MOVES)).astype(np.float32)
            if fast is not None:
                gamma[np.asarray(fast, bool)] = 0.0        # a row whose sum is not positive keeps its priors un-noised
            eng.set_root_noise(gamma, float(self.args["dirichlet_epsilon"]))
        else:
            eng.set_root_noise(None, 0.0)
        if keep_idx is not None and any(int(k) < 0 for k in keep_idx):
            # refill (fpc_search_advance_refill): keep_idx[i] == -1 starts a new game in row i on pods[i]
            kept = eng.search_advance_refill(flats, keep_idx, fresh=pods, roots=pods)
        else:
            kept = eng.search_advance(flats, keep_idx, roots=pods)
        if fast is not None:
            eng.search_set_fast_rows(fast)
            if budgets is None:
                budgets = self._fast_budgets(kept, fast, eng.max_sims)
        eng.set_live_rows(self.live_rows)
        eng.set_solver(self.solver)
        eng.set_forced(self.forced)
        if budgets is None:
            budgets = budgets_for(kept, int(self.args["num_searches"]), eng.max_sims, self.sim_budget, self.born)
        if budgets is not None:
            budgets = [int(b) for b in budgets]
            eng.search_set_budget(budgets)
            sims = max(budgets)
        else:
            sims = min(int(self.args["num_searches"]), eng.max_sims - (int(kept.max()) - self.born))
        if self._native:
            self.sync_weights(eng)
            eng.set_policy_mode(self.policy_head == "legal")
            eng.search_run(sims)
        else:
            self._search_external(eng, G, sims)
        return eng.search_results(roots=pods)

    def _search_external(self, eng, G, sims):
        dev = str(getattr(self.neural_net, "device", "cpu"))
        on_gpu = dev.startswith("cuda") or dev == "gpu"
        host_engine = eng.host_memory                  # only true for the test-suite's emulator build
        R, A = eng.R, eng.A
        keep = None
        # leaf-parallel: ceil(sims / K) steps of K leaves per game, the last one of the remainder (set before the
        # selection of that step, which the preceding expand_select performs)
        K = self.leaves
        steps = math.ceil(sims / K)
        last_k = sims - K * (steps - 1)

        def leaves_of(step):
            return K if step + 1 < steps else last_k

        rows = G * leaves_of(0)
        if steps > 0 and leaves_of(0) != K:
            eng.set_leaves(leaves_of(0), self.virtual_loss)
        # mcts.py:36-38: select -> evaluate -> expand per simulation; between two evaluations the expansion and the
        # next selection are one launch (fpc_search_expand_select)
        n_live, enc_ptr = eng.search_select() if steps > 0 else (0, None)
        for i in range(steps):
            last = i == steps - 1
            if not last and leaves_of(i + 1) != leaves_of(i):
                eng.set_leaves(leaves_of(i + 1), self.virtual_loss)
            if n_live == 0:
                if not last:
                    n_live, enc_ptr = eng.search_select()
                    rows = G * leaves_of(i + 1)
                continue
            if self.live_rows:                         # the live leaves lead the batch, in ascending row order
                rows = n_live
            if host_engine:
                import ctypes
                import numpy as np
                enc = torch.from_numpy(np.ctypeslib.as_array(ctypes.cast(enc_ptr, ctypes.POINTER(ctypes.c_float)),
                                                             shape=(rows, 24, R, R)).copy())
                logits, value = self.neural_net(enc)
                logits = logits.to(torch.float32).contiguous().view(rows, A)
                value = value.to(torch.float32).contiguous().view(rows)
            else:
                enc = torch.as_tensor(_DevPtr(enc_ptr, (rows, 24, R, R)), device="cuda")
                logits, value = self.neural_net(enc if on_gpu else enc.cpu())
                logits = logits.to(device="cuda", dtype=torch.float32).contiguous().view(rows, A)
                value = value.to(device="cuda", dtype=torch.float32).contiguous().view(rows)
                torch.cuda.synchronize()
            keep = (logits, value)
            if last:
                eng.search_expand(logits.data_ptr(), value.data_ptr())
            else:
                n_live, enc_ptr = eng.search_expand_select(logits.data_ptr(), value.data_ptr())
                rows = G * leaves_of(i + 1)
            if not host_engine:
                torch.cuda.synchronize()
        del keep
        if last_k != K:
            eng.set_leaves(K, self.virtual_loss)
