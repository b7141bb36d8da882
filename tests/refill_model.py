"""The plain-Python model of fpc_search_advance_refill: search_model.Model whose advance may also start games.  A row
with src -1 gets the root fpc_search_begin gives a game (N = 1, W = 0, no children, the start board as its state); every
other row is Model.advance's, word for word."""
import search_model as sm
from oracle import orc


class Model(sm.Model):
    def advance_refill(self, src, flats, fresh):
        """new game i continues old game src[i] from the root child flats[i], or -- src[i] == -1 -- starts on the orc
        board fresh[i] (flats[i] is ignored).  Returns the kept visit counts."""
        src = list(range(len(flats))) if src is None else list(src)
        keep = [i for i, s in enumerate(src) if s >= 0]
        noise = self.noise
        if noise is not None:                        # a kept root takes the noise row of its NEW index
            self.noise = noise[keep]
        try:
            super().advance([src[i] for i in keep], [flats[i] for i in keep])      # asserts that the kept entries ascend
        finally:
            self.noise = noise
        kept = iter(self.roots)
        self.roots = [next(kept) if s >= 0 else sm._Node(0.0, -1, None, state=orc.clone(fresh[i])) for i, s in enumerate(src)]
        self.alive = [True] * len(src)
        self.sims_done = [0] * len(src)
        return [r.N for r in self.roots]
