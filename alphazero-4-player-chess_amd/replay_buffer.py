"""Ring replay buffer of training tuples (counterpart of the reference's src/py/replay_buffer.py:4-20:
fixed capacity, overwrite-oldest, uniform sampling without replacement), and its device-resident form."""
import random


class ReplayBuffer:
    def __init__(self, capacity, rng=None):
        self.capacity = int(capacity)
        self._items = []
        self._next = 0
        self._rng = rng or random

    def add(self, experience):
        if len(self._items) < self.capacity:
            self._items.append(experience)
        else:
            self._items[self._next] = experience
        self._next = (self._next + 1) % self.capacity

    def sample(self, batch_size):
        return self._rng.sample(self._items, batch_size)

    def __len__(self):
        return len(self._items)


class DeviceReplayBuffer:
    """The same ring kept in device memory as fpc_tuple records (include/fpc_engine.h fpc_replay_*): ring 0 or 1 of
    `engine`, filled by Engine.replay_push / replay_load.  sample() draws the positions ReplayBuffer.sample draws from a
    buffer of the same length (random.sample picks by position from the population size alone) and decodes them in one
    kernel launch: (x [n,24,R,R], pi [n,A], z [n,1]) f32 on `device` (None: host memory, the emulator backend).
    decode / sample with weights=True return a fourth tensor w [n,1]: 0.0 for a record of a fast search (playout cap
    randomization, fpc_ffi.TUPLE_FAST), 1.0 otherwise -- the record's weight in the policy loss.
    An engine has one ring of each number: making a second buffer on the same engine and ring empties the ring under the
    first one, whose next use then raises."""

    def __init__(self, engine, ring, capacity, rng=None, device=None):
        self.eng, self.ring, self.capacity = engine, int(ring), int(capacity)
        self._rng = rng or random
        self.device = device
        engine.replay_reserve(self.ring, self.capacity)
        self._gen = engine.replay_gen[self.ring]

    def _mine(self):
        if self.eng.replay_gen[self.ring] != self._gen:
            raise RuntimeError("DeviceReplayBuffer: ring %d of this engine has been reserved again since this buffer was made "
                               "(another buffer on the same engine?): its contents are gone" % self.ring)

    def __len__(self):
        self._mine()
        return self.eng.replay_size(self.ring)

    def decode(self, slots, weights=False):
        import torch
        self._mine()
        n, e = len(slots), self.eng
        kw = {"dtype": torch.float32, "device": self.device if self.device is not None else "cpu"}
        x, pi, z = torch.empty((n, 24, e.R, e.R), **kw), torch.empty((n, e.A), **kw), torch.empty((n, 1), **kw)
        w = torch.empty((n, 1), **kw) if weights else None
        if n:
            if self.device is not None:
                torch.cuda.current_stream(self.device).synchronize()    # the allocator may hand out blocks queued work still reads
            e.replay_batch(self.ring, slots, x, pi, z, w=w)
        return (x, pi, z, w) if weights else (x, pi, z)

    def sample(self, batch_size, weights=False):
        return self.decode(self._rng.sample(range(len(self)), batch_size), weights=weights)
