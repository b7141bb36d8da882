"""Shared builders of the int8 policy-Linear tests (k_fcw8, blob version 4): Tail8, the int8 counterpart
of tower_probe.Tail built by numpy alone from a given q, scale and bias; the decode of the fragment-pair order; the
float64 reference of `bias + scale * (x . q)`; and single faults of the kind a rewrite of k_fcw8 makes, in the kernel's
own decomposition (tests/test_fc8_cpu.py proves every one of them changes a logit).  Everything else -- the integer
networks, their inputs, the float64 tower, the comparators -- is tower_probe's."""
import struct

import numpy as np
import torch

import tower_probe as tp

W8 = 1          # the header's fc_wtype / FPC_FC_W8


def geometry(R):
    A = (8 * R + 8) * R * R
    return A, (A + 383) // 384 * 384, (A + 511) // 512 * 512       # A, Np (layout 2), Kp


def pair_order(qp):
    """int8 [Np, Kp] in the engine's K order -> the blob's bytes: [Kp/32][Np/32][64 lanes = 16 q + c][2 tiles][8],
    element (ks, np, q, c, t, e) = qp[32 np + 16 t + c][32 ks + 8 q + e]"""
    Np, Kp = qp.shape
    return np.ascontiguousarray(qp.reshape(Np // 32, 2, 16, Kp // 32, 4, 8).transpose(3, 0, 4, 2, 1, 5)).tobytes()


def decode_pairs(buf, Np, Kp):
    """the inverse, written from the formula element by element of the index arrays (not as the transpose above): the
    int8 section of a version-4 blob -> int8 [Np, Kp]"""
    raw = np.frombuffer(buf, np.int8, Np * Kp)
    n = np.arange(Np, dtype=np.int64)[:, None]
    k = np.arange(Kp, dtype=np.int64)[None, :]
    ks, qq, e = k // 32, (k % 32) // 8, k % 8
    npair, t, c = n // 32, (n % 32) // 16, n % 16
    off = ((((ks * (Np // 32) + npair) * 64 + 16 * qq + c) * 2 + t) * 8) + e
    return raw[off]


class Tail8:
    """the Linear sections of a version-4 blob: q int8 [A, A] indexed [out, in] in the reference's NCHW input order (as
    tower_probe.dense_weights), scale f32 [A], bias [A]; the value Linear is tower_probe.value_vector, or all zero
    (value_zero: the engine's value is tanh(0))"""
    def __init__(self, R, q, scale, bias, value_zero=False):
        A, self.Np, self.Kp = geometry(R)
        RR = R * R
        assert q.shape == (A, A) and q.dtype == np.int8
        self.R, self.dtype, self.layout = R, 1, 2
        qp = np.zeros((self.Np, self.Kp), np.int8)
        qp[:A, :A] = tp.engine_order(q, R)
        fs = np.ones(self.Np, np.float32)
        fs[:A] = np.asarray(scale, np.float32)
        fb = np.zeros(self.Np, np.float32)
        fb[:A] = np.asarray(bias, np.float32)
        vw = np.zeros((RR, 32), np.float32)
        vb = np.float32(0.0)
        if not value_zero:
            v, vb = tp.value_vector(R)
            vw[:, :24] = v.reshape(24, RR).T
        self.bytes = pair_order(qp) + fs.tobytes() + fb.tobytes() + vw.tobytes() + struct.pack("<f", float(vb))


def splice8(m, t):
    """tower_probe.splice with the version-4 header: m's convolutions (stub geometry) in front of t's Linears"""
    blob = tp.splice(m, t)
    magic, version, R, F, nb, dt, a_ch, Np, Kp, lay = struct.unpack_from("<4s9i", blob, 0)
    assert (version, dt, lay) == (3, 1, 2)
    return struct.pack("<4s10i20x", b"FPCW", 4, R, F, nb, dt, a_ch, Np, Kp, lay, W8) + blob[64:]


def header_of(blob):
    """(magic, version, R, F, nblocks, dtype, A_ch, Np, Kp, fc_layout, fc_wtype)"""
    return struct.unpack_from("<4s10i", blob, 0)


def fc_offset(F, nblocks):
    return tp.head_len(F, nblocks)


# ---------------------------------------------------------------------------------------------------------------------
# the cases: q, scales and bias of the bit-for-bit tests
# ---------------------------------------------------------------------------------------------------------------------
_cases = {}


def dense_case(R, lo=-128, hi=127, seed=0):
    """(q int8 [A, A] uniform in lo..hi, scale f32 [A] = 2^-(n mod 4), bias int64 [A] in -5..5); with the full range every
    one of the 256 byte values occurs in every tile of 16 columns (asserted)"""
    key = (R, lo, hi, seed)
    if key not in _cases:
        for k in [k for k in _cases if k[0] >= 12]:
            _cases.pop(k)
        A = geometry(R)[0]
        rng = np.random.default_rng(8000 + 10 * R + seed)
        q = rng.integers(lo, hi + 1, size=(A, A), dtype=np.int8)
        if (lo, hi) == (-128, 127):
            for t in range(0, A, 16):
                assert np.bincount(q[t:t + 16].view(np.uint8).ravel(), minlength=256).min() > 0, t
        scale = np.exp2(-(np.arange(A) % 4)).astype(np.float32)
        _cases[key] = (q, scale, rng.integers(-5, 6, size=A))
    return _cases[key]


def conditions8(flat, q, scale, bias):
    """tower_probe.linear_conditions for the scaled Linear: a column's logit is s_n * (integer partial sums of x . q +
    bias / s_n) with s_n a power of two and bias / s_n an integer, so every partial sum, in any order and grouping and on
    either side of the scale, is exact in fp32 once  max_row sum|x| * max|q| + max|bias / s| < 2^24.  Returns the lhs."""
    sc = np.asarray(scale, np.float64)
    assert np.array_equal(np.exp2(np.rint(np.log2(sc))), sc)
    units = np.asarray(bias, np.float64) / sc
    assert np.array_equal(units, np.rint(units))
    qmax = max(int(q.max()), -int(q.min()))                    # not np.abs: |-128| does not exist in int8
    return tp.linear_conditions(flat, np.array([qmax], np.int64), units)


def expected8(policy, q, scale, bias):
    """float64 logits: bias + scale * (flat @ q.T), from the reference's policy-conv output [n, A_ch, R, R]"""
    flat = policy.reshape(policy.shape[0], -1)
    return tp.dense_apply(flat, q, np.zeros(q.shape[0])) * np.asarray(scale, np.float64)[None, :] + np.asarray(bias, np.float64)[None, :]


MUTATIONS8 = ("pair_swap", "scale_neighbour", "unsigned_byte", "scale_before_seam", "drop_kstep", "drop_last_slab")


def mutated8(policy, R, q, scale, bias, name):
    """expected8 with ONE fault in k_fcw8's own decomposition: k-steps of 32 in NHWC order, 1-KiB pieces of two column
    tiles, per-column scales in the epilogue, K-split slabs per column group of 384"""
    A = q.shape[0]
    flat = policy.reshape(policy.shape[0], -1)
    acc = tp.dense_apply(flat, q, np.zeros(A))                 # the unscaled sums
    sc, b = np.asarray(scale, np.float64), np.asarray(bias, np.float64)
    X, Wp = tp.engine_order(flat, R), tp.engine_order(q, R).astype(np.float64)
    Kp = (A + 511) // 512 * 512
    gw, sk = tp.linear_splits(R, 2)
    klen = Kp // sk
    g0, ct, ks = 1, gw // 16 + 5, klen // 32 + 3               # column group 1; a column tile and a k-step inside it

    def part(cols, k0, k1, W=Wp):
        k1 = min(k1, A)
        return X[:, k0:k1] @ W[cols, k0:k1].T

    if name == "scale_neighbour":                               # column n scaled by s_{n+1}
        return acc * np.roll(sc, -1)[None, :] + b[None, :]
    if name == "pair_swap":                                     # the two tiles of one 1-KiB piece exchanged
        pr = ct // 2
        c0, c1 = slice(32 * pr, 32 * pr + 16), slice(32 * pr + 16, 32 * pr + 32)
        p0, p1 = part(c0, 32 * ks, 32 * ks + 32), part(c1, 32 * ks, 32 * ks + 32)
        acc[:, c0] += p1 - p0
        acc[:, c1] += p0 - p1
    elif name == "unsigned_byte":                               # a negative q read as q + 256 (one tile, one k-step)
        cols = slice(16 * ct, 16 * ct + 16)
        acc[:, cols] += part(cols, 32 * ks, 32 * ks + 32, np.where(Wp < 0, 256.0, 0.0))
    elif name == "drop_kstep":                                  # one k-step of one column tile never multiplied
        cols = slice(16 * ct, 16 * ct + 16)
        acc[:, cols] -= part(cols, 32 * ks, 32 * ks + 32)
    elif name == "drop_last_slab":                              # k_fc_reduce / logit_at: one slab short
        cols = slice(g0 * gw, min((g0 + 1) * gw, A))
        acc[:, cols] -= part(cols, (sk - 1) * klen, sk * klen)
    elif name == "scale_before_seam":                           # the scale applied to slab 0 only, the others added raw
        cols = slice(g0 * gw, min((g0 + 1) * gw, A))
        first = part(cols, 0, klen)
        out = acc * sc[None, :] + b[None, :]
        out[:, cols] = b[None, cols] + first * sc[None, cols] + (acc[:, cols] - first)
        return out
    else:
        raise ValueError(name)
    return acc * sc[None, :] + b[None, :]


def dead_fragment_products8(policy, R, q):
    """tower_probe.dead_fragment_products' criterion on the int8 weights: (dead, total) over every (16-row tile, 16-column
    tile, 32-deep k-step) of real indices; dead = the fragment product is zero in all 256 elements"""
    A = q.shape[0]
    X = torch.from_numpy(tp.engine_order(policy.reshape(policy.shape[0], -1), R).astype(np.float32))
    Wk = torch.from_numpy(np.ascontiguousarray(tp.engine_order(q, R).T))
    n, nct = X.shape[0], A // 16
    assert n % 16 == 0 and A % 16 == 0
    dead = total = 0
    for k0 in range(0, A, 32):
        c = X[:, k0:k0 + 32] @ Wk[k0:k0 + 32].to(torch.float32)
        live = (c != 0).view(n // 16, 16, nct, 16).any(dim=3).any(dim=1)
        dead += int((~live).sum())
        total += live.numel()
    return dead, total


# ---------------------------------------------------------------------------------------------------------------------
# quantize_fc's numeric spec, restated in numpy float32 independently of weights.py
# ---------------------------------------------------------------------------------------------------------------------
def quantize_spec(w):
    w = np.asarray(w, np.float32)
    if not np.isfinite(w).all():
        raise ValueError("non-finite weight")
    N, K = w.shape
    q = np.zeros((N, K), np.int8)
    s = np.ones(N, np.float32)
    floor = np.float32(127.0) * np.float32(2.0 ** -100)
    for n in range(N):
        m = np.float32(np.max(np.abs(w[n])))
        if not m < floor:
            s[n] = np.float32(m / np.float32(127.0))
        r = np.rint((w[n] / s[n]).astype(np.float32))          # numpy's rint: ties to even
        q[n] = np.clip(r, -127.0, 127.0).astype(np.int8)
    return q, s
