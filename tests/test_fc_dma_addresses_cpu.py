"""The LDS-DMA addressing of k_fcw / k_fcw8 (csrc/fpc_fc.h), modelled in NumPy: no GPU.

Until this change every piece of the two kernels was a statement of its own: M0 = the piece's LDS address, source = a
scalar base + a per-lane offset, immediate 0 (the second piece of a k_fcw weight pair: 1024).  Now the kernel writes M0
once per GROUP (the 8 activation pieces of a stage; the weight pieces of k-step 0; those of k-step 1) to the middle of the
group's LDS bytes, and a piece is one instruction whose immediate moves BOTH its LDS destination and its global source.
A wrong address here is a GPU fault or silently misplaced operands, so both forms are written down side by side, from
the kernels' own expressions, and compared for every piece of the first four stages, the last two and the clamped tail
(both forms are affine in the stage up to the clamp and the buffer parity) of the first, a middle and the last column
group, every K-split, every wave, the first and the last row tile -- for every plan plan_fcw accepts at 8x8 .. 14x14:
  * every piece reads the same source bytes and fills the same LDS bytes as before,
  * every immediate lies in -4096 .. 3072 and is a multiple of 1024,
  * every per-lane offset is below 2^32, and base + offset + immediate never leaves the allocation it reads
    (activations [Mtot][Kp] 16 bit; weights [Kp/32][Np/16] fragments of 1 KiB, half of that in int8),
  * every LDS destination lies in the part of LDS the wave owns for that stage.
"""
import os
import re

import numpy as np
import pytest

import weights

HERE = os.path.dirname(os.path.abspath(__file__))
FC_H = os.path.join(os.path.dirname(HERE), "alphazero-4-player-chess_amd", "csrc", "fpc_fc.h")

FC_XBUF = 256 * 64 * 2
RING = {"k_fcw": 24 * 1024, "k_fcw8": 12 * 1024}
XMID = 4096
WMID = {"k_fcw": 3072, "k_fcw8": 1024}
TILES = {"k_fcw": 6, "k_fcw8": 3}          # weight pieces per k-step and wave
LANE = np.arange(64, dtype=np.int64)


def test_the_model_uses_the_header_s_constants():
    src = open(FC_H).read()

    def const(name):
        m = re.search(r"constexpr int %s = ([^;]+);" % name, src)
        assert m, name
        return int(eval(m.group(1), {"__builtins__": {}}, {"FC_XBUF": FC_XBUF, "FC_WRING": 16 * 1024,
                                                          "FCW_WRING": RING["k_fcw"], "FCW8_WRING": RING["k_fcw8"]}))

    assert const("FC_XBUF") == FC_XBUF
    assert const("FCW_WRING") == RING["k_fcw"] and const("FCW8_WRING") == RING["k_fcw8"]
    assert const("FCW_XMID") == XMID and const("FCW_WMID") == WMID["k_fcw"] and const("FCW8_WMID") == WMID["k_fcw8"]
    assert const("FCW_LDS") == 2 * FC_XBUF + 4 * RING["k_fcw"] and const("FCW8_LDS") == 2 * FC_XBUF + 4 * RING["k_fcw8"]


def _geom(R):
    A = (8 * R + 8) * R * R
    return A, (A + 383) // 384 * 384, (A + 511) // 512 * 512


def _plans():
    out = []
    for R in range(8, 15):
        seen = set()
        for cus in (64, 80, 104, 128, 228, 256, 304):
            sk = weights.fcw_split(R, cus)
            if sk and sk not in seen:
                seen.add(sk)
                out.append((R, sk))
    return out


def _xlane(par, Kp):
    j = (LANE & 7) ^ ((par * 4 + (LANE >> 4)) & 7)
    return (LANE >> 3) * Kp * 2 + j * 16


def _pieces(kernel, R, sk, block, wave, tile_y, Mtot):
    """yields (what, old (src, lds), new (src, lds, imm, lane_off)) per piece: src / lds are per-lane byte addresses
    relative to the allocation / to LDS 0, for every stage any statement of the kernel issues"""
    A, Np, Kp = _geom(R)
    ksteps = Kp // 16
    split = block % sk
    group = block // sk
    KS = ksteps // sk
    ks0 = split * KS
    S = KS // 4
    assert KS % 4 == 0 and S >= 4
    mrow0 = tile_y * 256
    T = TILES[kernel]
    frag_cols = 16 if kernel == "k_fcw" else 32
    wbase = ((ks0 // 2) * (Np // frag_cols) + group * 4 * T + wave * T) * 1024
    wk32 = (Np // frag_cols) * 1024
    wlane = LANE * 16
    xbase = ((mrow0 + wave * 64) * Kp + ks0 * 16) * 2
    xpiece = 8 * Kp * 2
    lds_w = 2 * FC_XBUF + wave * RING[kernel]
    wmid = WMID[kernel]
    # activations: the prologue issues stage 0, k-step (s, 0) issues stage s + 1 for s < S: stages 0 .. S
    for s in sorted({0, 1, 2, 3, S - 2, S - 1, S}):
        sc = min(s, S - 1)
        m0 = (s & 1) * FC_XBUF + wave * 64 * 128 + XMID
        for p in range(8):
            old_src = xbase + p * xpiece + sc * 128 + _xlane(p & 1, Kp)
            old_lds = (s & 1) * FC_XBUF + (wave * 64 + p * 8) * 128 + LANE * 16
            imm = p * 1024 - XMID
            off = _xlane(p & 1, Kp)
            base = xbase + p * (xpiece - 1024) + XMID + sc * 128
            yield ("X", s, p), (old_src, old_lds), (base + off + imm, m0 + imm + LANE * 16, imm, off, base)
    # weights: the prologue issues stages 0 and 1, the stage loop s + 2 for s < S: stages 0 .. S + 1
    for s in sorted({0, 1, 2, 3, S - 1, S, S + 1}):
        sc = min(s, S - 1)
        for j in range(2):
            m0 = lds_w + ((s & 1) * 2 * T + j * T) * 1024 + wmid
            base = wbase + (2 * sc + j) * wk32 + wmid
            for n in range(T):
                if kernel == "k_fcw":       # pairs: fc_dma2_nt(base of tile n0) + an immediate of 1024 for tile n0 + 1
                    n0 = n & ~1
                    old_src = wbase + (2 * sc + j) * wk32 + n0 * 1024 + wlane + (n - n0) * 1024
                    old_lds = lds_w + ((s & 1) * 12 + j * 6 + n0) * 1024 + (n - n0) * 1024 + LANE * 16
                else:
                    old_src = wbase + (2 * sc + j) * wk32 + n * 1024 + wlane
                    old_lds = lds_w + ((s & 1) * 6 + j * 3 + n) * 1024 + LANE * 16
                imm = n * 1024 - wmid
                yield ("W", s, j, n), (old_src, old_lds), (base + wlane + imm, m0 + imm + LANE * 16, imm, wlane, base)


@pytest.mark.parametrize("kernel", ["k_fcw", "k_fcw8"])
@pytest.mark.parametrize("R,sk", _plans(), ids=lambda v: str(v))
def test_every_piece_reads_and_fills_what_it_did(kernel, R, sk):
    A, Np, Kp = _geom(R)
    groups = Np // 384
    lds_total = 2 * FC_XBUF + 4 * RING[kernel]
    imms = set()
    count = 0
    for Mtot, tile_y in ((256, 0), (512, 1)):
        x_bytes = Mtot * Kp * 2
        w_bytes = Np * Kp * (2 if kernel == "k_fcw" else 1)
        for group in sorted({0, groups // 2, groups - 1}):
            for split in range(sk):
                for wave in range(4):
                    for what, old, new in _pieces(kernel, R, sk, group * sk + split, wave, tile_y, Mtot):
                        src, lds, imm, off, base = new
                        assert np.array_equal(src, old[0]), (what, "source")
                        assert np.array_equal(lds, old[1]), (what, "LDS destination")
                        assert -4096 <= imm <= 3072 and imm % 1024 == 0, (what, imm)
                        assert off.min() >= 0 and off.max() < 2 ** 32, (what, "lane offset")
                        assert base >= 0 and base + int(off.min()) + imm >= 0, (what, "address below the allocation")
                        limit = x_bytes if what[0] == "X" else w_bytes
                        assert src.min() >= 0 and src.max() + 16 <= limit, (what, int(src.max()), limit)
                        if what[0] == "X":
                            lo = (what[1] & 1) * FC_XBUF + wave * 8192
                            assert lo <= lds.min() and lds.max() + 16 <= lo + 8192, what
                        else:
                            lo = 2 * FC_XBUF + wave * RING[kernel] + (what[1] & 1) * (RING[kernel] // 2)
                            assert lo <= lds.min() and lds.max() + 16 <= lo + RING[kernel] // 2, what
                        assert lds.max() + 16 <= lds_total
                        imms.add((what[0], imm))
                        count += 1
    T = TILES[kernel]
    assert {i for w, i in imms if w == "X"} == {p * 1024 - XMID for p in range(8)}
    assert {i for w, i in imms if w == "W"} == {n * 1024 - WMID[kernel] for n in range(T)}
    assert count > 0


def test_the_model_can_fail():
    """a piece distance left in the immediate only (the source 1 KiB per piece instead of eight rows) is caught"""
    R, sk = 8, weights.fcw_split(8)
    A, Np, Kp = _geom(R)
    xpiece = 8 * Kp * 2
    p, XB = 3, 0
    right = XB + p * xpiece + _xlane(p & 1, Kp)
    wrong = (XB + XMID) + _xlane(p & 1, Kp) + (p * 1024 - XMID)
    assert not np.array_equal(right, wrong)
    good = (XB + p * (xpiece - 1024) + XMID) + _xlane(p & 1, Kp) + (p * 1024 - XMID)
    assert np.array_equal(right, good)
