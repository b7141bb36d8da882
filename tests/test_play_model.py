"""selfplay.sample_move, the plain-Python statement of the device draw (include/fpc_engine.h fpc_search_play): CPU only."""
import numpy as np

import selfplay


def test_temperature_one_is_the_integer_inverse_cdf():
    flats, visits = [7, 3, 50, 11], [1, 4, 2, 3]              # prefix sums 1 5 7 10
    pick = lambda u: selfplay.sample_move(flats, visits, 1.0, u)
    assert pick(0.0) == 7 and pick(0.0999) == 7
    assert pick(0.1) == 3                                     # c_0 = 1 > 0.1 * 10 is false: the boundary belongs to the next child
    assert pick(0.4999) == 3 and pick(0.5) == 50 and pick(0.6999) == 50 and pick(0.7) == 11
    assert pick(np.nextafter(1.0, 0.0)) == 11
    # S = 8: every u = j / 8 and u * S are exact, child k owns the integers j in [c_{k-1}, c_k)
    owners = [0, 1, 1, 1, 2, 2, 3, 3]                        # visits 1 3 2 2: prefix sums 1 4 6 8
    for j in range(8):
        assert selfplay.sample_move([20, 21, 22, 23], [1, 3, 2, 2], 1.0, j / 8.0) == 20 + owners[j], j
    assert selfplay.sample_move([9], [5], 1.0, 0.7) == 9
    assert selfplay.sample_move(np.array([4, 2]), np.array([3, 1], np.int32), 1.0, 0.75) == 2


def test_temperature_zero_is_the_first_maximum():
    assert selfplay.sample_move([5, 6, 7, 8], [2, 9, 9, 1], 0, 0.99) == 6
    assert selfplay.sample_move([5, 6, 7], [1, 1, 1], 0.0, 0.0) == 5
    assert selfplay.sample_move([5, 6, 7], [1, 2, 3], 0, 0.5) == 7


def test_other_temperatures_weigh_by_pow():
    flats, visits = [1, 2, 3], [1, 4, 9]                      # T = 2: weights 1 2 3, sums 1 3 6
    pick = lambda u: selfplay.sample_move(flats, visits, 2.0, u)
    assert pick(0.16) == 1 and pick(0.17) == 2 and pick(0.49) == 2 and pick(0.51) == 3
    # T = 0.5: weights 1 16 81, sums 1 17 98
    pick = lambda u: selfplay.sample_move(flats, visits, 0.5, u)
    assert pick(0.0102) == 1 and pick(0.0103) == 2 and pick(0.173) == 2 and pick(0.174) == 3


def test_agrees_with_sample_action_away_from_the_boundaries():
    """sample_action normalises in f32 twice; its boundaries sit within ~1e-6 * S of sample_move's.  Wherever u * S is
    farther than 1e-5 * S from every c_k the two pick the same child.  Each case has at most one boundary that close, an
    interval of 2e-5 in u per boundary a uniform u can hit: about 0.1 % of the cases with up to 60 children are
    expected to be excluded (measured on these seeds: 0.07 %), and the bound asserted is 1 %."""
    rng = np.random.default_rng(2024)
    cases, excluded = 10000, 0
    for i in range(cases):
        n = int(rng.integers(2, 61))
        visits = rng.integers(1, 40, size=n).astype(np.int32)
        flats = np.sort(rng.choice(4608, size=n, replace=False)).astype(np.int32)
        T = (1.0, 1.1, 0.5, 1.25)[i % 4]
        u = float(rng.random())
        c = np.cumsum(np.power(visits.astype(np.float64), 1.0 / T))
        if np.abs(c - u * c[-1]).min() <= 1e-5 * c[-1]:
            excluded += 1
            continue
        assert selfplay.sample_move(flats, visits, T, u) == selfplay.sample_action(flats, visits, T, u), (i, T, u)
    print("excluded by the guard: %d of %d cases (%.2f %%)" % (excluded, cases, 100.0 * excluded / cases))
    assert excluded < cases // 100
