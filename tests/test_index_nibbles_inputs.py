"""CPU: the inputs of test_index_nibbles_gpu.py have the properties those
tests rely on, by exact integer arithmetic over every value the kernels'
bucket scale can take (index_inputs)."""
import numpy as np
import pytest

import index_inputs as I


@pytest.mark.parametrize("tile", [1024, 2048])
@pytest.mark.parametrize("c", [13, 14, 15, 16, 17, 18, 1000])
def test_crafted_tile_occupancy_and_margins(tile, c):
    D, x0 = I.crowded_D(tile, c)
    assert D.size == 3 * tile + 17
    assert np.all(D[1:] > D[:-1])
    mid = [int(x) for x in D[tile:2 * tile]]
    assert mid[-1] - mid[0] >= 1 << 40
    run = list(range(x0, x0 + c))
    assert set(run) <= set(mid)
    klo, s2, r32 = I.tile_map(mid)
    muls = I.mul_candidates(r32, tile)
    assert 1 <= len(muls) <= 3
    width = (mid[-1] - mid[0]) // tile
    for mul, occ in zip(muls, I.occupancy(mid, tile)):
        b = I.bucket(x0, klo, s2, r32, mul, tile)
        # the run, and 1 % of a bucket width on either side of it, in one bucket
        for x in (x0 - width // 100, x0 + c - 1, x0 + c - 1 + width // 100):
            assert I.bucket(x, klo, s2, r32, mul, tile) == b
        # that bucket holds the run and at most one grid key; every other at most 2
        assert c <= occ[b] <= c + 1
        assert max(n for bb, n in occ.items() if bb != b) <= 2
        # stored for c <= 13, marked for c >= 15 (c = 14 may be either)
        if c <= 13:
            assert max(occ.values()) <= 14
        if c >= 15:
            assert max(occ.values()) >= 15


@pytest.mark.parametrize("tile", [1024, 2048])
def test_uniform_neighbours_are_stored(tile):
    """The uniform tiles next to the crafted one hold no bucket past 14 keys."""
    D, _ = I.crowded_D(tile, 16)
    for lo in (0, 2 * tile):
        keys = [int(x) for x in D[lo:lo + tile]]
        for occ in I.occupancy(keys, tile):
            assert max(occ.values()) <= 14
    tail = [int(x) for x in D[3 * tile:]]
    for occ in I.occupancy(tail, tile):
        assert max(occ.values()) <= 14


def test_pushes_reach_the_crowded_bucket():
    D, x0 = I.crowded_D(1024, 16)
    ps = I.pushes_over(D, 8, 300, 66, hot=(x0, 16))
    for k, vs in ps:
        assert np.all(k[1:] > k[:-1]) and np.isin(k, D).all()
        assert np.count_nonzero((k >= x0) & (k < x0 + 16)) >= 10
        assert 250 <= k.size <= 330 and vs[0].size == k.size


@pytest.mark.parametrize("ntiles", [1, 15, 16, 17, 63, 64, 65])
def test_partition_inputs(ntiles):
    """The pushes of test_partition_lines_gpu.py: sorted, unique; the one-key,
    below, above and single-tile pushes lie where their names say; the
    geometric push's keys grow geometrically, so a linear guess inside any
    bracket of 8 or more keys lands above the true position."""
    D, ps = I.partition_case(ntiles)
    assert D.size == ntiles * I.PTILE and np.all(D[1:] > D[:-1])
    for k, vs in ps:
        assert np.all(k[1:] > k[:-1]) and vs[0].size == k.size
    assert ps[1][0].size == 0 and ps[2][0].size == 1
    assert int(ps[3][0][-1]) < int(D[0]) and int(ps[4][0][0]) > int(D[-1])
    t0 = ntiles // 2
    assert int(D[t0 * I.PTILE]) <= int(ps[5][0][0]) and int(ps[5][0][-1]) <= int(D[(t0 + 1) * I.PTILE - 1])
    g = [int(x) for x in ps[6][0]]
    assert np.isin(ps[6][0], D).all() and len(g) >= 16
    # the upper half of the push (past the part where D's spacing saturates
    # the progression): every window of 9 keys has its middle key below the
    # middle of its value range -- interpolation overshoots
    h = g[len(g) // 2:]
    bad = sum(1 for i in range(0, len(h) - 8) if 2 * h[i + 4] >= h[i] + h[i + 8])
    assert bad * 4 <= max(1, len(h) - 8)
    # and over the whole push the middle key lies in the lowest quarter of the range
    assert g[len(g) // 2] - g[0] < (g[-1] - g[0]) // 4
