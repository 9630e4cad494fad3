"""Inputs of the resident-bucket-index tests (test_index_nibbles*.py): server
key sets whose middle tile holds one crowded bucket, built and checked with
exact integer arithmetic.

The kernels' bucket map over a tile with first key klo and last key khi
(psg_tile.hip; psg_device.h bucket_scale):
    range = khi - klo, s2 = max(0, bitlength(range) - 32), r32 = range >> s2
    bucket(k) = min(nb - 1, ((k - klo) >> s2) * mul >> 32)
with mul an f32 estimate of nb * 2^32 * (1 - 2^-20) / (r32 + 1), rounded
down.  The estimate's relative error is below 2^-21 (reciprocal 2^-23,
two conversions and two products 2^-24 each), so mul lies in
[floor(x (1 - 2^-19)) - 1, floor(x)] for x = nb 2^32 / (r32 + 1): the
helpers below evaluate every claim for each integer in that interval."""
import numpy as np

RANGE = 1 << 41          # key range of the crafted tile (>= 2^40)
MID_BASE = 1 << 52       # its first key; tile 0 lies below 2^50, tile 2 above 2^53


def mul_candidates(r32, nb):
    hi = (nb << 32) // (r32 + 1)
    lo = ((nb << 32) * ((1 << 19) - 1) // ((r32 + 1) << 19)) - 1
    return list(range(lo, min(hi, (1 << 32) - 1) + 1))


def tile_map(keys):
    """(klo, s2, r32) of a tile's sorted keys (python ints)."""
    klo, khi = int(keys[0]), int(keys[-1])
    rng = khi - klo
    s2 = max(0, rng.bit_length() - 32)
    return klo, s2, rng >> s2


def bucket(k, klo, s2, r32, mul, nb):
    x = (int(k) - klo) >> s2
    if x > r32:
        return nb - 1
    return min(nb - 1, (x * mul) >> 32)


def occupancy(keys, nb):
    """Per candidate mul: the bucket counts of a tile (list of dicts)."""
    klo, s2, r32 = tile_map(keys)
    out = []
    for mul in mul_candidates(r32, nb):
        cnt = {}
        for k in keys:
            b = bucket(k, klo, s2, r32, mul, nb)
            cnt[b] = cnt.get(b, 0) + 1
        out.append(cnt)
    return out


def crafted_tile(tile, c):
    """`tile` sorted unique keys: tile - c on an even grid over RANGE plus c
    consecutive integers inside one bucket, at least 1 % of a bucket width
    from both of its edges under every candidate mul.  Returns (keys, run
    start)."""
    ng = tile - c
    assert ng >= 2
    grid = [MID_BASE + (i * RANGE) // (ng - 1) for i in range(ng)]
    klo, s2, r32 = tile_map([grid[0], grid[-1]])
    muls = mul_candidates(r32, tile)
    width = RANGE // tile
    margin = width // 100 + 1
    gset = set(grid)
    # candidates: the middle of each nominal bucket from the tile's middle on
    for b0 in range(tile // 2, tile - 2):
        x0 = MID_BASE + b0 * width + width // 2 - c // 2
        lo, hi = x0 - margin, x0 + c - 1 + margin
        bs_per_mul = [{bucket(x, klo, s2, r32, mul, tile) for x in (lo, hi)} for mul in muls]
        if any(len(s) != 1 for s in bs_per_mul):
            continue
        if any(x0 <= g < x0 + c for g in grid):
            continue
        run = list(range(x0, x0 + c))
        keys = sorted(gset | set(run))
        assert len(keys) == tile
        return np.array(keys, np.uint64), x0
    raise AssertionError("no bucket takes the run")


def crowded_D(tile, c, seed=0, tail=17):
    """3 tiles + `tail` slots: uniform, crafted (crafted_tile), uniform."""
    rng = np.random.default_rng(1000 + seed)
    t0 = np.unique(rng.integers(1, 1 << 50, 2 * tile, dtype=np.uint64))[:tile]
    t2 = np.unique(rng.integers(1 << 53, 1 << 54, 2 * (tile + tail), dtype=np.uint64))[:tile + tail]
    assert t0.size == tile and t2.size == tile + tail
    mid, x0 = crafted_tile(tile, c)
    return np.concatenate([t0, mid, t2]), x0


def pushes_over(D, npush, n, seed, dtype=np.float32, m=1, hot=None, nhot=24):
    """npush sorted pushes of about n keys of D; `hot` = (first, count): nhot
    more keys from that run of D (the crowded bucket)."""
    rng = np.random.default_rng(seed)
    out = []
    for p in range(npush):
        k = rng.choice(D, min(n, D.size), replace=False)
        if hot is not None:
            i0 = int(np.searchsorted(D, np.uint64(hot[0])))
            k = np.concatenate([k, rng.choice(D[i0:i0 + hot[1]], min(nhot, hot[1]), replace=False)])
        k = np.unique(k)
        vs = [rng.standard_normal(k.size).astype(dtype) for _ in range(m)]
        if p % 3 == 1:
            vs[0][::4] = -0.0
        out.append((k, vs))
    return out


# ------------------------------------------------ partition tests' inputs
PTILE = 1024


def geometric_indices(D, count):
    """Indices of D whose keys follow a geometric progression from D's
    typical spacing up to its top (linear interpolation is wrong in every
    bracket of such a push)."""
    lo, hi = float(D[min(2, D.size - 1)]) + 1.0, float(D[-1])
    t = lo * (hi / lo) ** (np.arange(count) / max(1, count - 1))
    return np.unique(np.searchsorted(D, t.astype(np.uint64)).clip(0, D.size - 1))


def partition_case(ntiles):
    """A job of ntiles 1024-slot tiles and its pushes (test_partition_lines_gpu)."""
    rng = np.random.default_rng(4000 + ntiles)
    n = ntiles * PTILE
    D = np.unique(rng.integers(1 << 30, 1 << 60, 2 * n, dtype=np.uint64))[:n]
    assert D.size == n

    def vals(k):
        return [rng.standard_normal(k.size).astype(np.float32)]

    keysets = [
        np.sort(rng.choice(D, min(n, 200 * ntiles), replace=False)),       # regular
        np.zeros(0, np.uint64),                                            # empty
        D[n // 3: n // 3 + 1].copy(),                                      # one key
        np.unique(rng.integers(1, 1 << 29, 50, dtype=np.uint64)),          # wholly below D
        np.unique(rng.integers(int(D[-1]) + 1, (1 << 61), 50, dtype=np.uint64)),  # wholly above
        np.sort(rng.choice(D[(ntiles // 2) * PTILE:(ntiles // 2 + 1) * PTILE], 100, replace=False)),
        D[geometric_indices(D, 40 * ntiles + 64)].copy(),                  # geometric
    ]
    for o in range(16):  # placed at offset o keys into a 128-B aligned arena (arena_pushes)
        keysets.append(np.sort(rng.choice(D, min(n, 37 * ntiles + o), replace=False)))
    return D, [(k, vals(k)) for k in keysets]
