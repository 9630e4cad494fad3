"""The tile kernels' bucket search at the edges of its LDS reads: the window
of server keys read from a bucket's start (psg_device.h lds_window4 /
lds_window2) and the bucket table reads around it, in the 32-push, 64-push
and packed forms, f32 and f64, one and two value arrays, serial and parallel.
Every case is a plan or a context flush over a few thousand keys at most,
compared bit for bit with the oracle: the sums and the per-push matched
counts."""
import numpy as np
import pytest

import oracle_py as O
from test_gpu_parity import ALL, assert_bitexact, plan_for, run_ctx, torch_cuda  # noqa: F401

pytestmark = pytest.mark.gpu

# form: pushes, keys per push beyond its share of D (as a multiple of that
# share), tile slots, plan flags, the kernel the plan must report
FORMS = {
    "tile32": (8, 3.0, 1024, "PSG_FORM_UNIFORM PSG_GROUP32 PSG_NO_DENSE", "PSG_KERNEL_TILE"),
    "tile64": (33, 3.0, 2048, "PSG_FORM_UNIFORM PSG_GROUP64 PSG_NO_DENSE", "PSG_KERNEL_TILE64"),
    # pieces under 16 keys: 1.2 / 160 of a tile's keys
    "packed": (160, 0.2, 2048, "PSG_FORM_PACKED PSG_NO_DENSE", "PSG_KERNEL_PACKED"),
}
TYPES = [(np.float32, 1), (np.float32, 2), (np.float64, 1), (np.float64, 2)]
by_form = pytest.mark.parametrize("form", list(FORMS))
by_type = pytest.mark.parametrize("dtype,m", TYPES)


def form_of(name):
    from parameter_server_amd import _lib
    npush, more, ts, flags, kernel = FORMS[name]
    fl = 0
    for f in flags.split():
        fl |= getattr(_lib, f)
    return (npush, more), ts, fl, getattr(_lib, kernel)


def values(rng, n, dtype, m):
    vs = []
    for _ in range(m):
        v = rng.standard_normal(n).astype(dtype)
        v[rng.random(n) < 0.05] = -0.0  # the serial fold's "+0.0" shows on these
        vs.append(v)
    return vs


def covering_pushes(rng, D, shape, dtype, m, whole=(), extra=None):
    """npush sorted pushes that together hold every key of D: key i lies in
    push i % npush, each push holds further keys with probability more / npush
    (none is empty) and pushes 0 and 1 hold all of `whole`; extra[p] are
    keys outside D merged into push p."""
    npush, more = shape
    pushes = []
    idx = np.arange(D.size)
    for p in range(npush):
        sel = (idx % npush == p) | (rng.random(D.size) < more / npush)
        if p < 2:
            sel |= np.isin(D, np.asarray(whole, np.uint64))
        if not sel.any():
            sel[rng.integers(D.size)] = True
        k = D[sel]
        if extra and p in extra:
            k = np.unique(np.concatenate([k, np.asarray(extra[p], np.uint64)]))
        pushes.append((k, values(rng, k.size, dtype, m)))
    return pushes


def check(torch, form, D, pushes, dtype, m, ctx=True):
    """Plan (resident index) and, with every key present, a context flush
    (histogram in the kernel), serial and parallel, against the oracle."""
    _, _, flags, kernel = form_of(form)
    for parallel in (False, True):
        rc, _, _, want, wm = O.aggregate(D, *ALL, pushes, parallel, 1, dtype)
        assert rc == 0
        plan, keep = plan_for(torch, [(D, pushes)], dtype=dtype, parallel=parallel, flags=flags)
        assert plan.form == kernel
        plan.run()
        assert plan.matched().tolist() == [int(x) for x in wm]
        for i in range(m):
            assert_bitexact(keep[3][i].cpu().numpy()[: D.size], want[i])
        plan.close()
        if ctx:
            assert [int(x) for x in wm] == [k.size for k, _ in pushes]
            out = run_ctx(D, pushes, dtype=dtype, parallel=parallel, flags=flags)
            assert len(out) == m
            for i in range(m):
                assert_bitexact(out[i][1], want[i])


# ------------------------------------------------- window past the tile's end
@by_form
@by_type
def test_window_past_tile_end(torch_cuda, form, dtype, m):
    """Every server key is pushed, so the windows of a tile's last keys run
    into the sentinels past it; the last tile is partial (or, at 1024 and
    2048 slots, exactly full)."""
    npush = form_of(form)[0]
    for nslots in (1, 2, 3, 4, 5, 1023, 1024, 1025, 2047, 2049):
        rng = np.random.default_rng(1000 + nslots)
        D = np.unique(rng.integers(1, 1 << 62, nslots + 64, dtype=np.uint64))[:nslots]
        assert D.size == nslots
        check(torch_cuda, form, D, covering_pushes(rng, D, npush, dtype, m), dtype, m)


# ---------------------------------------------------------- bucket occupancies
def clustered_keys(rng, runs, odd, nspread=1000):
    """About nspread keys spread over [0, 2^40) and, for each (base, n,
    stride) of runs, n keys `stride` apart from base on, alone in a gap of
    2^33 (8 buckets of a tile of 1024 keys here, more of any other), so each
    run is one bucket that starts at the run's first slot; the first run's
    first slot is odd or even as asked.  Returns D and the runs' keys."""
    s = np.unique(rng.integers(0, 1 << 40, nspread, dtype=np.uint64))
    rs = []
    for base, n, stride in runs:
        gap = np.uint64(1 << 32)
        s = s[(s < np.uint64(base) - gap) | (s > np.uint64(base) + gap)]
        rs.append(np.uint64(base) + np.arange(n, dtype=np.uint64) * np.uint64(stride))
    D = np.unique(np.concatenate([s] + rs))
    if int(np.searchsorted(D, rs[0][0])) % 2 != int(odd):
        D = D[1:]  # one spread key fewer below the runs
    assert D[0] < rs[0][0] and int(np.searchsorted(D, rs[0][0])) % 2 == int(odd)
    return D, rs


@by_form
@by_type
@pytest.mark.parametrize("odd", [False, True])
def test_bucket_occupancies(torch_cuda, form, dtype, m, odd):
    """Buckets of 1 to 4 keys (the spread keys), of more than 4 (the deep
    path, which reads the bucket's end itself) and of more than 14 (a marked
    tile, whose table the kernel builds although the plan has an index); the
    long bucket starts at an even and at an odd slot."""
    npush = form_of(form)[0]
    for run in (2, 4, 5, 6, 14, 15, 20):
        rng = np.random.default_rng(2000 + 2 * run + odd)
        D, (r,) = clustered_keys(rng, [(1 << 39, run, 1)], odd)
        check(torch_cuda, form, D, covering_pushes(rng, D, npush, dtype, m, whole=r), dtype, m)


# ------------------------------------------------------------------ absent keys
@by_form
@by_type
def test_absent_keys(torch_cuda, form, dtype, m):
    """Sorted pushes with keys that are not server keys: between two keys of
    a long bucket, just below a tile's first key, just above its last key,
    below and above all of D, and above every key of a bucket of exactly 4
    keys (all 4 window keys below it, nothing left to bisect).  A push's
    matched count falls by its absent keys; every sum stays exact.

    The order check compares a key's slot with the lower bound of the
    element before it, found or not, and an absent key's lower bound is the
    slot of the server key after it: that server key, as the push's next
    element in the same tile, is reported out of order and the count falls
    below the oracle's (a property of the order check, not of the window
    reads, and older than them).  A push here does not hold the server
    key right after one of its absent keys, unless that key opens the next
    tile, where the check starts anew."""
    torch = torch_cuda
    npush, ts, flags, _ = form_of(form)
    for odd in (False, True):
        rng = np.random.default_rng(3000 + odd)
        # two tiles and a partial one; runs 2 apart: 6 keys (deep), 4 keys (not)
        D, (r6, r4) = clustered_keys(rng, [(1 << 39, 6, 2), (1 << 38, 4, 2)], odd,
                                     nspread=2 * ts + 300)
        assert D.size > 2 * ts and int(D[0]) > 1
        one = np.uint64(1)
        absent = np.array([D[0] - one, r4[1] + one, r4[3] + one, r4[3] + np.uint64(9),
                           r6[0] + one, r6[4] + one, r6[5] + one,
                           D[ts - 1] + one, D[ts] - one, D[2 * ts - 1] + one, D[2 * ts] - one,
                           D[-1] + one], np.uint64)
        assert not np.isin(absent, D).any()
        extra = {1: absent, 3: absent[1::2], npush[0] - 1: absent[::3]}
        pushes = covering_pushes(rng, D, npush, dtype, m, whole=np.concatenate([r4, r6]),
                                 extra=extra)
        for p, ab in extra.items():
            nxt = np.searchsorted(D, ab)
            nxt = nxt[(nxt < D.size) & (nxt % ts != 0)]
            k, vs = pushes[p]
            keep = ~np.isin(k, D[nxt])
            pushes[p] = (k[keep], [v[keep] for v in vs])
        check(torch, form, D, pushes, dtype, m, ctx=False)
        wm = O.aggregate(D, *ALL, pushes, False, 1, dtype)[4]
        assert int(wm[1]) == pushes[1][0].size - absent.size
        assert np.isin(r4[:2], pushes[1][0]).all() and np.isin(r6[:1], pushes[1][0]).all()
        # the context reports them (the reference's CHECK_EQ(matched, n))
        if odd and m == 1:
            from parameter_server_amd._lib import PSGError, PSG_ERR_UNMATCHED
            with pytest.raises(PSGError) as e:
                run_ctx(D, pushes, dtype=dtype, flags=flags)
            assert e.value.status == PSG_ERR_UNMATCHED
