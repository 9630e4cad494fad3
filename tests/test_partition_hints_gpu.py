"""GPU: the hinted search partition of plans (psg_partition.hip search_item:
the cut the last run left in seg is verified against its two neighbouring
keys and kept, else searched).  A plan's push keys are overwritten in place
between runs (same buffers, same lengths), so the cuts in seg are those of
other keys; every state is checked through the merge -- sums bit for bit and
matched counts -- against the oracle, a plan built fresh on those keys and a
plan that runs with PSG_NO_HINTS.  That cuts are really kept, that a wave
stops testing after a run in which most of its cuts failed, and that it
tests again once its keys repeat, is read from psg_plan_hint_state.

The f32 and f64 jobs are 70,000 slots = 69 tiles of 1024: 70 boundaries in
two waves, the second with 6 valid lanes (edge lanes 0, 16, 32, 48 of the
first, 0 and 5 of the second).  The 64-push form is 33 pushes over 140,000
slots = 69 tiles of 2048."""
import numpy as np
import pytest

import oracle_py as O

pytestmark = pytest.mark.gpu

ALL = (0, (1 << 64) - 1)


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "GPU test run without a GPU"
    from parameter_server_amd import _lib
    _lib.lib()
    return torch


def assert_bitexact(got, want):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype
    u = np.uint32 if got.dtype == np.float32 else np.uint64
    assert np.array_equal(got.view(u), want.view(u))


def to_dev(torch, a):
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a.view(np.int64) if a.dtype == np.uint64 else a).cuda()


KINDS = {  # nslots, tile, pushes, keys per push, value type
    "f32": (70000, 1024, 3, 10000, np.float32),
    "f64": (70000, 1024, 3, 10000, np.float64),
    "wide": (140000, 2048, 33, 5000, np.float32),
}


def flags_of(kind, hints=True):
    from parameter_server_amd import _lib as L
    f = L.PSG_FORM_UNIFORM | L.PSG_PART_SEARCH | (L.PSG_GROUP64 if kind == "wide" else L.PSG_GROUP32)
    return f | (0 if hints else L.PSG_NO_HINTS)


_base = {}


def base(kind):
    """(D, pushes): sorted unique keys drawn from D, fixed values (shared)."""
    if kind not in _base:
        nslots, _, npush, n, dt = KINDS[kind]
        rng = np.random.default_rng(len(kind) * 1000 + nslots)
        D = np.unique(rng.integers(1 << 20, 1 << 60, 2 * nslots, dtype=np.uint64))[:nslots]
        assert D.size == nslots
        ps = [(np.sort(rng.choice(D, n, replace=False)), [rng.standard_normal(n).astype(dt)])
              for _ in range(npush)]
        _base[kind] = (D, ps)
    return _base[kind]


_want = {}


def oracle(kind, name, keys):
    """The oracle's sums and matched counts of base(kind)'s job with the
    pushes' keys replaced by `keys`; once per named state."""
    if (kind, name) not in _want:
        D, ps = base(kind)
        pushes = [(k, vs) for k, (_, vs) in zip(keys, ps)]
        _, _, _, want, wm = O.aggregate(D, *ALL, pushes, dtype=KINDS[kind][4])
        _want[kind, name] = (np.array(want[0]), [int(x) for x in wm])
    return _want[kind, name]


class Rig:
    """A one-job plan over base(kind) whose push keys can be overwritten."""

    def __init__(self, torch, kind, keys, hints=True):
        from parameter_server_amd import _lib as L
        from parameter_server_amd.kv_vector import MergePlan
        D, ps = base(kind)
        dt = KINDS[kind][4]
        self.torch, self.n = torch, D.size
        self.dD = to_dev(torch, D)
        self.pk = [to_dev(torch, k) for k in keys]
        self.pv = [to_dev(torch, vs[0]) for _, vs in ps]
        self.out = torch.full((D.size,), float("nan"), device="cuda",
                              dtype=torch.float32 if dt == np.float32 else torch.float64)
        job = {"keys": self.dD.data_ptr(), "nslots": D.size,
               "push_keys": [t.data_ptr() for t in self.pk],
               "push_vals": [[t.data_ptr()] for t in self.pv],
               "push_n": [k.size for k in keys], "out": [self.out.data_ptr()]}
        self.plan = MergePlan(0, L.PSG_F32 if dt == np.float32 else L.PSG_F64, 1, [job], False,
                              flags_of(kind, hints))
        assert self.plan.form == (L.PSG_KERNEL_TILE64 if kind == "wide" else L.PSG_KERNEL_TILE)

    def set_keys(self, keys):
        for t, k in zip(self.pk, keys):
            assert t.numel() == k.size
            t.copy_(to_dev(self.torch, k))

    def run(self):
        self.out.fill_(float("nan"))
        self.plan.run()
        return self.out.cpu().numpy(), self.plan.matched().tolist()

    def state(self):
        """Waves [searched, searching untested, kept every cut, not run]."""
        return self.plan.hint_state()

    def close(self):
        self.plan.close()


def walk(torch, kind, states):
    """One hinted and one unhinted plan taken through `states` ([(name,
    keys)]) in place; each state also on a freshly built plan."""
    on = Rig(torch, kind, states[0][1])
    off = Rig(torch, kind, states[0][1], hints=False)
    for name, keys in states:
        want, wm = oracle(kind, name, keys)
        fresh = Rig(torch, kind, keys)
        on.set_keys(keys)
        off.set_keys(keys)
        for rig in (on, off, fresh):
            got, mt = rig.run()
            assert mt == wm, name
            assert_bitexact(got, want)
        fresh.close()
    on.close()
    off.close()


def redraw(kind, seed):
    """Other keys of D for every push, the same lengths."""
    D, ps = base(kind)
    rng = np.random.default_rng(seed)
    return [np.sort(rng.choice(D, k.size, replace=False)) for k, _ in ps]


def cut(k, D, tile, b):
    """Push k's cut at boundary b."""
    x = int(D[b * tile]) if b * tile < D.size else int(D[-1]) + 1
    return int(np.searchsorted(k, np.uint64(x)))


def shift_cut(k, D, tile, b):
    """k with one key taken out of its piece of tile b - 1 and one key of tile
    b put in: the cut at boundary b moves down by one and every other cut
    stays (still a lower bound: the old cut's test passes there).  b ==
    ntiles: the key put in lies above D."""
    nt = (D.size + tile - 1) // tile
    c0, c1 = cut(k, D, tile, b - 1), cut(k, D, tile, b)
    assert c1 - c0 >= 3
    if b == nt:
        new = np.uint64(int(D[-1]) + 5)
    else:
        c2 = cut(k, D, tile, b + 1)
        assert c2 - c1 >= 2
        inside = D[b * tile + 1: min((b + 1) * tile, D.size)]
        free = inside[~np.isin(inside, k) & (inside > k[c1])]
        new = free[0]
    out = np.sort(np.concatenate([np.delete(k, c0 + 1), [new]]).astype(np.uint64))
    assert out.size == k.size and np.unique(out).size == out.size
    assert cut(out, D, tile, b) == c1 - 1
    for o in range(nt + 1):
        assert o == b or cut(out, D, tile, o) == cut(k, D, tile, o)
    return out


# ------------------------------------------------------------ repeating keys
@pytest.mark.parametrize("kind", list(KINDS))
def test_same_keys_three_runs(torch_cuda, kind):
    """Run one searches (zeroed hints), runs two and three keep every cut:
    all three equal the oracle and the unhinted plan, bit for bit."""
    keys = [k for k, _ in base(kind)[1]]
    want, wm = oracle(kind, "base", keys)
    assert wm == [k.size for k in keys]
    on, off = Rig(torch_cuda, kind, keys), Rig(torch_cuda, kind, keys, hints=False)
    waves = 2 * len(keys)  # two boundary groups per push
    assert on.state() == [0, 0, 0, waves] and off.state() == [0, 0, 0, 0]
    for r in range(3):
        for rig in (on, off):
            got, mt = rig.run()
            assert mt == wm
            assert_bitexact(got, want)
        # the first run searches, every later one keeps every cut of every wave
        assert on.state() == ([waves, 0, 0, 0] if r == 0 else [0, 0, waves, 0])
        assert off.state() == [0, 0, 0, 0]
    on.close()
    off.close()


# ------------------------------------------------- keys replaced between runs
@pytest.mark.parametrize("kind", list(KINDS))
def test_all_keys_new(torch_cuda, kind):
    """Every hint of the second and third state is another key set's cut."""
    keys = [k for k, _ in base(kind)[1]]
    walk(torch_cuda, kind, [("base", keys), ("redraw1", redraw(kind, 1)),
                            ("redraw2", redraw(kind, 2)), ("base", keys)])


@pytest.mark.parametrize("kind", list(KINDS))
def test_one_region_new(torch_cuda, kind):
    """The keys inside tiles 20..27 redrawn (the same number of them): the
    lanes of boundaries 21..27 miss in a wave whose other lanes hit."""
    D, ps = base(kind)
    tile = KINDS[kind][1]
    rng = np.random.default_rng(7)
    keys = []
    for k, _ in ps:
        c0, c1 = cut(k, D, tile, 20), cut(k, D, tile, 28)
        new = np.sort(rng.choice(D[20 * tile: 28 * tile], c1 - c0, replace=False))
        keys.append(np.concatenate([k[:c0], new, k[c1:]]))
        assert keys[-1].size == k.size
    walk(torch_cuda, kind, [("base", [k for k, _ in ps]), ("region", keys)])


def test_edge_and_inner_lanes_miss_alone(torch_cuda):
    """One cut moved per push, all others kept: an edge lane misses between
    inner lanes that hit (boundary 16; the last valid lane, boundary 69, whose
    cut moves from n to n - 1) and an inner lane misses between edge lanes
    that hit (boundaries 17 and 66)."""
    D, ps = base("f32")
    keys = [k for k, _ in ps]
    edge = [shift_cut(keys[0], D, 1024, 16), shift_cut(keys[1], D, 1024, 69), keys[2]]
    inner = [shift_cut(keys[0], D, 1024, 17), shift_cut(keys[1], D, 1024, 66),
             shift_cut(keys[2], D, 1024, 1)]
    walk(torch_cuda, "f32", [("base", keys), ("edge", edge), ("base", keys), ("inner", inner),
                             ("edge", edge)])


def test_pushes_below_and_above_D(torch_cuda):
    """Every cut 0 (all keys below D[0]) or n (all above the last key), after
    and before the cuts of keys inside D."""
    D, ps = base("f32")
    keys = [k for k, _ in ps]
    n = keys[0].size
    below = np.arange(1, n + 1, dtype=np.uint64)
    above = np.uint64(int(D[-1]) + 1) + np.arange(n, dtype=np.uint64)
    assert below[-1] < D[0]
    lo_hi = [below, above, keys[2]]
    hi_lo = [above, below, keys[2]]
    walk(torch_cuda, "f32", [("base", keys), ("lo_hi", lo_hi), ("hi_lo", hi_lo), ("base", keys)])
    assert oracle("f32", "lo_hi", lo_hi)[1] == [0, 0, n]


def test_push_key_equal_to_boundary_key(torch_cuda):
    """x = D[b * tile] in the push next to x - 1 (absent from D): first at the
    old cut's index (x - 1 below it: the hint holds), then one index lower
    (the old cut now points past x: it must not be kept)."""
    D, ps = base("f32")
    keys = [k for k, _ in ps]
    st_a, st_b = [], []
    # per push an edge lane, an inner lane, the second wave's first lane (or
    # the next such boundary whose key the push does not hold already)
    for p, bs in enumerate(((16, 32, 48), (40, 41, 42, 43), (64, 48, 32))):
        k = keys[p]
        b = [b for b in bs if D[b * 1024] not in k][0]
        x = D[b * 1024]
        assert x - np.uint64(1) > D[b * 1024 - 1]
        c = cut(k, D, 1024, b)
        a = k.copy()
        a[c - 1], a[c] = x - np.uint64(1), x
        bb = k.copy()
        bb[c - 2], bb[c - 1] = x - np.uint64(1), x
        for z, cz in ((a, c), (bb, c - 1)):
            assert np.all(z[1:] > z[:-1]) and cut(z, D, 1024, b) == cz
        st_a.append(a)
        st_b.append(bb)
    walk(torch_cuda, "f32", [("base", keys), ("at_cut", st_a), ("below_cut", st_b), ("at_cut", st_a)])


# ------------------------------------------------------------ unsorted pushes
def _swapped(k, D, how):
    k = k.copy()
    n = k.size
    if how == "in_piece":       # two keys of one piece
        c = cut(k, D, 1024, 30)
        i, j = c + 5, c + 6
    elif how == "blocks":       # two blocks, tiles apart
        a, b = slice(n // 8, n // 8 + 40), slice(n - 100, n - 60)
        k[a], k[b] = k[b].copy(), k[a].copy()
        return k
    else:                       # across the first and the last boundary
        i, j = 0, n - 1
    k[i], k[j] = k[j], k[i]
    return k


@pytest.mark.parametrize("how", ["in_piece", "blocks", "first_last"])
def test_unsorted_after_a_sorted_run_is_reported(torch_cuda, how):
    """Push 1 made unsorted in place after a sorted run: every hint that still
    passes its two-key test is kept, and the aggregate kernel's own order
    check reports the push (matched < n) while the others stay exact;
    restoring the keys restores exact results."""
    D, ps = base("f32")
    keys = [k for k, _ in ps]
    want, wm = oracle("f32", "base", keys)
    rig = Rig(torch_cuda, "f32", keys)
    got, mt = rig.run()
    assert mt == wm
    assert_bitexact(got, want)
    rig.set_keys([keys[0], _swapped(keys[1], D, how), keys[2]])
    for _ in range(2):
        _, mt = rig.run()
        assert mt[1] < keys[1].size and mt[0] == wm[0] and mt[2] == wm[2]
    rig.set_keys(keys)
    got, mt = rig.run()
    assert mt == wm
    assert_bitexact(got, want)
    rig.close()


# ------------------------------------------- the switch: stop and resume testing
class Model:
    """The waves' states as search_item's comment defines them, from the cuts
    alone (the old cut of a sorted push passes its test iff it is the new
    cut): 0 searched / 1 searching untested / 2 kept every cut / 3 not run."""

    def __init__(self, kind):
        self.D, ps = base(kind)
        self.tile = KINDS[kind][1]
        self.nb = (self.D.size + self.tile - 1) // self.tile + 1  # boundaries
        self.seg = [np.zeros(self.nb, np.int64) for _ in ps]
        self.st = [[3] * ((self.nb + 63) // 64) for _ in ps]

    def run(self, keys):
        for p, k in enumerate(keys):
            new = np.array([cut(k, self.D, self.tile, b) for b in range(self.nb)])
            for w in range(len(self.st[p])):
                sl = slice(64 * w, min(64 * w + 64, self.nb))
                same = self.seg[p][sl] == new[sl]
                st = self.st[p][w]
                if st == 3:
                    nst = 0
                elif st == 1:
                    nst = 0 if same.all() else 1
                elif same.all():
                    nst = 2
                else:
                    nst = 1 if 2 * int((~same).sum()) > same.size else 0
                self.st[p][w] = nst
            self.seg[p] = new
        flat = [x for w in self.st for x in w]
        return [flat.count(v) for v in range(4)]


@pytest.mark.parametrize("kind", list(KINDS))
def test_waves_stop_testing_after_missing_and_resume_when_keys_repeat(torch_cuda, kind):
    """All keys replaced: the waves test, find most of their cuts wrong and
    stop testing (state 1); they stay there while the keys keep changing; the
    first run on repeated keys searches the old cuts again and resumes
    (state 0); the next keeps every cut (state 2).  Every run's results equal
    the oracle's, whichever state the waves are in, and the states are the
    model's."""
    keys = [k for k, _ in base(kind)[1]]
    waves = 2 * len(keys)
    seq = [("base", keys), ("base", keys), ("redraw1", redraw(kind, 1)),
           ("redraw2", redraw(kind, 2)), ("base", keys), ("base", keys), ("base", keys)]
    rig, model, seen = Rig(torch_cuda, kind, keys), Model(kind), []
    for name, k in seq:
        want, wm = oracle(kind, name, k)
        rig.set_keys(k)
        got, mt = rig.run()
        assert mt == wm, name
        assert_bitexact(got, want)
        seen.append(rig.state())
        assert seen[-1] == model.run(k), name
    rig.close()
    assert seen[0] == [waves, 0, 0, 0] and seen[1] == [0, 0, waves, 0]
    # every 64-boundary wave stopped testing and stayed so until the keys repeated
    assert seen[2][1] >= len(keys) and seen[3][1] >= len(keys) and seen[4][1] >= len(keys)
    assert seen[5][1] == 0 and seen[6] == [0, 0, waves, 0]


def test_a_few_missing_cuts_keep_the_wave_testing(torch_cuda):
    """One cut moved in each wave of push 0 (1 of 64, 1 of 6 boundaries): the
    wave searches that run (state 0), keeps testing, and keeps every cut of
    the next run."""
    D, ps = base("f32")
    keys = [k for k, _ in ps]
    moved = [shift_cut(shift_cut(keys[0], D, 1024, 17), D, 1024, 66), keys[1], keys[2]]
    rig = Rig(torch_cuda, "f32", keys)
    rig.run()
    rig.run()
    assert rig.state() == [0, 0, 6, 0]
    rig.set_keys(moved)
    want, wm = oracle("f32", "moved", moved)
    for st in ([2, 0, 4, 0], [0, 0, 6, 0]):
        got, mt = rig.run()
        assert mt == wm
        assert_bitexact(got, want)
        assert rig.state() == st
    rig.close()
