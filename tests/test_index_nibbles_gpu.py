"""GPU: a plan's resident bucket index, 4 bits per bucket (psg_device.h),
through every kernel that decodes it -- bit for bit against the oracle, sums
and matched counts (a wrong bucket start shows up as unmatched keys).

Jobs are 3 tiles + 17 slots with pushes of about 300 keys; the middle tile of
the crafted jobs (index_inputs.crowded_D) holds one bucket of c + 1 keys, so
its table is stored for c <= 13 and marked "not stored" for c >= 15."""
import numpy as np
import pytest

import index_inputs as I
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


def bits(a):
    a = np.asarray(a)
    return a.view(np.uint32 if a.dtype == np.float32 else np.uint64)


def assert_bitexact(got, want):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape
    assert np.array_equal(np.isnan(got), np.isnan(want))
    assert np.array_equal(bits(got), bits(want))


def to_dev(torch, a, shift=0):
    """On the device; `shift`: as a view `shift` elements into its buffer."""
    a = np.ascontiguousarray(a)
    if a.dtype == np.uint64:
        a = a.view(np.int64)
    if shift:
        a = np.concatenate([np.zeros(shift, a.dtype), a])
    t = torch.from_numpy(a).cuda()
    return t[shift:] if shift else t


def plan_for(torch, cases, dtype=np.float32, parallel=False, flags=0, dshift=0):
    from parameter_server_amd.kv_vector import MergePlan
    from parameter_server_amd._lib import PSG_F32, PSG_F64
    keep, jobs = [], []
    m = len(cases[0][1][0][1])
    tdt = torch.float32 if dtype == np.float32 else torch.float64
    for D, pushes in cases:
        dD = to_dev(torch, D, dshift)
        pk = [to_dev(torch, k) for k, _ in pushes]
        pv = [[to_dev(torch, np.asarray(x, dtype)) for x in vs] for _, vs in pushes]
        out = [torch.full((max(1, D.size),), float("nan"), dtype=tdt, device="cuda")
               for _ in range(m)]
        keep += [dD, pk, pv, out]
        jobs.append({"keys": dD.data_ptr(), "nslots": D.size,
                     "push_keys": [t.data_ptr() for t in pk],
                     "push_vals": [[t.data_ptr() for t in vs] for vs in pv],
                     "push_n": [k.size for k, _ in pushes],
                     "out": [o.data_ptr() for o in out]})
    plan = MergePlan(0, PSG_F32 if dtype == np.float32 else PSG_F64, m, jobs, parallel, flags)
    return plan, keep


_want = {}


def oracle(key, D, pushes, parallel, m, dtype):
    """O.aggregate once per named input (shared, left unchanged)."""
    k = (key, parallel, m, np.dtype(dtype).name)
    if k not in _want:
        _, _, _, want, wm = O.aggregate(D, *ALL, pushes, parallel, m, dtype)
        _want[k] = ([np.array(w) for w in want], [int(x) for x in wm])
    return _want[k]


def check(torch, named_cases, dtype=np.float32, parallel=False, flags=0, dshift=0, reps=1,
          want_form=None, tile=1024):
    """Runs a plan over [(name, D, pushes)]; sums and matched counts against
    the oracle; returns (index_bytes, marked_tiles)."""
    cases = [(D, ps) for _, D, ps in named_cases]
    m = len(cases[0][1][0][1])
    plan, keep = plan_for(torch, cases, dtype, parallel, flags, dshift)
    if want_form is not None:
        assert plan.form == want_form
    for _ in range(reps):
        plan.run()
        mt = plan.matched().tolist()
        want_mt = []
        for j, (name, D, ps) in enumerate(named_cases):
            want, wm = oracle(name, D, ps, parallel, m, dtype)
            want_mt += wm
            for i in range(m):
                assert_bitexact(keep[4 * j + 3][i].cpu().numpy()[: D.size], want[i])
        assert mt == want_mt
    info = (plan.index_bytes, plan.marked_tiles)
    if plan.index_bytes:
        ntiles = sum((D.size + tile - 1) // tile for D, _ in cases)
        assert plan.index_bytes == ntiles * tile // 2
    plan.close()
    return info


def uniform_case(name, nslots, npush, seed, dtype=np.float32, m=1):
    rng = np.random.default_rng(seed)
    D = np.unique(rng.integers(1, 1 << 60, 2 * nslots + 8, dtype=np.uint64))[:nslots]
    assert D.size == nslots
    return (name, D, I.pushes_over(D, npush, 300, seed + 1, dtype, m))


def crowded_case(tile, c, npush=8, dtype=np.float32, m=1, seed=0):
    D, x0 = I.crowded_D(tile, c, seed)
    name = "crowd-%d-%d-%d-%d-%s-%d" % (tile, c, npush, seed, np.dtype(dtype).name, m)
    return (name, D, I.pushes_over(D, npush, 300, 50 + c, dtype, m, hot=(x0, c)))


# ------------------------------------------------------- sizes and alignment
def test_small_and_edge_sizes(torch_cuda):
    """Jobs of 1, 1023, 1024, 1025 slots and one of 3 tiles + 17 in one plan
    (1024-slot tiles: a partial tile takes the path without LDS-DMA), and
    the 64-push form (33 pushes, 2048-slot tiles) at 2047, 2048, 2049."""
    from parameter_server_amd._lib import PSG_KERNEL_TILE, PSG_KERNEL_TILE64, PSG_FORM_UNIFORM
    cases = [uniform_case("u32-%d" % n, n, 8, 100 + n) for n in (1, 1023, 1024, 1025, 3 * 1024 + 17)]
    ib, mk = check(torch_cuda, cases, flags=PSG_FORM_UNIFORM, want_form=PSG_KERNEL_TILE, reps=2)
    assert ib == (1 + 1 + 1 + 2 + 4) * 512 and mk == 0
    cases = [uniform_case("u64-%d" % n, n, 33, 200 + n) for n in (2047, 2048, 2049)]
    ib, mk = check(torch_cuda, cases, flags=PSG_FORM_UNIFORM, want_form=PSG_KERNEL_TILE64,
                   tile=2048)
    assert ib == (1 + 1 + 2) * 1024 and mk == 0


def test_server_keys_at_odd_offset(torch_cuda):
    """D as a view at an odd 8-B offset: every tile takes the path through
    registers; the index is decoded the same way (a marked tile included)."""
    from parameter_server_amd._lib import PSG_FORM_UNIFORM
    cases = [uniform_case("u32-%d" % n, n, 8, 100 + n) for n in (1025, 3 * 1024 + 17)]
    cases.append(crowded_case(1024, 16))
    ib, mk = check(torch_cuda, cases, flags=PSG_FORM_UNIFORM, dshift=1)
    assert mk == 1


# ------------------------------------------------------------- crowded tile
@pytest.mark.parametrize("c", [13, 14, 15, 16, 17, 18, 1000])
def test_crowded_middle_tile(torch_cuda, c):
    """One bucket of c + 1 keys in the middle tile, uniform neighbours: the
    tile is marked from 15 keys on and then builds its own table; both
    neighbours (checked with the whole job) decode theirs."""
    from parameter_server_amd._lib import PSG_KERNEL_TILE, PSG_FORM_UNIFORM
    ib, mk = check(torch_cuda, [crowded_case(1024, c)], flags=PSG_FORM_UNIFORM,
                   want_form=PSG_KERNEL_TILE, reps=2)
    assert ib == 4 * 512
    if c <= 13:
        assert mk == 0
    if c >= 15:
        assert mk == 1


# ---------------------------------------------------------- forms and modes
def _form(name):
    from parameter_server_amd import _lib as L
    return {
        "tile64": (L.PSG_FORM_UNIFORM | L.PSG_GROUP64, L.PSG_KERNEL_TILE64, 2048),
        "packed": (L.PSG_FORM_PACKED, L.PSG_KERNEL_PACKED, 2048),
        "cursor": (L.PSG_FORM_UNIFORM | L.PSG_FORM_CURSOR, L.PSG_KERNEL_CURSOR, 1024),
        "packed_cursor": (L.PSG_FORM_PACKED | L.PSG_FORM_CURSOR, L.PSG_KERNEL_PACKED_CURSOR, 2048),
    }[name]


@pytest.mark.parametrize("c", [13, 16, 1000])
@pytest.mark.parametrize("form", ["tile64", "packed", "cursor", "packed_cursor"])
def test_forms_over_crowded_tile(torch_cuda, form, c):
    """The 64-push form, the packed form (many short pieces: 40 pushes of
    about 60 keys more) and both cursor forms over the crafted job at their
    own tile size, stored (c = 13) and marked (c = 16, 1000)."""
    flags, kernel, tile = _form(form)
    case = crowded_case(tile, c)
    if form in ("packed", "packed_cursor"):
        name, D, ps = case
        ps = ps + I.pushes_over(D, 40, 60, 7, hot=(I.crowded_D(tile, c)[1], c), nhot=6)
        case = (name + "+short", D, ps)
    ib, mk = check(torch_cuda, [case, uniform_case("u-%s" % form, 2 * tile + 5, 8, 31)],
                   flags=flags, want_form=kernel, tile=tile, reps=2)
    assert mk == (0 if c <= 13 else 1)


@pytest.mark.parametrize("parallel", [False, True])
@pytest.mark.parametrize("dtype,m", [(np.float32, 1), (np.float32, 2), (np.float64, 1),
                                     (np.float64, 2)])
def test_value_types_and_match_modes(torch_cuda, dtype, m, parallel):
    from parameter_server_amd._lib import PSG_FORM_UNIFORM
    cases = [crowded_case(1024, 16, dtype=dtype, m=m), crowded_case(1024, 13, dtype=dtype, m=m)]
    ib, mk = check(torch_cuda, cases, dtype=dtype, parallel=parallel, flags=PSG_FORM_UNIFORM)
    assert mk == 1


@pytest.mark.parametrize("group", [32, 64])
def test_job_continued_over_push_groups(torch_cuda, group):
    """33 pushes in groups of 32 (65 in groups of 64): the second group folds
    into the first one's sums, searching the same decoded (or rebuilt) table."""
    from parameter_server_amd import _lib as L
    flags = L.PSG_FORM_UNIFORM | (L.PSG_GROUP32 if group == 32 else L.PSG_GROUP64)
    tile = 1024 if group == 32 else 2048
    cases = [crowded_case(tile, 16, npush=group + 1), crowded_case(tile, 13, npush=group + 1)]
    ib, mk = check(torch_cuda, cases, flags=flags, tile=tile,
                   want_form=L.PSG_KERNEL_TILE if group == 32 else L.PSG_KERNEL_TILE64)
    assert mk == 1


def test_no_index_agrees(torch_cuda):
    from parameter_server_amd._lib import PSG_FORM_UNIFORM, PSG_NO_INDEX
    cases = [crowded_case(1024, 16), crowded_case(1024, 1000), uniform_case("u32-3089", 3089, 8, 3189)]
    assert check(torch_cuda, cases, flags=PSG_FORM_UNIFORM)[1] == 2
    assert check(torch_cuda, cases, flags=PSG_FORM_UNIFORM | PSG_NO_INDEX) == (0, 0)


def test_unmatched_keys_are_reported(torch_cuda):
    """A key absent from D (next to the crowded run) is counted as the oracle
    counts it; a push with two blocks swapped reports matched < n while the
    sorted pushes stay exact."""
    from parameter_server_amd._lib import PSG_FORM_UNIFORM
    torch = torch_cuda
    for c in (13, 16):
        name, D, ps = crowded_case(1024, c)
        x0 = I.crowded_D(1024, c)[1]
        absent = np.array([x0 + c, int(D[5]) + 1], np.uint64)  # just past the run; tile 0
        assert not np.isin(absent, D).any()
        k = np.unique(np.concatenate([ps[2][0], absent]))
        ps2 = list(ps)
        ps2[2] = (k, [np.ones(k.size, np.float32)])
        check(torch, [(name + "+absent", D, ps2)], flags=PSG_FORM_UNIFORM)
        bad = [(k.copy(), vs) for k, vs in ps]
        kb = bad[4][0]
        n = kb.size
        a = kb[20:60].copy()
        kb[20:60] = kb[n - 60:n - 20]
        kb[n - 60:n - 20] = a
        plan, keep = plan_for(torch, [(D, bad)], flags=PSG_FORM_UNIFORM)
        plan.run()
        mt = plan.matched().tolist()
        assert mt[4] < n
        assert [mt[i] for i in range(8) if i != 4] == [ps[i][0].size for i in range(8) if i != 4]
        plan.close()
