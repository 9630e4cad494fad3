"""GPU: every merge form against the reference's RECORDED fold
(tests/golden/reference_pin/fold_*.npz, written by tools/record_reference.py
from the reference's own match / oldMatch compiled in place), not against the
oracle: serial and parallel, bit for bit.

psg.h promises "the results are bit-identical whichever form runs"; here each
form is forced by its flag (PSG_GROUP32 / PSG_GROUP64 / PSG_NO_INDEX /
PSG_NO_ZERO_COPY among them) and, on the plan path, the kernel that ran is
asserted.  The inputs are rebuilt by tests/pin_cases.py and their SHA-256
checked against the fixture first.

Below them, the device evaluation (psg_auc_*) and the worker's localizer
(psg_mb_uniq / psg_mb_localize) against the recorded AUC, Evaluation and
Localizer of the reference, in the same way.
"""
import numpy as np
import pytest

import pin_cases as P
from test_gpu_parity import kvv, msg, plan_for, to_dev, torch_cuda  # noqa: F401

pytestmark = pytest.mark.gpu

FIXTURES = [("F1", 0), ("F2", 0), ("F2", 1), ("F3", 0)]
_cache = {}


def recorded(name, r):
    """(case, pushes cut to range r, meta, arrays); built once, read only."""
    if (name, r) not in _cache:
        if name not in _cache:
            _cache[name] = P.fold_case(name)
        c = _cache[name]
        meta, fx = P.load_fixture(c.fixture(r))
        assert meta["input_sha256"] == c.digest()
        _cache[(name, r)] = (c, c.sliced(r), meta, fx)
    return _cache[(name, r)]


def assert_fold(got, c, fx, mode):
    assert len(got) == c.m
    for i in range(c.m):
        assert np.array_equal(P.fbits(np.asarray(got[i], c.dtype)), fx["%s%d" % (mode, i)]), (mode, i)


def flag(name):
    from parameter_server_amd import _lib
    v = 0
    for part in name.split("|"):
        v |= 0 if part == "0" else getattr(_lib, part)
    return v


def run_ctx(torch, c, pushes, meta, parallel, flags, flush, pinned):
    v = kvv(c.dtype, parallel, flags)
    if flush:
        v.set_flush_pushes(flush)
    v.setValue(msg(c.D))
    keep = []

    def host(a):
        if not pinned:
            return a
        a = np.ascontiguousarray(a)
        t = torch.empty(a.nbytes, dtype=torch.uint8).pin_memory()
        h = t.numpy().view(a.dtype)
        h[:] = a
        keep.append(t)
        return h
    for k, vals in pushes:
        v.setValue(msg(host(k), [host(np.asarray(x, c.dtype)) for x in vals], t=7,
                       rng=tuple(meta["key_range"])))
    out = v.received(7)
    v.close()
    assert all(list(rng) == meta["positions"] for rng, _ in out)
    return [a for _, a in out]


CTX_FORMS = ["0", "PSG_FORM_PACKED", "PSG_FORM_UNIFORM|PSG_GROUP32", "PSG_FORM_UNIFORM|PSG_GROUP64",
             "PSG_PART_SEARCH", "PSG_PART_STREAM", "PSG_NO_DENSE"]
CTX_VARIANTS = [(f, False) for f in CTX_FORMS] + [("PSG_NO_ZERO_COPY", True), ("PSG_NO_ZERO_COPY", False),
                                                   ("0", True)]  # pinned, flags 0: the zero-copy reads


@pytest.mark.parametrize("form,pinned", CTX_VARIANTS)
@pytest.mark.parametrize("name,r", FIXTURES)
def test_context_forms_against_the_recorded_fold(torch_cuda, name, r, form, pinned):
    c, pushes, meta, fx = recorded(name, r)
    for flush in (None, 7):
        for mode, parallel in (("serial", False), ("parallel", True)):
            got = run_ctx(torch_cuda, c, pushes, meta, parallel, flag(form), flush, pinned)
            assert_fold(got, c, fx, mode)


PLAN_ROWS = [("F1", "PSG_FORM_UNIFORM|PSG_GROUP32", "PSG_KERNEL_TILE", 70),
             ("F1", "PSG_FORM_UNIFORM|PSG_GROUP64", "PSG_KERNEL_TILE64", 70),
             ("F2", "PSG_FORM_UNIFORM|PSG_GROUP64", "PSG_KERNEL_TILE64", 9),
             ("F3", "PSG_FORM_PACKED", "PSG_KERNEL_PACKED", 150),
             ("F2", "PSG_FORM_CURSOR", "PSG_KERNEL_CURSOR", 9),
             ("F3", "PSG_FORM_CURSOR", "PSG_KERNEL_PACKED_CURSOR", 150)]
PLAN_CASES = [row + (extra,) for row in PLAN_ROWS[:4]
              for extra in ("0", "PSG_NO_INDEX", "PSG_PART_SEARCH", "PSG_PART_STREAM")] + \
             [row + ("0",) for row in PLAN_ROWS[4:]]


@pytest.mark.parametrize("name,form,kernel,npush,extra", PLAN_CASES)
def test_plan_forms_against_the_recorded_fold(torch_cuda, name, form, kernel, npush, extra):
    from parameter_server_amd import _lib
    c, pushes, meta, fx = recorded(name, 0)
    assert len(pushes) == npush
    for mode, parallel in (("serial", False), ("parallel", True)):
        plan, keep = plan_for(torch_cuda, [(c.D, pushes)], c.dtype, parallel, flag(form) | flag(extra))
        assert plan.form == getattr(_lib, kernel)
        for _ in range(2):  # a second run lands in the same buffers
            plan.run()
            assert np.array_equal(plan.matched(), fx["matched"])
            assert_fold([o.cpu().numpy()[: c.D.size] for o in keep[3]], c, fx, mode)
        plan.close()


@pytest.mark.parametrize("name,r", FIXTURES)
def test_gather_and_slice_against_the_recorded(torch_cuda, name, r):
    """psg_gather / psg_gather_dev on the recorded request (absent and
    repeated keys) and psg_slice_dev on the recorded cut positions."""
    torch = torch_cuda
    from parameter_server_amd import _lib
    L = _lib.lib()
    c, _, meta, fx = recorded(name, r)
    v = kvv(c.dtype)
    v.setValue(msg(c.D))
    v.set_value_array(0, c.W)
    req = msg(c.R)
    assert v.getValue(req) == meta["gather_matched"]
    assert np.array_equal(P.fbits(req.value[0]), fx["gather"])
    v.close()
    dD, dW, dR = to_dev(torch, c.D), to_dev(torch, c.W), to_dev(torch, c.R)
    dout = torch.empty(c.R.size, dtype=dW.dtype, device="cuda")
    dm = torch.zeros(1, dtype=torch.int64, device="cuda")
    _lib.check(L.psg_gather_dev(_lib.PSG_F32 if c.dtype == np.float32 else _lib.PSG_F64,
                                dD.data_ptr(), c.D.size, dW.data_ptr(), dR.data_ptr(), c.R.size,
                                dout.data_ptr(), dm.data_ptr(), None))
    torch.cuda.synchronize()
    assert int(dm.item()) == meta["gather_matched"]
    assert np.array_equal(P.fbits(dout.cpu().numpy()), fx["gather"])
    sep = fx["slice_sep"]
    dsep = to_dev(torch, sep)
    dpos = torch.empty(sep.size, dtype=torch.int64, device="cuda")
    kb, ke = meta["key_range"]
    _lib.check(L.psg_slice_dev(dD.data_ptr(), c.D.size, kb, ke, dsep.data_ptr(), sep.size,
                               dpos.data_ptr(), None))
    torch.cuda.synchronize()
    pos = dpos.cpu().numpy()
    ok = fx["slice_valid"] == 1
    assert ok.any()
    assert np.array_equal(pos[:-1][ok], fx["slice_begin"][ok])
    assert np.array_equal(pos[1:][ok], fx["slice_end"][ok])
    # an invalid piece (outside the key range) is empty
    assert np.array_equal(pos[:-1][~ok], pos[1:][~ok])


# ------------------------------------------------- evaluation and localizer
# psg_auc_* / psg_auc_exact_dev (psg_auc.hip) and psg_mb_uniq / psg_mb_localize
# (psg_worker.hip over psg_sort.h) against what the reference's own AUC,
# Evaluation<double>::auc and Localizer returned (auc.npz, auc_merge.npz,
# exact_auc.npz, localizer.npz): only the fixtures and tests/pin_cases.py are
# read here, never the reference tree or oracle/_ref.
AUC_PARTS = ("tp_key", "tp_count", "fp_key", "fp_count")
ZERO_ONLY = {"zero_only_negatives", "zero_only_both"}  # see tests/test_reference_pin.py


def dev(torch, a):
    """A host array as a device tensor (its bytes, whatever the dtype)."""
    a = np.ascontiguousarray(a)
    t = torch.from_numpy(a.view(np.uint8).reshape(-1).copy()).to("cuda:0")
    if t.numel() == 0:
        t = torch.zeros(8, dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    return t


def fb(v):
    """A double's bits as the fixtures spell them; every NaN is one value."""
    return "nan" if np.isnan(v) else "%016x" % int(P.fbits(np.array([v], np.float64))[0])


def recorded_double(hexbits):
    return fb(float(np.array([int(hexbits, 16)], np.uint64).view(np.float64)[0]))


@pytest.fixture(scope="module")
def f64_ctx(torch_cuda):
    import ctypes as C
    from parameter_server_amd import _lib
    L = _lib.lib()
    h = C.c_void_p()
    _lib.check(L.psg_create(0, _lib.PSG_F64, 0, C.byref(h)))
    yield h
    L.psg_destroy(h)


@pytest.fixture(scope="module")
def auc(f64_ctx):
    """One handle for all the cases: clear and set_goodness between them."""
    from parameter_server_amd.auc import AUC
    a = AUC(f64_ctx, 1000)
    yield a
    a.close()


@pytest.fixture(scope="module")
def mb(f64_ctx):
    from parameter_server_amd.worker import Minibatch
    m = Minibatch(f64_ctx)
    yield m
    m.close()


def fresh(auc, goodness):
    auc.clear()
    auc.setGoodness(goodness)
    return auc


def auc_case(name):
    if "auc" not in _cache:
        _cache["auc"] = {c.name: c for c in P.auc_cases()}
    return _cache["auc"][name]


def same_aucdata(fx, sha, name, data):
    return all(P.same_output(fx, sha, "%s.%s" % (name, part), a) for part, a in zip(AUC_PARTS, data))


def test_the_sort_tile_is_the_recorded_one():
    from parameter_server_amd.worker import sort_tile
    for name in ("auc", "exact_auc", "localizer"):
        assert P.load_fixture(name)[0]["tile"] == sort_tile() == P.PIN_TILE


@pytest.mark.parametrize("name", [c.name for c in P.auc_cases()])
def test_auc_add_dev_against_the_recorded(torch_cuda, auc, name):
    """One add over the whole case, and two adds split at T - 1 | rest (an
    empty rest where the case is shorter): the reference's AUCData both
    times.  The undefined_* cases hold what psg.h says of NaN and of products
    of magnitude >= 2^63."""
    c = auc_case(name)
    meta, fx = P.load_fixture("auc")
    assert meta["cases"][name]["input_sha256"] == c.digest()
    ty, tp = dev(torch_cuda, c.y), dev(torch_cuda, c.p)
    cut = min(meta["tile"] - 1, c.y.size)
    for pieces in ([(0, c.y.size)], [(0, cut), (cut, c.y.size)]):
        fresh(auc, c.g)
        for a, b in pieces:
            auc.add_dev(ty.data_ptr() + 8 * a, tp.data_ptr() + 8 * a, b - a)
        data = auc.data()  # waits
        assert (data[0].size, data[2].size) == (meta["cases"][name]["ntp"], meta["cases"][name]["nfp"])
        assert same_aucdata(fx, meta["sha256"], name, data), pieces


@pytest.mark.parametrize("name", sorted(P.auc_merge_sequences()))
def test_auc_merge_against_the_recorded(auc, name):
    """psg_auc_merge of each sequence, then the histogram, accuracy at the
    three thresholds and evaluate() as written (PSG_AUC_AS_WRITTEN; PSG_AUC_BY_KEY
    is a defined deviation with no reference and stays on the restatements)."""
    g, datas = P.auc_merge_sequences()[name]
    meta, fx = P.load_fixture("auc_merge")
    info = meta["sequences"][name]
    assert info["input_sha256"] == P.auc_sequence_digest(g, datas)
    maps = tuple(fx["%s.%s" % (name, part)] for part in AUC_PARTS)
    assert same_aucdata(fx, meta["sha256"], name, maps)
    fresh(auc, g)
    for d in datas:
        auc.merge(*d)
    got = auc.data()
    # defined deviation: the zero-count entries of the reference's maps are dropped
    want = P.auc_without_zeros(maps)
    assert all(a.dtype == b.dtype and np.array_equal(a, b) for a, b in zip(got, want))
    assert (info["zero_count_entries"] > 0) == name.startswith("zero_")
    for th, bits in zip(P.AUC_THRESHOLDS, info["accuracy_bits"]):
        assert fb(auc.accuracy(th)) == recorded_double(bits), th
    ev = fb(auc.evaluate(as_written=True))
    if name in ZERO_ONLY:
        # ... which shows where a side holds zero counts only: the reference's
        # map is not empty() and its evaluate is 0 / 0; the product's is .5
        assert recorded_double(info["evaluate_bits"]) == "nan" and ev == fb(0.5)
    else:
        assert ev == recorded_double(info["evaluate_bits"])


@pytest.mark.parametrize("name", [c.name for c in P.exact_auc_cases()])
def test_exact_auc_dev_against_the_recorded(torch_cuda, f64_ctx, name):
    """Tie-free inputs only (all predictions distinct, or ties within one
    class): ties across the classes are a defined deviation and not pinned."""
    from parameter_server_amd.auc import exact_auc_dev
    cases = P.exact_auc_cases()
    i = [c.name for c in cases].index(name)
    c = cases[i]
    meta, fx = P.load_fixture("exact_auc")
    assert meta["cases"][name]["input_sha256"] == c.digest()
    ty, tp = dev(torch_cuda, c.y), dev(torch_cuda, c.p)
    got = exact_auc_dev(f64_ctx, ty.data_ptr(), tp.data_ptr(), c.y.size)
    assert fb(got) == recorded_double("%016x" % int(fx["bits"][i]))


@pytest.mark.parametrize("name", P.LOC_NAMES)
def test_localizer_against_the_recorded(torch_cuda, mb, name):
    """psg_mb_load -> psg_mb_uniq -> psg_mb_localize per dictionary.  The
    order of positions inside a run of equal ids (PSG_MB_SORTED_POS) is not
    pinned: the reference's sort leaves it open, the product defines it as
    stable (tests/test_worker_gpu.py)."""
    if name not in _cache:
        _cache[name] = P.loc_case(name)
    c = _cache[name]
    meta, fx = P.load_fixture("localizer")
    info, sha = meta["cases"][name], meta["sha256"]
    assert info["input_sha256"] == c.digest()
    mb.load(c.offset, c.index, c.value, np.ones(c.offset.size - 1))
    assert mb.uniq() == info["n_uniq"]
    assert P.same_output(fx, sha, name + ".uniq_idx", mb.read("uniq_key"))
    assert P.same_output(fx, sha, name + ".idx_frq", mb.read("key_cnt"))
    for dname in sorted(c.dicts):
        if dname == "empty":  # the reference returns null; the product's Z is its own deviation
            assert info["matched"][dname] is None
            continue
        d = dev(torch_cuda, c.dicts[dname])
        mb.localize(d.data_ptr(), c.dicts[dname].size)
        got = {"remapped_idx": mb.read("remapped"), "new_offset": mb.read("new_offset"),
               "new_index": mb.read("new_index"), "new_value": P.fbits(mb.read("new_value"))}
        assert got["new_index"].size == info["matched"][dname], dname
        for k, a in got.items():
            assert P.same_output(fx, sha, "%s.%s.%s" % (name, dname, k), a), (dname, k)
