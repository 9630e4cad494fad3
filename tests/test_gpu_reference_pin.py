"""GPU: every merge form against the reference's RECORDED fold
(tests/golden/reference_pin/fold_*.npz, written by tools/record_reference.py
from the reference's own match / oldMatch compiled in place), not against the
oracle: serial and parallel, bit for bit.

psg.h promises "the results are bit-identical whichever form runs"; here each
form is forced by its flag (PSG_GROUP32 / PSG_GROUP64 / PSG_NO_INDEX /
PSG_NO_ZERO_COPY among them) and, on the plan path, the kernel that ran is
asserted.  The inputs are rebuilt by tests/pin_cases.py and their SHA-256
checked against the fixture first.
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
