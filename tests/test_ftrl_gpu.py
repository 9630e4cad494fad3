"""GPU: the device-resident FTRL model (psg_ftrl_*, parameter_server_amd/
csrc/psg_ftrl.hip) against the CPU restatements of the reference's
FTRLModel::setValue (tests/ftrl_ref.py), bit for bit."""
import ctypes as C
import math

import numpy as np
import pytest

import ftrl_ref as R
from parameter_server_amd import _lib
from parameter_server_amd.ftrl import FTRLModel
from parameter_server_amd.kv_vector import Message

pytestmark = pytest.mark.gpu

U64 = (1 << 64) - 1


def ptr(a):
    return a.ctypes.data


def new_model(hint=0, **param):
    p = dict(R.PARITY_PARAM, **param)
    m = FTRLModel(0, capacity_hint=hint)
    m.setLearningRate(p["alpha"], p["beta"])
    m.setPenalty(p["lambda1"], p["lambda2"])
    m._model()
    return m


def push(m, keys, pos, neg, grad):
    """psg_ftrl_push with the status returned, not raised."""
    k = np.ascontiguousarray(keys, np.uint64)
    a, b = np.ascontiguousarray(pos, np.uint32), np.ascontiguousarray(neg, np.uint32)
    g = np.ascontiguousarray(grad, np.float64)
    return m._L.psg_ftrl_push(m._h, ptr(k), k.size, ptr(a), ptr(b), ptr(g))


def status(m):
    e, z = C.c_size_t(), C.c_size_t()
    n1, n2 = C.c_double(), C.c_double()
    rc = m._L.psg_ftrl_status(m._h, C.byref(e), C.byref(z), C.byref(n1), C.byref(n2))
    return rc, e.value, z.value, n1.value, n2.value


def assert_state(m, ref, keys):
    got, want = m.lookup(keys), ref.lookup(keys)
    for name, g, w in zip(("pos", "neg", "w", "z", "found"), got, want):
        assert np.array_equal(g.view(np.uint8), w.view(np.uint8)), name


@pytest.fixture(scope="module")
def parity():
    """The parity case and its restatement after each message (read only)."""
    uni, msgs = R.parity_case(seed=1)
    ref = R.VectorFTRL(**R.PARITY_PARAM)
    after = []
    for msg in msgs:
        ref.push(*msg)
        after.append((ref.lookup(uni), ref.entries, ref.nnz))
    for kind in R.TRANSITIONS:
        assert ref.transitions[kind] >= 1
    return uni, msgs, ref, after


def test_parity_with_rehashes(parity):
    uni, msgs, ref, after = parity
    absent = R.absent_keys(uni, 500)
    m = new_model(hint=64)   # 1,200-key messages: the table is rehashed as they come
    for msg, (want, entries, nnz) in zip(msgs, after):
        assert push(m, *msg) == _lib.PSG_OK
        got = m.lookup(uni)
        for name, g, w in zip(("pos", "neg", "w", "z", "found"), got, want):
            assert np.array_equal(g.view(np.uint8), w.view(np.uint8)), name
        rc, e, z, _, _ = status(m)
        assert (rc, e, z) == (_lib.PSG_OK, entries, nnz)
    req = Message(key=np.random.default_rng(3).permutation(np.concatenate([uni, absent, uni[:99]])))
    m.getValue(req)
    want = R.pull(ref, req.key)
    assert np.array_equal(R.bits(req.value[0]), R.bits(want))
    neg_zero = R.bits(np.array([-0.0]))[0]
    assert int(np.count_nonzero(R.bits(want) == neg_zero)) >= 1      # thresholded: -0.0
    assert not R.bits(req.value[0])[np.isin(req.key, absent)].any()  # absent: +0.0
    m.close()


def test_every_key_value_is_legal():
    i = np.arange(64, dtype=np.uint64)
    sets = [i, np.uint64(U64 - 63) + i, i << np.uint64(40), i << np.uint64(58)]
    m, ref = new_model(hint=16), R.VectorFTRL(**R.PARITY_PARAM)
    rng = np.random.default_rng(5)
    for _ in range(2):
        for k in sets:
            k = np.unique(k)
            msg = (k, rng.integers(0, 6, k.size).astype(np.uint32),
                   rng.integers(0, 6, k.size).astype(np.uint32), 2.0 * rng.standard_normal(k.size))
            assert push(m, *msg) == _lib.PSG_OK
            ref.push(*msg)
    allk = np.unique(np.concatenate(sets))
    assert allk.size == 4 * 64 - 2 and allk[0] == 0 and allk[-1] == U64  # three sets hold key 0
    assert_state(m, ref, allk)
    assert m.lookup(allk)[4].all()
    rc, e, z, _, _ = status(m)
    assert (rc, e, z) == (_lib.PSG_OK, ref.entries, ref.nnz)
    m.close()


def test_special_values():
    denormal = 5e-324
    grads = [math.nan, math.inf, -math.inf, -0.0, denormal, 0.75, -3.0, 3.0, 1.0]
    n = len(grads)
    keys = np.arange(10, 10 + n + 1, dtype=np.uint64)
    pos = np.array([1, 2, 3, 0, 0, 0, 0, 4, 5, 0xFFFFFFFF], np.uint32)
    neg = np.array([1, 0, 2, 0, 0, 0, 0, 4, 0, 0xFFFFFFFF], np.uint32)
    first = (keys, pos, neg, np.array(grads + [0.5]))
    again = (keys[-1:], pos[-1:], neg[-1:], np.array([1.5]))
    m = new_model(hint=8)
    s, v = R.ScalarFTRL(**R.PARITY_PARAM), R.VectorFTRL(**R.PARITY_PARAM)
    for msg in (first, again, again):
        assert push(m, *msg) == _lib.PSG_OK
        s.push(*msg)
        v.push(*msg)
        assert_state(m, s, keys)
        assert_state(m, v, keys)
    p, ng, w, z, found = m.lookup(keys)
    assert int(p[-1]) == 3 * 0xFFFFFFFF > 1 << 32 and int(ng[-1]) == 3 * 0xFFFFFFFF
    assert math.isnan(z[0]) and R.bits(w[:1])[0] == R.bits(np.array([-0.0]))[0]
    rc, e, nz, _, _ = status(m)
    assert (rc, e, nz) == (_lib.PSG_OK, s.entries, s.nnz)
    m.close()


def test_unsorted_message_is_rejected_whole(parity):
    uni, msgs, _, _ = parity
    m, ref = new_model(hint=64), R.VectorFTRL(**R.PARITY_PARAM)
    assert push(m, *msgs[0]) == _lib.PSG_OK
    ref.push(*msgs[0])
    k, pos, neg, g = msgs[1]
    repeated = k.copy()
    repeated[700] = repeated[699]
    swapped = k.copy()
    swapped[[300, 301]] = swapped[[301, 300]]
    for bad in (repeated, swapped):
        before = m.lookup(uni)
        assert push(m, bad, pos, neg, g) == _lib.PSG_OK      # asynchronous: reported later
        after = m.lookup(uni)
        for b, a in zip(before, after):
            assert np.array_equal(b.view(np.uint8), a.view(np.uint8))
        assert status(m)[0] == _lib.PSG_ERR_UNSORTED
        rc, e, z, _, _ = status(m)
        assert (rc, e, z) == (_lib.PSG_OK, ref.entries, ref.nnz)
    assert push(m, *msgs[1]) == _lib.PSG_OK
    ref.push(*msgs[1])
    assert_state(m, ref, uni)
    assert status(m)[:3] == (_lib.PSG_OK, ref.entries, ref.nnz)
    m.close()


def test_shapes_at_the_seams():
    rng = np.random.default_rng(11)
    pool = np.unique(rng.integers(0, 1 << 64, size=204_000, dtype=np.uint64))
    small, fresh = np.sort(rng.permutation(pool[:3000])), pool[3000:203_000]
    assert fresh.size == 200_000
    m, ref = new_model(hint=64), R.VectorFTRL(**R.PARITY_PARAM)

    def message(k):
        return (k, rng.integers(0, 6, k.size).astype(np.uint32),
                rng.integers(0, 6, k.size).astype(np.uint32), 2.0 * rng.standard_normal(k.size))

    for n in (0, 1, 63, 64, 65, 255, 256, 257, 1023, 1025):   # wave, workgroup and grid seams
        msg = message(np.sort(rng.choice(small, size=n, replace=False)))
        assert push(m, *msg) == _lib.PSG_OK
        ref.push(*msg)
    assert_state(m, ref, small)
    m.reserve(ref.entries + fresh.size)
    msg = message(fresh)
    assert push(m, *msg) == _lib.PSG_OK
    ref.push(*msg)
    allk = np.concatenate([small, fresh])
    assert_state(m, ref, allk)
    rc, e, z, _, _ = status(m)
    assert (rc, e, z) == (_lib.PSG_OK, ref.entries, ref.nnz)
    m.close()


def test_messages_apply_in_call_order():
    rng = np.random.default_rng(13)
    k = np.unique(rng.integers(0, 1 << 64, size=1000, dtype=np.uint64))
    a = (k, rng.integers(0, 6, k.size).astype(np.uint32), rng.integers(0, 6, k.size).astype(np.uint32),
         2.0 * rng.standard_normal(k.size))
    b = (k, rng.integers(0, 6, k.size).astype(np.uint32), rng.integers(0, 6, k.size).astype(np.uint32),
         2.0 * rng.standard_normal(k.size))
    got = []
    for order in ((a, b), (b, a)):
        m, ref = new_model(), R.VectorFTRL(**R.PARITY_PARAM)
        for msg in order:
            assert push(m, *msg) == _lib.PSG_OK
            ref.push(*msg)
        assert_state(m, ref, k)
        got.append(m.lookup(k))
        m.close()
    assert not np.array_equal(R.bits(got[0][3]), R.bits(got[1][3]))   # z depends on the order
    assert np.array_equal(got[0][0], got[1][0])                       # the counts do not


def test_device_forms_agree_with_host_forms(parity):
    import torch
    uni, msgs, ref, after = parity
    dev = torch.device("cuda:0")
    stream = torch.cuda.current_stream().cuda_stream

    def dt(a):
        a = np.ascontiguousarray(a)
        view = {8: np.int64, 4: np.int32}[a.dtype.itemsize] if a.dtype.kind == "u" else a.dtype
        return torch.from_numpy(a.view(view)).to(dev)

    m = new_model(hint=64)
    for k, pos, neg, g in msgs:
        tk, tp, tn, tg = dt(k), dt(pos), dt(neg), dt(g)
        torch.cuda.synchronize()
        _lib.check(m._L.psg_ftrl_push_dev(m._h, tk.data_ptr(), k.size, tp.data_ptr(),
                                          tn.data_ptr(), tg.data_ptr(), stream))
        torch.cuda.synchronize()
    want, entries, nnz = after[-1]
    got = m.lookup(uni)
    for g, w in zip(got, want):
        assert np.array_equal(g.view(np.uint8), w.view(np.uint8))
    req = np.concatenate([uni[::-1], R.absent_keys(uni, 500)])
    tk = dt(req)
    out = torch.full((req.size,), 7.0, dtype=torch.float64, device=dev)
    torch.cuda.synchronize()
    _lib.check(m._L.psg_ftrl_pull_dev(m._h, tk.data_ptr(), req.size, out.data_ptr(), stream))
    torch.cuda.synchronize()
    host = Message(key=req)
    m.getValue(host)
    assert np.array_equal(R.bits(out.cpu().numpy()), R.bits(host.value[0]))
    assert np.array_equal(R.bits(host.value[0]), R.bits(R.pull(ref, req)))
    assert status(m)[:3] == (_lib.PSG_OK, entries, nnz)
    m.close()


def test_status_and_dump(parity, tmp_path):
    uni, msgs, ref, after = parity
    m = new_model(hint=64)
    for msg in msgs:
        assert push(m, *msg) == _lib.PSG_OK
    rc, entries, nnz, norm1, norm2 = status(m)
    assert (rc, entries, nnz) == (_lib.PSG_OK, ref.entries, ref.nnz)
    # any order of summation of n terms is within n * 2^-53 * sum |x_i| of the exact sum
    w = ref.lookup(uni)[2]
    for got, terms in ((norm1, np.abs(w)), (norm2, w * w)):
        exact = math.fsum(terms.tolist())
        bound = entries * 2.0 ** -53 * math.fsum(np.abs(terms).tolist())
        print("norm: got %r exact %r |diff| %.3g bound %.3g" % (got, exact, abs(got - exact), bound))
        assert abs(got - exact) <= bound
    assert m.objv() == norm1 * 1.0 + .5 * 0.1 * math.sqrt(norm2)
    # export: the nonzero set, bit for bit
    keys, wx = m.export()
    wk, ww = R.nonzero(ref, uni)
    assert np.array_equal(keys, wk) and np.array_equal(R.bits(wx), R.bits(ww))
    assert keys.size == nnz
    path = tmp_path / "model.txt"
    m.writeToFile(str(path))
    assert path.read_text() == R.dump_text(ref, uni)
    # too small a cap: PSG_ERR_SIZE and the needed count
    n = C.c_size_t()
    kbuf, wbuf = np.zeros(nnz, np.uint64), np.zeros(nnz, np.float64)
    assert m._L.psg_ftrl_export(m._h, ptr(kbuf), ptr(wbuf), nnz - 1, C.byref(n)) == _lib.PSG_ERR_SIZE
    assert n.value == nnz and not kbuf.any()
    assert m._L.psg_ftrl_export(m._h, ptr(kbuf), ptr(wbuf), nnz, C.byref(n)) == _lib.PSG_OK
    assert n.value == nnz and np.array_equal(np.sort(kbuf), wk)
    m.close()


def test_arguments():
    L = _lib.lib()
    p = _lib.FtrlParam(1.0, 1.0, 1.0, 0.1)
    k = np.arange(1, 5, dtype=np.uint64)
    a = np.ones(4, np.uint32)
    g = np.ones(4, np.float64)
    out = np.zeros(4, np.float64)
    n = C.c_size_t()
    # an F32 context has no FTRL model, and stays usable
    h32 = C.c_void_p()
    _lib.check(L.psg_create(0, _lib.PSG_F32, 0, C.byref(h32)))
    assert L.psg_ftrl_init(h32, C.byref(p), 0) == _lib.PSG_ERR_ARG
    assert b"PSG_F64" in L.psg_last_error()
    assert L.psg_ftrl_push(h32, ptr(k), 4, ptr(a), ptr(a), ptr(g)) == _lib.PSG_ERR_ARG
    _lib.check(L.psg_key_union(h32, 0, ptr(k), 4))
    _lib.check(L.psg_key_size(h32, 0, C.byref(n)))
    assert n.value == 4
    L.psg_destroy(h32)
    # calls before psg_ftrl_init
    h = C.c_void_p()
    _lib.check(L.psg_create(0, _lib.PSG_F64, 0, C.byref(h)))
    assert L.psg_ftrl_push(h, ptr(k), 4, ptr(a), ptr(a), ptr(g)) == _lib.PSG_ERR_ARG
    assert L.psg_ftrl_pull(h, ptr(k), 4, ptr(out)) == _lib.PSG_ERR_ARG
    assert L.psg_ftrl_status(h, None, None, None, None) == _lib.PSG_ERR_ARG
    assert L.psg_ftrl_reserve(h, 10) == _lib.PSG_ERR_ARG
    assert L.psg_ftrl_export(h, None, None, 0, C.byref(n)) == _lib.PSG_ERR_ARG
    assert L.psg_ftrl_lookup(h, ptr(k), 4, None, None, None, None, None) == _lib.PSG_ERR_ARG
    assert L.psg_ftrl_init(h, None, 0) == _lib.PSG_ERR_ARG
    _lib.check(L.psg_ftrl_init(h, C.byref(p), 0))
    # null arrays with n > 0; n == 0 is a no-op whatever the pointers
    assert L.psg_ftrl_push(h, None, 4, ptr(a), ptr(a), ptr(g)) == _lib.PSG_ERR_ARG
    assert L.psg_ftrl_push(h, ptr(k), 4, ptr(a), None, ptr(g)) == _lib.PSG_ERR_ARG
    assert L.psg_ftrl_push(h, ptr(k), 4, ptr(a), ptr(a), None) == _lib.PSG_ERR_ARG
    assert L.psg_ftrl_pull(h, ptr(k), 4, None) == _lib.PSG_ERR_ARG
    assert L.psg_ftrl_lookup(h, None, 4, None, None, None, None, None) == _lib.PSG_ERR_ARG
    assert L.psg_ftrl_push(h, None, 0, None, None, None) == _lib.PSG_OK
    assert L.psg_ftrl_pull(h, None, 0, None) == _lib.PSG_OK
    # the context stays usable
    assert L.psg_ftrl_push(h, ptr(k), 4, ptr(a), ptr(a), ptr(g)) == _lib.PSG_OK
    assert L.psg_ftrl_pull(h, ptr(k), 4, ptr(out)) == _lib.PSG_OK
    ref = R.ScalarFTRL(**R.PARITY_PARAM)
    ref.push(k, a, a, g)
    assert np.array_equal(R.bits(out), R.bits(R.pull(ref, k)))
    L.psg_destroy(h)


# ------------------------------------------- against the reference's recording
# tests/golden/reference_pin/ftrl_*.npz: what the reference's own FTRLModel
# (compiled in place, oracle/ref_ftrl_shim.cc) held after each of six
# messages, written by tools/record_reference.py.  The keys are chosen through
# fmix64's inverse: 60 land in the last bucket of every table and 60 in bucket
# 0, so chains longer than a bucket that wrap from the last bucket to the
# first exist in every table the model passes through.
@pytest.fixture(scope="module")
def pinned_case():
    import pin_cases as P
    c = P.ftrl_case()
    fixtures = {}
    for pname in P.FTRL_PARAMS:
        meta, fx = P.load_fixture("ftrl_" + pname)
        assert meta["input_sha256"] == c.digest() and meta["param"] == P.FTRL_PARAMS[pname]
        fixtures[pname] = (meta, fx)
    return P, c, fixtures


NO_REHASH_HINT = 4096  # 4,096 buckets hold 6,144 keys; the six messages push 3,418


@pytest.mark.parametrize("mode", ["one_bucket", "no_rehash", "reserve_between", "device_forms"])
@pytest.mark.parametrize("pname", ["parity", "steep"])
def test_against_the_recorded_reference_model(pinned_case, tmp_path, pname, mode):
    import torch
    P, c, fixtures = pinned_case
    meta, fx = fixtures[pname]
    if mode == "no_rehash":
        # the table's arithmetic (psg_ctx.h buckets_for): the smallest
        # power of two whose 3 * nb / 2 slots hold the hint, and no growth while
        # every key pushed so far fits
        nb = 1
        while 3 * nb // 2 < NO_REHASH_HINT:
            nb *= 2
        assert sum(m[0].size for m in c.msgs) <= 3 * nb // 2
        home = P.fmix64(c.keys) & np.uint64(nb - 1)
        assert int((home == nb - 1).sum()) >= 60 and int((home == 0).sum()) >= 60
        assert np.isin(c.last_bucket, c.msgs[0][0]).all()
        # 60 keys of home nb - 1 at 3 per bucket: a chain of >= 20 buckets
        # starting in the last bucket, so it wraps to bucket 0 and on
        assert int((home == nb - 1).sum()) // 3 >= 20
    m = new_model(hint={"one_bucket": 1, "no_rehash": NO_REHASH_HINT}.get(mode, 64),
                  **P.FTRL_PARAMS[pname])
    dev = torch.device("cuda:0")
    side = torch.cuda.Stream()

    def dt(a):
        a = np.ascontiguousarray(a)
        view = {8: np.int64, 4: np.int32}[a.dtype.itemsize] if a.dtype.kind == "u" else a.dtype
        return torch.from_numpy(a.view(view)).to(dev)

    for t, (msg, want) in enumerate(zip(c.msgs, meta["after"])):
        if mode == "reserve_between":
            m.reserve([700, 100, 1500, 1500, 5000, 20000][t])
        if mode == "device_forms":
            bufs = [dt(a) for a in msg]
            torch.cuda.synchronize()
            _lib.check(m._L.psg_ftrl_push_dev(m._h, bufs[0].data_ptr(), msg[0].size, bufs[1].data_ptr(),
                                              bufs[2].data_ptr(), bufs[3].data_ptr(), side.cuda_stream))
            side.synchronize()
        else:
            assert push(m, *msg) == _lib.PSG_OK
        rc, e, nz, _, _ = status(m)
        assert (rc, e, nz) == (_lib.PSG_OK, want["size"], want["nnz"])
        assert P.entry_digest(*m.lookup(c.keys)) == want["entries_sha256"]
    pos, neg, w, z, found = m.lookup(c.keys)
    assert np.array_equal(pos, fx["pos"]) and np.array_equal(neg, fx["neg"])
    assert np.array_equal(R.bits(w), fx["w"]) and np.array_equal(R.bits(z), fx["z"])
    assert np.array_equal(found, fx["found"])
    if mode == "device_forms":
        tk = dt(c.request)
        out = torch.full((c.request.size,), 7.0, dtype=torch.float64, device=dev)
        torch.cuda.synchronize()
        _lib.check(m._L.psg_ftrl_pull_dev(m._h, tk.data_ptr(), c.request.size, out.data_ptr(),
                                          side.cuda_stream))
        side.synchronize()
        pulled = out.cpu().numpy()
    else:
        req = Message(key=c.request)
        m.getValue(req)
        pulled = req.value[0]
    assert np.array_equal(R.bits(pulled), fx["pull"])
    keep = (fx["found"] == 1) & (fx["w"].view(np.float64) != 0)
    k, wn = m.export()
    assert np.array_equal(k, c.keys[keep]) and np.array_equal(R.bits(wn), fx["w"][keep])
    path = tmp_path / "model.txt"
    m.writeToFile(str(path))
    assert path.read_text() == fx["dump_text"].tobytes().decode()
    m.close()


@pytest.mark.parametrize("pname", ["parity", "steep"])
def test_norms_and_objv_within_the_stated_bound_on_the_recorded_case(pinned_case, pname):
    """psg_ftrl_status's norms are a defined deviation (a reduction, not the
    reference's running sums): each lies within entries * 2^-53 * (the exact
    sum) of it, and objv with them inside the interval that also holds the
    reference's recorded objv (tests/test_reference_pin.py).  On the recorded
    messages without the two infinite-gradient keys, whose weights are
    infinite; every other key's entry is what the reference recorded."""
    from fractions import Fraction
    P, c, fixtures = pinned_case
    meta, fx = fixtures[pname]
    param = P.FTRL_PARAMS[pname]
    m = new_model(hint=1, **param)
    for msg in c.finite_msgs():
        assert push(m, *msg) == _lib.PSG_OK
    rest = ~np.isin(c.keys, c.inf_keys)
    pos, neg, w, z, found = m.lookup(c.keys[rest])
    assert np.array_equal(R.bits(w), fx["w"][rest]) and np.array_equal(R.bits(z), fx["z"][rest])
    assert np.array_equal(found, fx["found"][rest])
    rc, entries, nnz, norm1, norm2 = status(m)
    assert (rc, entries, nnz) == (_lib.PSG_OK, int(found.sum()), meta["finite_nnz"])
    wl = w[found == 1].tolist()
    assert all(math.isfinite(x) for x in wl)
    s1 = sum(Fraction(abs(x)) for x in wl)
    s2 = sum(Fraction(x) * Fraction(x) for x in wl)
    eps = Fraction(entries, 1 << 53)
    print("norm1 %r (exact %r), norm2 %r (exact %r)" % (norm1, float(s1), norm2, float(s2)))
    assert abs(Fraction(norm1) - s1) <= eps * s1
    assert abs(Fraction(norm2) - s2) <= eps * s2
    lo, hi = P.objv_interval(wl, entries, param["lambda1"], param["lambda2"])
    ref = float(np.array([int(meta["finite_objv_bits"], 16)], np.uint64).view(np.float64)[0])
    assert lo <= m.objv() <= hi and lo <= ref <= hi
    m.close()
