"""N-way merge (psg_nway.hip) at its seams, against the oracle and the
planning model of tests/nway_ref.py:

* keys and sums of every merge equal oracle_py's set_union / aggregate bit
  for bit, and for every sorted merge the splitters of the run
  (psg_nway_splitters) equal the model's exactly -- a rank that is off by a
  little moves a splitter long before it changes the output;
* push lengths around the sampling stride s (no candidate, one candidate,
  the last key a candidate), runs of equal keys across a thread's 8 outputs
  and a wave, the assign / add / trailing +0.0 rule on -0.0;
* the three rank kernels (16, 4 and 1 candidates per thread), the form
  asserted through psg_nway_shape, and a candidate list one past the LDS
  stage;
* disordered pushes: PSG_ERR_UNSORTED, never PSG_ERR_DEVICE, and no entry of
  the outputs at or past sum(n) is written.  The outputs of those tests hold
  T * 2048 entries -- a tile stores at most 2,048 entries behind the sum of
  the earlier tiles' counts -- so the check cannot itself store out of bounds.

Each batch's pushes live in one device buffer; merges get offsets into it."""
import ctypes as C

import numpy as np
import pytest

import nway_ref as R
import oracle_py as O

pytestmark = pytest.mark.gpu

ALL = (0, (1 << 64) - 1)
CANARY = 0x5A5A5A5A5A5A5A5A
_u = np.uint64


def _bits(a):
    a = np.asarray(a)
    return a.view(np.uint32 if a.dtype == np.float32 else np.uint64)


def _union(pushes):
    D = np.zeros(0, np.uint64)
    for k, _ in pushes:
        D = O.set_union(D, k)
    return D


class _Batch:
    """merges: [[(keys, [vals] * m)] per merge] in ONE key buffer and m value
    buffers on the device; outputs in one key buffer and m value buffers,
    merge j at out_off[j] with out_cap[j] entries, all filled with CANARY."""

    def __init__(self, merges, dtype=np.float32, m=1, parallel=False, out_cap=None, single=False):
        import torch
        from parameter_server_amd._lib import PSG_F32, PSG_F64
        from parameter_server_amd.kv_vector import NWayMerge, NWayMergeBatch
        dev = torch.device("cuda", 0)
        self.merges, self.m, self.dtype, self.parallel = merges, m, np.dtype(dtype), parallel
        esz = self.dtype.itemsize
        ks = [np.ascontiguousarray(k, np.uint64) for ps in merges for k, _ in ps]
        lens = [k.size for k in ks]
        off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
        allk = np.concatenate(ks + [np.zeros(1, np.uint64)])
        self.dk = torch.from_numpy(allk.view(np.int64)).to(dev)
        self.dv = []
        for i in range(m):
            allv = np.concatenate([np.ascontiguousarray(vs[i], dtype) for ps in merges for _, vs in ps]
                                  + [np.zeros(1, dtype)])
            self.dv.append(torch.from_numpy(allv).to(dev))
        tots = [sum(k.size for k, _ in ps) for ps in merges]
        self.out_cap = list(out_cap) if out_cap is not None else [max(1, t) for t in tots]
        self.out_off = np.concatenate([[0], np.cumsum(self.out_cap)]).astype(np.int64)
        self.ok = torch.full((int(self.out_off[-1]),), CANARY, dtype=torch.int64, device=dev)
        tdt = torch.float32 if self.dtype == np.float32 else torch.float64
        cv = np.array([CANARY], np.uint64).view(self.dtype)[0]
        self.cv = cv
        self.ov = [torch.full((int(self.out_off[-1]),), float(cv), dtype=tdt, device=dev)
                   for _ in range(m)]
        specs, p = [], 0
        for j, ps in enumerate(merges):
            pk = [self.dk.data_ptr() + 8 * int(off[p + q]) for q in range(len(ps))]
            pv = [[t.data_ptr() + esz * int(off[p + q]) for t in self.dv] for q in range(len(ps))]
            specs.append(dict(push_keys=pk, push_n=[k.size for k, _ in ps], push_vals=pv,
                              out_keys=self.ok.data_ptr() + 8 * int(self.out_off[j]),
                              out_vals=[t.data_ptr() + esz * int(self.out_off[j]) for t in self.ov]))
            p += len(ps)
        code = PSG_F32 if self.dtype == np.float32 else PSG_F64
        if single:
            (x,) = specs
            self.u = NWayMerge(0, code, x["push_keys"], x["push_n"], x["push_vals"], x["out_keys"],
                               x["out_vals"], parallel)
        else:
            self.u = NWayMergeBatch(0, code, specs, parallel)
        self.single = single

    def run(self, stream=None):
        self.u.run(stream)

    def counts(self):
        r = self.u.result()
        return [r] if self.single else r

    def out_keys(self, j):
        a = self.ok[int(self.out_off[j]): int(self.out_off[j + 1])].cpu().numpy()
        return a.view(np.uint64)

    def out_vals(self, j, i):
        return self.ov[i][int(self.out_off[j]): int(self.out_off[j + 1])].cpu().numpy()

    def close(self):
        self.u.close()


def _check_sorted(b, counts=None, values=True):
    """Every merge of the batch: count, keys, sums against the oracle and the
    splitters against the model."""
    counts = counts if counts is not None else b.counts()
    for j, pushes in enumerate(b.merges):
        D = _union(pushes)
        assert counts[j] == D.size, "merge %d" % j
        got = b.out_keys(j)
        assert np.array_equal(got[: D.size], D), "merge %d" % j
        if got.size > D.size and D.size:  # nothing behind the merged keys
            assert np.all(got[D.size:] == _u(CANARY)), "merge %d" % j
        model = R.Merge([k for k, _ in pushes])
        assert b.u.shape[j] == tuple(model.shape[x] for x in ("K", "s", "cw", "B", "T"))
        assert b.u.splitters(j).tolist() == model.split, "merge %d" % j
        if values and b.m and D.size:
            # Range::all() = [0, 2^64 - 1): a key 2^64 - 1 is in the union but
            # outside the oracle's aligned range; compare [lo, hi)
            rc, lo, hi, want, _ = O.aggregate(D, *ALL, [(k, vs[: b.m]) for k, vs in pushes],
                                              b.parallel, 1, b.dtype)
            assert rc == 0
            for i in range(b.m):
                assert np.array_equal(_bits(b.out_vals(j, i)[lo:hi]),
                                      _bits(np.asarray(want[i], b.dtype))), "merge %d" % j


def _with_values(seed, keys, m, dtype, neg_zero=True):
    out = []
    for q, k in enumerate(keys):
        vs = [R.values(seed * 1009 + 17 * q + i, k.size, dtype) for i in range(m)]
        if neg_zero:
            for i, v in enumerate(vs):
                v[(R.draws(seed * 31 + 5 * q + i, k.size) % _u(8)) == 0] = -0.0
        out.append((k, vs))
    return out


def _subsets(seed, ns, bits=64, spread=2):
    """Pushes of lengths ns drawn from one universe (so keys repeat across
    pushes), each sorted."""
    U = R.sorted_keys(seed, spread * max(ns) + 8, bits)
    out = []
    for q, n in enumerate(ns):
        pick = np.sort(np.argsort(R.draws(seed * 131 + q + 1, U.size), kind="stable")[:n])
        out.append(np.ascontiguousarray(U[pick]))
    return out


# ------------------------------------------------------------ stride seams
def _seam_lengths(K):
    s = R.shape([1] * K)["s"]
    return s, [1, s - 1, s, s + 1, 2 * s - 1, 2 * s, 2 * s + 1]


def _seam_merges():
    merges = []
    for K in (1, 2, 3, 8, 33, 64):
        s, L = _seam_lengths(K)
        nm = -(-len(L) // K)  # enough merges of K pushes to use every length
        for j in range(nm):
            ns = [L[(j * K + q) % len(L)] for q in range(K)]
            merges.append(_subsets(100 * K + j, ns, bits=20))
    s2 = R.shape([1, 1])["s"]
    s3 = R.shape([1, 1, 1])["s"]
    none = _subsets(701, [1, s3 - 1, s3 - 1], bits=20)          # no candidate at all
    one = _subsets(702, [s2, s2 - 1], bits=20)                  # exactly one candidate
    # keys 0 and 2^64 - 1 in the merge, 2^64 - 1 twice a candidate (the last
    # key of a push of s and of a push of 2 s keys); 0 can be no candidate (it
    # can only be a push's first key and s >= 4)
    a = R.sorted_keys(703, 2 * s2, 64)
    a[0], a[-1] = 0, R.M64
    b = R.sorted_keys(704, s2, 64)
    b[0], b[-1] = 0, R.M64
    ends = [a, b]
    return merges, [none, one, ends]


@pytest.mark.parametrize("dtype,m", [(np.float32, 1), (np.float64, 2)])
@pytest.mark.parametrize("parallel", [False, True])
def test_stride_seams(dtype, m, parallel):
    merges, (none, one, ends) = _seam_merges()
    assert R.Merge(none).shape["ncand"] == 0 and R.Merge(one).shape["ncand"] == 1
    assert R.Merge(ends).cand_keys.count(R.M64) == 2
    cases = [_with_values(11 + j, ks, m, dtype) for j, ks in enumerate(merges + [none, one, ends])]
    b = _Batch(cases, dtype, m, parallel)
    b.run()
    _check_sorted(b)
    b.close()
    # a merge without a candidate on its own: the candidate stages are skipped
    for j in (-3, -2, -1):
        b = _Batch([cases[j]], dtype, m, parallel, single=True)
        b.run()
        _check_sorted(b)
        b.close()


# -------------------------------------------------------- tile fill and runs
def _run_at(p):
    """64 pushes that all hold X; in the merged order p keys come before it."""
    X = 1 << 32
    fill = R.sorted_keys(900 + p, 64 * 40 + p, 30)
    pushes = []
    for q in range(64):
        hi = fill[p + 40 * q: p + 40 * (q + 1)] + _u(X + 1)
        lo = fill[:p] if q == 0 else fill[:0]
        pushes.append(np.concatenate([lo, [_u(X)], hi]).astype(np.uint64))
    return X, pushes


def _membership(K=5):
    """One merge: filler keys, and per pattern of holders and per kind of
    value one special key."""
    pats = {"first": [0], "last": [K - 1], "all": list(range(K)),
            "not_first": list(range(1, K)), "not_last": list(range(K - 1))}
    fill = _subsets(950, [700 + 30 * q for q in range(K)], bits=40)
    keys = [[int(x) * 16 + 8 for x in f.tolist()] for f in fill]  # specials: multiples of 16
    vals = [R.values(960 + q, len(keys[q]), np.float64).tolist() for q in range(K)]
    special = {}
    for i, (name, holders) in enumerate(sorted(pats.items())):
        for kind in (0, 1):
            x = ((1 << 38) // 11 * (2 * i + kind + 1)) // 16 * 16
            special[(name, kind)] = x
            for q in holders:
                keys[q].append(x)
                vals[q].append(-0.0 if kind == 0 else (-1) ** q * (q + 1.25) * 2.0 ** -20)
    out = []
    for q in range(K):
        o = np.argsort(np.array(keys[q], np.uint64), kind="stable")
        out.append((np.array(keys[q], np.uint64)[o], np.array(vals[q], np.float64)[o]))
    return special, out


@pytest.mark.parametrize("parallel", [False, True])
def test_tile_fill_and_runs(parallel):
    same3 = [np.arange(600, dtype=np.uint64) * _u(3)] * 3
    assert max(R.Merge(same3).tile_sizes) == 1782  # the fullest tile the model finds
    same64 = [np.arange(48, dtype=np.uint64) * _u(7) + _u(1)] * 64
    merges = [same3, same64]
    for p in (5, 8, 61):  # inside a thread's 8 outputs, at their edge, run across the wave's edge
        X, pushes = _run_at(p)
        assert R.Merge(pushes).locate(X) == (0, p)
        merges.append(pushes)
    # push 0 has keys, but none in the later tiles
    low = [np.arange(100, dtype=np.uint64)] + _subsets(970, [2000, 1900, 2100], bits=40)
    low = [low[0]] + [k + _u(1000) for k in low[1:]]
    mlow = R.Merge(low)
    assert mlow.shape["T"] >= 4 and any(pc[0] == 0 and sum(pc) > 0 for pc in mlow.piece)
    merges.append(low)
    for dtype, m in ((np.float32, 1), (np.float64, 2)):
        cases = [_with_values(40 + j, ks, m, dtype) for j, ks in enumerate(merges)]
        if dtype == np.float64:
            special, mem = _membership()
            cases.append([(k, [v, -v]) for k, v in mem])
        b = _Batch(cases, dtype, m, parallel)
        b.run()
        _check_sorted(b)
        if dtype == np.float64:
            # -0.0 tells the rules apart: push 0 assigns, later pushes add to
            # +0.0, serial adds +0.0 when a push lacked the key
            j = len(cases) - 1
            D, got = b.out_keys(j), b.out_vals(j, 0)
            at = lambda name: got[int(np.searchsorted(D, _u(special[(name, 0)])))]  # noqa: E731
            neg = lambda x: bool(np.signbit(x)) and x == 0  # noqa: E731
            assert neg(at("all"))
            assert neg(at("first")) == parallel and neg(at("not_last")) == parallel
            assert not neg(at("last")) and not neg(at("not_first"))
        b.close()


# ---------------------------------------------------------------- rank forms
def _form16_merges(nm=512):
    return [_subsets(2000 + j, ns, bits=44) for j, ns in enumerate(R.form16_lengths(nm))]


def test_rank_form_16_ragged_batch():
    merges = _form16_merges()
    cases = [_with_values(50 + j, ks, 1, np.float32) for j, ks in enumerate(merges)]
    b = _Batch(cases, np.float32, 1)
    assert b.u.rank_form == 16
    b.run()
    _check_sorted(b)
    b.close()


def test_rank_form_4_batch_of_64_pushes():
    merges = [_subsets(3000 + j, [200] * 64, bits=44) for j in range(128)]
    cases = [_with_values(60 + j, ks, 1, np.float32) for j, ks in enumerate(merges)]
    b = _Batch(cases, np.float32, 1, parallel=True)
    assert b.u.rank_form == 4 and sum(sum(k.size for k in ks) for ks in merges) == 128 * 64 * 200
    b.run()
    _check_sorted(b)
    b.close()


def test_rank_form_1_single_merge():
    keys = _subsets(4000, [5000, 1, 3333, 8192, 700], bits=50)
    b = _Batch([_with_values(70, keys, 2, np.float64)], np.float64, 2, single=True)
    assert b.u.rank_form == 1
    b.run()
    _check_sorted(b)
    b.close()


def test_rank_form_16_list_past_the_lds_stage():
    """Keys only: 511 small merges and one K = 2 merge whose candidate lists
    hold 8,192 (staged in LDS) and 8,193 candidates (searched in global
    memory)."""
    small = [_subsets(5000 + j, [300, 280 + j % 40], bits=44) for j in range(511)]
    s = R.shape([1, 1])["s"]
    assert s == 128
    U = R.sorted_keys(5999, (R.RK_LIST + 1) * s * 3 // 2, 64)
    a = np.ascontiguousarray(U[np.sort(np.argsort(R.draws(6001, U.size), kind="stable")[: R.RK_LIST * s])])
    c = np.ascontiguousarray(U[np.sort(np.argsort(R.draws(6002, U.size), kind="stable")[: (R.RK_LIST + 1) * s])])
    merges = small + [[a, c]]
    big = R.Merge([a, c]).shape
    assert [big["cbase"][1], big["cbase"][2] - big["cbase"][1]] == [R.RK_LIST, R.RK_LIST + 1]
    b = _Batch([[(k, []) for k in ks] for ks in merges], np.float32, 0)
    assert b.u.rank_form == 16
    b.run()
    _check_sorted(b)
    b.close()


# ------------------------------------------------------------ the count word
def _read_word(ptr):
    out = np.zeros(1, np.uint64)
    hip = C.CDLL("libamdhip64.so")
    assert hip.hipMemcpy(C.c_void_p(out.ctypes.data), C.c_void_p(ptr), C.c_size_t(8), 2) == 0
    return int(out[0])


def test_count_word_on_the_device():
    """psg_nway_count_dev's word equals psg_nway_result's count after each
    of two runs, the second on a side stream."""
    import torch
    keys = _subsets(7000, [3000, 2500, 4000], bits=40)
    b = _Batch([_with_values(80, keys, 1, np.float32)], single=True)
    want = _union(b.merges[0]).size
    b.run()
    assert b.counts() == [want] and _read_word(b.u.count_dev()) == want
    side = torch.cuda.Stream()
    b.ok.fill_(CANARY)
    torch.cuda.synchronize()
    b.run(side.cuda_stream)
    assert b.counts() == [want] and _read_word(b.u.count_dev()) == want
    _check_sorted(b, [want])
    b.close()


# ---------------------------------------------------------- disordered pushes
def _disordered_cases():
    cases = {"A": R.case_a(), "B": R.case_b(), "reversed": R.case_reversed(),
             "dup_run": R.case_dup_run(),
             "block_overflow": R.case_c(R.CASE_C_OVERFLOW_SEED),
             "block_over_produce": R.case_c(R.CASE_C_OVERPRODUCE_SEED)}
    return cases


def _expect_unsorted(b):
    from parameter_server_amd._lib import PSG_ERR_UNSORTED, PSGError
    b.run()
    with pytest.raises(PSGError) as e:
        b.counts()
    assert e.value.status == PSG_ERR_UNSORTED, e.value


def _canary_holds(b, j, ntot):
    keys = b.out_keys(j)
    assert keys.size >= ntot + 1
    assert np.all(keys[ntot:] == _u(CANARY)), "keys stored at or past sum(n)"
    for i in range(b.m):
        assert np.all(_bits(b.out_vals(j, i)[ntot:]) == _bits(np.array([b.cv]))), \
            "values stored at or past sum(n)"


@pytest.mark.parametrize("name", ["A", "B", "reversed", "dup_run", "block_overflow",
                                  "block_over_produce"])
def test_disordered_pushes_are_unsorted_and_bounded(name):
    keys = _disordered_cases()[name]
    model = R.Merge(keys, device=True)
    if name in ("A", "B", "reversed", "block_overflow"):
        assert model.overflows()
    if name == "block_over_produce":
        assert not model.overflows() and model.distinct() > model.ntot
    ntot, cap = model.ntot, model.shape["T"] * R.CAP
    assert cap > ntot
    bad = _with_values(90, keys, 1, np.float32)
    good = [_with_values(91 + j, _subsets(8000 + j, [900, 1100, 40], bits=30), 1, np.float32)
            for j in range(2)]
    # alone
    b = _Batch([bad], out_cap=[cap], single=True)
    _expect_unsorted(b)
    _canary_holds(b, 0, ntot)
    b.close()
    # as one merge of a batch whose other merges are fine
    b = _Batch([good[0], bad, good[1]], out_cap=[2041, cap, 2041])
    assert b.u.rank_form == 1
    _expect_unsorted(b)
    _canary_holds(b, 1, ntot)
    for j in (0, 2):
        D = _union(b.merges[j])
        assert np.array_equal(b.out_keys(j)[: D.size], D)
    b.close()
    # a following good run on a fresh handle works
    b = _Batch(good)
    b.run()
    _check_sorted(b)
    b.close()


@pytest.mark.parametrize("name", ["A", "B", "reversed"])
def test_disordered_key_unions_are_unsorted(name):
    """psg_key_union_dev and a key-only Message to a context: the outputs
    are sized by sum(n), which the model shows these cases to stay within."""
    import torch
    from parameter_server_amd._lib import PSG_ERR_UNSORTED, PSGError, check, lib
    from parameter_server_amd.kv_vector import KVVector, Message
    good, bad = _disordered_cases()[name]
    model = R.Merge([good, bad], device=True)
    assert model.overflows() and model.kept_elements() <= model.ntot
    dev = torch.device("cuda", 0)
    da = torch.from_numpy(good.view(np.int64)).to(dev)
    db = torch.from_numpy(np.ascontiguousarray(bad).view(np.int64)).to(dev)
    out = torch.full((model.ntot + 64,), CANARY, dtype=torch.int64, device=dev)
    n = C.c_uint64(0)
    with pytest.raises(PSGError) as e:
        check(lib().psg_key_union_dev(da.data_ptr(), good.size, db.data_ptr(), bad.size,
                                      out.data_ptr(), C.byref(n), None))
    assert e.value.status == PSG_ERR_UNSORTED, e.value
    assert np.all(out.cpu().numpy()[model.ntot:].view(np.uint64) == _u(CANARY))
    v = KVVector(0)
    v.setValue(Message(key=good))
    with pytest.raises(PSGError) as e:
        v.setValue(Message(key=np.ascontiguousarray(bad)))
    assert e.value.status == PSG_ERR_UNSORTED, e.value
    assert np.array_equal(v.key(0), good)
    more = R.sorted_keys(8100, 3000, 20)
    v.setValue(Message(key=more))  # and the context goes on working
    assert np.array_equal(v.key(0), O.set_union(good, more))
    v.close()
