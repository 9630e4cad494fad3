"""TEST INFRASTRUCTURE: ctypes binding of the reference's own code compiled in
place (oracle/_ref/libref_match.so, libref_ftrl.so, libref_countmin.so,
libref_auc.so, libref_localizer.so; see oracle/ref_*_shim.cc and
oracle/Makefile).  Only tools/record_reference.py
and the live tests of tests/test_reference_pin.py load it; no GPU test does.
"""
import ctypes as C
import os
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF_DIR = os.path.join(ROOT, "oracle", "_ref")
LIBS = {"match": "libref_match.so", "ftrl": "libref_ftrl.so", "countmin": "libref_countmin.so",
        "auc": "libref_auc.so", "localizer": "libref_localizer.so"}

_p, _sz, _u64, _psz = C.c_void_p, C.c_size_t, C.c_uint64, C.POINTER(C.c_size_t)
_pu64 = C.POINTER(C.c_uint64)
_loaded = {}


def path(which):
    return os.path.join(REF_DIR, LIBS[which])


def available(which):
    return os.path.exists(path(which))


def _agg_sig():
    return (C.c_int, [_p, _sz, _u64, _u64, C.c_int, _p, _p, C.c_int, _p, C.c_int, C.c_int, _p,
                      _psz, _psz, _p])


_SIG = {
    "match": {
        "ref_match_f32": (_sz, [C.c_int, _sz, _sz, _p, _sz, _p, _p, _p, _sz, C.c_int]),
        "ref_match_f64": (_sz, [C.c_int, _sz, _sz, _p, _sz, _p, _p, _p, _sz, C.c_int]),
        "ref_old_match_f32": (C.c_int, [_p, _sz, _p, _sz, _p, _u64, _u64, _p, _psz, _psz, _psz]),
        "ref_old_match_f64": (C.c_int, [_p, _sz, _p, _sz, _p, _u64, _u64, _p, _psz, _psz, _psz]),
        "ref_aggregate_f32": _agg_sig(),
        "ref_aggregate_f64": _agg_sig(),
        "ref_gather_f32": (None, [_p, _sz, _p, _p, _sz, _p, _psz]),
        "ref_gather_f64": (None, [_p, _sz, _p, _p, _sz, _p, _psz]),
        "ref_slice_key_ordered": (None, [_p, _sz, _u64, _u64, _p, _sz, _p, _p, _p, _p]),
        "ref_even_divide_u64": (None, [_u64, _u64, _sz, _sz, _pu64, _pu64]),
        "ref_range_all_u64": (None, [_pu64, _pu64]),
    },
    "ftrl": {
        "ref_ftrl_create": (_p, [C.c_double] * 4),
        "ref_ftrl_destroy": (None, [_p]),
        "ref_ftrl_set_value": (None, [_p, _p, _p, _p, _p, _sz]),
        "ref_ftrl_get_value": (None, [_p, _p, _sz, _p]),
        "ref_ftrl_nnz": (_sz, [_p]),
        "ref_ftrl_objv": (C.c_double, [_p]),
        "ref_ftrl_entries": (_sz, [_p]),
        "ref_ftrl_write_to_file": (None, [_p, C.c_char_p]),
        "ref_ftrl_lookup": (None, [_p, _p, _sz, _p, _p, _p, _p, _p]),
    },
    "countmin": {
        "ref_ff_create": (_p, []),
        "ref_ff_destroy": (None, [_p]),
        "ref_ff_resize": (None, [_p, C.c_int, C.c_int]),
        "ref_ff_clear": (None, [_p]),
        "ref_ff_empty": (C.c_int, [_p]),
        "ref_ff_insert_keys": (None, [_p, _p, _p, _sz]),
        "ref_ff_query_keys": (_sz, [_p, _p, _sz, C.c_int, _p]),
        "ref_ff_table": (None, [_p, C.POINTER(C.c_int), C.POINTER(C.c_int), _p]),
    },
    "auc": {
        "ref_auc_compute": (None, [C.c_int64, _p, _p, _sz, _p, _p, _psz, _p, _p, _psz]),
        "ref_auc_create": (_p, [C.c_int64]),
        "ref_auc_destroy": (None, [_p]),
        "ref_auc_merge": (None, [_p, _p, _p, _sz, _p, _p, _sz]),
        "ref_auc_accuracy": (C.c_double, [_p, C.c_double]),
        "ref_auc_evaluate": (C.c_double, [_p]),
        "ref_auc_maps": (None, [_p, _psz, _psz, _p, _p, _p, _p]),
        "ref_eval_auc": (C.c_double, [_p, _p, _sz]),
    },
    "localizer": {
        "ref_loc_create": (_p, []),
        "ref_loc_destroy": (None, [_p]),
        "ref_loc_count_uniq": (_sz, [_p, _p, _sz, C.c_int, _p, _p]),
        "ref_loc_remap": (C.c_int, [_p, _p, _sz, _p, _sz, _p, _p, _sz, C.c_int, _p, _p, _psz, _p,
                                    _psz]),
    },
}


def lib(which):
    if which not in _loaded:
        L = C.CDLL(path(which))
        for name, (res, args) in _SIG[which].items():
            f = getattr(L, name)
            f.restype, f.argtypes = res, args
        _loaded[which] = L
    return _loaded[which]


def _a(x):
    return x.ctypes.data


def u64(x):
    return np.ascontiguousarray(np.asarray(x, dtype=np.uint64))


def _sfx(dtype):
    return "_f32" if np.dtype(dtype) == np.float32 else "_f64"


# ------------------------------------------------------------------ message.h
def match(D, lo, hi, dst, keys, vals, add, threads, dtype):
    """The reference's match over positions [lo, hi) of D; dst (hi - lo
    values) is updated on a copy.  Returns (dst, matched)."""
    D, keys = u64(D), u64(keys)
    dst = np.array(dst, dtype)
    vals = np.ascontiguousarray(vals, dtype)
    f = getattr(lib("match"), "ref_match" + _sfx(dtype))
    n = f(threads, lo, hi, _a(D), D.size, _a(dst), _a(keys), _a(vals), keys.size, int(add))
    return dst, n


def old_match(D, keys, vals, kb, ke, dtype):
    D, keys = u64(D), u64(keys)
    vals = np.ascontiguousarray(vals, dtype)
    out = np.zeros(max(1, D.size), dtype)
    lo, hi, mt = C.c_size_t(), C.c_size_t(), C.c_size_t()
    f = getattr(lib("match"), "ref_old_match" + _sfx(dtype))
    f(_a(D), D.size, _a(keys), keys.size, _a(vals), int(kb), int(ke), _a(out),
      C.byref(lo), C.byref(hi), C.byref(mt))
    return lo.value, hi.value, out[: hi.value - lo.value], mt.value


def aggregate(D, kb, ke, pushes, parallel=False, nthreads=1, dtype=np.float32):
    """As oracle_py.aggregate: (rc, lo, hi, [out] * m, matched)."""
    D = u64(D)
    dtype = np.dtype(dtype)
    npush = len(pushes)
    m = len(pushes[0][1]) if npush else 1
    keys = [u64(k) for k, _ in pushes]
    vals = [np.ascontiguousarray(v, dtype=dtype) for _, vs in pushes for v in vs]
    kp = (C.c_void_p * max(1, npush))(*[_a(k) for k in keys])
    ns = (C.c_size_t * max(1, npush))(*[k.size for k in keys])
    vp = (C.c_void_p * max(1, len(vals)))(*[_a(v) for v in vals])
    outs = [np.zeros(max(1, D.size), dtype) for _ in range(m)]
    op = (C.c_void_p * m)(*[_a(o) for o in outs])
    lo, hi = C.c_size_t(), C.c_size_t()
    matched = np.zeros(max(1, npush), np.uint64)
    f = getattr(lib("match"), "ref_aggregate" + _sfx(dtype))
    rc = f(_a(D), D.size, int(kb), int(ke), npush, kp, ns, m, vp, int(parallel), nthreads, op,
           C.byref(lo), C.byref(hi), _a(matched))
    n = hi.value - lo.value
    return rc, lo.value, hi.value, [o[:n] for o in outs], matched[:npush]


def gather(D, W, req, dtype=np.float32):
    D, req = u64(D), u64(req)
    W = np.ascontiguousarray(W, dtype=dtype)
    out = np.zeros(max(1, req.size), dtype)
    mt = C.c_size_t()
    getattr(lib("match"), "ref_gather" + _sfx(dtype))(_a(D), D.size, _a(W), _a(req), req.size,
                                                       _a(out), C.byref(mt))
    return out[: req.size], mt.value


def slice_key_ordered(keys, rb, re, sep):
    """(begin, end, vbegin, valid) per piece; -1 where the piece is invalid."""
    keys, sep = u64(keys), u64(sep)
    n = sep.size - 1
    b, e, vb = (np.zeros(n, np.int64) for _ in range(3))
    valid = np.zeros(n, np.int32)
    lib("match").ref_slice_key_ordered(_a(keys), keys.size, int(rb), int(re), _a(sep), sep.size,
                                       _a(b), _a(e), _a(vb), _a(valid))
    return b, e, vb, valid


def even_divide(b, e, n, i):
    ob, oe = C.c_uint64(), C.c_uint64()
    lib("match").ref_even_divide_u64(int(b), int(e), n, i, C.byref(ob), C.byref(oe))
    return ob.value, oe.value


def range_all():
    ob, oe = C.c_uint64(), C.c_uint64()
    lib("match").ref_range_all_u64(C.byref(ob), C.byref(oe))
    return ob.value, oe.value


# --------------------------------------------------------------- ftrl_model.h
class RefFTRL:
    """The reference's FTRLModel<uint64, double>, with ftrl_ref's interface."""

    def __init__(self, alpha, beta, lambda1, lambda2):
        self._L = lib("ftrl")
        self._h = self._L.ref_ftrl_create(alpha, beta, lambda1, lambda2)

    def __del__(self):
        if getattr(self, "_h", None):
            self._L.ref_ftrl_destroy(self._h)
            self._h = None

    def push(self, keys, pos, neg, grad):
        k = u64(keys)
        a, b = np.ascontiguousarray(pos, np.uint32), np.ascontiguousarray(neg, np.uint32)
        g = np.ascontiguousarray(grad, np.float64)
        self._L.ref_ftrl_set_value(self._h, _a(k), _a(a), _a(b), _a(g), k.size)

    def get_value(self, keys):
        """getValue: inserts a zero entry for every absent key."""
        k = u64(keys)
        out = np.zeros(max(1, k.size), np.float64)
        self._L.ref_ftrl_get_value(self._h, _a(k), k.size, _a(out))
        return out[: k.size]

    @property
    def entries(self):
        return self._L.ref_ftrl_entries(self._h)

    @property
    def nnz(self):
        return self._L.ref_ftrl_nnz(self._h)

    def objv(self):
        return self._L.ref_ftrl_objv(self._h)

    def lookup(self, keys):
        k = u64(keys)
        pos, neg = np.zeros(k.size, np.uint64), np.zeros(k.size, np.uint64)
        w, z = np.zeros(k.size, np.float64), np.zeros(k.size, np.float64)
        found = np.zeros(k.size, np.uint8)
        self._L.ref_ftrl_lookup(self._h, _a(k), k.size, _a(pos), _a(neg), _a(w), _a(z), _a(found))
        return pos, neg, w, z, found

    def dump_text(self):
        """writeToFile's text as written (the map's order)."""
        with tempfile.TemporaryDirectory() as d:
            p = os.path.join(d, "model.txt")
            self._L.ref_ftrl_write_to_file(self._h, p.encode())
            with open(p) as f:
                return f.read()


# ------------------------------------------------- frequency_filter.h, countmin.h
class RefFilter:
    def __init__(self):
        self._L = lib("countmin")
        self._h = self._L.ref_ff_create()

    def __del__(self):
        if getattr(self, "_h", None):
            self._L.ref_ff_destroy(self._h)
            self._h = None

    def resize(self, n, k):
        self._L.ref_ff_resize(self._h, n, k)

    def clear(self):
        self._L.ref_ff_clear(self._h)

    def empty(self):
        return bool(self._L.ref_ff_empty(self._h))

    def insert_keys(self, keys, counts):
        k, c = u64(keys), np.ascontiguousarray(counts, np.uint32)
        self._L.ref_ff_insert_keys(self._h, _a(k), _a(c), k.size)

    def query_keys(self, keys, freq):
        k = u64(keys)
        out = np.zeros(max(1, k.size), np.uint64)
        n = self._L.ref_ff_query_keys(self._h, _a(k), k.size, freq, _a(out))
        return out[:n].copy()

    def table(self):
        """(n_, k_, data_ bytes)."""
        n, k = C.c_int(), C.c_int()
        self._L.ref_ff_table(self._h, C.byref(n), C.byref(k), None)
        out = np.zeros(max(1, n.value), np.uint8)
        self._L.ref_ff_table(self._h, C.byref(n), C.byref(k), _a(out))
        return n.value, k.value, out[: n.value]


# ------------------------------------------------------- auc.h, evaluation.h
def _f64(x):
    return np.ascontiguousarray(x, np.float64)


def auc_compute(y, predict, goodness):
    """AUC::compute<double>: the AUCData (tp_key, tp_count, fp_key, fp_count)."""
    y, p = _f64(y), _f64(predict)
    assert y.size == p.size >= 1  # the reference CHECKs both
    tk, fk = np.zeros(y.size, np.int64), np.zeros(y.size, np.int64)
    tc, fc = np.zeros(y.size, np.uint64), np.zeros(y.size, np.uint64)
    nt, nf = C.c_size_t(), C.c_size_t()
    lib("auc").ref_auc_compute(int(goodness), _a(y), _a(p), y.size, _a(tk), _a(tc), C.byref(nt),
                               _a(fk), _a(fc), C.byref(nf))
    return (tk[:nt.value].copy(), tc[:nt.value].copy(), fk[:nf.value].copy(), fc[:nf.value].copy())


class RefAUC:
    """The reference's AUC as the root uses it: merge, accuracy, evaluate."""

    def __init__(self, goodness):
        self._L = lib("auc")
        self._h = self._L.ref_auc_create(int(goodness))

    def __del__(self):
        if getattr(self, "_h", None):
            self._L.ref_auc_destroy(self._h)
            self._h = None

    def merge(self, tp_key, tp_count, fp_key, fp_count):
        tk, fk = (np.ascontiguousarray(a, np.int64) for a in (tp_key, fp_key))
        tc, fc = (np.ascontiguousarray(a, np.uint64) for a in (tp_count, fp_count))
        assert tk.size == tc.size and fk.size == fc.size  # the reference CHECKs both
        self._L.ref_auc_merge(self._h, _a(tk), _a(tc), tk.size, _a(fk), _a(fc), fk.size)

    def accuracy(self, threshold):
        return self._L.ref_auc_accuracy(self._h, float(threshold))

    def evaluate(self):
        return self._L.ref_auc_evaluate(self._h)

    def maps(self):
        """The two maps as an AUCData, zero counts included."""
        nt, nf = C.c_size_t(), C.c_size_t()
        self._L.ref_auc_maps(self._h, C.byref(nt), C.byref(nf), None, None, None, None)
        tk, fk = np.zeros(max(1, nt.value), np.int64), np.zeros(max(1, nf.value), np.int64)
        tc, fc = np.zeros(max(1, nt.value), np.uint64), np.zeros(max(1, nf.value), np.uint64)
        self._L.ref_auc_maps(self._h, C.byref(nt), C.byref(nf), _a(tk), _a(tc), _a(fk), _a(fc))
        return tk[:nt.value], tc[:nt.value], fk[:nf.value], fc[:nf.value]


def exact_auc(y, predict):
    """Evaluation<double>::auc."""
    y, p = _f64(y), _f64(predict)
    assert y.size == p.size
    return lib("auc").ref_eval_auc(_a(y), _a(p), y.size)


# ---------------------------------------------------------------- localizer.h
class RefLocalizer:
    """The reference's Localizer<uint64, double>: count_uniq, then remap
    against any number of dictionaries (it keeps the sorted pairs)."""

    def __init__(self):
        self._L = lib("localizer")
        self._h = self._L.ref_loc_create()

    def __del__(self):
        if getattr(self, "_h", None):
            self._L.ref_loc_destroy(self._h)
            self._h = None

    def count_uniq(self, index, threads=1):
        """(uniq_idx, idx_frq)."""
        idx = u64(index)
        assert idx.size >= 1
        uniq, frq = np.zeros(idx.size, np.uint64), np.zeros(idx.size, np.uint32)
        n = self._L.ref_loc_count_uniq(self._h, _a(idx), idx.size, threads, _a(uniq), _a(frq))
        return uniq[:n].copy(), frq[:n].copy()

    def remap(self, offset, index, value, dic, threads=1):
        """(new_offset, new_index, new_value), or None where the reference
        returns a null pointer.  value None: a binary matrix."""
        off, idx, d = u64(offset), u64(index), u64(dic)
        assert idx.size == 0 or d.size == 0 or int(off[-1]) == idx.size  # CHECKed
        val = None if value is None else _f64(value)
        no = np.zeros(off.size, np.uint64)
        ni, nv = np.zeros(max(1, idx.size), np.uint32), np.zeros(max(1, idx.size), np.float64)
        nni, nnv = C.c_size_t(), C.c_size_t()
        rc = self._L.ref_loc_remap(self._h, _a(off), off.size, _a(idx), idx.size,
                                   None if val is None else _a(val), _a(d), d.size, threads,
                                   _a(no), _a(ni), C.byref(nni), _a(nv), C.byref(nnv))
        if rc != 0:
            return None
        return no, ni[:nni.value].copy(), nv[:nnv.value].copy()
