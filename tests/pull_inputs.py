"""Inputs of the pull-path seam tests (test_pull_inputs.py, test_pull_edges_gpu.py):
server key sets, values and sorted requests that put a repeat, an inversion,
a span length or a search length on a chosen seam of the gather, pull,
order-check and slice kernels.  No GPU and no library here: exact integer
arithmetic and NumPy only, seeded from pin_cases.splitmix64.

The constants mirror parameter_server_amd/csrc/psg_kernels.hip (kGR, kGS and
gather_block's layout; check_sorted_kernel's and slice_kernel's launch shapes)
and psg_device.h (wave_search's 64 probes per round):

    GR = 1024         requests per workgroup             (kGR)
    PER_THREAD = 4    consecutive requests per thread    (kI = kGR / 256)
    WAVE = 256        requests per 64-lane wave          (64 * kI)
    GS = 4096         server keys staged in LDS          (kGS)
    SORT_BLOCK = 256  keys per check_sorted_kernel workgroup
    ARY = 64          wave_search's fan-out: lengths 64^k - 1, 64^k, 64^k + 1

Every gather builder takes the value type and returns named cases
(name, D, W, req): sorted unique server keys, their values, the request.
Server keys are even wherever a builder needs absent keys between neighbours,
so key + 1 is absent."""
import numpy as np

from pin_cases import splitmix64

GR = 1024
PER_THREAD = 4
WAVE = 256
GS = 4096
SORT_BLOCK = 256
ARY = 64
SLICE_WAVES = 4  # separators per slice_kernel workgroup

U64_MAX = (1 << 64) - 1
ND = 20_000  # server keys of families a, b, c, e, f

# server-key counts at the 64-ary search's corners (families d and g)
D_SIZES = [0, 1, 2, ARY - 1, ARY, ARY + 1, ARY ** 2 - 1, ARY ** 2, ARY ** 2 + 1,
           ARY ** 3 - 1, ARY ** 3, ARY ** 3 + 1]

NREQ_A = [1, 2, 3, 4, 5, 255, 256, 257, 1023, 1024, 1025, 2047, 2048, 2049, 3073]
SPANS_C = [0, 1, GS - 1, GS, GS + 1]
ORDER_AT = [1, 2, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 2099]
NREQ_F = [700, 2500, 1024, 4100, 1025]  # 1, 3, 1, 5 and 2 workgroups
NSEP_G = [1, 2, 3, 4, 5, 9]

# family b, first case: req[i] == req[i - 1] at these i, by the source the
# kernel reads req[i - 1] from
REPEATS_B = {
    "thread": [5, 10, 15, 1101, 2090],   # i % 4 in {1, 2, 3}: the thread's own register
    "lane": [8, 252, 1292],              # i % 4 == 0, i % 256 != 0: lane - 1's last key
    "wave": [256, 512, 768, 1280],       # i % 256 == 0, i % 1024 != 0: wlast[w - 1]
    "workgroup": [1024, 2048],           # i % 1024 == 0: `before`
    "triple": [1024, 1025],              # req[1023] == req[1024] == req[1025]
    "absent_wave": [1536],               # an absent key repeated across a wave seam
}
NREQ_B = 2100
B2_COPIES, B2_TAIL = 1030, 10


# ------------------------------------------------------------------ values --
def even_keys(seed, n):
    """n sorted distinct even keys below 2^62 (key + 1 is never a key)."""
    k = np.unique((splitmix64(seed, n + n // 8 + 16) >> np.uint64(3)) << np.uint64(1))
    assert k.size >= n
    return np.ascontiguousarray(k[:n])


def progression(n, base=1000, step=3):
    """base + step * [0, n): key - 1 and key + 1 are absent."""
    return np.uint64(base) + np.uint64(step) * np.arange(n, dtype=np.uint64)


def special_bits(dtype):
    """-0.0, +inf, -inf and a quiet NaN with a payload, as bit patterns."""
    if np.dtype(dtype) == np.float32:
        return np.array([0x80000000, 0x7F800000, 0xFF800000, 0x7FC00123], np.uint32)
    return np.array([0x8000000000000000, 0x7FF0000000000000, 0xFFF0000000000000,
                     0x7FF8000000000123], np.uint64)


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32 if a.dtype.itemsize == 4 else np.uint64)


def plant(W, D, req):
    """Write the four special values into W at positions the request hits
    (spread over the hit positions, first hit first, so a request with one
    present key reads -0.0)."""
    if D.size == 0:
        return
    req = np.unique(np.asarray(req, np.uint64))
    p = np.searchsorted(D, req).clip(0, D.size - 1)
    hit = p[D[p] == req]
    sp = special_bits(W.dtype)
    if hit.size:
        at = hit[:: max(1, hit.size // sp.size)][: sp.size]
        bits(W)[at] = sp[: at.size]


def values(D, req, dtype, seed=1):
    """Standard-normal W over D with the special values planted for req."""
    W = np.random.default_rng(seed).standard_normal(D.size).astype(dtype)
    plant(W, D, req)
    return W


def spans(D, req):
    """Per workgroup of GR requests: upper_bound(last) - lower_bound(first)."""
    out = []
    for r0 in range(0, req.size, GR):
        r1 = min(req.size, r0 + GR)
        lo = int(np.searchsorted(D, req[r0], "left"))
        hi = int(np.searchsorted(D, req[r1 - 1], "right"))
        out.append(max(hi, lo) - lo)
    return out


def numpy_gather(D, W, req):
    """The rule in NumPy: the first occurrence of a present key reads W,
    everything else +0.0; matched counts the distinct present keys."""
    out = np.zeros(req.size, W.dtype)
    if D.size == 0 or req.size == 0:
        return out, 0
    p = np.searchsorted(D, req).clip(0, D.size - 1)
    first = np.ones(req.size, bool)
    first[1:] = req[1:] != req[:-1]
    take = (D[p] == req) & first
    out[take] = W[p[take]]
    return out, int(take.sum())


def _mixed(D, a, b, n, seed, present_first=True, present_last=True):
    """n sorted distinct requests over positions [a, b] of even-gapped D:
    positions a and b always, the rest drawn from between them; every third
    one is made absent (key + 1), the ends as the flags say."""
    assert b - a - 1 >= n - 2 >= 0
    order = np.argsort(splitmix64(seed, b - a - 1), kind="stable")[: n - 2]
    pos = np.concatenate([[a], np.sort(order) + a + 1, [b]]).astype(np.int64)
    req = D[pos].copy()
    absent = np.arange(n) % 3 == 2
    absent[0], absent[-1] = not present_first, not present_last
    req[absent] += np.uint64(1)
    return req


# ------------------------------------------------- a. request-count seams --
def family_a(dtype):
    D = even_keys(11, ND)
    cases = []
    for nreq in NREQ_A:
        # the last request is absent where no interior one can be
        req = (_mixed(D, 7, ND - 9, nreq, 100 + nreq, present_last=nreq > 3) if nreq > 1
               else D[4321:4322].copy())
        cases.append(("a_nreq%d" % nreq, D, values(D, req, dtype, nreq), req))
    return cases


# --------------------------------------------------------- b. repeat seams --
def repeat_request():
    """(D, req) of the first case of family b."""
    D = even_keys(12, ND)
    pos = np.sort(np.argsort(splitmix64(120, ND), kind="stable")[:NREQ_B])
    req = D[pos].copy()
    rep = sorted({i for v in REPEATS_B.values() for i in v})
    keep = set(rep) | {i - 1 for i in rep}
    for t in range(3, NREQ_B, 7):  # absent keys away from the repeats
        if t not in keep:
            req[t] += np.uint64(1)
    t = REPEATS_B["absent_wave"][0]
    req[t - 1] += np.uint64(1)
    for i in rep:  # ascending: a triple copies twice
        req[i] = req[i - 1]
    return D, req


def family_b(dtype):
    D, req = repeat_request()
    D2 = even_keys(13, ND)
    req2 = np.concatenate([np.full(B2_COPIES, D2[9000], np.uint64),
                           D2[9001:9001 + 40:4][:B2_TAIL]])
    return [("b_seams", D, values(D, req, dtype, 2), req),
            ("b_one_key_workgroup", D2, values(D2, req2, dtype, 3), req2)]


# -------------------------------------------------------- c. staging seams --
C_STEP = 1 << 20  # gaps hold more than GR absent keys


def staging_keys():
    return np.uint64(1 << 30) + np.uint64(C_STEP) * np.arange(ND, dtype=np.uint64)


def family_c(dtype):
    D = staging_keys()
    s = 5000
    one = np.arange(1, GR, dtype=np.uint64)
    reqs = [
        ("c_span0_gap", D[s] + np.arange(1, GR + 1, dtype=np.uint64)),
        ("c_span0_below", D[0] - np.uint64(2 * GR) + np.arange(GR, dtype=np.uint64)),
        ("c_span0_above", D[-1] + np.arange(1, GR + 1, dtype=np.uint64)),
        # one key: absent requests below it, then the key; or the key, then key + 1
        ("c_span1_keys", np.concatenate([D[s] - one[::-1], D[s:s + 1]])),
        ("c_span1_absent_top", np.concatenate([D[s] - one[:0:-1], D[s:s + 1],
                                               D[s:s + 1] + np.uint64(1)])),
    ]
    for n in SPANS_C[2:]:
        reqs.append(("c_span%d_keys" % n, _mixed(D, s, s + n - 1, GR, 300 + n)))
        top = _mixed(D, s, s + n - 1, GR - 1, 400 + n)
        reqs.append(("c_span%d_absent_top" % n,
                     np.concatenate([top, top[-1:] + np.uint64(1)])))
    # one launch: a sparse workgroup (global search), then spans of GS (staged)
    # and GS + 1 (global)
    a = 10_000
    reqs.append(("c_three_workgroups", np.concatenate([
        _mixed(D, 3, a - 5, GR, 501), _mixed(D, a, a + GS - 1, GR, 502),
        _mixed(D, a + GS, a + 2 * GS, GR, 503)])))
    return [(name, D, values(D, r, dtype, 4 + i), np.ascontiguousarray(r, np.uint64))
            for i, (name, r) in enumerate(reqs)]


C_SPANS = {"c_span0_gap": [0], "c_span0_below": [0], "c_span0_above": [0],
           "c_span1_keys": [1], "c_span1_absent_top": [1],
           "c_three_workgroups": [None, GS, GS + 1]}  # None: far above GS
for _n in SPANS_C[2:]:
    C_SPANS["c_span%d_keys" % _n] = C_SPANS["c_span%d_absent_top" % _n] = [_n]


# ------------------------------------- d. server sizes of the 64-ary search --
def search_request(D):
    """The request of family d for server keys D (python-int arithmetic)."""
    want = {0, U64_MAX}
    if D.size:
        want |= {int(D[0]) - 1, int(D[0]), int(D[min(1, D.size - 1)]), int(D[-1]), int(D[-1]) + 1}
    for p in list(range(ARY - 2, ARY + 2)) + list(range(GS - 2, GS + 2)) + [D.size // 2]:
        if p < D.size:
            want |= {int(D[p]) - 1, int(D[p]), int(D[p]) + 1}
    return np.array(sorted(k for k in want if 0 <= k <= U64_MAX), np.uint64)


def family_d(dtype):
    cases = []
    for nd in D_SIZES:
        D = progression(nd)
        req = search_request(D)
        cases.append(("d_nd%d" % nd, D, values(D, req, dtype, 20), req))
    Dz = np.concatenate([[np.uint64(0)], progression(GS)])
    Dm = np.concatenate([progression(GS), [np.uint64(U64_MAX)]])
    for name, D in (("d_key_zero", Dz), ("d_key_max", Dm)):
        req = search_request(D)
        cases.append((name, D, values(D, req, dtype, 21), req))
    return cases


# ----------------------------------------------------------- e. order seams --
def family_e(dtype):
    """(name, D, W, req, i, kind): kind "swap" has req[i - 1] and req[i]
    exchanged (one inversion), kind "equal" has req[i] = req[i - 1]."""
    D = even_keys(14, ND)
    base = D[np.sort(np.argsort(splitmix64(140, ND), kind="stable")[:NREQ_B])]
    W = values(D, base, dtype, 5)
    cases = []
    for i in ORDER_AT:
        swap = base.copy()
        swap[[i - 1, i]] = swap[[i, i - 1]]
        cases.append(("e_swap%d" % i, D, W, swap, i, "swap"))
        eq = base.copy()
        eq[i] = eq[i - 1]
        cases.append(("e_equal%d" % i, D, W, eq, i, "equal"))
    return cases


# ------------------------------------------------- f. matched-word sequence --
def family_f(dtype):
    D = even_keys(15, ND)
    reqs = [_mixed(D, 11 + j, ND - 13 - j, nreq, 600 + j) for j, nreq in enumerate(NREQ_F)]
    W = values(D, reqs[0], dtype, 6)  # one value array for the whole sequence
    for r in reqs[1:]:
        plant(W, D, r)
    return [("f_%d_nreq%d" % (j, r.size), D, W, r) for j, r in enumerate(reqs)]


# ----------------------------------------------------------- g. slice seams --
def family_g():
    """(name, D, kb, ke, sep): psg_slice_dev's inputs."""
    cases = []
    for ni, n in enumerate(D_SIZES):
        D = progression(n)
        full = (0, U64_MAX)
        if n >= 4:
            inner = (int(D[n // 4]) + 1, int(D[3 * n // 4]) + 1)
        else:
            inner = (1001, 1002 + 3 * n)  # between and around the keys there are
        for ri, (kb, ke) in enumerate((full, inner)):
            key = int(D[n // 2]) if n else 1000
            pool = [0, max(0, kb - 31), kb, key, key + 1, ke, min(U64_MAX, ke + 31), U64_MAX]
            for si, nsep in enumerate(NSEP_G):
                off = ni + 3 * ri + 5 * si
                sep = sorted(pool[(off + 3 * j) % len(pool)] for j in range(nsep))
                cases.append(("g_n%d_nsep%d_%s" % (n, nsep, "full" if ri == 0 else "inner"),
                              D, kb, ke, np.array(sep, np.uint64)))
    return cases
