"""GPU: row-valued pushes (RowMergePlan, gather_rows_dev) bit for bit against
the oracle applied column by column: column c of a fold of rows is
oracle_py.aggregate of the m = 1 pushes (keys, rows[:, c]), sums and matched
counts, in serial and parallel mode.  Shapes sit on the seams rows_shape gives."""
import numpy as np
import pytest

import oracle_py as O
from test_gpu_parity import assert_bitexact, torch_cuda  # noqa: F401

from parameter_server_amd import _lib
from parameter_server_amd.kv_vector import MergePlan, RowMergePlan, gather_rows_dev, rows_shape

pytestmark = pytest.mark.gpu
ALL = (0, (1 << 64) - 1)
F32, F64 = np.float32, np.float64
GUARD = 7.0


def psg_dtype(dtype):
    return _lib.PSG_F32 if dtype == F32 else _lib.PSG_F64


def max_width():
    return _lib.lib().psg_rows_max_width()


WIDTHS = [(F32, 1), (F32, 3), (F32, 4), (F32, 16), (F32, 65), (F64, 2), (F64, 5), (F32, None),
          (F64, None)]  # None: the widest row
WIDTH_IDS = ["%s-%s" % (np.dtype(d).name, k or "max") for d, k in WIDTHS]


def server_keys(rng, n):
    """n sorted keys with room between, below and above them."""
    return (np.sort(rng.choice(1 << 20, n, replace=False)).astype(np.uint64) + 1) * 4


def rows_of(rng, n, k, dtype):
    """5 % of the values -0.0; the first row holds NaN and both infinities."""
    r = rng.standard_normal((n, k)).astype(dtype)
    r[rng.random((n, k)) < 0.05] = -0.0
    if n:
        r[0, :3] = np.array([np.nan, np.inf, -np.inf], dtype)[: min(k, 3)]
    return r


def push_of(rng, D, slots, k, dtype):
    slots = np.unique(np.asarray(slots, np.int64))
    return D[slots], rows_of(rng, slots.size, k, dtype)


def run_plan(torch, jobs, k, dtype, parallel, offset=0):
    """jobs: [(D, [(keys, rows)])].  Returns (plan, [out tensors], device
    inputs); every out has a guard row behind it, rows and out start `offset`
    elements past a 16-B boundary."""
    tdt = torch.float32 if dtype == F32 else torch.float64
    dev, spec, outs = [], [], []
    for D, pushes in jobs:
        dD = torch.from_numpy(D.view(np.int64)).cuda()
        dk = [torch.from_numpy(np.ascontiguousarray(s).view(np.int64)).cuda() for s, _ in pushes]
        dr = [torch.empty(r.size + offset, dtype=tdt, device="cuda")[offset:] for _, r in pushes]
        for t, (_, r) in zip(dr, pushes):
            t.copy_(torch.from_numpy(r.reshape(-1)))
        out = torch.full(((D.size + 1) * k + offset,), GUARD, dtype=tdt, device="cuda")[offset:]
        dev.append((dD, dk, dr))
        outs.append(out)
        spec.append(dict(keys=dD.data_ptr(), nslots=D.size, push_keys=[t.data_ptr() for t in dk],
                         push_rows=[t.data_ptr() for t in dr], push_n=[s.size for s, _ in pushes],
                         out=out.data_ptr()))
    plan = RowMergePlan(0, psg_dtype(dtype), k, spec, parallel)
    plan.run(torch.cuda.current_stream().cuda_stream)
    return plan, outs, dev


def assert_oracle(torch, plan, outs, jobs, k, dtype, parallel):
    got_m = plan.matched()
    torch.cuda.synchronize()
    at = 0
    for (D, pushes), out in zip(jobs, outs):
        got = out.cpu().numpy().reshape(D.size + 1, k)
        assert np.all(got[D.size] == GUARD), "written past out"
        for c in range(k):
            _, _, _, want, wm = O.aggregate(D, *ALL, [(s, [r[:, c]]) for s, r in pushes],
                                            parallel=parallel, dtype=dtype)
            assert_bitexact(got[: D.size, c], want[0] if pushes else np.zeros(D.size, dtype))
            assert np.array_equal(got_m[at: at + len(pushes)], wm), "matched, column %d" % c
        at += len(pushes)


def check(torch, jobs, k, dtype, offset=0):
    for parallel in (False, True):
        plan, outs, _ = run_plan(torch, jobs, k, dtype, parallel, offset)
        assert_oracle(torch, plan, outs, jobs, k, dtype, parallel)
        plan.close()


@pytest.mark.parametrize("dtype,k", WIDTHS, ids=WIDTH_IDS)
def test_widths_and_types(torch_cuda, dtype, k):
    k = k or max_width()
    T = rows_shape(psg_dtype(dtype), k)[0]
    rng = np.random.default_rng(k)
    D = server_keys(rng, T + 5)
    pushes = [push_of(rng, D, rng.choice(D.size, D.size * 2 // 3, replace=False), k, dtype)
              for _ in range(3)]
    check(torch_cuda, [(D, pushes)], k, dtype)
    if k == 1:  # today's scalar plan
        torch = torch_cuda
        plan, outs, (dev,) = run_plan(torch, [(D, pushes)], 1, dtype, False)
        old = torch.empty(D.size, dtype=outs[0].dtype, device="cuda")
        mp = MergePlan(0, psg_dtype(dtype), 1, [dict(
            keys=dev[0].data_ptr(), nslots=D.size, push_keys=[t.data_ptr() for t in dev[1]],
            push_vals=[[t.data_ptr()] for t in dev[2]], push_n=[s.size for s, _ in pushes],
            out=[old.data_ptr()])])
        mp.run(torch.cuda.current_stream().cuda_stream)
        assert np.array_equal(mp.matched(), plan.matched())
        assert_bitexact(outs[0].cpu().numpy()[: D.size], old.cpu().numpy())


def seam_pushes(rng, D, T, N, k, dtype):
    """N pushes over D whose keys sit on the tile seams (slots 0, T - 1, T and
    the last): N = 1 a subset; N = 2 a subset, then every key; N = 9 also an
    empty push, one inside the first tile, one with no key in the middle tile."""
    n = D.size
    seams = [s for s in (0, T - 1, T, n - 1) if s < n]
    sub = lambda: np.concatenate([seams, rng.choice(n, (n + 2) // 3, replace=False)])  # noqa: E731
    every = np.arange(n)
    mid = (n - 1) // T // 2
    slots = {1: [sub()], 2: [sub(), every],
             9: [sub(), np.zeros(0, np.int64), rng.choice(min(n, T), min(n, 5), replace=False),
                 every[every // T != mid] if n > T else sub(), every] + [sub() for _ in range(4)]}[N]
    return [push_of(rng, D, s, k, dtype) for s in slots]


@pytest.mark.parametrize("N", (1, 2, 9))
@pytest.mark.parametrize("a,b", ((0, 1), (1, -1), (1, 0), (1, 1), (3, 7)),
                         ids=("1", "T-1", "T", "T+1", "3T+7"))
def test_tile_seams(torch_cuda, a, b, N):
    dtype, k = F32, 64  # T = 256: four tiles at 3T + 7
    T = rows_shape(psg_dtype(dtype), k)[0]
    n = a * T + b
    rng = np.random.default_rng(1000 * N + n)
    D = server_keys(rng, n)
    check(torch_cuda, [(D, seam_pushes(rng, D, T, N, k, dtype))], k, dtype)


@pytest.mark.parametrize("dtype,k", ((F32, 16), (F64, 4)), ids=("f32-16", "f64-4"))
def test_base_pointers_off_by_one_element(torch_cuda, dtype, k):
    T = rows_shape(psg_dtype(dtype), k)[0]
    rng = np.random.default_rng(5)
    D = server_keys(rng, T + 9)
    check(torch_cuda, [(D, seam_pushes(rng, D, T, 2, k, dtype))], k, dtype, offset=1)


def test_unmatched_keys(torch_cuda):
    dtype, k = F32, 16
    T = rows_shape(psg_dtype(dtype), k)[0]
    rng = np.random.default_rng(6)
    D = server_keys(rng, T + 3)
    S, R = push_of(rng, D, rng.choice(D.size, 200, replace=False), k, dtype)
    extra = np.array([1, D[T - 1] + 1, D[T] + 2, D[-1] + 1], np.uint64)  # below, between, above
    keys = np.sort(np.concatenate([S, extra]))
    rows = rows_of(rng, keys.size, k, dtype)
    rows[np.isin(keys, S)] = R
    check(torch_cuda, [(D, [(S, R), (keys, rows), (extra, rows[: extra.size])])], k, dtype)


def test_plan_state_two_jobs_rerun(torch_cuda):
    torch, dtype, k = torch_cuda, F64, 5
    T = rows_shape(psg_dtype(dtype), k)[0]
    rng = np.random.default_rng(7)
    sizes = (T + 11, 40)
    jobs = [(server_keys(rng, n), None) for n in sizes]
    pick = [[rng.choice(n, n // 2, replace=False) for _ in range(3)] for n in sizes]
    first = [(D, [push_of(rng, D, s, k, dtype) for s in sl]) for (D, _), sl in zip(jobs, pick)]
    plan, outs, dev = run_plan(torch, first, k, dtype, False)
    assert_oracle(torch, plan, outs, first, k, dtype, False)
    # other keys (of the same counts) and other rows in the same buffers
    again = [(D, [push_of(rng, D, rng.choice(D.size, s.size, replace=False), k, dtype) for s in sl])
             for (D, _), sl in zip(jobs, pick)]
    for (_, dk, dr), (_, pushes) in zip(dev, again):
        for tk, tr, (s, r) in zip(dk, dr, pushes):
            tk.copy_(torch.from_numpy(s.view(np.int64)))
            tr.copy_(torch.from_numpy(r.reshape(-1)))
    plan.run(torch.cuda.current_stream().cuda_stream)
    assert_oracle(torch, plan, outs, again, k, dtype, False)
    plan.close()


def gather(torch, D, W, req, k, dtype, scalar=False):
    """gather_rows_dev, or (scalar) one psg_gather_dev per column: (rows, matched)."""
    tdt = torch.float32 if dtype == F32 else torch.float64
    dD, dreq = (torch.from_numpy(a.view(np.int64)).cuda() for a in (D, req))
    cnt = torch.zeros(1, dtype=torch.int64, device="cuda")
    st = torch.cuda.current_stream().cuda_stream
    if not scalar:
        dW = torch.from_numpy(W).cuda()
        out = torch.full(((req.size + 1) * k,), GUARD, dtype=tdt, device="cuda")
        gather_rows_dev(psg_dtype(dtype), k, dD.data_ptr(), D.size, dW.data_ptr(), dreq.data_ptr(),
                        req.size, out.data_ptr(), cnt.data_ptr(), st)
        got = out.cpu().numpy().reshape(req.size + 1, k)
        assert np.all(got[req.size] == GUARD), "written past out"
        return got[: req.size], int(cnt.item())
    cols = []
    for c in range(k):
        dW = torch.from_numpy(np.ascontiguousarray(W[:, c])).cuda()
        out = torch.empty(req.size, dtype=tdt, device="cuda")
        _lib.check(_lib.lib().psg_gather_dev(psg_dtype(dtype), dD.data_ptr(), D.size, dW.data_ptr(),
                                             dreq.data_ptr(), req.size, out.data_ptr(),
                                             cnt.data_ptr(), st))
        cols.append(out.cpu().numpy())
    return np.stack(cols, 1), int(cnt.item()) // k


@pytest.mark.parametrize("nd", (1, 1000))
@pytest.mark.parametrize("dtype,k", WIDTHS, ids=WIDTH_IDS)
def test_row_gather(torch_cuda, dtype, k, nd):
    k = k or max_width()
    R = rows_shape(psg_dtype(dtype), k)[3]
    rng = np.random.default_rng(100 * k + nd)
    D = server_keys(rng, nd)
    W = rows_of(rng, nd, k, dtype)
    W[-1] = -0.0  # a present row of -0.0 keeps its sign
    for nreq in sorted({0, 1, max(R - 1, 1), R + 1, 1000}):
        present = np.concatenate([D[-1:], rng.choice(D, min(nd, nreq * 2 // 3), replace=False)])
        # about a third absent: between the server keys, and one above them
        absent = np.concatenate([D[rng.integers(0, nd, nreq)], D[-1:]]) + 1
        req = np.unique(np.concatenate([present, absent]))[-nreq:] if nreq else D[:0]
        got, matched = gather(torch_cuda, D, W, req, k, dtype)
        for c in range(k):
            want, wm = O.gather(D, W[:, c], req, dtype)
            assert_bitexact(got[:, c], want)
            assert matched == wm, (nreq, c)
        if nreq > 1:
            assert np.signbit(got[req == D[-1]]).all() and 0 < matched < nreq


def test_row_gather_out_of_order_as_scalar_gather(torch_cuda):
    """psg_gather_dev has no context to report to: an inversion is searched on
    its own and found; a repeat reads +0.0.  The row gather does the same."""
    dtype, k = F32, 4
    rng = np.random.default_rng(9)
    D = server_keys(rng, 1000)
    W = rows_of(rng, D.size, k, dtype)
    req = D[::3].copy()
    req[[100, 101]] = req[[101, 100]]  # one inversion
    req[200] = req[199]                # one repeat
    got, matched = gather(torch_cuda, D, W, req, k, dtype)
    want, wm = gather(torch_cuda, D, W, req, k, dtype, scalar=True)
    assert_bitexact(got, want)
    assert matched == wm == req.size - 1
