"""CPU: the blocked summation order B of include/psg.h (PSG_SUM_BLOCKED),
restated in numpy here, against the host twin psg_sum_blocked_host.

Bit for bit on sums whose bits depend on the order; where the restatement
gives a NaN the twin must, and payloads are not compared.  The distance to
the exact sum is held to the derived bound gamma_{h+1} * sum |t|, h = 70 per
level (64 chain adds and 6 tree adds), gamma_k = k u / (1 - k u), u = 2^-53."""
import ctypes as C
import math

import numpy as np
import pytest

import worker_ref as R
from parameter_server_amd import _lib

pytestmark = pytest.mark.filterwarnings("ignore:invalid value:RuntimeWarning")  # inf - inf

SERIAL, LANES, SEG = 32, 64, 4096


def _tree(p):  # p[..., j] += p[..., j + d] for j < d, d = 32 .. 1
    d = LANES // 2
    while d:
        p[..., :d] = p[..., :d] + p[..., d:2 * d]
        d //= 2
    return p[..., 0]


def _partials(rows):  # rows [..., steps, 64]: every lane's ((+0.0 + t[j]) + t[j + 64]) + ...
    zero = np.zeros(rows.shape[:-2] + (1, LANES))
    return np.add.accumulate(np.concatenate([zero, rows], axis=-2), axis=-2)[..., -1, :]


def blocked_sum(t):
    """B(t) as include/psg.h states it."""
    t = np.asarray(t, np.float64)
    n = t.size
    if n <= SERIAL:
        return np.add.accumulate(np.concatenate([[0.0], t]))[-1]
    if n <= SEG:
        full = n // LANES
        p = _partials(t[:full * LANES].reshape(full, LANES))
        p[:n - full * LANES] += t[full * LANES:]  # the lanes that have one more term
        return _tree(p)
    k = n // SEG  # the full segments at once, then the last one
    q = _tree(_partials(t[:k * SEG].reshape(k, SEG // LANES, LANES)))
    if n > k * SEG:
        q = np.append(q, blocked_sum(t[k * SEG:]))
    return blocked_sum(q)


def host_twin(t, stride=1, n=None):
    t = np.ascontiguousarray(t, np.float64)
    out = C.c_double()
    n = t.size // stride if n is None else n
    _lib.check(_lib.lib().psg_sum_blocked_host(t.ctypes.data_as(C.c_void_p), n, stride,
                                               C.byref(out)))
    return out.value


def same_sum(got, want):
    return got != got if want != want else \
        np.float64(got).view(np.uint64) == np.float64(want).view(np.uint64)


LENGTHS = (0, 1, 32, 33, 63, 64, 65, 127, 128, 129, 4095, 4096, 4097, 4096 + 32, 4096 + 33,
           2 * 4096, 2 * 4096 + 1, 33 * 4096 + 5, 4096 ** 2 + 1)


@pytest.mark.parametrize("n", LENGTHS)
def test_host_twin_is_the_blocked_order(n):
    rng = np.random.default_rng(n + 7)
    t = R.sensitive_values(rng, n)
    want = blocked_sum(t)
    assert same_sum(host_twin(t), want)
    # within the derived bound of the exact sum
    levels = 1 if n <= SEG else 2 if n <= SEG ** 2 else 3
    k = (70 * levels + 1) * 2.0 ** -53
    assert abs(want - math.fsum(t)) <= k / (1 - k) * math.fsum(np.abs(t))
    # +-0.0 and infinities of one sign among the terms, then one of the other sign: NaN
    if n >= 4:
        at = rng.choice(n, size=min(n, 9), replace=False)
        t[at[0::3]], t[at[1::3]], t[at[2::3]] = 0.0, -0.0, math.inf if n % 2 else -math.inf
        assert same_sum(host_twin(t), blocked_sum(t))
        t[at[3 % at.size]] = -t[at[2]]
        want = blocked_sum(t)
        assert want != want and same_sum(host_twin(t), want)


def test_host_twin_strides_and_signed_zero():
    """One column of a row array; and +0.0 + -0.0 = +0.0 under every rule."""
    t = R.sensitive_values(np.random.default_rng(3), 3 * 4200)
    for j in range(3):
        assert same_sum(host_twin(t[j:], stride=3, n=4200), blocked_sum(t[j::3]))
    for n in (1, 32, 33, 5000):
        assert same_sum(host_twin(np.full(n, -0.0)), 0.0)
