"""GPU: the pull path at its seams -- gather_block (behind psg_gather,
psg_gather_dev and psg_pull_dev), pull_kernel's matched word,
check_sorted_kernel and slice_kernel of psg_kernels.hip, and the 64-ary
wave_search of psg_device.h under all of them.

The inputs come from tests/pull_inputs.py, which puts each repeat, inversion,
span length and search length on a chosen seam; tests/test_pull_inputs.py
proves on the CPU that they sit there.  Every expected value comes from the
oracle (oracle_py.gather, oracle_py.slice_key_ordered), never from the
library, and every comparison is on bits or on integer counts: a gather moves
values and adds nothing, so no tolerance applies, and -0.0, the infinities
and a NaN's payload must arrive as stored while an absent or repeated request
reads +0.0.

Device outputs are allocated GUARD elements longer than the request and
prefilled with a sentinel bit pattern; the guard must still hold it after the
call."""
import functools

import numpy as np
import pytest
import torch

import oracle_py as O
import pull_inputs as P
from parameter_server_amd import _lib
from parameter_server_amd.kv_vector import KVVector, Message

pytestmark = pytest.mark.gpu

GUARD = 8
SENTINEL = {4: 0xA5A5A5A5, 8: 0xA5A5A5A5A5A5A5A5}
GARBAGE = 0x0123456789ABCDEF  # a matched word before psg_pull_dev sets it
DTYPES = (np.float32, np.float64)
FAMILIES = {"a": P.family_a, "b": P.family_b, "c": P.family_c, "d": P.family_d,
            "f": P.family_f}


def psg_dtype(dtype):
    return _lib.PSG_F32 if dtype == np.float32 else _lib.PSG_F64


def signed(x, size):
    return int(np.array([x], np.uint32 if size == 4 else np.uint64)
               .view(np.int32 if size == 4 else np.int64)[0])


def to_dev(a):
    """A host array's bits in device memory; an empty one becomes one valid
    element, so that no entry point is handed a null pointer."""
    a = np.ascontiguousarray(a)
    if a.size == 0:
        return torch.zeros(1, dtype=torch.int64, device="cuda:0")
    v = a.view(np.int32 if a.dtype.itemsize == 4 else np.int64)
    return torch.from_numpy(v.copy()).to("cuda:0")


def guarded(n, size):
    """n + GUARD elements of `size` bytes, every one the sentinel."""
    return torch.full((n + GUARD,), signed(SENTINEL[size], size),
                      dtype=torch.int32 if size == 4 else torch.int64, device="cuda:0")


def host_bits(t):
    a = t.cpu().numpy()
    return a.view(np.uint32 if a.dtype.itemsize == 4 else np.uint64)


def assert_guarded(buf, want_bits, name):
    got = host_bits(buf)
    n = want_bits.size
    bad = np.flatnonzero(got[:n] != want_bits)
    assert bad.size == 0, "%s: %d wrong, first at %d: got %#x, want %#x" % (
        name, bad.size, bad[0], got[bad[0]], want_bits[bad[0]])
    assert np.all(got[n:] == SENTINEL[got.dtype.itemsize]), name + ": wrote past the request"


def word(value=GARBAGE):
    return torch.full((1,), signed(value, 8), dtype=torch.int64, device="cuda:0")


def word_value(t):
    return int(host_bits(t)[0])


def stream():
    return torch.cuda.current_stream().cuda_stream


def status_of(fn):
    try:
        fn()
    except _lib.PSGError as e:
        return e.status
    return _lib.PSG_OK


@functools.lru_cache(maxsize=None)
def expected(family, dtype):
    """[(name, D, W, req, oracle bits, oracle matched)], computed once."""
    out = []
    for name, D, W, req in FAMILIES[family](dtype):
        want, matched = O.gather(D, W, req, dtype)
        out.append((name, D, W, req, P.bits(want).copy(), matched))
    return out


class Server:
    """One context; every distinct server key set on a channel of its own."""

    def __init__(self, dtype):
        self.v = KVVector(0, psg_dtype(dtype))
        self.channels = {}

    def channel(self, D, W):
        if id(D) not in self.channels:
            self.channels[id(D)] = len(self.channels)
            self.v.setValue(Message(key=D, key_channel=self.channels[id(D)]))
        ch = self.channels[id(D)]
        self.v.set_value_array(ch, W)
        return ch

    def close(self):
        self.v.close()


# ------------------------------------- 1. families a to d, three entry points --
@pytest.mark.parametrize("dtype", DTYPES, ids=("f32", "f64"))
@pytest.mark.parametrize("family", ("a", "b", "c", "d"))
def test_gather_seams(family, dtype):
    L = _lib.lib()
    size = np.dtype(dtype).itemsize
    srv = Server(dtype)
    try:
        for name, D, W, req, want, matched in expected(family, dtype):
            ch = srv.channel(D, W)
            # psg_gather
            msg = Message(key=req, key_channel=ch)
            assert srv.v.getValue(msg) == matched, name
            assert np.array_equal(P.bits(msg.value[0]), want), name + ": psg_gather"
            # psg_gather_dev: matched is added to
            dD, dW, dreq = to_dev(D), to_dev(W), to_dev(req)
            out, cnt = guarded(req.size, size), word(0)
            _lib.check(L.psg_gather_dev(psg_dtype(dtype), dD.data_ptr(), D.size, dW.data_ptr(),
                                        dreq.data_ptr(), req.size, out.data_ptr(),
                                        cnt.data_ptr(), stream()))
            torch.cuda.synchronize()
            assert_guarded(out, want, name + ": psg_gather_dev")
            assert word_value(cnt) == matched, name + ": psg_gather_dev"
            # psg_pull_dev: matched is set
            out, cnt = guarded(req.size, size), word()
            srv.v.pull_dev(ch, dreq.data_ptr(), req.size, out.data_ptr(), cnt.data_ptr(),
                           stream=stream())
            torch.cuda.synchronize()
            assert_guarded(out, want, name + ": psg_pull_dev")
            assert word_value(cnt) == matched, name + ": psg_pull_dev"
        assert status_of(srv.v.dev_status) == _lib.PSG_OK
    finally:
        srv.close()


# ------------------------------------------------------------ 2. order seams --
@pytest.mark.parametrize("dtype", DTYPES, ids=("f32", "f64"))
def test_order_seams(dtype):
    size = np.dtype(dtype).itemsize
    srv = Server(dtype)
    try:
        for name, D, W, req, i, kind in P.family_e(dtype):
            ch = srv.channel(D, W)
            dreq = to_dev(req)
            out, cnt = guarded(req.size, size), word()
            msg = Message(key=req, key_channel=ch)
            matched = []
            rc = status_of(lambda: matched.append(srv.v.getValue(msg)))
            srv.v.pull_dev(ch, dreq.data_ptr(), req.size, out.data_ptr(), cnt.data_ptr(),
                           stream=stream())
            first, second = status_of(srv.v.dev_status), status_of(srv.v.dev_status)
            if kind == "swap":  # one inversion, at i
                assert rc == _lib.PSG_ERR_UNSORTED, name + ": psg_gather"
                assert first == _lib.PSG_ERR_UNSORTED, name + ": psg_pull_dev"
                assert second == _lib.PSG_OK, name + ": reported twice"
            else:  # req[i] == req[i - 1]: legal, and the repeat reads +0.0
                assert (rc, first, second) == (_lib.PSG_OK,) * 3, name
                want, wm = O.gather(D, W, req, dtype)
                assert P.bits(want)[i] == 0 and P.bits(want)[i - 1] != 0, name
                assert matched == [wm] and word_value(cnt) == wm, name
                assert np.array_equal(P.bits(msg.value[0]), P.bits(want)), name + ": psg_gather"
                torch.cuda.synchronize()
                assert_guarded(out, P.bits(want), name + ": psg_pull_dev")
    finally:
        srv.close()


# --------------------------------------------------- 3. matched-word sequence --
@pytest.mark.parametrize("dtype", DTYPES, ids=("f32", "f64"))
def test_matched_word_sequence(dtype):
    """Launches of 1, 3, (3 without a matched word,) 1, 5 and 2 workgroups
    back to back on one channel, twice: the ticket counter and the sum are
    left zero by every launch, so every word is its own request's count."""
    size = np.dtype(dtype).itemsize
    cases = expected("f", dtype)
    counts = [c[5] for c in cases]
    assert len(set(counts)) == len(counts)
    order = [0, 1, 1, 2, 3, 4]
    with_word = [True, True, False, True, True, True]
    srv = Server(dtype)
    try:
        ch = srv.channel(cases[0][1], cases[0][2])
        dreq = [to_dev(c[3]) for c in cases]
        issued = []
        for _ in range(2):
            for j, has in zip(order, with_word):
                n = cases[j][3].size
                out, cnt = guarded(n, size), word()
                srv.v.pull_dev(ch, dreq[j].data_ptr(), n, out.data_ptr(),
                               cnt.data_ptr() if has else None, stream=stream())
                issued.append((j, has, out, cnt))
        torch.cuda.synchronize()
        for at, (j, has, out, cnt) in enumerate(issued):
            name = "launch %d (%s)" % (at, cases[j][0])
            assert word_value(cnt) == (cases[j][5] if has else GARBAGE), name
            assert_guarded(out, cases[j][4], name)
        assert status_of(srv.v.dev_status) == _lib.PSG_OK
    finally:
        srv.close()


# ------------------------------------------------------------ 4. slice seams --
def test_slice_seams():
    L = _lib.lib()
    dD, of = None, None
    done = set()
    for name, D, kb, ke, sep in P.family_g():
        if of is not D:
            dD, of = to_dev(D), D
        dsep, pos = to_dev(sep), guarded(sep.size, 8)
        _lib.check(L.psg_slice_dev(dD.data_ptr(), D.size, kb, ke, dsep.data_ptr(), sep.size,
                                   pos.data_ptr(), stream()))
        torch.cuda.synchronize()
        want, _ = O.slice_key_ordered(D, kb, ke, sep)
        assert_guarded(pos, want, name)
        done.add((D.size, sep.size, kb == 0))
    assert len(done) == len(P.D_SIZES) * len(P.NSEP_G) * 2
