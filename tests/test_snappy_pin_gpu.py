"""GPU: the three device snappy decoders (psg_snappy.hip: the table form, the
streamed form it falls back to, the per-wave form of launches of more than 64
parts) on streams made by the real snappy compressor.

The streams are the recorded ones of tests/golden/snappy_pin/*.npz
(tools/record_snappy.py; tests/test_snappy_pin.py checks on the CPU what they
hold and that the oracle decodes them); the expected bytes are the inputs
rebuilt by pin_cases.snappy_cases().  Nothing here loads a snappy library.

Which form decodes a part follows from the launch and from the stream (the
tallies in the fixtures' meta): a launch of <= 64 parts runs the table form,
which hands a part of more than kTabMax = 4096 elements, or of more than
kTabPend = 64 copies that do not reach a literal within kTabDepth = 4 table
look-ups (`table_npend`, pin_cases.snappy_table_npend's host replay of the
kernel's step 2), to the streamed form; a larger launch runs the per-wave
form.  Key and value arrays are copies of copies, so every such real stream
ends in the streamed form; the parts the table form decodes itself are the
single literals, rep2047, rep2048 and `records` (short matches whose sources
are literal data: 349 copy-1 elements with non-zero high offset bits, 17
copies left to the table form's step 3).

psg_snappy_uncompress_dev takes the parts' capacities as consecutive
offsets, so a gap behind a part is a part of its own: an empty stream declared
as 16 bytes, which reports PSG_ERR_SIZE and writes nothing.  The destination
is pre-filled, and every gap and the tail must come back as filled.
"""
import ctypes as C

import numpy as np
import pytest

import oracle_py as O
import pin_cases as P
from test_gpu_parity import kvv, msg, torch_cuda  # noqa: F401

pytestmark = pytest.mark.gpu

FILL, GAP, TAIL = 0xA5, 16, 64
ALONE = ("keys40_le", "keys40_gt", "f32_eighths", "records")
_cache = {}


def recorded():
    """{name: (stream, expected bytes, tally)} in case order; built once, read
    only."""
    if not _cache:
        for name, (c, stream, info) in P.snappy_recorded().items():
            _cache[name] = (stream, c.data, info["tally"])
    return _cache


def lead_part(n):
    """A literal of n <= 60 bytes: n + 2 bytes of stream."""
    data = bytes(range(1, n + 1))
    return bytes([n, (n - 1) << 2]) + data, data


def gpu_snappy(torch, parts, caps, gaps=True):
    """test_wire._gpu_snappy with a pre-filled destination and, with gaps, an
    untouched 16-byte gap part behind every part.  Returns (bytes of each
    part's capacity, status of each part, number of parts launched)."""
    from parameter_server_amd import _lib
    L = _lib.lib()
    if gaps:
        parts = [x for p in parts for x in (p, b"")]
        caps = [x for c in caps for x in (c, GAP)]
    soff = np.concatenate([[0], np.cumsum([len(p) for p in parts])]).astype(np.uint64)
    doff = np.concatenate([[0], np.cumsum(caps)]).astype(np.uint64)
    total = int(doff[-1])
    blob = b"".join(parts) + b"\0"
    ds = torch.tensor(np.frombuffer(blob, np.uint8).copy(), device="cuda")
    dd = torch.full((total + TAIL,), FILL, dtype=torch.uint8, device="cuda")
    dso = torch.tensor(soff.view(np.int64), device="cuda")
    ddo = torch.tensor(doff.view(np.int64), device="cuda")
    st = torch.full((len(parts),), 7, dtype=torch.int32, device="cuda")
    _lib.check(L.psg_snappy_uncompress_dev(ds.data_ptr(), dso.data_ptr(), len(parts),
                                           dd.data_ptr(), ddo.data_ptr(), st.data_ptr(), None))
    torch.cuda.synchronize()
    out = dd.cpu().numpy().tobytes()
    st = st.cpu().tolist()
    assert out[total:] == bytes([FILL]) * TAIL, "the tail behind the last part was written"
    got = [out[int(doff[i]):int(doff[i + 1])] for i in range(len(parts))]
    if gaps:
        for i in range(1, len(parts), 2):
            assert got[i] == bytes([FILL]) * GAP, "the gap behind part %d was written" % (i // 2)
            assert st[i] == _lib.PSG_ERR_SIZE
        got, st = got[0::2], st[0::2]
    return got, st, len(parts)


def assert_decoded(got, st, names):
    R = recorded()
    assert st == [0] * len(names), [(n, s) for n, s in zip(names, st) if s]
    for g, n in zip(got, names):
        want = R[n][1]
        if g != want:
            a, b = np.frombuffer(g, np.uint8), np.frombuffer(want, np.uint8)
            bad = np.nonzero(a != b)[0]
            raise AssertionError("%s: %d bytes differ, the first at %d" % (n, bad.size, bad[0]))


def launch(torch, names, gaps=True, lead=None):
    R = recorded()
    parts, caps = [R[n][0] for n in names], [len(R[n][1]) for n in names]
    if lead is not None:
        ls, ld = lead_part(lead)
        parts, caps = [ls] + parts, [len(ld)] + caps
    got, st, nparts = gpu_snappy(torch, parts, caps, gaps)
    if lead is not None:
        assert st[0] == 0 and got[0] == ld
        got, st = got[1:], st[1:]
    assert_decoded(got, st, names)
    return nparts


def test_table_form_and_its_fallbacks(torch_cuda):
    """Every recorded stream in launches of <= 64 parts: once all in one
    launch, back to back (an overrun would land in the next part), and in two
    launches with a gap behind every part."""
    names = list(recorded())
    assert launch(torch_cuda, names, gaps=False) == len(names) < 64
    half = (len(names) + 1) // 2
    for group in (names[:half], names[half:]):
        assert launch(torch_cuda, group) < 64


def test_per_wave_form(torch_cuda):
    """The same streams twice over in one launch of more than 64 parts, with
    gaps and without."""
    names = list(recorded()) * 2
    assert launch(torch_cuda, names, gaps=False) > 64
    assert launch(torch_cuda, names) > 64


@pytest.mark.parametrize("name", ALONE)
def test_alone_and_off_alignment(torch_cuda, name):
    """The kTabMax pair, the quantised-f32 stream and the stream that the
    table form decodes itself, each alone; then behind a lead part of 1, 7 and
    15 decoded bytes (3, 9 and 17 bytes of stream), so that source and
    destination both start off 16-byte alignment; then the same in a launch
    that the per-wave form takes."""
    assert launch(torch_cuda, [name], gaps=False) == 1
    assert launch(torch_cuda, [name]) == 2
    for lead in (1, 7, 15):
        assert launch(torch_cuda, [name], lead=lead) == 4
        assert launch(torch_cuda, [name] + ["len%d" % n for n in P.SNAPPY_EDGE_LENGTHS] * 4,
                      lead=lead) > 64


def test_corrupt_parts_among_real_streams(torch_cuda):
    """A real key stream cut after its preamble, inside a copy-1, inside a
    literal and one byte short, each between good real streams:
    PSG_ERR_ARG for the cut parts alone.  A capacity one byte too large is
    PSG_ERR_SIZE."""
    torch = torch_cuda
    from parameter_server_amd import _lib
    R = recorded()
    stream, data, _ = R["keys24"]
    cuts = P.snappy_truncations(stream)
    for _, cut in cuts:
        assert O.snappy_uncompress(cut) is None
    good = ["keys24", "records", "keys40_gt", "f32_eighths", "abc"]
    parts, caps, want = [], [], []
    for i, n in enumerate(good):
        parts.append(R[n][0])
        caps.append(len(R[n][1]))
        want.append(n)
        if i < len(cuts):
            parts.append(cuts[i][1])
            caps.append(len(data))  # what its preamble declares
            want.append(None)
    for rep in (1, 4):  # the table form with its fallbacks; the per-wave form
        got, st, nparts = gpu_snappy(torch, parts * rep, caps * rep)
        assert (nparts <= 64) == (rep == 1)
        for g, s, n in zip(got, st, want * rep):
            if n is None:
                assert s == _lib.PSG_ERR_ARG
            else:
                assert s == 0 and g == R[n][1], n
    for rep in (1, 40):
        got, st, nparts = gpu_snappy(torch, [stream] * rep, [len(data) + 1] * rep)
        assert (nparts <= 64) == (rep == 1)
        assert st == [_lib.PSG_ERR_SIZE] * rep


@pytest.mark.parametrize("parallel", [False, True], ids=["serial", "parallel"])
@pytest.mark.parametrize("which", P.SNAPPY_PUSH_NAMES)
def test_push_compressed_real_parts(torch_cuda, which, parallel):
    """psg_push_compressed fed the recorded key and value parts of a push as
    they would arrive: received(t) has the bits of the same pushes sent
    uncompressed and of the oracle's aggregate -- the all-ones sentinel's
    among them.  A push holding a key the server lacks is PSG_ERR_UNMATCHED
    either way."""
    from parameter_server_amd import _lib
    R = recorded()
    c = P.snappy_push(which)
    comp, plain = kvv(c.dtype, parallel), kvv(c.dtype, parallel)
    for v in (comp, plain):
        v.setValue(msg(c.D))

    def cpush(t, p):
        names = c.part_names(p)
        ck = R[names[0]][0]
        cv = [R[n][0] for n in names[1:]]
        bufs = [C.create_string_buffer(b, len(b)) for b in cv]
        arr = _lib.ptr_array([C.cast(b, C.c_void_p).value for b in bufs])
        sizes = (C.c_size_t * len(cv))(*[len(b) for b in cv])
        _lib.check(comp._L.psg_push_compressed(comp._h, 0, t, 0, P.U64, ck, len(ck), len(cv), arr,
                                               sizes))

    clean = [c.pushes[p] for p in c.clean]
    for p in c.clean:
        cpush(1, p)
    for k, vs in clean:
        plain.setValue(msg(k, vs, t=1))
    got, ref = comp.received(1), plain.received(1)
    rc, lo, hi, want, mt = O.aggregate(c.D, 0, P.U64, clean, parallel, 1, c.dtype)
    assert rc == 0 and mt.tolist() == [k.size for k, _ in clean] and len(got) == len(ref) == c.m
    for i in range(c.m):
        assert tuple(got[i][0]) == tuple(ref[i][0]) == (lo, hi)
        assert got[i][1].dtype == c.dtype
        assert np.array_equal(P.fbits(got[i][1]), P.fbits(ref[i][1])), i
        assert np.array_equal(P.fbits(got[i][1]), P.fbits(want[i])), i
    if which == "B":  # the sentinel came through where one push alone holds the key
        sent = np.uint64(P.SENTINEL)
        n_sent = sum(int((P.fbits(vs[0]) == sent).sum()) for _, vs in clean)
        assert n_sent > 1000
        for i in range(c.m):
            assert int((P.fbits(got[i][1]) == sent).sum()) == n_sent
    for p in range(len(c.pushes)):
        if p in c.clean:
            continue
        k, vs = c.pushes[p]
        assert int(O.aggregate(c.D, 0, P.U64, [(k, vs)], parallel, 1, c.dtype)[4][0]) == k.size - 1
        cpush(2, p)
        plain.setValue(msg(k, vs, t=2))
        for v in (comp, plain):
            with pytest.raises(_lib.PSGError) as e:
                v.received(2)
            assert e.value.status == _lib.PSG_ERR_UNMATCHED
    comp.close()
    plain.close()
