"""The snappy encoder's rule on the CPU: psg_snappy_compress_host
(parameter_server_amd/csrc/psg_snappy_enc.cc), the host twin that gives the
device encoder's stream byte for byte (tests/test_snappy_compress_gpu.py holds
the device to it).

Every stream is decoded by the oracle (orc_snappy_uncompress) and by the
installed google snappy (tests/snappy_lib.py; those checks skip only where
the library is absent), and walked element by element: the declared length,
no copy-4, no offset of 65536 or more, nothing across a 64 KB fragment seam.
"""
import json
import os

import pytest

import oracle_py as O
import pin_cases as P
import snappy_enc_inputs as I
from parameter_server_amd import _lib, snappy

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PROFILE = os.path.join(ROOT, "profiles", "snappy_compress.json")
_streams = {}


def twin(name, data):
    """The twin's stream of a named input; computed once, read only."""
    if name not in _streams:
        _streams[name] = snappy.compress_host(data)
    return _streams[name]


@pytest.fixture(scope="module")
def libsnappy():
    from snappy_lib import Snappy
    try:
        return Snappy()
    except OSError as e:
        pytest.skip("no libsnappy on this machine: %s" % e)


def check_valid(stream, data):
    assert len(stream) <= snappy.max_compressed_length(len(data))
    assert O.snappy_uncompress(stream) == data
    return I.check_structure(stream, len(data))


def test_max_compressed_length():
    for n in (0, 1, 5, 6, 65536, 10 ** 9):
        assert snappy.max_compressed_length(n) == 32 + n + n // 6


@pytest.mark.parametrize("name,data", I.all_inputs(), ids=[n for n, _ in I.all_inputs()])
def test_valid_oracle(name, data):
    check_valid(twin(name, data), data)


def test_valid_libsnappy(libsnappy):
    """The real library reads every stream back, and reports the length the
    preamble declares."""
    import ctypes as C
    for name, data in I.all_inputs():
        s = twin(name, data)
        n = C.c_size_t()
        assert libsnappy.lib.snappy_uncompressed_length(s, len(s), C.byref(n)) == 0
        assert n.value == len(data), name
        assert libsnappy.uncompress(s) == data, name


def test_room_is_checked():
    """dst below the maximum length is PSG_ERR_SIZE, whatever the stream needs."""
    import ctypes as C
    L = _lib.lib()
    data = bytes(1000)
    cap = snappy.max_compressed_length(len(data))
    out, n = C.create_string_buffer(cap), C.c_size_t()
    assert L.psg_snappy_compress_host(data, len(data), out, cap - 1, C.byref(n)) == _lib.PSG_ERR_SIZE
    assert L.psg_snappy_compress_host(data, len(data), out, cap, C.byref(n)) == 0


def kinds(name):
    data = dict(I.edge_inputs())[name]
    return [(k, ln, off) for k, ln, off, _ in I.check_structure(twin(name, data), len(data))]


def test_literal_length_forms():
    """Incompressible runs of up to 60, 256 and 65536 bytes: the tag alone,
    one and two length bytes."""
    for name, n, head in (("len60", 60, 1), ("len61", 61, 2), ("rand256", 256, 2),
                          ("rand257", 257, 3), ("rand65536", 65536, 3)):
        assert kinds(name) == [(0, n, 0)], name
        data = dict(I.edge_inputs())[name]
        assert len(twin(name, data)) == P.snappy_elements(twin(name, data))[1][0][0] + head + n


def test_offset_seam():
    """An 8-byte repeat at distance 2047 is a copy-1, at 2048 a copy-2."""
    assert (1, 8, 2047) in kinds("at2047")
    assert (2, 8, 2048) in kinds("at2048")
    assert all(k != 1 for k, _, _ in kinds("at2048"))


def test_match_lengths():
    """A repeat of 3 bytes is no match; 4 and 11 are a copy-1; 12 and 64 a
    copy-2; 65 bytes are a 64-byte copy and a literal."""
    copies = {m: [(k, ln, off) for k, ln, off in kinds("match%d" % m) if k] for m in I.MATCH_LENGTHS}
    assert copies[3] == []
    assert copies[4] == [(1, 4, 500)] and copies[11] == [(1, 11, 500)]
    assert copies[12] == [(2, 12, 500)] and copies[64] == [(2, 64, 500)]
    assert copies[65] == [(2, 64, 500)]
    assert kinds("match65")[-1][0] == 0


def test_step_seams():
    """The first step of a fragment goes out as a literal; from the second on
    the period is found, also by a match whose source ends at, or reaches
    into, the step it lies in."""
    for n in (I.STEP - 1, I.STEP):
        assert kinds("step%d" % n) == [(0, n, 0)]
    assert kinds("step%d" % (I.STEP + 1)) == [(0, I.STEP + 1, 0)]  # one position: no 4 bytes
    for n in (2 * I.STEP - 1, 2 * I.STEP, 2 * I.STEP + 1):
        k = kinds("step%d" % n)
        assert k[0] == (0, I.STEP, 0) and all(e[0] for e in k[1:-1]) and len(k) >= 4
    assert [(k, ln, off) for k, ln, off in kinds("src_before_step") if k] == [(2, 16, 60)]
    assert [(k, ln, off) for k, ln, off in kinds("src_into_step") if k] == [(2, 16, 59)]


def test_fragment_seams():
    """A periodic input across fragment seams: every fragment starts over
    with a literal of one step, and the copies end at the seam."""
    for n in (I.FRAGMENT - 1, I.FRAGMENT, I.FRAGMENT + 1, 2 * I.FRAGMENT + 1):
        name = "periodic%d" % n
        data = dict(I.edge_inputs())[name]
        el = I.check_structure(twin(name, data), n)
        starts = [x for k, ln, off, x in el if k == 0 and x % I.FRAGMENT == 0]
        assert starts == list(range(0, n, I.FRAGMENT))


def test_fuzz(libsnappy):
    """200 seeded inputs of 0 .. 200,000 bytes: alphabets of 1, 2, 4 and 256
    symbols, and 8-byte records."""
    for seed in range(200):
        data = I.fuzz_input(seed)
        s = snappy.compress_host(data)
        check_valid(s, data)
        assert libsnappy.uncompress(s) == data, seed


def test_compression_is_real():
    """Period 1, 8 and 3: ideal 64-byte copies cost 3 / 64 of n; 1 / 8 leaves
    room for each fragment's first step going out as a literal.  And wherever
    libsnappy's recorded stream is at most 0.7 of the raw bytes, ours is
    shorter than the raw bytes."""
    R = P.snappy_recorded()
    for name in ("f32_zero", "f64_sent_all", "abc"):
        data = R[name][0].data
        assert len(twin("pin_" + name, data)) <= len(data) // 8, name
    held = []
    for name, (c, recorded, _) in R.items():
        if len(c.data) and len(recorded) <= 0.7 * len(c.data):
            held.append(name)
            assert len(twin("pin_" + name, c.data)) < len(c.data), name
    want = {"keys24", "keys_dense", "f32_eighths", "f64_sent70", "f64_sent98", "f64_sent_all",
            "f32_zero", "abc", "rep2047", "rep2048", "alpha4"}
    want |= {n for n in R if n.startswith("push") and not n.endswith("keys")}
    assert set(held) == want


def test_recorded_sizes_are_the_twins():
    """profiles/snappy_compress.json (tools/bench_snappy_compress.py) holds
    the raw, libsnappy and our length of every pinned case: ours must be what
    the twin gives today, libsnappy's what the fixture holds."""
    with open(PROFILE) as f:
        sizes = json.load(f)["sizes"]
    R = P.snappy_recorded()
    assert set(sizes) == set(R)
    for name, (c, recorded, _) in R.items():
        assert sizes[name] == {"raw": len(c.data), "libsnappy": len(recorded),
                               "ours": len(twin("pin_" + name, c.data))}, name
