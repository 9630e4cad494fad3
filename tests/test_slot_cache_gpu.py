"""GPU: SlotReader's cache arrays on the device (psg_mb_cache_pack,
psg_mb_load_cache, CachedSlotReader).

Pack: every stream is psg_snappy_compress_host of the restated raw partition
(tests/slot_cache_ref.py).  Load: the recorded reference-format files
(tests/golden/slot_cache, streams of the real snappy compressor) give the
recorded arrays bit for bit; synthetic files sit on the scan's tile edges
(T = psg_cache_scan_tile()).  Everything is integer, a copy, or an exact
float <-> double conversion, so every comparison is exact."""
import ctypes as C
import os

import numpy as np
import pytest

import slot_cache_ref as R
from parameter_server_amd import DarlingWorker, _lib, slot_cache as SC, slots
from parameter_server_amd.kv_vector import KVVector
from parameter_server_amd.snappy import compress_host
from parameter_server_amd.worker import Minibatch
from test_slot_cache import CASES, FORMATS, load_case

pytestmark = pytest.mark.gpu

WHATS = {"colidx": _lib.PSG_CACHE_COLIDX, "rowsiz": _lib.PSG_CACHE_ROWSIZ,
         "value": _lib.PSG_CACHE_VALUE, "label": _lib.PSG_CACHE_LABEL}


@pytest.fixture(scope="module")
def ctx():
    v = KVVector(0, _lib.PSG_F64)
    yield v
    v.close()


@pytest.fixture(scope="module")
def mbs(ctx):
    a, b = Minibatch(ctx._h), Minibatch(ctx._h)
    yield a, b
    a.close()
    b.close()


def same(a, b):
    if a is None or b is None:
        return a is None and b is None
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def csr(rows, nnz, valued, seed):
    rng = np.random.default_rng(seed)
    cuts = np.sort(rng.integers(0, nnz + 1, max(rows - 1, 0))).astype(np.uint64)
    offset = np.r_[np.uint64(0), cuts, np.uint64(nnz)].astype(np.uint64) if rows else \
        np.zeros(1, np.uint64)
    index = rng.integers(0, 1 << 40, nnz, dtype=np.uint64)  # compressible: the high bytes repeat
    value = rng.standard_normal(nnz).astype(np.float32).astype(np.float64) if valued else None
    y = rng.choice([-1.0, 1.0], rows)
    return offset, index, value, y


def arrays_of(mb, valued):
    return (mb.read("offset"), mb.read("index"), mb.read("value") if valued else None,
            mb.read("y"))


def is_empty(mb):
    n = C.c_size_t()
    return _lib.lib().psg_mb_read(mb._h, _lib.PSG_MB_OFFSET, None, 0, C.byref(n)) == _lib.PSG_ERR_ARG


# ---- 1. pack ------------------------------------------------------------------
# (rows, nnz): 0, 1 and part_bytes / elt +- 1 elements of every array for
# part_bytes 8 (1, 4, 2) and 4096 (512, 2048, 1024)
SHAPES = [(0, 0), (1, 0), (1, 1), (3, 2), (4, 3), (5, 1), (2, 511), (1023, 512), (1024, 513),
          (1025, 1023), (2047, 1024), (2048, 1025), (2049, 3000)]


@pytest.mark.parametrize("valued", (False, True))
def test_pack_streams_equal_the_host_compressor(mbs, valued):
    mb = mbs[0]
    for k, (rows, nnz) in enumerate(SHAPES):
        data = csr(rows, nnz, valued, 100 + k)
        mb.load(*data)
        raw = R.cache_arrays(*data)
        for name, what in WHATS.items():
            if name == "value" and not valued:
                rc, _, got, parts = SC.mb_cache_pack(mb, what, 4096, check=False)
                assert rc == _lib.PSG_ERR_ARG and got == b"" and parts == []
                continue
            for pb in (0, 8, 4096):
                got, parts = SC.mb_cache_pack(mb, what, pb)
                want = [compress_host(p) for p in R.partitions(raw[name], pb)]
                where = (rows, nnz, name, pb)
                assert len(parts) == len(want) == SC.pack_bound(len(raw[name]), pb)[1], where
                at = 0
                for (start, size), w in zip(parts, want):
                    assert start == at and got[start:start + size] == w, where
                    at += size
                assert at == len(got), where


def test_pack_after_group_extract_and_bad_arguments(ctx, mbs):
    src, dst = mbs
    offset, index, value, y = csr(40, 300, True, 7)
    slot = np.where(np.arange(300) % 3 == 0, 5, 9).astype(np.uint16)
    for r in range(40):  # one run of each id per row
        b, e = int(offset[r]), int(offset[r + 1])
        slot[b:e] = np.sort(slot[b:e])
    src.load(offset, index, value, y)
    slots.mb_set_slots(src, slot)
    info, bad = slots.mb_groups(src)
    assert bad == -1
    slots.mb_group_extract(src, 9, dst, int((slot == 9).sum()))
    m = slot == 9
    before = np.r_[0, np.cumsum(m)].astype(np.uint64)
    raw = R.cache_arrays(before[offset.astype(np.int64)], index[m], value[m], y)
    for name, what in WHATS.items():
        got, parts = SC.mb_cache_pack(dst, what, 64)
        assert [got[a:a + b] for a, b in parts] == [compress_host(p)
                                                    for p in R.partitions(raw[name], 64)]
    assert SC.mb_cache_pack(dst, _lib.PSG_CACHE_COLIDX, 12, check=False)[0] == _lib.PSG_ERR_ARG
    assert SC.mb_cache_pack(dst, 4, 8, check=False)[0] == _lib.PSG_ERR_ARG
    fresh = Minibatch(ctx._h)  # nothing loaded
    try:
        assert SC.mb_cache_pack(fresh, _lib.PSG_CACHE_ROWSIZ, 8, check=False)[0] == _lib.PSG_ERR_ARG
    finally:
        fresh.close()


def test_pack_row_of_65535_entries_and_one_too_long(mbs):
    mb = mbs[0]
    sizes = np.array([2, 65535, 0, 0, 3], np.uint64)
    offset = np.r_[np.uint64(0), np.cumsum(sizes)].astype(np.uint64)
    n = int(offset[-1])
    index = (np.arange(n, dtype=np.uint64) * np.uint64(7)) % np.uint64(1000)
    y = np.ones(5)
    mb.load(offset, index, None, y)
    got, parts = SC.mb_cache_pack(mb, _lib.PSG_CACHE_ROWSIZ, 0)
    assert got == compress_host(sizes.astype(np.uint16).tobytes()) and parts == [(0, len(got))]
    sizes = np.array([2, 65535, 65536, 0, 70000, 1], np.uint64)
    offset = np.r_[np.uint64(0), np.cumsum(sizes)].astype(np.uint64)
    n = int(offset[-1])
    index = (np.arange(n, dtype=np.uint64) * np.uint64(7)) % np.uint64(1000)
    mb.load(offset, index, None, np.ones(6))
    rc, bad_row, got, parts = SC.mb_cache_pack(mb, _lib.PSG_CACHE_ROWSIZ, 8, check=False)
    assert (rc, bad_row, got, parts) == (_lib.PSG_ERR_RANGE, 2, b"", [])
    # the other arrays of that minibatch pack as ever
    got, parts = SC.mb_cache_pack(mb, _lib.PSG_CACHE_COLIDX, 0)
    assert got == compress_host(index.tobytes())


# ---- 2. the recorded reference-format files -----------------------------------
def recorded_files(z, slot_id, whole_file=False):
    """The psg_mb_load_cache input of one slot; whole_file: no .partition
    files (every recorded file of the "single" form is one stream)."""
    files = []
    for i, num_ex in enumerate(z["num_ex"]):
        f = {"num_ex": int(num_ex)}
        for ext, sid, key in (("colidx", slot_id, "colidx"), ("rowsiz", slot_id, "rowsiz"),
                              ("value", slot_id, "value"), ("value", 0, "label")):
            name = "f%d_s%d_%s" % (i, sid, ext)
            if name in z.files:
                parts = [(int(a), int(b)) for a, b in z[name + "_parts"]]
                f[key] = (z[name].tobytes(), None if whole_file else parts)
        files.append(f)
    return files


@pytest.mark.parametrize("name", CASES)
def test_load_recorded_files(mbs, name):
    mb = mbs[0]
    z, case, form, _ = load_case(name)
    valued = FORMATS[case] == "libsvm"
    for s in [int(s) for s in z["slots"]]:
        for whole in ((False, True) if form == "single" else (False,)):
            r = SC.mb_load_cache(mb, recorded_files(z, s, whole), valued)
            offset, index, value, y = arrays_of(mb, valued)
            assert same(offset, z["s%d_offset" % s]) and same(index, z["s%d_index" % s])
            assert same(y, z["y"])
            assert (int(r.rows), int(r.nnz)) == (y.size, index.size) == (mb.rows, mb.nnz)
            if valued:
                assert same(value, z["s%d_value" % s])
            else:
                assert mb.read("value").size == 0


def test_load_file_lacking_the_slot_gives_empty_rows(mbs):
    mb = mbs[0]
    z, _, _, _ = load_case("adfea_two_files_multi")
    files = recorded_files(z, 4)
    assert "colidx" in files[0] and "colidx" not in files[1] and "label" in files[1]
    SC.mb_load_cache(mb, files, False)
    offset = mb.read("offset")
    n0, n1 = [int(n) for n in z["num_ex"]]
    assert offset.size == n0 + n1 + 1 and np.all(offset[n0:] == offset[n0]) and offset[n0] > 0
    # a slot no file holds: num_ex empty rows, the labels still there
    SC.mb_load_cache(mb, recorded_files(z, 77), False)
    assert same(mb.read("offset"), np.zeros(n0 + n1 + 1, np.uint64)) and same(mb.read("y"), z["y"])
    # no file at all: an empty minibatch that is loaded
    r = SC.mb_load_cache(mb, [], False)
    assert (int(r.rows), int(r.nnz)) == (0, 0) and same(mb.read("offset"), np.zeros(1, np.uint64))


# ---- 3. the scan's seams --------------------------------------------------------
def synth_files(sizes_per_file, valued, seed, part_bytes=4096):
    """Cache files (streams of the host compressor, cut every part_bytes) for
    the given row sizes of each file, and the arrays they must load to."""
    rng = np.random.default_rng(seed)
    files, idx, val, lab, siz = [], [], [], [], []
    for sizes in sizes_per_file:
        sizes = np.asarray(sizes, np.uint16)
        n = int(sizes.astype(np.int64).sum())
        index = rng.integers(0, 1 << 30, n, dtype=np.uint64)
        value = rng.standard_normal(n).astype(np.float32)
        label = rng.choice([-1.0, 1.0], sizes.size).astype(np.float32)
        f = {"num_ex": sizes.size,
             "colidx": SC._host_streams(index.tobytes(), part_bytes),
             "rowsiz": SC._host_streams(sizes.tobytes(), part_bytes),
             "label": SC._host_streams(label.tobytes(), part_bytes)}
        if valued:
            f["value"] = SC._host_streams(value.tobytes(), part_bytes)
        files.append(f)
        idx.append(index), val.append(value), lab.append(label), siz.append(sizes)
    offset = np.r_[np.uint64(0), np.cumsum(np.concatenate(siz).astype(np.uint64), dtype=np.uint64)]
    want = (offset.astype(np.uint64), np.concatenate(idx),
            np.concatenate(val).astype(np.float64) if valued else None,
            np.concatenate(lab).astype(np.float64))
    return files, want


@pytest.mark.parametrize("mult,delta", [(m, d) for m in (1, 2) for d in (-1, 0, 1)])
def test_scan_at_tile_edges(mbs, mult, delta):
    mb = mbs[0]
    T = int(_lib.lib().psg_cache_scan_tile())
    rows = mult * T + delta
    rng = np.random.default_rng(rows)
    sizes = rng.integers(0, 4, rows).astype(np.uint16)
    sizes[T - 6:T + 5] = 0            # a run of empty rows across the first tile edge
    sizes[T - 7] = 3
    big = min(T + 5, rows - 1)        # 65535 entries beside empty rows, just past the edge
    sizes[big] = 65535
    sizes[rows - 1] = max(int(sizes[rows - 1]), 1) if big != rows - 1 else 65535
    # three files: a seam on the tile edge (or in the middle of a short set), one beside it
    a = T if rows > T else rows // 2
    b = min(a + 1, rows)
    files, want = synth_files([sizes[:a], sizes[a:b], sizes[b:]], mult == 2, rows)
    r = SC.mb_load_cache(mb, files, mult == 2)
    assert int(r.rows) == rows and int(r.nnz) == int(want[0][-1])
    for got, w in zip(arrays_of(mb, mult == 2), want):
        assert same(got, w)
    assert same(mb.read("offset"), np.r_[0, np.cumsum(sizes.astype(np.uint64))].astype(np.uint64))


# ---- 4. the round trip against the text path ------------------------------------
CHUNK = SC.MIN_CHUNK_BYTES
LINES, BAD = 12000, 5000  # lines per file; the rejected line of the middle file


def adfea_text(file_no, lines, rng):
    """~48 bytes a line.  Slot 2 is everywhere; slot 3 only in the first third
    of file 0 and the last third of file 2 (it skips chunks, and file 1);
    slot 7 first appears in the middle of file 1."""
    out = []
    for i in range(lines):
        ent = ["%d:2" % k for k in np.sort(rng.integers(1, 1 << 40, int(rng.integers(0, 4))))]
        third = 3 * i // lines
        if (file_no == 0 and third == 0) or (file_no == 2 and third == 2):
            ent += ["%d:3" % k for k in rng.integers(1, 5000, int(rng.integers(1, 3)))]
        if (file_no == 1 and third >= 1) or file_no == 2:
            if i % 5 == 0:
                ent.append("%d:7" % rng.integers(1 << 50, 1 << 60))
        out.append("l%d_%d 1 %d %s\n" % (file_no, i, int(rng.integers(0, 2)), " ".join(ent)))
    return out


@pytest.fixture(scope="module")
def cached_set(ctx, tmp_path_factory):
    """Three ADFEA files of more than three chunks each, one rejected line in
    the middle file; the cold CachedSlotReader over them."""
    d = tmp_path_factory.mktemp("slot_cache")
    rng = np.random.default_rng(42)
    paths, texts = [], []
    for f in range(3):
        lines = adfea_text(f, LINES, rng)
        if f == 1:
            lines[BAD] = "bad 1 1 5:9999\n"  # a slot id outside [1, 4095]: rejected
        text = "".join(lines).encode()
        assert len(text) > 3 * CHUNK
        p = str(d / ("part-%d.txt" % f))
        open(p, "wb").write(text)
        paths.append(p)
        texts.append(text)
    prefix = str(d / "cache") + "/"
    os.makedirs(prefix)
    rd = SC.CachedSlotReader(ctx._h, prefix, "adfea", chunk_bytes=CHUNK, part_bytes=65536)
    rd.read(paths)
    yield rd, paths, b"".join(texts), prefix
    rd.close()


def test_round_trip_equals_the_text_path(ctx, mbs, cached_set):
    rd, paths, text, prefix = cached_set
    a, b = mbs
    assert rd.hit_cache == 0 and rd.bad_lines == [(paths[1], BAD)]
    sr = slots.SlotReader(ctx._h)
    try:
        sr.read(text, "adfea")
        assert sr.bad_lines == [LINES + BAD]
        assert rd.example_info() == sr.example_info() and rd.num_ex == 3 * LINES - 1
        assert rd.slots() == sr.slots() == [2, 3, 7]
        for s in sr.slots() + [11]:  # 11: a slot no file holds
            rd.extract(s, a)
            sr.extract(s, b)
            assert (a.rows, a.nnz) == (b.rows, b.nnz)
            for x, y in zip(arrays_of(a, False), arrays_of(b, False)):
                assert same(x, y)
    finally:
        sr.close()
    # the zero padding is in the files: slot 7's row sizes of file 1 start with a
    # partition of zeros, slot 3 has no file for file 1
    assert not os.path.exists(SC.cache_name(prefix, paths[1], 3) + ".rowsiz")
    assert os.path.exists(SC.cache_name(prefix, paths[1], 7) + ".rowsiz.partition")
    assert not os.path.exists(SC.cache_name(prefix, paths[0], 0) + ".colidx")


def test_second_reader_hits_the_cache_without_the_texts(ctx, mbs, cached_set, tmp_path):
    rd, paths, text, prefix = cached_set
    a, b = mbs
    hidden = [str(tmp_path / os.path.basename(p)) for p in paths]
    for p, h in zip(paths, hidden):
        os.rename(p, h)
    try:
        warm = SC.CachedSlotReader(ctx._h, prefix, "adfea", chunk_bytes=CHUNK)
        try:
            warm.read(paths)
            assert warm.hit_cache == 3 and warm.example_info() == rd.example_info()
            for s in rd.slots():
                rd.extract(s, a)
                warm.extract(s, b)
                for x, y in zip(arrays_of(a, False), arrays_of(b, False)):
                    assert same(x, y)
        finally:
            warm.close()
    finally:
        for p, h in zip(paths, hidden):
            os.rename(h, p)


def test_round_trip_libsvm(ctx, mbs, tmp_path):
    rng = np.random.default_rng(3)
    lines = []
    for i in range(7000):
        k = np.sort(rng.integers(1, 1 << 33, int(rng.integers(0, 5))))
        lines.append("%s %s\n" % (("1", "-1", "0.5")[i % 3],
                                  " ".join("%d:%s" % (x, ("1", "0.25", "-3.5", "7")[int(x) % 4])
                                           for x in k)))
    text = "".join(lines).encode()
    assert len(text) > CHUNK
    p = str(tmp_path / "train.libsvm")
    open(p, "wb").write(text)
    rd = SC.CachedSlotReader(ctx._h, str(tmp_path) + "/c_", "libsvm", chunk_bytes=CHUNK,
                             part_bytes=8192)
    sr = slots.SlotReader(ctx._h)
    try:
        rd.read([p])
        sr.read(text, "libsvm")
        assert rd.example_info() == sr.example_info()
        rd.extract(1, mbs[0])
        sr.extract(1, mbs[1])
        for x, y in zip(arrays_of(mbs[0], True), arrays_of(mbs[1], True)):
            assert same(x, y)
        # a binary reader over these files refuses the values
        wrong = SC.CachedSlotReader(ctx._h, str(tmp_path) + "/c_", "adfea", chunk_bytes=CHUNK)
        wrong.read([p])
        assert wrong.hit_cache == 1
        with pytest.raises(_lib.PSGError):
            wrong.extract(1, mbs[0])
    finally:
        rd.close()
        sr.close()


# ---- 5. errors --------------------------------------------------------------------
def good_files():
    rng = np.random.default_rng(9)
    return synth_files([rng.integers(0, 5, 300), rng.integers(0, 5, 200)], True, 9, part_bytes=512)


def check_error(mb, files, want_rc, want_bad):
    rc, r = SC.mb_load_cache(mb, files, True, check=False)
    assert rc == want_rc
    got = (int(r.bad_file), int(r.bad_what), int(r.bad_part))
    assert got[:len(want_bad)] == want_bad
    assert is_empty(mb)
    good, want = good_files()
    SC.mb_load_cache(mb, good, True)  # the next load works
    for g, w in zip(arrays_of(mb, True), want):
        assert same(g, w)


def test_error_corrupt_stream(mbs):
    files, _ = good_files()
    data, parts = files[1]["colidx"]
    assert len(parts) >= 3
    start = parts[1][0]
    pre = 1
    while data[start + pre - 1] & 0x80:  # the length preamble of partition 1
        pre += 1
    # its first element becomes a copy of 4 bytes from before the output's start
    bad = bytearray(data)
    bad[start + pre] = 0x01
    files[1]["colidx"] = (bytes(bad), parts)
    check_error(mbs[0], files, _lib.PSG_ERR_ARG, (1, _lib.PSG_CACHE_COLIDX, 1))


def test_error_partition_of_seven_bytes(mbs):
    files, _ = good_files()
    data, parts = files[0]["rowsiz"]
    odd = compress_host(b"\x01\x00\x02\x00\x03\x00\x04")
    files[0]["rowsiz"] = (data + odd, parts + [(len(data), len(odd))])
    check_error(mbs[0], files, _lib.PSG_ERR_SIZE, (0, _lib.PSG_CACHE_ROWSIZ, len(parts)))


def test_error_row_sizes_do_not_sum_to_the_entries(mbs):
    rng = np.random.default_rng(9)
    sizes = [rng.integers(0, 5, 300), rng.integers(0, 5, 200)]
    files, _ = synth_files(sizes, True, 9, part_bytes=512)
    # file 1's row sizes with two of them exchanged for others of another sum:
    # the counts all agree, only the scanned offsets at the file's seams tell
    s1 = np.asarray(sizes[1], np.uint16).copy()
    s1[7] += 1
    files[1]["rowsiz"] = SC._host_streams(s1.tobytes(), 512)
    check_error(mbs[0], files, _lib.PSG_ERR_SIZE, (1, _lib.PSG_CACHE_ROWSIZ))
    # the sums of two files that cancel are caught at the seam between them
    s0 = np.asarray(sizes[0], np.uint16).copy()
    s0[0] += 1
    s1 = np.asarray(sizes[1], np.uint16).copy()
    s1[np.flatnonzero(s1)[0]] -= 1
    files[0]["rowsiz"] = SC._host_streams(s0.tobytes(), 512)
    files[1]["rowsiz"] = SC._host_streams(s1.tobytes(), 512)
    check_error(mbs[0], files, _lib.PSG_ERR_SIZE, (0, _lib.PSG_CACHE_ROWSIZ))


def test_error_label_count(mbs):
    files, _ = good_files()
    files[0]["label"] = SC._host_streams(np.ones(299, np.float32).tobytes(), 512)
    check_error(mbs[0], files, _lib.PSG_ERR_SIZE, (0, _lib.PSG_CACHE_LABEL))
    files, _ = good_files()
    files[1]["num_ex"] = 201
    check_error(mbs[0], files, _lib.PSG_ERR_SIZE, (1,))
    files, _ = good_files()
    data, parts = files[0]["value"]
    files[0]["value"] = (data, parts[:-1])  # fewer values than entries
    check_error(mbs[0], files, _lib.PSG_ERR_SIZE, (0, _lib.PSG_CACHE_VALUE))
    files, _ = good_files()
    data, parts = files[0]["colidx"]
    files[0]["colidx"] = (data, parts[:-1] + [(parts[-1][0], parts[-1][1] + 1)])  # past the file
    check_error(mbs[0], files, _lib.PSG_ERR_SIZE, (0, _lib.PSG_CACHE_COLIDX, len(parts) - 1))


# ---- 6. Darling ---------------------------------------------------------------------
def test_darling_load_group_from_the_cache(ctx, cached_set):
    rd, paths, text, prefix = cached_set
    sr = slots.SlotReader(ctx._h)
    a = DarlingWorker(ctx._h, 1.0, 5.0)
    b = DarlingWorker(ctx._h, 1.0, 5.0)
    try:
        sr.read(text, "adfea")
        sr.extract(3, a.mb)
        keys = np.unique(a.mb.read("index"))
        w = np.random.default_rng(1).standard_normal(keys.size) * 0.1
        a.load_group(sr, 3, keys, w)
        b.load_group(rd, 3, keys, w)
        assert (a.mb.rows, a.mb.nnz) == (b.mb.rows, b.mb.nnz) and a.mb.nnz > 0
        cb, ce = keys.size // 4, keys.size // 2
        ga, ua = a.gradients(cb, ce)
        gb, ub = b.gradients(cb, ce)
        assert same(ga, gb) and same(ua, ub) and np.any(ga != 0)
    finally:
        a.close()
        b.close()
        sr.close()
