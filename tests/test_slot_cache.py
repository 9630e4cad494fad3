"""CPU: the SlotReader cache's names, its .info and .partition files, the
partition arithmetic, and the restatement of the cache arrays
(tests/slot_cache_ref.py) against the recorded reference-format files."""
import glob
import os

import numpy as np
import pytest

from parameter_server_amd import _lib, slot_cache as SC
from parameter_server_amd.snappy import max_compressed_length

import slot_cache_ref as R

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "slot_cache")
CASES = sorted(os.path.basename(p)[:-4] for p in glob.glob(os.path.join(GOLDEN, "*.npz")))
FORMATS = {"adfea3": "adfea", "libsvm": "libsvm", "adfea_two_files": "adfea"}
DUMP_ROWS = {"adfea3": 3, "libsvm": 2, "adfea_two_files": 2}


def load_case(name):
    z = np.load(os.path.join(GOLDEN, name + ".npz"))
    case, form = name.rsplit("_", 1)
    texts, at = [], 0
    for n in z["text_len"]:
        texts.append(z["texts"][at:at + int(n)].tobytes())
        at += int(n)
    return z, case, form, texts


def test_cases_recorded():
    assert CASES == sorted("%s_%s" % (c, f) for c in FORMATS for f in ("single", "multi"))


def test_djb_hash32():
    assert SC.djb_hash32("") == 5381
    assert SC.djb_hash32("a") == 177670
    path = "data/café/part-0".encode("utf-8")
    assert any(b >= 0x80 for b in path)
    h = 5381
    for b in path:
        c = b - 256 if b >= 0x80 else b  # const char&, then static_cast<uint32_t>
        h = ((h << 5) + h + (c & 0xFFFFFFFF)) & 0xFFFFFFFF
    assert SC.djb_hash32(path) == h == SC.djb_hash32(path.decode("utf-8"))
    plain = 5381
    for b in path:
        plain = (plain * 33 + b) & 0xFFFFFFFF
    assert h != plain  # the sign extension matters


def test_cache_names():
    h = str(SC.djb_hash32("/data/train/part-07"))
    assert SC.cache_name("/tmp/cache/", "/data/train/part-07", 3) == "/tmp/cache/" + h + "-part-07_slot_3"
    assert SC.info_name("/tmp/cache/", "/data/train/part-07") == "/tmp/cache/" + h + "-part-07.info"
    # the prefix is concatenated as given, not joined
    assert SC.cache_name("/tmp/c", "x", 0) == "/tmp/c" + str(SC.djb_hash32("x")) + "-x_slot_0"
    # getFilename: the last item of a getline split
    assert SC.cache_name("", "a/b/", 1).endswith("-b_slot_1")
    assert SC.info_name("p", "") == "p5381-.info"


INFO = {"num_ex": 7, "slot": [
    {"id": 0, "format": 1, "min_key": 0, "max_key": 1, "nnz_ele": 7, "nnz_ex": 7},
    {"id": 3, "format": 3, "min_key": 5, "max_key": (1 << 64) - 1, "nnz_ele": 19, "nnz_ex": 6},
    {"id": 4095, "format": 2, "min_key": 1 << 63, "max_key": 0, "nnz_ele": 1, "nnz_ex": 1}]}


def test_info_round_trip(tmp_path):
    p = str(tmp_path / "x.info")
    SC.write_info(p, INFO)
    assert SC.read_info(p) == INFO
    text = open(p).read()
    assert text.startswith("slot {\n  format: DENSE\n  id: 0\n  min_key: 0\n  max_key: 1\n"
                           "  nnz_ele: 7\n  nnz_ex: 7\n}\n")
    assert "format: SPARSE_BINARY\n  id: 3\n" in text and text.endswith("num_ex: 7\n")
    assert SC.parse_info(SC.format_info({"num_ex": 0, "slot": []})) == {"num_ex": 0, "slot": []}


def test_info_reference_style_text():
    text = ("slot {\n  format: SPARSE_BINARY\n  id: 3\n  min_key: 12\n  max_key: 99\n"
            "  nnz_ele: 40\n  nnz_ex: 10\n}\n"
            "slot{format:2 id:7\tmin_key:1 max_key:2 nnz_ele:3\n\n nnz_ex:4}   num_ex:   11 ")
    assert SC.parse_info(text) == {"num_ex": 11, "slot": [
        {"id": 3, "format": 3, "min_key": 12, "max_key": 99, "nnz_ele": 40, "nnz_ex": 10},
        {"id": 7, "format": 2, "min_key": 1, "max_key": 2, "nnz_ele": 3, "nnz_ex": 4}]}
    # a field left out keeps the proto's default
    assert SC.parse_info("slot { id: 1 }")["slot"][0]["min_key"] == (1 << 64) - 1
    for bad in ("slot { id: 1", "slot { colour: 1 }", "num_ex 3", "slot { format: ROUND }"):
        with pytest.raises((ValueError, KeyError)):
            SC.parse_info(bad)


def test_partitions(tmp_path):
    parts = [(0, 17), (17, 0), (17, 1 << 40)]
    text = SC.format_partitions(parts)
    assert text == "0\t17\n17\t0\n17\t1099511627776\n"
    assert SC.parse_partitions(text) == parts
    assert SC.parse_partitions("") == []
    with pytest.raises(ValueError):
        SC.parse_partitions("1 2\n")
    name = str(tmp_path / "x_slot_3.colidx")
    assert SC.read_array_file(name) == (b"", None)  # a missing file: an empty array
    open(name, "wb").write(b"abc")
    assert SC.read_array_file(name) == (b"abc", None)  # no .partition file: one stream
    open(name + ".partition", "w").close()
    assert SC.read_array_file(name) == (b"abc", None)  # an empty one too
    open(name + ".partition", "w").write("0\t2\n2\t1\n")
    assert SC.read_array_file(name) == (b"abc", [(0, 2), (2, 1)])


@pytest.mark.parametrize("part_bytes", [0, 8, 4096])
def test_pack_bound(part_bytes):
    m = max_compressed_length
    for raw in (0, 1, 7, 8, 9, 16, 4088, 4096, 4104, 3 * 4096, 3 * 4096 + 2, 1 << 20):
        cap, n = SC.pack_bound(raw, part_bytes)
        if raw == 0:
            assert (cap, n) == (0, 0)
        elif part_bytes == 0:
            assert (cap, n) == (m(raw), 1)
        else:
            sizes = [min(part_bytes, raw - b) for b in range(0, raw, part_bytes)]
            assert n == len(sizes) and cap == sum(m(s) for s in sizes)
            assert [len(p) for p in R.partitions(bytes(raw), part_bytes)] == sizes


def test_pack_bound_rejects_odd_part_bytes():
    with pytest.raises(_lib.PSGError) as e:
        SC.pack_bound(100, 12)
    assert e.value.status == _lib.PSG_ERR_ARG


@pytest.mark.parametrize("name", CASES)
def test_restatement_matches_recording(name):
    """readOneFile's arrays restated, assembled as index() / offset() /
    value() do: the recorded expectation (another restatement's) bit for
    bit; and, where libsnappy is present, the recorded bytes."""
    z, case, form, texts = load_case(name)
    fmt = FORMATS[case]
    per_file = [R.read_one_file(t, fmt, DUMP_ROWS[case] if form == "multi" else None)
                for t in texts]
    assert [n for n, _ in per_file] == [int(n) for n in z["num_ex"]]
    slots = sorted(set(s for _, f in per_file for s in f if s != 0))
    assert slots == [int(s) for s in z["slots"]]
    for s in slots:
        offset, index, value, y = R.assemble(per_file, s, fmt == "libsvm")
        assert np.array_equal(offset, z["s%d_offset" % s])
        assert np.array_equal(index, z["s%d_index" % s])
        assert y.tobytes() == z["y"].tobytes()
        if value is not None:
            assert value.tobytes() == z["s%d_value" % s].tobytes()
    # the partitions' layout: one line per dump in each of the slot's files
    for i, (_, files) in enumerate(per_file):
        for s, f in files.items():
            for ext in R.EXTS:
                parts = z["f%d_s%d_%s_parts" % (i, s, ext)]
                assert len(parts) == len(f[ext]) >= 1
                assert (form == "multi") or len(parts) == 1
                assert [int(b) for _, b in parts if not b] == [0] * sum(1 for p in f[ext] if not p)
    try:
        from snappy_lib import Snappy
        snappy = Snappy()
    except OSError:
        return
    for i, (_, files) in enumerate(per_file):
        for s, f in files.items():
            for ext in R.EXTS:
                data = b"".join(snappy.compress(p) if p else b"" for p in f[ext])
                assert data == z["f%d_s%d_%s" % (i, s, ext)].tobytes()


def test_multi_form_exercises_padding():
    """The recorded texts reach what they are for: a slot that first appears
    after a dump (a partition that starts with zero row sizes) and a slot
    absent from a whole file."""
    z, _, _, texts = load_case("adfea3_multi")
    _, files = R.read_one_file(texts[0], "adfea", 3)
    first = np.frombuffer(files[5]["rowsiz"][0], np.uint16)
    assert len(files[5]["rowsiz"]) < len(files[2]["rowsiz"]) and first[0] == 0 and first.any()
    z, _, _, texts = load_case("adfea_two_files_single")
    assert 4 in R.read_one_file(texts[0], "adfea")[1] and 4 not in R.read_one_file(texts[1], "adfea")[1]
