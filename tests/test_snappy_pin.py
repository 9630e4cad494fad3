"""The snappy decoders against streams from the real snappy compressor (CPU).

tests/golden/snappy_pin/*.npz hold what google snappy's RawCompress made of
the cases of pin_cases.snappy_cases() (tools/record_snappy.py; the library's
file and version are in each fixture's meta).  Here the oracle's decoder
(oracle/psg_oracle.c orc_snappy_uncompress) reproduces every input from its
recorded stream, and a host tag walk asserts that the streams still hold what
they were chosen for -- 1-byte-offset copies with non-zero high offset bits in
a part that the table form decodes itself (by a host replay of its own
criterion) and in parts it hands to the streamed form for either reason, long
copy runs, the 2047 / 2048 offset edge, every literal header, two compressor
blocks -- so that a later edit of the cases cannot silently lose the point.  tests/test_snappy_pin_gpu.py
feeds the same streams to the device decoders.

Where the library itself loads, the cases are compressed again and must give
the fixture's bytes, and the oracle compressor's output must decode through
the real decoder; elsewhere those checks skip.
"""
import hashlib

import numpy as np
import pytest

import oracle_py as O
import pin_cases as P

from pin_cases import K_TAB_MAX, K_TAB_PEND
from pin_cases import snappy_recorded as recorded


def tallies():
    if "tally" not in tallies.__dict__:
        tallies.tally = {n: P.snappy_tally(s) for n, (_, s, _) in recorded().items()}
    return tallies.tally


def test_fixtures_name_their_source():
    for g in P.SNAPPY_GROUPS:
        meta, _ = P.load_fixture(g, P.SNAPPY_GOLDEN)
        assert meta["source"]["library"].startswith("libsnappy.so")
        assert meta["source"]["version"][0].isdigit()


def test_oracle_decodes_every_recorded_stream():
    for name, (c, stream, info) in recorded().items():
        assert c.digest() == info["input_sha256"], name
        assert len(c.data) == info["uncompressed"], name
        got = O.snappy_uncompress(stream)  # orc_snappy_uncompressed_length, then _uncompress
        assert got is not None and len(got) == len(c.data), name
        assert hashlib.sha256(got).hexdigest() == info["input_sha256"], name
        assert got == c.data, name
        assert P.snappy_tally(stream) == info["tally"], name


def test_recorded_streams_cover_what_they_were_chosen_for():
    T = tallies()

    def high(name):
        return T[name]["copy1_high"]
    # the table form decodes a part only if it has few enough elements AND the
    # kernel's own count of copies it cannot place from the input
    # (pin_cases.snappy_table_npend, a host replay of its step 2) stays within
    # kTabPend: >= 10 copy-1 with non-zero high offset bits in such a part,
    # some of them left to its step 3
    table = [n for n, t in T.items() if P.snappy_form(t) == "table" and t["copy1_high"] >= 10]
    assert table == ["records"], table
    assert T["records"]["elements"] <= K_TAB_MAX and 1 <= T["records"]["table_npend"] <= K_TAB_PEND
    assert T["records"]["copy1_high"] >= 300
    # key and value arrays are copies of copies: the table form walks them and
    # then hands them to the streamed form, over the pending limit ...
    pend = [n for n, t in T.items() if t["table_npend"] is not None
            and t["table_npend"] > K_TAB_PEND and t["copy1_high"] >= 10]
    assert {"keys40_le", "f64_sent70", "f64_sent98", "alpha4"} <= set(pend), pend
    # ... or over the element limit
    full = [n for n, t in T.items() if t["elements"] > K_TAB_MAX and t["copy1_high"] >= 10]
    assert {"keys40_gt", "keys_dense", "f32_eighths"} <= set(full), full
    assert all(T[n]["table_npend"] is None for n in full)
    # the kTabMax pair
    le, gt = T["keys40_le"]["elements"], T["keys40_gt"]["elements"]
    assert K_TAB_MAX - 64 <= le <= K_TAB_MAX < gt <= K_TAB_MAX + 64, (le, gt)
    # copy runs past kTabPend, overlapping their own output
    assert T["f64_sent_all"]["longest_copy_run"] > 1000 and T["f64_sent_all"]["overlapping"] > 1000
    assert T["f32_eighths"]["longest_copy_run"] > K_TAB_PEND and high("f32_eighths") >= 100
    assert T["abc"]["copy2_min_offset"] == 3 and T["abc"]["overlapping"] > K_TAB_PEND
    # the offset edge between copy-1 and copy-2
    assert T["rep2047"]["copy1_max_offset"] == 2047 and T["rep2047"]["copy1"] == 1
    assert T["rep2048"]["copy2_min_offset"] == 2048 and T["rep2048"]["copy1"] == 0
    assert P.snappy_form(T["rep2047"]) == P.snappy_form(T["rep2048"]) == "table"
    _, el = P.snappy_elements(recorded()["rep2048"][1])
    assert el[-1][1:] == (2, 11, 2048)  # short enough for a copy-1, but for its offset
    # literal headers: inline, one length byte, two
    assert T["len60"]["lit_inline"] == 1 and T["len61"]["lit_1byte"] == 1
    assert T["keys63"]["lit_2byte"] == 1 and T["keys63"]["elements"] == 1
    assert T["f32_gauss"]["lit_2byte"] == 1 and T["f32_gauss"]["elements"] == 1
    assert T["len0"]["elements"] == 0 and T["len0"]["uncompressed"] == 0
    # two 64 KB compressor blocks
    for name in ("keys_dense", "f64_sent98", "f64_sent_all", "f32_zero"):
        assert T[name]["uncompressed"] > 65536, name
    assert high("keys_dense") >= 10
    # every part of the two pushes ends in the streamed form
    assert all(P.snappy_form(T[n]) == "streamed" and high(n) >= 10 for n in T if n.startswith("push"))


def test_push_cases_are_what_the_gpu_test_assumes():
    a, b = P.snappy_push("A"), P.snappy_push("B")
    assert a.clean == (0, 1, 2) and len(a.pushes) == 4
    for p, (k, vs) in enumerate(a.pushes):
        rc, _, _, _, mt = O.aggregate(a.D, 0, P.U64, [(k, vs)], False, 1, a.dtype)
        assert int(mt[0]) == k.size - (p == 3), p  # one key of the last push is not in D
    sent = np.uint64(P.SENTINEL)
    for k, vs in b.pushes:
        frac = (P.fbits(vs[0]) == sent).mean()
        assert 0.5 < frac < 0.7 and np.array_equal(P.fbits(vs[0]) == sent, P.fbits(vs[1]) == sent)
    k0, k1 = b.pushes[0][0], b.pushes[1][0]
    both = np.intersect1d(k0, k1)
    assert both.size > 100  # finite sums too
    for k, vs in b.pushes:  # no sentinel on a key both pushes hold
        assert not (P.fbits(vs[0])[np.isin(k, both)] == sent).any()


def test_oracle_refuses_truncated_real_streams():
    c, stream, _ = recorded()["keys24"]
    cuts = P.snappy_truncations(stream)
    assert [w for w, _ in cuts] == ["preamble", "copy1", "literal", "short"]
    for what, cut in cuts:
        assert 0 < len(cut) < len(stream) and stream.startswith(cut), what
        assert O.snappy_uncompress(cut) is None, what
    # the cuts are where they claim to be
    assert len(cuts[0][1]) == 2  # 8,000 as a varint
    assert cuts[1][1][-1] & 3 == 1


@pytest.fixture(scope="module")
def snappy():
    from snappy_lib import Snappy
    try:
        return Snappy()
    except OSError as e:
        pytest.skip("google snappy is not installed here (%s)" % e)


def test_library_decodes_the_fixtures(snappy):
    for name, (c, stream, _) in recorded().items():
        assert snappy.uncompress(stream) == c.data, name


def test_library_reproduces_the_fixtures(snappy):
    """A stale fixture (cases edited, recorder not rerun) shows here.  Another
    version of the library may choose other elements for the same input: the
    bytes are compared only under the version that recorded them."""
    meta, _ = P.load_fixture("keys", P.SNAPPY_GOLDEN)
    if snappy.version != meta["source"]["version"]:
        pytest.skip("snappy %s here, the fixtures were recorded with %s"
                    % (snappy.version, meta["source"]["version"]))
    for name, (c, stream, _) in recorded().items():
        assert snappy.compress(c.data) == stream, name


def test_library_decodes_the_oracle_compressor(snappy):
    for name, (c, _, _) in recorded().items():
        assert snappy.uncompress(O.snappy_compress(c.data)) == c.data, name


def test_library_refuses_the_truncated_streams(snappy):
    for what, cut in P.snappy_truncations(recorded()["keys24"][1]):
        assert snappy.uncompress(cut) is None, what
