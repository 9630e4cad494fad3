"""CPU: the device-array forms of the server context are exported and bound,
and darling_pass's block-to-columns mapping follows psg_find_range's rule
(SArray::findRange: two lower_bounds, shared_array_inl.h:164-171).  No device
call."""
import bisect
import ctypes as C

import numpy as np
import pytest

from parameter_server_amd import _lib
from parameter_server_amd.darling import block_columns, pass_schedule

NEW = ("psg_push_dev", "psg_pull_dev", "psg_darling_update_dev", "psg_darling_progress",
       "psg_dev_status")
KMAX = (1 << 64) - 1


def test_new_symbols_exported_and_bound():
    L = _lib.lib()
    raw = C.CDLL(_lib.LIB_PATH)
    for name in NEW:
        assert name in _lib.SIGNATURES, name
        assert C.cast(getattr(raw, name), C.c_void_p).value, name
        assert getattr(L, name).argtypes == _lib.SIGNATURES[name][1], name
    assert _lib.PSG_NO_SLICE == C.c_size_t(-1).value
    # argument validation needs no device
    assert L.psg_dev_status(None) == _lib.PSG_ERR_ARG
    assert L.psg_pull_dev(None, 0, None, 0, None, None, None) == _lib.PSG_ERR_ARG
    assert L.psg_darling_update_dev(None, 0, 0, None) == _lib.PSG_ERR_ARG


def find_range(keys, kb, ke):
    """psg_find_range's rule on a Python list of ints."""
    return bisect.bisect_left(keys, kb), bisect.bisect_left(keys, ke)


DICT = [10, 11, 20, 35, 36, 37, 90, KMAX - 1]
BLOCKS = {
    "before": (0, 10),
    "before, touching": (3, 11),
    "inside": (11, 37),
    "inside, between keys": (21, 35),
    "one key": (35, 36),
    "straddling the front": (0, 21),
    "straddling the back": (37, KMAX),
    "after": (KMAX, KMAX),
    "everything but the last key value": (0, KMAX),
    "empty block": (20, 20),
    "ke = 2^64 - 1 from a key": (90, KMAX),
}


@pytest.mark.parametrize("name", sorted(BLOCKS))
def test_block_columns_is_find_range(name):
    kb, ke = BLOCKS[name]
    d = np.array(DICT, np.uint64)
    assert block_columns(d, kb, ke) == find_range(DICT, kb, ke), name


def test_block_columns_edge_dictionaries():
    assert block_columns(np.zeros(0, np.uint64), 0, KMAX) == (0, 0)
    assert block_columns(np.zeros(0, np.uint64), 5, 5) == (0, 0)
    # a dictionary that holds the largest key: [kb, 2^64 - 1) excludes it, as
    # Range<uint64>::all() does in the reference
    d = [0, 1 << 63, KMAX]
    assert block_columns(np.array(d, np.uint64), 0, KMAX) == find_range(d, 0, KMAX) == (0, 2)
    assert block_columns(np.array(d, np.uint64), 1, (1 << 63) + 1) == (1, 2)
    # keys above 2^63 compare as unsigned
    assert block_columns(np.array(d, np.uint64), (1 << 63) + 1, KMAX) == (2, 2)


def test_block_columns_random_against_find_range():
    rng = np.random.default_rng(5)
    d = np.unique(rng.integers(0, 1 << 64, size=300, dtype=np.uint64))
    dl = [int(x) for x in d]
    cuts = sorted(int(x) for x in rng.integers(0, 1 << 64, size=40, dtype=np.uint64))
    cuts = [0] + cuts + [KMAX]
    for kb, ke in zip(cuts[:-1], cuts[1:]):
        assert block_columns(d, kb, ke) == find_range(dl, kb, ke)
    # consecutive blocks tile the dictionary (minus a key equal to 2^64 - 1)
    got = [block_columns(d, kb, ke) for kb, ke in zip(cuts[:-1], cuts[1:])]
    assert got[0][0] == 0 and all(a[1] == b[0] for a, b in zip(got[:-1], got[1:]))


def test_pass_schedule_skips_workers_without_keys():
    a = np.array([1, 5, 9, 40], np.uint64)
    b = np.array([5, 6, 100], np.uint64)
    e = np.zeros(0, np.uint64)
    blocks = [(0, 6), (6, 10), (10, 40), (41, 99), (40, KMAX)]
    assert pass_schedule([a, b, e], blocks) == [
        [(0, 0, 2), (1, 0, 1)],  # both hold keys (5 is shared)
        [(0, 2, 3), (1, 1, 2)],
        [],                      # 40 is the block's end: nobody
        [],
        [(0, 3, 4), (1, 2, 3)],
    ]
