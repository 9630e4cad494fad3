"""GPU: one dual for the feature groups of a worker
(psg_mb_darling_share_dual), and the batch path from grouped text to the
server's weights (SlotReader, DarlingWorker.load_group, feature_blocks,
darling_pass).

The shared dual is compared with the existing, reference-tested path: two
groups with disjoint, ordered key sets are one matrix whose columns are group
1's then group 2's.  A block of one group's columns sums, per column, the same
terms in the same order whether the other group's entries are in the matrix
or not, and multiplies, per row, the same factors in the same order; so G, U,
dual, cur_w, delta and the active bytes agree bit for bit."""
import ctypes as C

import numpy as np
import pytest

import slot_ref as S
from parameter_server_amd import DarlingWorker, _lib, slots
from parameter_server_amd.darling import darling_pass, server_progress
from parameter_server_amd.kv_vector import KVVector, Message
from parameter_server_amd.worker import Minibatch

pytestmark = pytest.mark.gpu

DELTA_INIT, DELTA_MAX = 1.0, 5.0
ROWS = 300  # past one 256-row block


def same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


@pytest.fixture(scope="module")
def server():
    v = KVVector(0, _lib.PSG_F64)
    yield v
    v.close()


def two_groups(binary, seed=11):
    """(combined CSR + slot ids, dict of group 1, dict of group 2): every key
    of group 1 (slot 3) is below every key of group 2 (slot 40); rows hold 0..5
    entries of each, group 1's first."""
    rng = np.random.default_rng(seed)
    d1 = np.sort(rng.choice(1 << 20, 70, replace=False)).astype(np.uint64)
    d2 = (np.sort(rng.choice(1 << 20, 50, replace=False)) + (1 << 21)).astype(np.uint64)
    offset, index, slot = [0], [], []
    for r in range(ROWS):
        for d, s in ((d1, 3), (d2, 40)):
            k = int(rng.integers(0, 6)) if r % 17 else 0
            index += sorted(rng.choice(d, k, replace=False).tolist())
            slot += [s] * k
        offset.append(len(index))
    index = np.array(index, np.uint64)
    value = None if binary else rng.choice([-1.0, 1.0], index.size) * (0.5 + rng.random(index.size))
    y = rng.choice([-1.0, 1.0], ROWS)
    return (np.array(offset, np.uint64), index, value, y, np.array(slot, np.uint16)), d1, d2


def reader_of(ctx, data):
    """A SlotReader over host arrays (valued data has no text form with groups)."""
    rd = slots.SlotReader(ctx)
    rd.mb.load(*data[:4])
    slots.mb_set_slots(rd.mb, data[4])
    rd.info, bad = slots.mb_groups(rd.mb)
    assert bad == -1
    rd.num_ex = data[3].size
    return rd


@pytest.mark.parametrize("binary", (True, False))
def test_shared_dual_equals_the_combined_matrix(server, binary):
    data, d1, d2 = two_groups(binary)
    n1, n2 = d1.size, d2.size
    rng = np.random.default_rng(5)
    new_w = [np.where(rng.random(n) < 0.2, 0.0, rng.standard_normal(n) * 0.3) for n in (n1, n2)]
    whole = DarlingWorker(server._h, DELTA_INIT, DELTA_MAX)
    a = DarlingWorker(server._h, DELTA_INIT, DELTA_MAX)
    b = DarlingWorker(server._h, DELTA_INIT, DELTA_MAX)
    rd = reader_of(server._h, data)
    try:
        whole.load(*data[:4], np.concatenate([d1, d2]))
        a.load_group(rd, 3, d1)
        b.load_group(rd, 40, d2, dual_of=a)
        assert a.mb.nnz + b.mb.nnz == data[1].size and a.mb.rows == b.mb.rows == ROWS
        for sweep in range(2):  # the second sweep starts from a dual that is not all ones
            g, u = whole.gradients(0, n1)
            ga, ua = a.gradients(0, n1)
            assert same(g, ga) and same(u, ua)
            whole.update_dual(0, n1, new_w[0] * (sweep + 1))
            a.update_dual(0, n1, new_w[0] * (sweep + 1))
            assert same(whole.state()["dual"], a.state()["dual"])
            assert same(b.state()["dual"], a.state()["dual"])  # one block, read through either
            g, u = whole.gradients(n1, n1 + n2)
            gb, ub = b.gradients(0, n2)
            assert same(g, gb) and same(u, ub)
            whole.update_dual(n1, n1 + n2, new_w[1] * (sweep + 1))
            b.update_dual(0, n2, new_w[1] * (sweep + 1))
            sw, sa, sb = whole.state(), a.state(), b.state()
            assert same(sw["dual"], sa["dual"]) and same(sw["dual"], sb["dual"])
            assert not np.all(sw["dual"] == 1.0)
            for name in ("cur_w", "delta", "active"):
                assert same(sw[name], np.concatenate([sa[name], sb[name]])), name
            assert same(np.array([whole.objv()]), np.array([b.objv()]))
        # set_state on the sharer writes the owner's block
        b.set_state(dual=np.full(ROWS, 0.5))
        assert np.all(a.state()["dual"] == 0.5)
    finally:
        for w in (b, a, whole):
            w.close()
        rd.close()


def test_share_dual_errors(server):
    data, d1, d2 = two_groups(True)
    L = _lib.lib()
    rd = reader_of(server._h, data)
    a = DarlingWorker(server._h, DELTA_INIT, DELTA_MAX)
    b = DarlingWorker(server._h, DELTA_INIT, DELTA_MAX)
    c = DarlingWorker(server._h, DELTA_INIT, DELTA_MAX)
    other = KVVector(0, _lib.PSG_F64)
    far = DarlingWorker(other._h, DELTA_INIT, DELTA_MAX)
    share = L.psg_mb_darling_share_dual
    try:
        rd.extract(3, a.mb)
        rd.extract(40, b.mb)
        assert share(b.mb._h, a.mb._h) == _lib.PSG_ERR_ARG      # the owner is not initialised
        a.load_group(rd, 3, d1)
        assert share(a.mb._h, a.mb._h) == _lib.PSG_ERR_ARG      # itself
        assert share(None, a.mb._h) == _lib.PSG_ERR_ARG
        far.load(*data[:4], d1)
        assert share(far.mb._h, a.mb._h) == _lib.PSG_ERR_ARG    # two contexts
        c.load(data[0][:11], data[1][:int(data[0][10])], None, data[3][:10], d1)
        assert share(c.mb._h, a.mb._h) == _lib.PSG_ERR_ARG      # 10 rows, 300 rows
        b.load_group(rd, 40, d2, dual_of=a)
        c.load(*data[:4], d2)
        assert share(c.mb._h, b.mb._h) == _lib.PSG_ERR_ARG      # b shares a's
        assert share(a.mb._h, c.mb._h) == _lib.PSG_ERR_ARG      # a's own dual is shared
        # a sharer's init takes no weights
        w = np.zeros(d2.size)
        wd = b._upload(b._W, w)
        assert L.psg_mb_darling_init(b.mb._h, DELTA_INIT, wd, None) == _lib.PSG_ERR_ARG
        assert L.psg_mb_darling_init(b.mb._h, DELTA_INIT, None, None) == _lib.PSG_OK
        b.gradients(0, d2.size)
        with pytest.raises(_lib.PSGError):
            b.load_group(rd, 40, d2, w=w, dual_of=a)
        b.load_group(rd, 40, d2, dual_of=a)
        # a load of the owner invalidates the sharer
        a.load_group(rd, 3, d1)
        with pytest.raises(_lib.PSGError) as e:
            b.gradients(0, d2.size)
        assert e.value.status == _lib.PSG_ERR_ARG
        with pytest.raises(_lib.PSGError):
            b.state()
        b.load_group(rd, 40, d2, dual_of=a)
        b.gradients(0, d2.size)
        # ... and so does its destruction
        a.close()
        with pytest.raises(_lib.PSGError):
            b.gradients(0, d2.size)
        b.load_group(rd, 40, d2)  # on its own again
        assert np.all(b.state()["dual"] == 1.0)
    finally:
        for x in (b, a, c, far):
            x.close()
        other.close()
        rd.close()


# ---- text to weights --------------------------------------------------------------
def adfea_text(seed=3, rows=ROWS):
    """Two groups (slots 2 and 9) whose key ranges overlap, a row without
    group 9, one without any entry, "\\r\\n" ends, a slow slot token, and two
    lines that SlotReader skips (a slot id 0; a slot in two runs)."""
    rng = np.random.default_rng(seed)
    lines = []
    for r in range(rows):
        ent = []
        if r % 13:
            k2 = sorted(rng.choice(400, int(rng.integers(1, 7)), replace=False).tolist())
            ent += ["%d:%s" % (k, "2" if r % 5 else "02") for k in k2]
        if r % 7 and r % 13:
            k9 = sorted((rng.choice(300, int(rng.integers(1, 5)), replace=False) + 200).tolist())
            ent += ["%d:%s" % (k, "9" if r % 11 else "+9") for k in k9]
        lines.append("r%d 1 %d %s%s" % (r, int(rng.integers(0, 2)), " ".join(ent),
                                         "\r\n" if r % 3 == 0 else "\n"))
    lines.insert(40, "bad 1 1 5:0\n")
    lines.insert(200, "split 1 1 5:2 6:9 7:2\n")
    return "".join(lines).encode(), [40, 200]


def run_pass(server, chl_of, workers, info, param):
    """One pass over the feature blocks, each group on its own channel."""
    t = 0
    blocks = slots.feature_blocks(info, 0.5)
    for grp, kb, ke in blocks:
        t = darling_pass(server, [workers[grp]], chl_of[grp], t, [(kb, ke)], param)
    return blocks


def test_text_to_weights():
    text, want_bad = adfea_text()
    rows, bad = S.skip_parse(text, S.ADFEA)
    rows = [r for i, r in enumerate(rows) if i not in S.split_rows(rows)]
    want_info = S.info(rows, S.ADFEA)
    param = {"eta": 1.0, "lambda_": 0.05, "kkt_filter_threshold": 1e20}
    servers, workers, readers = [], [], []
    weights = []
    try:
        for path in ("device", "host"):
            v = KVVector(0, _lib.PSG_F64)
            servers.append(v)
            rd = slots.SlotReader(v._h)
            readers.append(rd)
            info = rd.read(text, "adfea")
            assert rd.bad_lines == want_bad and rd.num_ex == len(rows) == ROWS
            assert info == want_info and rd.slots() == [2, 9]
            ws, chl_of, first = {}, {2: 0, 9: 1}, None
            for grp in rd.slots():
                offset, index, value, y = S.storage(rows, grp, S.ADFEA)
                keys = np.unique(index)
                v.setValue(Message(key_channel=chl_of[grp], key=keys))
                v.set_value_array(chl_of[grp], np.zeros(keys.size))
                _lib.check(v._L.psg_darling_init(v._h, chl_of[grp], DELTA_INIT))
                w = DarlingWorker(v._h, DELTA_INIT, DELTA_MAX)
                workers.append(w)
                if path == "device":
                    w.load_group(rd, grp, keys, dual_of=first)
                    assert same(w.mb.read("offset"), offset) and same(w.mb.read("index"), index)
                    assert same(w.mb.read("y"), y)
                else:
                    w.load(offset, index, value, y, keys)
                    if first is not None:
                        _lib.check(w._L.psg_mb_darling_share_dual(w.mb._h, first.mb._h))
                        _lib.check(w._L.psg_mb_darling_init(w.mb._h, DELTA_INIT, None, None))
                first = first or w
                ws[grp] = w
            for _ in range(2):
                blocks = run_pass(v, chl_of, ws, rd.example_info(), param)
            assert len(blocks) >= 3 and {b[0] for b in blocks} == {2, 9}
            pr = [server_progress(v, chl_of[g], param["lambda_"]) for g in (2, 9)]
            assert all(p["nnz_w"] > 0 for p in pr)
            weights.append([v.value(chl_of[g]) for g in (2, 9)] + [ws[2].state()["dual"]])
        for a, b in zip(*weights):
            assert same(a, b)
        assert not np.all(weights[0][2] == 1.0)
    finally:
        for w in workers[::-1]:
            w.close()
        for rd in readers:
            rd.close()
        for v in servers:
            v.close()
