"""GPU: the device snappy encoder (psg_snappy_enc.hip) against its host twin
(psg_snappy_compress_host, which tests/test_snappy_compress.py holds to real
snappy decoders on the CPU), byte for byte, on the pinned cases and the edge
inputs of tests/snappy_enc_inputs.py; its output through the device decoders
and psg_push_compressed; and the compressed pull reply.

Nothing here loads a snappy library.  The destination of every launch is
pre-filled: what lies behind a part's stream, up to the next part's start and
64 bytes past the last, must come back as filled.
"""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import oracle_py as O
import pin_cases as P
import snappy_enc_inputs as I
from test_gpu_parity import assert_bitexact, kvv, msg, torch_cuda  # noqa: F401

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FILL, TAIL = 0xA5, 64
_twin = {}


def twin(data):
    """The host twin's stream; each input compressed once."""
    from parameter_server_amd import snappy
    if data not in _twin:
        _twin[data] = snappy.compress_host(data)
    return _twin[data]


def gpu_compress(torch, parts, stream=None, keep=False):
    """One launch of psg_snappy_compress_dev over `parts` (bytes), back to
    back in the source, each with exactly its maximum compressed length of
    room in a destination pre-filled with FILL.  Returns the streams (keep:
    also the device tensors dst, doff, clen); asserts that nothing behind a
    stream was written."""
    from parameter_server_amd import _lib, snappy
    L = _lib.lib()
    n = len(parts)
    soff = np.concatenate([[0], np.cumsum([len(p) for p in parts])]).astype(np.uint64)
    doff = np.concatenate([[0], np.cumsum([snappy.max_compressed_length(len(p))
                                           for p in parts])]).astype(np.uint64)
    total, room = int(soff[-1]), int(doff[-1])
    src = torch.tensor(np.frombuffer(b"".join(parts) + b"\0", np.uint8).copy(), device="cuda")
    dst = torch.full((room + TAIL,), FILL, dtype=torch.uint8, device="cuda")
    d_soff = torch.tensor(soff.view(np.int64), device="cuda")
    d_doff = torch.tensor(doff.view(np.int64), device="cuda")
    clen = torch.full((n,), -1, dtype=torch.int64, device="cuda")
    scratch = torch.empty(L.psg_snappy_compress_scratch_bytes(total, n), dtype=torch.uint8,
                          device="cuda")
    torch.cuda.synchronize()
    _lib.check(L.psg_snappy_compress_dev(src.data_ptr(), d_soff.data_ptr(), n, dst.data_ptr(),
                                         d_doff.data_ptr(), clen.data_ptr(), scratch.data_ptr(),
                                         stream))
    torch.cuda.synchronize()
    lens = clen.cpu().tolist()
    out = dst.cpu().numpy()
    got = []
    for i in range(n):
        a, b = int(doff[i]), int(doff[i + 1])
        assert 1 <= lens[i] <= b - a, (i, lens[i])
        got.append(out[a:a + lens[i]].tobytes())
        assert (out[a + lens[i]:b] == FILL).all(), "part %d: bytes behind its stream were written" % i
    assert (out[room:] == FILL).all(), "the tail behind the last part was written"
    return (got, dst, d_doff, clen) if keep else got


def assert_twin(got, parts, names):
    for g, p, n in zip(got, parts, names):
        want = twin(p)
        if g != want:
            m = min(len(g), len(want))
            a, b = np.frombuffer(g[:m], np.uint8), np.frombuffer(want[:m], np.uint8)
            bad = np.nonzero(a != b)[0]
            raise AssertionError("%s: %d bytes against the twin's %d, the first difference at %s"
                                 % (n, len(g), len(want), bad[0] if bad.size else m))


def lead_part(n):
    return bytes(range(1, n + 1))


def test_each_input_alone(torch_cuda):
    """Every pinned case and every edge input, one part per launch."""
    for name, data in I.all_inputs():
        assert_twin(gpu_compress(torch_cuda, [data]), [data], [name])


@pytest.mark.parametrize("rep", [1, 4], ids=["74parts", "296parts"])
def test_all_in_one_launch(torch_cuda, rep):
    """All of them back to back in one launch (more than 64 parts), and the
    list four times over (a few hundred)."""
    names = [n for n, _ in I.all_inputs()] * rep
    parts = [d for _, d in I.all_inputs()] * rep
    assert len(parts) > (64 if rep == 1 else 256)
    assert_twin(gpu_compress(torch_cuda, parts), parts, names)


@pytest.mark.parametrize("lead", [1, 7, 15])
def test_off_alignment(torch_cuda, lead):
    """A lead part of 1, 7 and 15 bytes in front: the sources start at that
    offset and the destinations at 33, 39 and 47, off 16-byte alignment; one
    input alone behind the lead, then all of them."""
    torch = torch_cuda
    names = [n for n, _ in I.all_inputs()]
    parts = [d for _, d in I.all_inputs()]
    ld = lead_part(lead)
    for name in ("pin_f32_eighths", "periodic%d" % (2 * I.FRAGMENT + 1)):
        data = dict(I.all_inputs())[name]
        assert_twin(gpu_compress(torch, [ld, data]), [ld, data], ["lead", name])
    assert_twin(gpu_compress(torch, [ld] + parts), [ld] + parts, ["lead"] + names)


def test_same_stream_alone_among_others_and_on_a_second_stream(torch_cuda):
    """A part's stream does not depend on what else the launch holds, nor on
    the stream handle it is enqueued on."""
    torch = torch_cuda
    A = dict(I.all_inputs())
    names = ["pin_keys_dense", "pin_alpha4", "periodic%d" % (I.FRAGMENT + 1), "match65"]
    alone = {n: gpu_compress(torch, [A[n]])[0] for n in names}
    parts = [A[n] for n in names]
    among = gpu_compress(torch, [A["pin_abc"]] + parts + [A["pin_records"]])[1:-1]
    side = torch.cuda.Stream()
    second = gpu_compress(torch, parts, stream=side.cuda_stream)
    for i, n in enumerate(names):
        assert alone[n] == among[i] == second[i] == twin(A[n]), n


def test_python_mirror(torch_cuda):
    """parameter_server_amd.snappy.compress_dev: device tensors and (pointer,
    nbytes) pairs, an empty part among them, on torch's current stream and on
    a second stream handle; and its device-side result."""
    torch = torch_cuda
    from parameter_server_amd import snappy
    A = dict(I.all_inputs())
    datas = [A["pin_f32_eighths"], b"", A["periodic%d" % (I.FRAGMENT + 1)], A["len3"]]
    dev = [torch.tensor(np.frombuffer(d + b"\0", np.uint8).copy(), device="cuda")[:len(d)]
           for d in datas]
    want = [twin(d) for d in datas]
    assert snappy.compress_dev(dev) == want
    pairs = [(t.data_ptr(), t.numel()) for t in dev]
    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    assert snappy.compress_dev(pairs, stream=side.cuda_stream) == want
    dst, doff, clen = snappy.compress_dev(dev[:1], to_host=False)
    torch.cuda.synchronize()
    n = int(clen.cpu()[0])
    assert int(doff.cpu()[0]) == 0 and dst[:n].cpu().numpy().tobytes() == want[0]
    assert snappy.compress_dev([]) == []


@pytest.mark.parametrize("rep", [1, 2], ids=["table_and_streamed", "per_wave"])
def test_round_trip_on_the_device(torch_cuda, rep):
    """The encoder's output through psg_snappy_uncompress_dev, in launches of
    <= 64 parts (the table and streamed forms) and of more (the per-wave
    form): status 0 and the input's bytes."""
    torch = torch_cuda
    from parameter_server_amd import _lib
    L = _lib.lib()
    inputs = I.all_inputs()
    groups = [inputs[:len(inputs) // 2], inputs[len(inputs) // 2:]] if rep == 1 else [inputs * rep]
    for group in groups:
        parts = [d for _, d in group]
        assert (len(parts) <= 64) == (rep == 1)
        got, dst, d_doff, clen = gpu_compress(torch, parts, keep=True)
        lens = clen.cpu().tolist()
        offs = d_doff.cpu().tolist()
        # the streams back to back, gathered on the device
        packed = torch.cat([dst[offs[i]:offs[i] + lens[i]] for i in range(len(parts))] +
                           [torch.zeros(1, dtype=torch.uint8, device="cuda")])
        soff = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
        doff = np.concatenate([[0], np.cumsum([len(p) for p in parts])]).astype(np.int64)
        out = torch.full((int(doff[-1]) + TAIL,), FILL, dtype=torch.uint8, device="cuda")
        st = torch.full((len(parts),), 7, dtype=torch.int32, device="cuda")
        d_soff, d_out = torch.tensor(soff, device="cuda"), torch.tensor(doff, device="cuda")
        _lib.check(L.psg_snappy_uncompress_dev(packed.data_ptr(), d_soff.data_ptr(), len(parts),
                                               out.data_ptr(), d_out.data_ptr(), st.data_ptr(),
                                               None))
        torch.cuda.synchronize()
        assert st.cpu().tolist() == [0] * len(parts)
        back = out.cpu().numpy().tobytes()
        assert back[:int(doff[-1])] == b"".join(parts)
        assert back[int(doff[-1]):] == bytes([FILL]) * TAIL


def test_push_compressed_accepts_the_encoders_parts(torch_cuda):
    """The key and value parts of pin_cases.snappy_push("A"), compressed on
    the device, through psg_push_compressed: received(t) has the bits of the
    plain push."""
    torch = torch_cuda
    from parameter_server_amd import _lib, snappy
    c = P.snappy_push("A")
    comp, plain = kvv(c.dtype), kvv(c.dtype)
    for v in (comp, plain):
        v.setValue(msg(c.D))
    clean = [c.pushes[p] for p in c.clean]
    for k, vs in clean:
        dev = [torch.tensor(k.view(np.int64), device="cuda")] + \
              [torch.tensor(x, device="cuda") for x in vs]
        streams = snappy.compress_dev(dev)
        assert streams == [twin(P.le_bytes(a)) for a in [k] + [P.fbits(x) for x in vs]]
        ck, cv = streams[0], streams[1:]
        bufs = [C.create_string_buffer(b, len(b)) for b in cv]
        arr = _lib.ptr_array([C.cast(b, C.c_void_p).value for b in bufs])
        sizes = (C.c_size_t * len(cv))(*[len(b) for b in cv])
        _lib.check(comp._L.psg_push_compressed(comp._h, 0, 1, 0, P.U64, ck, len(ck), len(cv), arr,
                                               sizes))
        plain.setValue(msg(k, vs, t=1))
    got, ref = comp.received(1), plain.received(1)
    assert len(got) == len(ref) == c.m
    for i in range(c.m):
        assert tuple(got[i][0]) == tuple(ref[i][0])
        assert np.array_equal(P.fbits(got[i][1]), P.fbits(ref[i][1])), i
    comp.close()
    plain.close()


def _server(dtype):
    """20,000 server keys below 2^40 with values in eighths, and a request of
    6,000 of them with repeats and with keys the server does not hold."""
    D = P.keys_below(47000, 20000, 40)
    W = P.quantised(47001, D.size).astype(dtype)
    pick = D[(P.splitmix64(47002, 6000) % np.uint64(D.size)).astype(np.int64)]  # repeats
    absent = P.splitmix64(47003, 600) >> np.uint64(24)
    absent = absent[~np.isin(absent, D)]
    req = np.sort(np.concatenate([pick, absent, pick[:50]]))
    return D, W, req


@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
def test_gather_compressed(torch_cuda, dtype):
    """The compressed pull reply: out_bytes is the twin's length for the
    gathered values, the stream decodes (oracle) to exactly psg_gather's
    bytes, matched is equal; n = 1 and n = 0; a cap one byte short is
    PSG_ERR_SIZE with nothing written; unsorted keys are PSG_ERR_UNSORTED."""
    from parameter_server_amd import _lib, snappy
    D, W, req = _server(dtype)
    assert np.unique(req).size < req.size and not np.isin(req, D).all()
    v = kvv(dtype)
    v.setValue(msg(D))
    v.set_value_array(0, W)
    for r in (req, req[:1], req[:0], req[-1:]):
        plain = msg(r)
        want_m = v.getValue(plain)
        want = plain.value[0].tobytes() if r.size else b""
        if r.size > 1:
            gw, gm = O.gather(D, W, r, dtype)
            assert gm == want_m and gw.tobytes() == want
        stream, got_m = v.getValueCompressed(msg(r))
        assert got_m == want_m
        assert len(stream) == len(twin(want)) and stream == twin(want)
        assert O.snappy_uncompress(stream) == want
    assert len(v.getValueCompressed(msg(req))[0]) < req.size * np.dtype(dtype).itemsize
    # room: one byte short of the maximum is refused before anything runs
    cap = snappy.max_compressed_length(req.size * np.dtype(dtype).itemsize)
    out = np.full(cap, FILL, np.uint8)
    nb, mt = C.c_size_t(77), C.c_size_t(77)
    rc = v._L.psg_gather_compressed(v._h, 0, req.ctypes.data, req.size, out.ctypes.data, cap - 1,
                                    C.byref(nb), C.byref(mt))
    assert rc == _lib.PSG_ERR_SIZE and (out == FILL).all() and nb.value == 77 and mt.value == 77
    # unsorted keys, as psg_gather
    bad = req.copy()
    bad[[10, 4000]] = bad[[4000, 10]]
    for call in (v.getValue, v.getValueCompressed):
        with pytest.raises(_lib.PSGError) as e:
            call(msg(bad))
        assert e.value.status == _lib.PSG_ERR_UNSORTED
    rc = v._L.psg_gather_compressed(v._h, 0, bad.ctypes.data, bad.size, out.ctypes.data, cap,
                                    C.byref(nb), C.byref(mt))
    assert rc == _lib.PSG_ERR_UNSORTED and (out == FILL).all()
    # and the context still answers
    assert v.getValueCompressed(msg(req))[0] == twin(
        O.gather(D, W, req, dtype)[0].tobytes())
    v.close()


def test_cpp_adapter_get_value_compressed(torch_cuda, tmp_path):
    """KVVector::getValueCompressed of csrc/kv_vector.h, built with plain g++
    against libpsg.so as tests/test_cpp_adapter.py builds its driver."""
    lib, orc = os.path.join(ROOT, "parameter_server_amd"), os.path.join(ROOT, "oracle")
    exe = str(tmp_path / "test_kv_vector_compressed")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror",
                    os.path.join(ROOT, "tests", "cpp", "test_kv_vector_compressed.cc"),
                    "-o", exe, f"-L{lib}", "-lpsg", f"-L{orc}", "-lorc",
                    f"-Wl,-rpath,{lib}", f"-Wl,-rpath,{orc}"], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
