"""Snappy compression of message parts: the device encoder
``psg_snappy_compress_dev`` and its host twin ``psg_snappy_compress_host``,
which give the same stream byte for byte.  What Van::send does per key and
value part (system/van.cc:121-131, SArray::compressTo).
"""
from __future__ import annotations

import ctypes as C
from typing import Optional, Sequence

import numpy as np

from . import _lib


def max_compressed_length(n: int) -> int:
    """32 + n + n // 6 (snappy::MaxCompressedLength): the room a part of n
    bytes needs."""
    return int(_lib.lib().psg_snappy_max_compressed_length(n))


def compress_host(data: bytes) -> bytes:
    """The stream of ``data`` by the host twin."""
    L = _lib.lib()
    data = bytes(data)
    cap = max_compressed_length(len(data))
    out = C.create_string_buffer(cap)
    n = C.c_size_t()
    _lib.check(L.psg_snappy_compress_host(data, len(data), out, cap, C.byref(n)))
    return out.raw[:n.value]


class _Raw:
    """(device pointer, nbytes) as torch reads it."""

    def __init__(self, ptr, nbytes):
        self.__cuda_array_interface__ = {"shape": (int(nbytes),), "typestr": "|u1",
                                         "data": (int(ptr), False), "version": 2}


def _as_bytes(torch, part):
    if hasattr(part, "data_ptr"):
        return part.contiguous().reshape(-1).view(torch.uint8)
    ptr, nbytes = part
    if not nbytes:
        return torch.empty(0, dtype=torch.uint8, device="cuda")
    return torch.as_tensor(_Raw(ptr, nbytes), device="cuda")


def compress_dev(parts: Sequence, stream: Optional[int] = None, to_host: bool = True):
    """Compresses device-resident parts in one call of psg_snappy_compress_dev
    on ``stream`` (a stream handle; None: torch's current stream).  parts:
    device tensors or (device pointer, nbytes) pairs.  Returns a list of
    ``bytes``; with ``to_host=False`` nothing waits and (dst, doff, clen) is
    returned: a device uint8 tensor, the parts' offsets in it and their
    streams' lengths (device int64 tensors), valid after the stream's work."""
    import torch
    L = _lib.lib()
    n = len(parts)
    if n == 0:
        return [] if to_host else tuple(
            torch.empty(0, dtype=t, device="cuda") for t in (torch.uint8, torch.int64, torch.int64))
    run = torch.cuda.current_stream() if stream is None else torch.cuda.ExternalStream(stream)
    with torch.cuda.stream(run):
        flat = [_as_bytes(torch, p) for p in parts]
        # the entry takes the parts back to back
        src = flat[0] if n == 1 else torch.cat(flat)
        soff = np.zeros(n + 1, np.uint64)
        np.cumsum([f.numel() for f in flat], out=soff[1:])
        doff = np.zeros(n + 1, np.uint64)
        np.cumsum([max_compressed_length(f.numel()) for f in flat], out=doff[1:])
        total = int(soff[-1])
        if total == 0:
            src = torch.zeros(1, dtype=torch.uint8, device=src.device)
        dev = src.device
        dst = torch.empty(int(doff[-1]), dtype=torch.uint8, device=dev)
        d_soff = torch.tensor(soff.view(np.int64), device=dev)
        d_doff = torch.tensor(doff.view(np.int64), device=dev)
        clen = torch.zeros(n, dtype=torch.int64, device=dev)
        scratch = torch.empty(int(L.psg_snappy_compress_scratch_bytes(total, n)),
                              dtype=torch.uint8, device=dev)
        _lib.check(L.psg_snappy_compress_dev(src.data_ptr(), d_soff.data_ptr(), n, dst.data_ptr(),
                                             d_doff.data_ptr(), clen.data_ptr(),
                                             scratch.data_ptr(), run.cuda_stream or None))
        if not to_host:
            # src and scratch go back to torch's allocator, which reuses them
            # only for work enqueued on this stream
            return dst, d_doff[:-1], clen
        run.synchronize()
        lens = clen.cpu().tolist()
        host = dst.cpu().numpy()
    return [host[int(o):int(o) + ln].tobytes() for o, ln in zip(doff[:-1].tolist(), lens)]
