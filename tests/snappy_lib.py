"""TEST INFRASTRUCTURE: the locally installed google snappy through its C
interface (snappy-c.h), loaded by ctypes.  Used by tools/record_snappy.py and
by the CPU checks of tests/test_snappy_pin.py that re-compress the cases;
where the library is absent, Snappy() raises OSError and those checks skip.
Never loaded by a GPU test: those read the recorded streams only.
"""
import ctypes as C
import ctypes.util
import glob
import os
import re
import sys


class Snappy:
    """snappy_compress / snappy_uncompress of the installed libsnappy."""

    def __init__(self):
        path = ctypes.util.find_library("snappy")
        if not path:
            # a conda lib directory is not on the loader's path: the active
            # environment, this interpreter's prefix, then the usual install
            # roots (an inactive base environment sets no variable)
            home = os.path.expanduser("~")
            for prefix in (os.environ.get("CONDA_PREFIX"), sys.prefix, "/opt/conda",
                           os.path.join(home, "miniconda3"), os.path.join(home, "anaconda3")):
                found = sorted(glob.glob(os.path.join(prefix, "lib", "libsnappy.so*"))) if prefix else []
                if found:
                    path = found[-1]
                    break
        if not path:
            raise OSError("libsnappy not found")
        self.lib = C.CDLL(path)
        # the file as resolved on disk: find_library gives a soname only, so
        # ask the process what it mapped
        real = path
        try:
            with open("/proc/self/maps") as maps:
                real = next(ln.split()[-1] for ln in maps if "libsnappy" in ln)
        except (OSError, StopIteration):
            pass
        self.file = os.path.basename(os.path.realpath(real))
        m = re.search(r"\.so\.(\d+(?:\.\d+)*)$", self.file)
        self.version = m.group(1) if m else "unknown"
        L = self.lib
        L.snappy_max_compressed_length.restype = C.c_size_t
        L.snappy_max_compressed_length.argtypes = [C.c_size_t]
        for f in (L.snappy_compress, L.snappy_uncompress):
            f.restype = C.c_int
            f.argtypes = [C.c_char_p, C.c_size_t, C.c_char_p, C.POINTER(C.c_size_t)]
        L.snappy_uncompressed_length.restype = C.c_int
        L.snappy_uncompressed_length.argtypes = [C.c_char_p, C.c_size_t, C.POINTER(C.c_size_t)]

    def compress(self, data):
        n = C.c_size_t(self.lib.snappy_max_compressed_length(len(data)))
        out = C.create_string_buffer(n.value)
        if self.lib.snappy_compress(data, len(data), out, C.byref(n)) != 0:
            raise RuntimeError("snappy_compress failed")
        return out.raw[: n.value]

    def uncompress(self, stream):
        """bytes, or None for a stream the library refuses."""
        n = C.c_size_t()
        if self.lib.snappy_uncompressed_length(stream, len(stream), C.byref(n)) != 0:
            return None
        out = C.create_string_buffer(max(1, n.value))
        if self.lib.snappy_uncompress(stream, len(stream), out, C.byref(n)) != 0:
            return None
        return out.raw[: n.value]
