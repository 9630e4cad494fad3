"""parameter_server_amd -- MI355X-native server-side push aggregation for
the wakensky/parameter_server push/pull KV surface.

The product is libpsg.so (HIP kernels for gfx950 + host runtime) behind the
C ABI in include/psg.h; this package holds its ctypes binding, a Python
mirror of KVVector for tests and tools, and synthetic workload generators.
"""
from ._lib import PSGError, lib  # noqa: F401

from .ftrl import FTRLMultiModel  # noqa: F401,E402
from .worker import FTRLMultiWorker, FTRLWorker, Minibatch  # noqa: F401,E402
from .darling import (DarlingWorker, DarlingMultiWorker, DarlingMultiServer,  # noqa: F401,E402
                      darling_pass_rows)
from .auc import AUC, AUCRows, exact_auc, exact_auc_rows  # noqa: F401,E402
from .slots import SlotReader  # noqa: F401,E402
from .slot_cache import CachedSlotReader  # noqa: F401,E402
from .kv_vector import RowMergePlan, gather_rows_dev, rows_shape  # noqa: F401,E402

__all__ = ["PSGError", "lib", "FTRLWorker", "FTRLMultiModel", "FTRLMultiWorker", "Minibatch",
           "DarlingWorker", "DarlingMultiWorker", "DarlingMultiServer", "darling_pass_rows",
           "AUC", "AUCRows", "exact_auc", "exact_auc_rows", "SlotReader", "CachedSlotReader",
           "RowMergePlan",
           "gather_rows_dev", "rows_shape"]
