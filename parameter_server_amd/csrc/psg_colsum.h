// psg_colsum.h -- the blocked summation order of the per-key (column) sums
// (PSG_SUM_BLOCKED, include/psg.h): its shape constants, shared by the
// kernels (psg_colsum.hip) and the host twin (psg_colsum.cc), and what the
// product entries of psg_worker.hip and psg_worker_rows.hip call.  No HIP
// type in here: the host twin is built without the runtime.
#pragma once
#include <stddef.h>
#include <stdint.h>

struct psg_minibatch;

namespace psg {

constexpr uint32_t kColSerial = 32;  // runs up to this: the serial chain (= kLongRun)
constexpr uint32_t kColLanes = 64;   // strided partials of a block, one per lane of a wave
constexpr uint32_t kColSeg = 4096;   // terms of a block; a longer run is cut into such segments

// The table of the runs longer than kColSeg and of their (run, segment)
// units, built on the device from the localized minibatch; enqueues only.
// psg_mb_localize calls it for a minibatch in blocked order, and
// colsum_enqueue does when the order was chosen after the localize.
int colsum_prepare(psg_minibatch* mb, void* stream);

// The sums of the runs longer than kColSerial in blocked order, over term
// rows [nnz][m] laid out in run order; the shorter runs are the short
// kernels' in both orders.  u == nullptr: g[k * m + j] for every key k.
// Otherwise (m == 2, the Darling pair of terms): g[k - cb] and u[k - cb] for
// the active keys of [cb, ce).  long_bound: at least the length of the long
// list, as far as the host knows it.  Enqueues only; no host wait.
int colsum_enqueue(psg_minibatch* mb, const double* term, int m, double* g, double* u,
                   uint32_t cb, uint32_t ce, const uint8_t* active, size_t long_bound,
                   void* stream);

}  // namespace psg
