// psg_score.h -- the direct scorer (psg_score.hip) as the two model sides of
// the context see it (psg_ctx_ftrl.hip, psg_ctx_ftrlm.hip): they find the
// model and keep its call order, this scores a loaded minibatch against it.
#pragma once
#include <hip/hip_runtime.h>

#include "../../include/psg.h"
#include "psg_ftrl_rows.h"
#include "psg_internal.h"

namespace psg {
// Xw of the loaded minibatch `mb` of context `c` against the scalar table
// (*T1, Tm null: xw[rows], null = the minibatch's own Xw) or the sweep's (*Tm,
// T1 null: xw[rows][m]), in `real` (PSG_SCORE_*), enqueued on s in the
// minibatch's call order.  No host wait unless a scratch block has to grow.
int mb_score(psg_minibatch* mb, psg_ctx* c, const FtrlTable* T1, const FtrlmTable* Tm, int real,
             double* xw, hipStream_t s);
}  // namespace psg
