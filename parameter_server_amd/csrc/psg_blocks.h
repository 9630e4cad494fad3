// psg_blocks.h -- what the device-resident handles (psg_minibatch, psg_auc)
// are built on: N device blocks that only grow, a few control words on the
// device with their pinned mirror, and the event that orders a handle's work
// across the streams its calls name.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>

#include <initializer_list>

#include "../../include/psg.h"
#include "psg_host.h"

namespace psg {

template <int N>
struct DeviceBlocks {
  psg_ctx* ctx = nullptr;
  int device = 0;
  hipStream_t stream = nullptr;  // the context's
  hipEvent_t ev = nullptr;       // the last enqueue, for calls on another stream
  hipStream_t last_s = nullptr;
  struct Buf {
    void* p = nullptr;
    size_t cap = 0;
  } b[N];
  unsigned long long* d_small = nullptr;
  unsigned long long* h_small = nullptr;  // pinned, 8 words
  struct Want {
    int id;
    size_t bytes;
  };

  template <class T>
  T* at(int id) const {
    return (T*)b[id].p;
  }
  // Buffers only grow.  Growing one frees the old block, which waits for the
  // device, so nothing in flight can still use it.
  int need(int id, size_t bytes) {
    if (bytes <= b[id].cap) return PSG_OK;
    if (b[id].p) HIP_TRY(hipFree(b[id].p));
    b[id].p = nullptr;
    b[id].cap = 0;
    const size_t cap = (bytes + 4095) / 4096 * 4096;
    HIP_TRY(hipMalloc(&b[id].p, cap));
    b[id].cap = cap;
    return PSG_OK;
  }
  int need_all(std::initializer_list<Want> want) {
    for (const Want& w : want)
      if (int rc = need(w.id, w.bytes)) return rc;
    return PSG_OK;
  }
  int order(hipStream_t s) {
    if (last_s && last_s != s) HIP_TRY(hipStreamWaitEvent(s, ev, 0));
    return PSG_OK;
  }
  int mark(hipStream_t s) {
    HIP_TRY(hipEventRecord(ev, s));
    last_s = s;
    return PSG_OK;
  }
  // everything enqueued for this handle, on whatever stream, has run
  int settle() {
    if (last_s && last_s != stream) HIP_TRY(hipStreamSynchronize(last_s));
    HIP_TRY(hipStreamSynchronize(stream));
    return PSG_OK;
  }
  hipStream_t pick(void* s) const { return s ? (hipStream_t)s : stream; }

  // The context's device (the current one already) and stream, the control
  // words and the event.  false: something could not be had; close() frees
  // what was.
  bool open(psg_ctx* c, size_t small_bytes) {
    int dtype;
    ctx = c;
    ctx_info(c, &device, &dtype, &stream);
    if (hipMalloc((void**)&d_small, small_bytes) != hipSuccess ||
        hipHostMalloc((void**)&h_small, 64) != hipSuccess ||
        hipEventCreateWithFlags(&ev, hipEventDisableTiming) != hipSuccess) {
      (void)hipGetLastError();
      return false;
    }
    return true;
  }
  // waits for the handle's work, then frees the blocks, the control words and
  // the event
  void close() {
    (void)hipSetDevice(device);
    if (last_s && last_s != stream) (void)hipStreamSynchronize(last_s);
    (void)hipStreamSynchronize(stream);
    for (auto& x : b)
      if (x.p) (void)hipFree(x.p);
    if (d_small) (void)hipFree(d_small);
    if (h_small) (void)hipHostFree(h_small);
    if (ev) (void)hipEventDestroy(ev);
  }
};

}  // namespace psg
