// psg_ctx.h -- the server context behind the C ABI (include/psg.h), shared by
// the translation units that implement it: psg_runtime.hip (the context
// core), psg_ctx_freq.hip (frequency filter), psg_ctx_ftrl.hip (FTRL model),
// psg_ctx_dev.hip (device-array forms), psg_plan.hip (plans and the stateless
// device helpers).  Not installed.
//
// psg_ctx mirrors KVVector<uint64,V> (src/parameter/kv_vector.h:13-62): per
// channel sorted server keys key_[chl] and values val_[chl], and per time t
// the aggregate recved_val_[t].  Keys/values/aggregates live in the HBM of
// one device; a host mirror of key_[chl] serves findRange without a device
// round trip.  All device work is ordered on one HIP stream per context (the
// device-array forms run on their callers' streams and are tied to it by
// events, psg_ctx_dev.hip);
// a mutex gives the reference's threading contract (setValue on the
// executor thread, received() from the app thread, kv_vector.h:45,67).
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cmath>
#include <iterator>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <deque>
#include <map>
#include <memory>
#include <mutex>
#include <string>
#include <unordered_map>
#include <vector>

#include "../../include/psg.h"
#include "psg_host.h"
#include "psg_internal.h"
#include "psg_jobtable.h"

namespace psg {

inline size_t vsize(int dtype) { return dtype == PSG_F32 ? 4 : 8; }

inline int set_dev(int d) {
  HIP_TRY(hipSetDevice(d));
  return PSG_OK;
}

// Device keys of one push.  Shared: a key-cache entry (RNode::key_cache_,
// remote_node.h:92-93) and every pending push that was restored from it
// hold the same resident copy; the last owner returns it to the pool.
struct KeyBuf {
  uint64_t* d = nullptr;
  size_t n = 0, bytes = 0;
  // a dense push's keys left in the caller's pinned memory (d null): the
  // device-visible address its order check reads
  const uint64_t* host = nullptr;
};
using KeyRef = std::shared_ptr<KeyBuf>;

struct Channel {
  uint64_t* d_keys = nullptr;
  size_t n = 0, kbytes = 0;
  // host mirror of key_[chl] (findRange, key copies, psg_push's dense
  // test): after a key union the device key set is copied into pinned
  // memory asynchronously; readers wait for that copy (mirror())
  uint64_t* hk = nullptr;
  size_t hcap = 0;
  hipEvent_t hev = nullptr;
  bool hpend = false;
  const uint64_t* mirror() {
    if (hpend) {
      (void)hipEventSynchronize(hev);
      hpend = false;
    }
    return hk;
  }
  void* d_vals = nullptr;
  size_t nvals = 0;
  // Darling server state (darling.h:38-39): delta_[grp], active_set_[grp]
  double* d_delta = nullptr;
  uint32_t* d_active = nullptr;
  size_t dn = 0;
  // device forms (psg_ctx_dev.hip).  d_dev: kChanWordBytes of device words,
  // [0] the violation accumulated by psg_darling_update_dev, [1..2] the pull
  // kernel's count and ticket.  last / last_s: like a Filter's -- operations
  // on the channel's values run in call order whatever streams they are
  // enqueued on; each waits for the event recorded after the previous one
  // when their streams differ.
  unsigned long long* d_dev = nullptr;
  hipEvent_t last = nullptr;
  hipStream_t last_s = nullptr;
};
constexpr size_t kChanWordBytes = 64;

struct PendingPush {
  KeyRef keys;
  void* vblock = nullptr;  // the m value arrays
  size_t vbytes = 0;
  void* d_vals[psg::kMaxM] = {};
  int m = 0;  // value arrays of this push (the aggregate's list grows to the largest)
  uint64_t n = 0;
  // a contiguous slice of the server keys (psg_push's dense test): the merge
  // reads D[dpos, dpos + n) of the aggregate's range in place of the keys
  bool dense = false;
  uint64_t dpos = 0;           // position of the first key in [lo, hi)
  const uint64_t* kd = nullptr;  // D + lo + dpos
  // a compressed push's staging block (its parts, decoded on `copy`): held
  // until the merge that follows the decode
  void* sblock = nullptr;
  size_t sbytes = 0;
  // its parts still to decode (device addresses): input [cbeg, cend),
  // output cdst of ccap bytes -- decoded together with the other pending
  // compressed pushes right before the merge that needs them
  int cparts = 0;
  uint64_t cbeg[psg::kMaxM + 1] = {}, cend[psg::kMaxM + 1] = {};
  uint64_t cdst[psg::kMaxM + 1] = {}, ccap[psg::kMaxM + 1] = {};
};

// recved_val_[t] (kv_vector.h:189-196, 110-129): a list of value arrays that
// grows when a push brings more arrays than the earlier ones; array i is
// assigned by the first push holding an i-th array and added to by the later
// ones that hold one (a push without it leaves it alone)
// an aggregate's device counters: unmatched keys, compressed parts that failed
// to decode, pushes whose keys do not match their carried signature
constexpr size_t kBadBytes = 32;

struct Aggregate {
  int chl = 0, m = 0;                // m: arrays so far (the largest push's)
  size_t lo = 0, hi = 0;
  void* d_out[psg::kMaxM] = {};
  std::vector<PendingPush> pending;
  uint64_t folded = 0;               // pushes already merged into d_out
  uint64_t folded_arr[psg::kMaxM] = {};  // of them, those holding array i
  uint64_t expected_total = 0;
  // device: [0] pushed keys not matched so far, [1] compressed parts that
  // failed to decode (psg_push_compressed reports them here, asynchronously),
  // [2] pushes whose keys do not match their carried signature
  unsigned long long* d_bad = nullptr;
};

// key_cache_ of remote node `sender`, index (key_channel, key_range)
// (remote_node.cc:98-99,141-142)
struct CacheKey {
  int sender, chl;
  uint64_t kb, ke;
  bool operator<(const CacheKey& o) const {
    if (sender != o.sender) return sender < o.sender;
    return chl != o.chl ? chl < o.chl : kb != o.kb ? kb < o.kb : ke < o.ke;
  }
};
// The device check of a carried signature (keys + values message): its
// counter and the event after it on `copy`.  The entry that stored those
// keys is restorable only once the check passed; the reference checks before
// it stores (remote_node.cc:161-165).
struct SigCheck {
  unsigned long long* d = nullptr;  // the device counter (a slot of a counter slab)
  unsigned long long* h = nullptr;  // its pinned host copy, landed before `ev`
  uint32_t slot = 0;
  hipEvent_t ev = nullptr;
};
using SigCheckRef = std::shared_ptr<SigCheck>;
struct CacheEntry {
  uint32_t sig = 0;
  KeyRef keys;
  SigCheckRef chk;  // null: checked (or stored by a key-only message, checked at once)
};

// pinned host memory, and the address the device reads it at
inline bool host_pinned(const void* p, const void** dev = nullptr) {
  hipPointerAttribute_t a;
  if (hipPointerGetAttributes(&a, p) != hipSuccess) {
    (void)hipGetLastError();  // pageable memory: not an error for us
    return false;
  }
  if (a.type != hipMemoryTypeHost) return false;
  if (dev) {
    // the attribute's device pointer is the allocation's base: offset it
    const char* hb = (const char*)a.hostPointer;
    const char* db = (const char*)a.devicePointer;
    *dev = (hb && db) ? (const void*)(db + ((const char*)p - hb)) : nullptr;
  }
  return true;
}


// FreqencyFilter<uint64> of one channel (CountMin n_, k_, table)
struct Filter {
  uint8_t* d_table = nullptr;  // n byte counters (countmin.h:69)
  uint32_t n = 0;
  int k = 1;
  // the binned insert's records (psg_countmin.hip), grown on demand; the
  // filter's inserts are ordered on one stream (the context's, or the
  // caller's of psg_freq_insert_dev)
  void* d_bins = nullptr;
  size_t bins_bytes = 0;
  // the caller's stream of the last psg_freq_*_dev call: the table is not
  // recycled (clear / resize) before the kernels enqueued there finished
  hipStream_t ext = nullptr;
  bool ext_used = false;
  void sync_ext() {
    if (ext_used) (void)hipStreamSynchronize(ext);
    ext_used = false;
  }
  // the filter's operations run in call order whatever streams they are
  // enqueued on (the reference's calls are sequential): each one waits for
  // the event recorded after the previous one when their streams differ.
  // The binned insert reuses d_bins and writes table dwords with plain
  // read-modify-write stores, so two inserts must never overlap.
  hipEvent_t last = nullptr;
  hipStream_t last_s = nullptr;
};

// FTRLModel<uint64, double> of the context (ftrl_model.h:47-68): the
// parameters, the resident hash table (psg_ftrl.hip) and its head block
struct Ftrl {
  bool on = false;
  psg::FtrlParam P{};
  psg::FtrlBucket* d_tab = nullptr;
  uint64_t nb = 0;  // buckets, a power of two
  psg::FtrlHead* d_head = nullptr;
  // an upper bound on the entry count: the true count as last read plus
  // every key pushed since.  The device's count is read (a host wait) only
  // when the bound would pass the load limit.
  size_t bound = 0;
  // evaluation only (psg_ftrl_import's weights-only form: z is unknown, a
  // push would recompute w from it); pushes are refused
  bool frozen = false;
  // like a Filter's: the model's operations run in call order whatever
  // streams they are enqueued on
  hipEvent_t last = nullptr;
  hipStream_t last_s = nullptr;
  psg::FtrlTable table() const { return psg::FtrlTable{d_tab, nb - 1, d_head}; }
  // at most half of the 3 * nb slots are taken: probes stay short
  size_t limit() const { return (size_t)(3 * nb / 2); }
  static uint64_t buckets_for(size_t entries) {
    uint64_t nb = 1;
    while (3 * nb / 2 < entries) nb *= 2;
    return nb;
  }
};


#ifndef PSG_SPIN
#define PSG_SPIN 1
#endif
// the host waits for the end of a call's device work by polling its event
// for a bounded time: a pushing caller is blocked on it anyway, and the poll
// sees a short wait's completion sooner than a blocking wait's wake-up (the
// e2e pinned path waits once per push).  Past ~50 us it
// yields to a blocking wait, so threads waiting on long device work (the
// loopback exchange's ranks, several contexts) do not each burn a core
// (ADVICE r05).
inline hipError_t spin_wait(hipEvent_t e) {
#if PSG_SPIN
  const auto t0 = std::chrono::steady_clock::now();
  for (int i = 0;; ++i) {
    const hipError_t q = hipEventQuery(e);
    if (q != hipErrorNotReady) return q;
    if ((i & 15) == 15 && std::chrono::steady_clock::now() - t0 > std::chrono::microseconds(50))
      break;
  }
  return hipEventSynchronize(e);
#else
  return hipEventSynchronize(e);
#endif
}

// defined with their sections, called by psg_destroy
void filter_release(psg_ctx* c, Filter& F);
void ftrl_release(psg_ctx* c);

}  // namespace psg

// the translation units of the C ABI name these types unqualified
using namespace psg;

struct psg_ctx {
  int device = 0;
  int dtype = PSG_F32;
  unsigned flags = PSG_SERIAL_MATCH;
  hipStream_t stream = nullptr;  // kernels, D2H
  hipStream_t copy = nullptr;    // H2D of pushes / keys / values
  hipEvent_t copy_ev = nullptr;
  hipEvent_t done_ev = nullptr;  // end of a call's work on `stream` (spin_wait)

  std::mutex mu;
  std::unordered_map<int, Channel> ch;
  std::map<int, Aggregate> agg;
  std::map<CacheKey, CacheEntry> kcache;
  std::unordered_map<int, Filter> ff;
  Ftrl ftrl;
  JobTable table;
  unsigned long long* d_small = nullptr;  // 32 device words: counters, crc args
  unsigned long long* d_vio_slots = nullptr;  // psg::kVioSlots x 64 B, zero between updates
  unsigned long long* h_small = nullptr;  // 32 pinned host words
  // signature-check counters, pooled: slabs of kCtrSlab device
  // words and as many pinned host words their results are copied back into;
  // slot i lives in slab i / kCtrSlab
  static constexpr uint32_t kCtrSlab = 256;
  std::vector<unsigned long long*> ctr_d, ctr_h;
  std::vector<uint32_t> ctr_free;
  void* scratch = nullptr;
  size_t scratch_bytes = 0;
  size_t flush_pushes = psg::kMaxPush;  // pushes per aggregate launch

  // ---- device block pool.  Freed push, key and aggregate blocks, by size: a
  // server sees the same shapes every iteration, so after the first one no
  // push allocates.  A block is returned with an event recorded on `stream`
  // (the kernels that read it were enqueued there before); a writer on
  // another stream waits for that event before reusing it.
  struct Pooled {
    void* p;
    hipEvent_t ev;
  };
  std::multimap<size_t, Pooled> pool;
  size_t pool_bytes = 0;
  // the real size of every block this pool made (carved or allocated): a
  // reused block may be up to twice the size asked for, and the counts of
  // the pool and the slabs add and subtract that same size
  std::unordered_map<const void*, size_t> bsize;
  size_t real_size(const void* p, size_t b) const {
    auto it = bsize.find(p);
    return it == bsize.end() ? b : it->second;
  }
  std::vector<hipEvent_t> free_ev;
  static constexpr size_t kPoolCap = size_t(8) << 30;
  // ---- slabs: blocks up to kSlabBlock bytes (staged pushes, cached keys,
  // aggregates of a shard's range) are carved from kSlab-byte allocations
  // by a bump pointer and then cycle through the pool (never freed on their
  // own), so an aggregate's pushes sit back to back in a few large mappings
  // instead of one allocation each: the sparse kernel's tiles, which read a
  // few keys of each of hundreds of pushes, then touch far fewer address
  // translations (cfg5: 0.99 -> 0.74 ms for the same kernel, DESIGN.md 4.3;
  // bench.py --layout arena is this layout for the plan API)
#ifndef PSG_SLAB_BLOCK
#define PSG_SLAB_BLOCK (size_t(16) << 20)  // A/B builds: 0 = no slabs
#endif
  static constexpr size_t kSlab = size_t(256) << 20, kSlabBlock = PSG_SLAB_BLOCK;
  // carved: bytes handed out by the bump pointer; back: bytes of those
  // returned (in the pool, or dropped after a failed event).  A slab with
  // back == carved holds no live block and can be freed whole (reclaim_slabs:
  // when an allocation fails, or when idle carved bytes pass kPoolCap), so
  // blocks stranded by drifting sizes do not hold HBM for the context's life
  struct Slab {
    char* p;
    size_t size, carved, back;
  };
  std::vector<Slab> slabs;
  char* slab_cur = nullptr;
  size_t slab_left = 0;
  size_t slab_idle = 0;  // sum of back over the slabs
  int slab_of(const void* p) const {
    for (size_t i = 0; i < slabs.size(); ++i)
      if ((const char*)p >= slabs[i].p && (const char*)p < slabs[i].p + slabs[i].size)
        return (int)i;
    return -1;
  }
  bool in_slab(const void* p) const { return slab_of(p) >= 0; }
  // frees every slab none of whose blocks is live; returns the bytes freed
  size_t reclaim_slabs() {
    bool any = false;
    for (const Slab& s : slabs) any |= s.carved && s.back == s.carved;
    if (!any) return 0;
    // pooled blocks carry events on `stream`: once it is idle none is read
    (void)hipStreamSynchronize(stream);
    (void)hipStreamSynchronize(copy);
    size_t freed = 0;
    for (size_t i = 0; i < slabs.size();) {
      Slab& s = slabs[i];
      if (!(s.carved && s.back == s.carved)) {
        ++i;
        continue;
      }
      for (auto it = pool.begin(); it != pool.end();) {
        const char* q = (const char*)it->second.p;
        if (q >= s.p && q < s.p + s.size) {
          free_ev.push_back(it->second.ev);
          it = pool.erase(it);
        } else {
          ++it;
        }
      }
      for (auto it = bsize.begin(); it != bsize.end();) {
        const char* q = (const char*)it->first;
        it = (q >= s.p && q < s.p + s.size) ? bsize.erase(it) : std::next(it);
      }
      if (slab_cur >= s.p && slab_cur <= s.p + s.size) {
        slab_cur = nullptr;
        slab_left = 0;
      }
      slab_idle -= s.back;
      freed += s.size;
      (void)hipFree(s.p);
      slabs.erase(slabs.begin() + (ptrdiff_t)i);
    }
    return freed;
  }

  int event(hipEvent_t* e) {
    if (!free_ev.empty()) {
      *e = free_ev.back();
      free_ev.pop_back();
      return PSG_OK;
    }
    HIP_TRY(hipEventCreateWithFlags(e, hipEventDisableTiming));
    return PSG_OK;
  }

  int dev_get(size_t b, void** p, hipStream_t writer) {
    b = align_up(b ? b : 1, 4096);
    auto it = pool.lower_bound(b);
    if (it != pool.end() && it->first <= 2 * b) {
      *p = it->second.p;
      if (writer != stream) HIP_TRY(hipStreamWaitEvent(writer, it->second.ev, 0));
      free_ev.push_back(it->second.ev);
      const int si = slab_of(*p);
      if (si < 0) {
        pool_bytes -= it->first;
      } else {
        slabs[si].back -= it->first;
        slab_idle -= it->first;
      }
      pool.erase(it);
      return PSG_OK;
    }
    if (b <= kSlabBlock) {
      if (slab_left < b) {
        char* sp = nullptr;
        if (hipMalloc((void**)&sp, kSlab) != hipSuccess) {
          (void)hipGetLastError();
          if (reclaim_slabs() && hipMalloc((void**)&sp, kSlab) != hipSuccess) {
            (void)hipGetLastError();
            sp = nullptr;
          }
        }
        if (sp) {
          slabs.push_back(Slab{sp, kSlab, 0, 0});
          slab_cur = sp;
          slab_left = kSlab;
        }  // else no room for a slab: an allocation of its own
      }
      if (slab_left >= b) {
        *p = slab_cur;
        slab_cur += b;
        slab_left -= b;
        slabs[(size_t)slab_of(*p)].carved += b;
        bsize[*p] = b;
        return PSG_OK;
      }
    }
    if (hipMalloc(p, b) != hipSuccess) {
      (void)hipGetLastError();
      // idle slabs (blocks stranded by sizes that drifted) go back first
      if (!reclaim_slabs()) return fail(PSG_ERR_OOM, "device allocation of %zu bytes", b);
      HIP_TRY(hipMalloc(p, b));
    }
    bsize[*p] = b;
    return PSG_OK;
  }
  void dev_put(void* p, size_t b) {
    if (!p) return;
    // a deferred copy may target the block: issue it and order it before
    // the block's release event on `stream`
    if (zc.n) (void)join_copy();
    b = real_size(p, align_up(b ? b : 1, 4096));
    const int si = slab_of(p);  // a carved block is pooled (or counted back) always
    const bool carved = si >= 0;
    if (carved) {
      slabs[si].back += b;
      slab_idle += b;
    }
    hipEvent_t e = nullptr;
    if ((!carved && pool_bytes + b > kPoolCap) || event(&e) != PSG_OK ||
        hipEventRecord(e, stream) != hipSuccess) {
      if (e) free_ev.push_back(e);
      (void)hipStreamSynchronize(stream);
      if (!carved) {  // a carved block goes with its slab
        (void)hipFree(p);
        bsize.erase(p);
      }
      return;
    }
    pool.emplace(b, Pooled{p, e});
    if (!carved) pool_bytes += b;
    // idle carved bytes are bounded like the pool: whole idle slabs go back
    if (carved && slab_idle > kPoolCap) (void)reclaim_slabs();
  }
  void pool_release() {
    for (auto& kv : pool) {
      if (!in_slab(kv.second.p)) (void)hipFree(kv.second.p);
      (void)hipEventDestroy(kv.second.ev);
    }
    pool.clear();
    pool_bytes = 0;
    bsize.clear();
    for (auto& sl : slabs) (void)hipFree(sl.p);
    slabs.clear();
    slab_cur = nullptr;
    slab_left = 0;
    slab_idle = 0;
    for (hipEvent_t e : free_ev) (void)hipEventDestroy(e);
    free_ev.clear();
  }

  // the carried signature of resident keys checked on `copy` into a counter
  // of its own (the entry's), after the key copy, and -- one CRC for both
  //  -- into the aggregate's signature counter `agg` when given
  int ctr_get(uint32_t* slot) {
    if (ctr_free.empty()) {
      unsigned long long *d = nullptr, *h = nullptr;
      HIP_TRY(hipMalloc((void**)&d, 8 * kCtrSlab));
      if (hipHostMalloc((void**)&h, 8 * kCtrSlab) != hipSuccess) {
        (void)hipFree(d);
        return fail(PSG_ERR_DEVICE, "signature counter slab");
      }
      const uint32_t base = (uint32_t)ctr_d.size() * kCtrSlab;
      ctr_d.push_back(d);
      ctr_h.push_back(h);
      for (uint32_t i = kCtrSlab; i-- > 0;) ctr_free.push_back(base + i);
    }
    *slot = ctr_free.back();
    ctr_free.pop_back();
    return PSG_OK;
  }
  void ctr_release() {
    for (auto* d : ctr_d) (void)hipFree(d);
    for (auto* h : ctr_h) (void)hipHostFree(h);
    ctr_d.clear();
    ctr_h.clear();
    ctr_free.clear();
  }
  int sig_check_pending(const KeyRef& k, uint32_t sig, SigCheckRef* out,
                        unsigned long long* agg = nullptr) {
    SigCheck* s = new SigCheck();
    if (int rc = ctr_get(&s->slot)) {
      delete s;
      return rc;
    }
    s->d = ctr_d[s->slot / kCtrSlab] + s->slot % kCtrSlab;
    s->h = ctr_h[s->slot / kCtrSlab] + s->slot % kCtrSlab;
    int rc = event(&s->ev);
    if (rc == PSG_OK && (hipMemsetAsync(s->d, 0, 8, copy) != hipSuccess ||
                         psg::launch_sig_check((const uint8_t*)k->d, 8 * k->n, PSG_MAX_SIG_LEN,
                                               sig, s->d, copy, agg) != hipSuccess ||
                         hipMemcpyAsync(s->h, s->d, 8, hipMemcpyDeviceToHost, copy) != hipSuccess ||
                         hipEventRecord(s->ev, copy) != hipSuccess))
      rc = fail(PSG_ERR_DEVICE, "signature check launch");
    if (rc != PSG_OK) {
      (void)hipStreamSynchronize(copy);
      if (s->ev) free_ev.push_back(s->ev);
      ctr_free.push_back(s->slot);
      delete s;
      return rc;
    }
    *out = SigCheckRef(s, [this](SigCheck* q) {
      (void)hipEventSynchronize(q->ev);  // the counter slot is not reused under the check
      free_ev.push_back(q->ev);
      ctr_free.push_back(q->slot);
      delete q;
    });
    return PSG_OK;
  }
  // the result of a pending check: a wait for its event (once per stored
  // entry); the count is already in pinned host memory
  int sig_check_result(const SigCheckRef& s, bool* ok) {
    HIP_TRY(hipEventSynchronize(s->ev));
    *ok = *(volatile unsigned long long*)s->h == 0;
    return PSG_OK;
  }

  int new_keys(size_t n, KeyRef* out) { return new_keys(n, out, copy); }
  // `writer`: the stream the keys are written on
  int new_keys(size_t n, KeyRef* out, hipStream_t writer) {
    KeyBuf* k = new KeyBuf();
    k->n = n;
    k->bytes = 8 * n;
    if (int rc = dev_get(k->bytes, (void**)&k->d, writer)) {
      delete k;
      return rc;
    }
    *out = KeyRef(k, [this](KeyBuf* q) {
      dev_put(q->d, q->bytes);
      delete q;
    });
    return PSG_OK;
  }

  // ---- host -> device on `copy`.  The caller's buffer is free on return:
  // pinned memory is copied directly and waited for; pageable memory is
  // copied by the CPU into a pinned staging ring whose DMA runs on while
  // the caller goes on (no wait).
  char* ring = nullptr;
  size_t ring_cap = 0, ring_head = 0;
  struct Flight {
    size_t off, len;
    hipEvent_t ev;
  };
  std::deque<Flight> fly;
  static constexpr size_t kRingBytes = size_t(64) << 20;
  static constexpr size_t kRingPiece = size_t(4) << 20;

  int ring_reserve(size_t len, size_t* off) {
    if (!ring) {
      HIP_TRY(hipHostMalloc((void**)&ring, kRingBytes));
      ring_cap = kRingBytes;
    }
    if (ring_head + len > ring_cap) ring_head = 0;
    int last = -1;
    for (size_t i = 0; i < fly.size(); ++i)
      if (fly[i].off < ring_head + len && ring_head < fly[i].off + fly[i].len) last = (int)i;
    if (last >= 0) {  // events complete in order on `copy`
      HIP_TRY(hipEventSynchronize(fly[last].ev));
      for (int i = 0; i <= last; ++i) {
        free_ev.push_back(fly.front().ev);
        fly.pop_front();
      }
    }
    *off = ring_head;
    ring_head += len;
    return PSG_OK;
  }

  bool pinned_wait = false;  // a pinned copy of this call is still in flight
  bool zero_copy = true;     // pinned buffers read by a kernel, not a DMA copy
  // held pushes' pinned buffers (PSG_HOLD_BUFFERS: valid until received):
  // copied by one zero-copy launch when the merge needs them (join_copy)
  psg::HostCopyBatch zc;
  // a group of copies the caller flushes as one zero-copy launch (a
  // compressed push's parts), held buffers or not
  bool zc_group = false;
  int zc_flush() {
    if (zc.n == 0) return PSG_OK;
    const hipError_t e = psg::launch_host_copy_batch(zc, copy);
    zc.n = 0;
    HIP_TRY(e);
    return PSG_OK;
  }
  // `defer`: a push's keys or values, read by nothing before the merge
  int h2d(void* dst, const void* src, size_t len, bool defer = false) {
    if (!len) return PSG_OK;
    const void* sdev = nullptr;
    if (host_pinned(src, &sdev)) {
      // the GPU reads the caller's pinned buffer itself when both ends are
      // 16-B aligned (a DMA copy's fixed cost dominates at push sizes)
      const bool zok = zero_copy && sdev && (((uintptr_t)sdev | (uintptr_t)dst) & 15u) == 0;
      if (zok && ((defer && (flags & PSG_HOLD_BUFFERS)) || zc_group)) {
        if (zc.n == (uint32_t)psg::kHostCopyBatch)
          if (int rc = zc_flush()) return rc;
        zc.d[zc.n++] = psg::HostCopyDesc{sdev, dst, (uint64_t)len};
        if (!(flags & PSG_HOLD_BUFFERS)) pinned_wait = true;
        return PSG_OK;
      }
      if (zok)
        HIP_TRY(psg::launch_host_copy(dst, sdev, len, copy));
      else
        HIP_TRY(hipMemcpyAsync(dst, src, len, hipMemcpyHostToDevice, copy));
      pinned_wait = !(flags & PSG_HOLD_BUFFERS);
      return PSG_OK;
    }
    for (size_t done = 0; done < len;) {
      const size_t piece = std::min(len - done, kRingPiece);
      size_t off;
      if (int rc = ring_reserve(piece, &off)) return rc;
      memcpy(ring + off, (const char*)src + done, piece);
      HIP_TRY(hipMemcpyAsync((char*)dst + done, ring + off, piece, hipMemcpyHostToDevice, copy));
      hipEvent_t e;
      if (int rc = event(&e)) return rc;
      HIP_TRY(hipEventRecord(e, copy));
      fly.push_back(Flight{off, piece, e});
      done += piece;
    }
    return PSG_OK;
  }

  // device -> host on `stream`: into pinned memory the GPU writes itself
  // (zero-copy kernel, no DMA fixed cost), else a DMA copy
  int d2h(void* dst, const void* src, size_t len) {
    if (!len) return PSG_OK;
    const void* ddev = nullptr;
    if (zero_copy && host_pinned(dst, &ddev) && ddev &&
        (((uintptr_t)ddev | (uintptr_t)src) & 15u) == 0)
      HIP_TRY(psg::launch_host_copy((void*)ddev, src, len, stream));
    else
      HIP_TRY(hipMemcpyAsync(dst, src, len, hipMemcpyDeviceToHost, stream));
    return PSG_OK;
  }

  // end of an API call that staged caller buffers: they must be free on
  // return unless the caller holds them (PSG_HOLD_BUFFERS)
  int h2d_finish() {
    if (!pinned_wait) return PSG_OK;
    pinned_wait = false;
    HIP_TRY(hipEventRecord(copy_ev, copy));
    HIP_TRY(spin_wait(copy_ev));
    return PSG_OK;
  }

  // work enqueued on `stream` from now on sees every H2D issued so far
  int join_copy() {
    if (int rc = zc_flush()) return rc;
    HIP_TRY(hipEventRecord(copy_ev, copy));
    HIP_TRY(hipStreamWaitEvent(stream, copy_ev, 0));
    return PSG_OK;
  }

  // a channel's values in call order across streams (Channel::last)
  int chan_order(Channel& C, hipStream_t s) {
    if (C.last && C.last_s != s) HIP_TRY(hipStreamWaitEvent(s, C.last, 0));
    return PSG_OK;
  }
  int chan_mark(Channel& C, hipStream_t s) {
    if (!C.last)
      if (int rc = event(&C.last)) return rc;
    HIP_TRY(hipEventRecord(C.last, s));
    C.last_s = s;
    return PSG_OK;
  }

  int ensure_scratch(size_t b) {
    if (b <= scratch_bytes) return PSG_OK;
    HIP_TRY(hipStreamSynchronize(stream));
    if (scratch) HIP_TRY(hipFree(scratch));
    scratch = nullptr;
    scratch_bytes = 0;
    HIP_TRY(hipMalloc(&scratch, b));
    scratch_bytes = b;
    return PSG_OK;
  }

  void release_push(PendingPush& pp) {
    pp.keys.reset();
    dev_put(pp.vblock, pp.vbytes);
    pp.vblock = nullptr;
    // its decode (on `copy`) must be ordered before the release event
    // dev_put records on `stream`
    if (pp.sblock) (void)join_copy();
    dev_put(pp.sblock, pp.sbytes);
    pp.sblock = nullptr;
  }

  // Enqueue the merge of every pending push of `a` into its device output;
  // unmatched keys accumulate in a.d_bad.  No host wait.
  // `outs`: write the sums there instead of a.d_out (device-visible caller
  // arrays; only for a single launch that starts the aggregate).
  // `bad_host`: read a.d_bad back there right after the last launch, ahead
  // of the host-side release work (psg_received waits for it)
  int flush(Aggregate& a, void* const* outs = nullptr, void* bad_host = nullptr) {
    if (a.pending.empty()) return PSG_OK;
    while (!a.pending.empty()) {
      const size_t take = std::min(a.pending.size(), flush_pushes);
      // compressed pushes of this launch: all their parts decode in one
      // launch on `copy` (one wave per part, side by side), then the join
      void* dblk = nullptr;
      size_t dbytes = 0;
      if (int rc = decode_pending(a, take, &dblk, &dbytes)) return rc;
      if (int rc = join_copy()) return rc;
      // one job over every push and all arrays when each push holds all of
      // them and every array has the same history (the reference's apps:
      // always); otherwise one single-array job per array over the pushes
      // holding it (kv_vector.h:189-196).  Job 0 holds every push either way
      // (each has array 0): its unmatched count is the launch's
      bool uniform = true;
      for (size_t p = 0; p < take; ++p) uniform = uniform && a.pending[p].m == a.m;
      for (int i = 1; i < a.m; ++i)
        uniform = uniform && (a.folded_arr[i] > 0) == (a.folded_arr[0] > 0);
      const int jm = uniform ? a.m : 1;
      std::vector<JobSpec> jobs;
      for (int i = 0; i < (uniform ? 1 : a.m); ++i) {
        JobSpec js;
        js.keys = ch[a.chl].d_keys + a.lo;
        js.nslots = a.hi - a.lo;
        js.flags = (flags & PSG_PARALLEL_MATCH ? psg::kFlagParallel : 0u) |
                   (a.folded_arr[i] > 0 ? psg::kFlagCont : 0u);
        bool dense = true;
        for (size_t p = 0; p < take; ++p) {
          const PendingPush& pp = a.pending[p];
          if (pp.m <= i) continue;
          js.pkeys.push_back(pp.kd ? pp.kd : pp.keys->d);
          for (int k = 0; k < jm; ++k) js.pvals.push_back(pp.d_vals[i + k]);
          js.pn.push_back(pp.n);
          js.dpos.push_back(pp.dpos);
          dense = dense && pp.dense;
        }
        if (js.pn.empty()) continue;  // no push of this launch holds array i
        // every push a contiguous slice: the dense kernel (no key reads)
        js.dense = dense;
        if (!dense) js.dpos.clear();
        for (int k = 0; k < jm; ++k) js.out.push_back(outs ? outs[i + k] : a.d_out[i + k]);
        jobs.push_back(std::move(js));
      }
      if (int rc = table.build(device, dtype, jm, jobs, stream, true)) return rc;
      if (int rc = table.run(stream)) return rc;
      HIP_TRY(psg::launch_unmatched(table.d_jobs, 0, table.info[0].np, a.d_bad, stream));
      if (bad_host && take == a.pending.size())
        if (int rc = d2h(bad_host, a.d_bad, kBadBytes)) return rc;
      for (size_t p = 0; p < take; ++p) {
        for (int i = 0; i < a.pending[p].m; ++i) ++a.folded_arr[i];
        release_push(a.pending[p]);
      }
      a.pending.erase(a.pending.begin(), a.pending.begin() + take);
      a.folded += take;
      dev_put(dblk, dbytes);  // after the join: `stream` is past the decode
    }
    return PSG_OK;
  }

  void drop(Aggregate& a) {
    const size_t sv = vsize(dtype);
    for (auto& pp : a.pending) release_push(pp);
    a.pending.clear();
    for (int i = 0; i < a.m; ++i) dev_put(a.d_out[i], (a.hi - a.lo) * sv);
    dev_put(a.d_bad, kBadBytes);
  }

  // the value push behind psg_push / psg_push_cached / psg_push_compressed:
  // keys already resident; values staged from the host, or (vblock) already
  // resident in a pool block of m arrays of align_up(n * s_V, 256) bytes
  // `slice`: the push is D[*slice, *slice + n) (absolute positions) by its
  // end keys; its staged keys are checked strictly increasing on `copy`
  // (the order check that completes the proof, psg_push) into the
  // aggregate's unmatched counter
  int push_values(int chl, int time, uint64_t kb, uint64_t ke, const KeyRef& keys, int m,
                  const void* const* vals, void* vblock = nullptr,
                  const size_t* slice = nullptr, void* sblock = nullptr, size_t sbytes = 0,
                  const PendingPush* comp = nullptr);
  // findRange of a push and the consistency checks of setValue, before any
  // data is staged
  int check_push(int chl, int time, uint64_t kb, uint64_t ke, size_t n, int m, size_t* lo,
                 size_t* hi);
  int decode_pending(Aggregate& a, size_t take, void** blk, size_t* bytes);
  // the aggregate of `time` (created on first use) over [kb, ke) of chl
  int aggregate_for(int chl, int time, uint64_t kb, uint64_t ke, int m, Aggregate** out);
};
