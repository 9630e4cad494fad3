/*
 * psg.h -- C ABI of the MI355X-native server-side push aggregation path.
 *
 * This is the drop-in boundary that replaces the host-side hot path of
 * wakensky/parameter_server:
 *
 *   KVVector<uint64,V>::setValue / serialSetValue / parallelSetValue
 *       src/parameter/kv_vector.h:75-82, 84-137, 171-204
 *   KVVector<uint64,V>::received          src/parameter/kv_vector.h:65-73
 *   KVVector<uint64,V>::getValue (pull)   src/parameter/kv_vector.h:206-227
 *   match / oldMatch merge kernels        src/system/message.h:134-267
 *   SArray::setUnion / findRange          src/base/shared_array_inl.h:155-171
 *   sliceKeyOrderedMsg / Range::evenDivide src/system/message.h:89-123,
 *                                          src/base/range.h:85-98
 *
 * The reference calls these from SharedParameter<K>::process on the
 * customer's executor thread (src/parameter/shared_parameter.h:91-149).
 * Every entry point here takes plain pointers and sizes; none retains a
 * caller pointer past the call (host data is staged before return), and
 * every failure the reference turns into a glog CHECK abort is returned as
 * a negative psg_status instead (the C++ adapter converts it back to an
 * abort, see parameter_server_amd/csrc/kv_vector.h).
 *
 * Keys are uint64 (the reference's PS::Key); values are float or double
 * (KVVector<Key,double> in linear_method/batch_solver.h:32).
 */
#ifndef PSG_H_
#define PSG_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PSG_ABI_VERSION 1
#define PSG_MAX_VALUE_ARRAYS 4   /* m: value arrays per push (Darling: 2) */

typedef enum psg_status {
  PSG_OK = 0,
  PSG_ERR_ARG = -1,        /* bad argument (null pointer, m out of range ...) */
  PSG_ERR_UNMATCHED = -2,  /* CHECK_EQ(recv_key.size(), n)  kv_vector.h:134,192 */
  PSG_ERR_RANGE = -3,      /* CHECK_EQ(range, stored range) kv_vector.h:128,199 */
  PSG_ERR_NO_TIME = -4,    /* CHECK(it != recved_val_.end()) kv_vector.h:69 */
  PSG_ERR_OOM = -5,
  PSG_ERR_DEVICE = -6,     /* HIP runtime error / no device */
  PSG_ERR_UNSORTED = -7,   /* key-only push not strictly increasing */
  PSG_ERR_SIZE = -8,       /* CHECK_EQ(recv_data.size(), recv_key.size()) :108,187 */
  PSG_ERR_CHANNEL = -9,    /* pushes of one time t name different channels */
  PSG_ERR_EMPTY_KEYS = -10, /* value push to a channel with no server keys */
  PSG_ERR_SIGNATURE = -11   /* key signature / key cache mismatch
                               CHECK_EQ remote_node.cc:163,174 */
} psg_status;

typedef enum psg_dtype { PSG_F32 = 0, PSG_F64 = 1 } psg_dtype;

/* Aggregation semantics (FLAGS_parallel_match, system/postoffice.cc:24).
 * SERIAL (the shipped default, script/local.sh:35) adds an explicit +0.0 for
 * keys absent from a later push (kv_vector.h:200), so a -0.0 can become
 * +0.0; PARALLEL touches only matched keys (message.h:195-198).  Both are
 * reproduced bit-exactly. */
#define PSG_SERIAL_MATCH 0u
#define PSG_PARALLEL_MATCH 1u
/* Context option (psg_create / psg_set_match_flags flags): the caller keeps
 * the key and value buffers of psg_push / psg_push_cached valid and
 * unmodified until psg_received of that time returns -- as the reference's
 * MessagePtr keeps a message's SArrays alive -- so pinned buffers are DMA'd
 * without a wait per push.  Without it every push returns with the caller's
 * buffers free. */
#define PSG_HOLD_BUFFERS 0x100u
/* Kernel-form overrides, for tests and A/B measurements (flags of
 * psg_plan_create, psg_create and psg_set_match_flags).  By default the
 * runtime picks each form from the shape of the pushes; the results are
 * bit-identical whichever form runs.  No environment variable changes the
 * path. */
#define PSG_FORM_PACKED 0x1000u   /* rounds that pack several pushes (short pieces) */
#define PSG_FORM_UNIFORM 0x2000u  /* rounds of one push each (long pieces) */
#define PSG_PART_SEARCH 0x4000u   /* partition: one search per (push, tile boundary) */
#define PSG_PART_STREAM 0x8000u   /* partition: every push key read once */
#define PSG_GROUP32 0x10000u      /* uniform rounds: groups of 32 pushes, 1024-slot tiles */
#define PSG_GROUP64 0x20000u      /* uniform rounds: groups of 64 pushes, 2048-slot tiles */
#define PSG_NO_DENSE 0x40000u     /* never the dense (contiguous-slice) kernel */
#define PSG_NO_ZERO_COPY 0x80000u /* context: DMA copies instead of GPU reads of pinned memory */
#define PSG_NO_INDEX 0x100000u    /* plan: no resident bucket index (tables built per run) */
#define PSG_FORM_CURSOR 0x400000u /* plan: a cursor form (no partition pass) where it applies */
#define PSG_NO_CURSOR 0x800000u   /* plan: never a cursor form (the default) */
#define PSG_NO_HINTS 0x1000000u   /* plan: the search partition never tries the last run's cuts first */
/* Plan option (psg_plan_create): the caller promises that the push KEYS at
 * the job's device pointers stay as they were at creation for the plan's
 * lifetime (values may change between runs).  Only then may the plan take
 * the dense kernel for pushes that are contiguous slices of D: that kernel
 * reads no push keys, so it cannot see a key that changed.  Without this
 * flag every run partitions and order-checks the keys it merges, and a
 * changed key is reported through psg_plan_matched.  (D itself is always
 * fixed for a plan's lifetime: its bucket index is built at creation.) */
#define PSG_STATIC_KEYS 0x200000u

int psg_abi_version(void);
const char* psg_status_string(int status);
/* Thread-local text of the last error returned on this thread. */
const char* psg_last_error(void);
int psg_device_count(int* n);

/* ------------------------------------------------------------------ */
/* Server context: one KVVector<uint64,V> whose keys, values and      */
/* per-time aggregates are resident in the HBM of one device.         */
/* ------------------------------------------------------------------ */
typedef struct psg_ctx psg_ctx;

int psg_create(int device, int dtype, unsigned flags, psg_ctx** out);
int psg_destroy(psg_ctx* ctx);
int psg_set_match_flags(psg_ctx* ctx, unsigned flags);
/* Pushes of one time merged per launch (default and maximum
 * psg_plan_max_push()); an aggregate of more pushes continues across
 * launches with the same bits.  Lower values force launch seams (tests). */
int psg_set_flush_pushes(psg_ctx* ctx, int n);

/* Key-only push: key_[chl] = key_[chl].setUnion(keys); val_[chl].clear()
 * (kv_vector.h:177-182).  keys must be strictly increasing. */
int psg_key_union(psg_ctx* ctx, int chl, const uint64_t* keys, size_t n);
/* npush key-only pushes at once: the same key set as psg_key_union of each
 * in order (the union is order-free), merged on the device in one N-way
 * pass per psg_nway_max_push() - 1 pushes (BatchSolver::preprocessData's
 * key pushes, batch_solver.cc:318-323).  Empty pushes are ignored. */
int psg_key_union_batch(psg_ctx* ctx, int chl, const uint64_t* const* keys, const size_t* n,
                        int npush);
/* key(chl).size() / copy of key(chl)[off, off+n) (kv_vector.h:17). */
int psg_key_size(psg_ctx* ctx, int chl, size_t* n);
int psg_key_copy(psg_ctx* ctx, int chl, size_t off, size_t n, uint64_t* out);
/* find(chl, [kb,ke)) = key_[chl].findRange (kv_vector.h:21-23). */
int psg_find_range(psg_ctx* ctx, int chl, uint64_t kb, uint64_t ke,
                   size_t* lo, size_t* hi);
/* value(chl) (kv_vector.h:18): replace / read the server values. */
int psg_value_assign(psg_ctx* ctx, int chl, const void* vals, size_t n);
int psg_value_size(psg_ctx* ctx, int chl, size_t* n);
int psg_value_copy(psg_ctx* ctx, int chl, size_t off, size_t n, void* out);

/* Value push: setValue(msg) for msg->value of m arrays, each n entries,
 * msg->task.key_range() = [kb, ke), msg->task.time() = time,
 * msg->task.key_channel() = chl.  vals[i] points to array i.  The caller's
 * buffers are free on return: pinned host memory (hipHostMalloc /
 * hipHostRegister) is DMA'd directly, pageable memory is copied into a
 * pinned staging ring whose DMA continues after return.  The merge runs
 * asynchronously on the context's stream and its match check is reported
 * by psg_received for `time`.  Pushes of one `time` may carry different m:
 * the aggregate's list of arrays grows to the largest (recved_val_[t],
 * kv_vector.h:110-129,189-196); array i is assigned by the first push
 * holding an i-th array and added to by the later pushes holding one. */
int psg_push(psg_ctx* ctx, int chl, int time, uint64_t kb, uint64_t ke,
             const uint64_t* keys, size_t n, int m, const void* const* vals);

/* Value push of snappy-compressed parts, as they arrive off the wire
 * (Van::recv with task.uncompressed_size set, van.cc:204-214): the key part
 * (uint64 keys) and m value parts are DMA'd compressed and decompressed on
 * the device (psg_snappy_uncompress_dev), then pushed like psg_push.
 * Parts of inconsistent declared sizes are PSG_ERR_SIZE here (the
 * reference's CHECKs).  The decode runs asynchronously (the caller's
 * buffers are free on return, as for psg_push): a part that fails to decode
 * is reported by psg_received(time) as PSG_ERR_ARG, for the whole aggregate. */
int psg_push_compressed(psg_ctx* ctx, int chl, int time, uint64_t kb, uint64_t ke,
                        const void* ckeys, size_t ckeys_bytes, int m,
                        const void* const* cvals, const size_t* cvals_bytes);

/* Value or key push through the receiver's key cache: RNode::cacheKeyRecver
 * (src/system/remote_node.cc:139-184) followed by setValue.  The server
 * keeps one cache per remote node (RNode::key_cache_, remote_node.h:92-93):
 * `sender` names it (any caller-chosen id, e.g. the worker's rank).  `kc` carries
 * the task's key-cache fields:
 *   PSG_KC_SIG   task.has_key_signature(), signature `sig`;
 *   PSG_KC_KEYS  task.has_key(): the message carries keys[nkeys];
 *   PSG_KC_ERASE task.erase_key_cache().
 * Each cache is indexed by (chl, [kb, ke)).  No signature: the entry is
 * dropped and the message's keys are used.  Signature + keys: the keys'
 * crc32c over their first PSG_MAX_SIG_LEN bytes (computed on the GPU) must
 * equal `sig`, and the resident copy is cached under `sig`.  With values
 * (m > 0) the check runs on the device without a host wait and a mismatch
 * is reported by psg_received for `time` (PSG_ERR_SIGNATURE); a key-only
 * message (m == 0) is checked before its union and fails here.
 * Signature without keys: the cached keys are used in place (no key bytes
 * cross PCIe); a missing entry or another signature is PSG_ERR_SIGNATURE
 * (sig 0 against a missing entry restores no keys: the message is
 * ignored, as the reference's empty key list is).  m == 0 is a key-only
 * message (setUnion, merged on the device); otherwise nvals must equal the
 * key count (PSG_ERR_SIZE, nvals == 0 included: kv_vector.h:108,187). */
#define PSG_KC_SIG 1u
#define PSG_KC_KEYS 2u
#define PSG_KC_ERASE 4u
int psg_push_cached(psg_ctx* ctx, int sender, int chl, int time, uint64_t kb,
                    uint64_t ke, unsigned kc, uint32_t sig, const uint64_t* keys, size_t nkeys,
                    int m, const void* const* vals, size_t nvals);
/* RNode::clearCache (remote_node.h:54) / memSize (remote_node.cc:186-195)
 * of one sender's cache (sender < 0: every sender). */
int psg_key_cache_clear(psg_ctx* ctx, int sender);
int psg_key_cache_bytes(psg_ctx* ctx, int sender, size_t* bytes);
/* Shape of the aggregate of `time`: m arrays over server positions
 * [lo, hi) of key(chl).  PSG_ERR_NO_TIME if nothing was pushed. */
int psg_received_shape(psg_ctx* ctx, int time, int* m, size_t* lo,
                       size_t* hi);
/* received(t): copies the m aggregates (hi-lo entries each) into out[i] and
 * erases them.  Returns PSG_ERR_UNMATCHED if any push of `time` had a key
 * that is not a server key of its range (or was unsorted / duplicated). */
int psg_received(psg_ctx* ctx, int time, int m, void* const* out);

/* Pull reply: getValue(msg) (kv_vector.h:206-227): out[i] = value(chl) at
 * keys[i], 0 where keys[i] is not a server key.  keys sorted (repeats
 * allowed); PSG_ERR_UNSORTED otherwise. */
int psg_gather(psg_ctx* ctx, int chl, const uint64_t* keys, size_t n,
               void* out, size_t* matched);
/* The pull reply's value part as Van::send puts it on the wire (van.cc:121-131,
 * SArray::compressTo, shared_array_inl.h:244-256): psg_gather's n values,
 * snappy-compressed on the device (psg_snappy_compress_dev), and only the
 * stream's *out_bytes bytes copied to `out`.  Decoded, they are exactly what
 * psg_gather writes for the same request (n == 0: the one-byte stream of an
 * empty part).  cap below psg_snappy_max_compressed_length(n values' bytes)
 * is PSG_ERR_SIZE before anything runs; unsorted keys are PSG_ERR_UNSORTED
 * and nothing is written. */
int psg_gather_compressed(psg_ctx* ctx, int chl, const uint64_t* keys, size_t n, void* out,
                          size_t cap, size_t* out_bytes, size_t* matched);

/* ------------------------------------------------------------------ */
/* Device-array forms of the server context: push and pull for        */
/* producers and consumers whose arrays are already in HBM            */
/* (psg_mb_darling_gradients / _update_dual, psg_exchange_recv).      */
/* ------------------------------------------------------------------ */
/* Ordering rule of every device form of the context (here and
 * psg_darling_update_dev below): operations on one channel's values and on
 * one aggregate apply in CALL order, whatever streams they are given.  A pull
 * sees every update called before it; an update waits for every pull called
 * before it; pushes of one time fold in call order, host and device pushes
 * alike.  The order is kept with events between the streams: no caller's
 * stream is ever made to wait on the host.  stream == NULL is the device's
 * default stream, as for psg_ftrl_*_dev.
 *
 * Deferred errors: what a device form finds out only on the device -- an
 * update skipped because a push of its block did not match
 * (PSG_ERR_UNMATCHED), a pull request that was not sorted (PSG_ERR_UNSORTED)
 * -- is reported once by the next psg_dev_status or psg_darling_progress,
 * and then cleared; later operations apply normally.  If both kinds are
 * pending, PSG_ERR_UNMATCHED is the one returned and both are cleared. */

/* setValue of a value message (kv_vector.h:75-204), exactly as psg_push, for
 * keys_dev[n] and vals_dev[i][n] (the HOST array of m pointers) in the memory
 * of the context's device, produced by work enqueued on `stream`.  The
 * context takes its own copy by one launch enqueued on `stream` before the
 * call returns: the caller may overwrite its arrays with work enqueued on
 * `stream` afterwards.  Arrays need only element alignment.  No host wait,
 * and no allocation once the pool has seen the shape.  Unchanged from
 * psg_push: n == 0 is ignored; the errors psg_push finds before it stages
 * anything are immediate (PSG_ERR_EMPTY_KEYS, the pigeonhole
 * PSG_ERR_UNMATCHED, PSG_ERR_RANGE, PSG_ERR_CHANNEL, bad m); m may differ
 * between pushes of one time; host and device pushes may share an aggregate;
 * unmatched, unsorted or duplicated keys are reported by psg_received(time)
 * as PSG_ERR_UNMATCHED.
 * The host cannot read the keys, so psg_push's test for a contiguous slice
 * of the server keys is replaced by `slice`: PSG_NO_SLICE takes the searching
 * path (the match of kv_vector.h:84-137,171-204); any other value
 * is the caller's claim that the keys are exactly the server keys D[slice,
 * slice + n) (absolute positions), which leads to the dense kernel.  The
 * claim is checked on the device: every keys_dev[i] != D[slice + i] counts as
 * an unmatched key of the aggregate, so a false claim is PSG_ERR_UNMATCHED at
 * psg_received and skips psg_darling_update(_dev).  A claim outside the
 * positions of [kb, ke) is PSG_ERR_ARG at once. */
#define PSG_NO_SLICE ((size_t)-1)
int psg_push_dev(psg_ctx* ctx, int chl, int time, uint64_t kb, uint64_t ke,
                 const uint64_t* keys_dev, size_t n, int m, const void* const* vals_dev,
                 size_t slice, void* stream);
/* getValue(msg) (kv_vector.h:206-227), as psg_gather, in one launch on
 * `stream`: out_dev[i] = value(chl) at keys_dev[i], +0 where it is not a
 * server key (or repeats the key before it); *matched_dev (nullable) is set
 * to the matched count.  n == 0 is a no-op.  PSG_ERR_SIZE at once when the
 * channel's key and value counts differ (kv_vector.h:220); a request that is
 * not sorted (repeats are legal) is a deferred PSG_ERR_UNSORTED. */
int psg_pull_dev(psg_ctx* ctx, int chl, const uint64_t* keys_dev, size_t n, void* out_dev,
                 unsigned long long* matched_dev, void* stream);
/* Synchronises the context's streams and every channel's last device
 * operation, and returns the deferred error (above) or PSG_OK. */
int psg_dev_status(psg_ctx* ctx);

/* ------------------------------------------------------------------ */
/* Device-resident batched merge: the hot path with every buffer      */
/* already in HBM (benchmarks, multi-GPU shards, graph capture).      */
/* ------------------------------------------------------------------ */
typedef struct psg_merge_job {
  const uint64_t* keys;      /* device: server keys D[lo, hi) (sorted unique) */
  uint64_t nslots;           /* hi - lo */
  int npush;                 /* pushes of this (channel, time), arrival order */
  const uint64_t* const* push_keys; /* host array[npush] of device pointers */
  const void* const* push_vals;     /* host array[npush*m], [p*m + i] */
  const uint64_t* push_n;           /* host array[npush] */
  void* const* out;          /* host array[m] of device pointers, nslots each */
} psg_merge_job;

typedef struct psg_plan psg_plan;

/* All jobs share dtype, m and flags; npush <= psg_plan_max_push() per job.
 * CONTRACT: each job's server keys (the `keys` array, D) must keep their
 * contents for the plan's lifetime.  The plan builds a bucket index of D at
 * creation and every run searches with it; if D changes between runs, keys
 * are misplaced and show up as unmatched in psg_plan_matched.  To merge
 * against a different D, create a new plan (or pass PSG_NO_INDEX, which
 * rebuilds the tables from D in every run).  Push keys and values may
 * change between runs (see PSG_STATIC_KEYS for the one exception).  A run
 * whose push keys repeat the previous run's is cheaper: the search partition
 * first checks the cuts that run left behind, each against its two
 * neighbouring keys, and searches only where one no longer holds (off:
 * PSG_NO_HINTS; the results are the same either way). */
int psg_plan_create(int device, int dtype, int m, unsigned flags,
                    const psg_merge_job* jobs, int njobs, psg_plan** out);
int psg_plan_max_push(void);
/* Enqueue the merge on `stream` (a hipStream_t; NULL = default stream).
 * No allocation, no synchronisation: capturable into a hipGraph. */
int psg_plan_run(psg_plan* plan, void* stream);
/* One stage of psg_plan_run: 0 = partition (findRange / slice lower
 * bounds), 1 = aggregate.  Lets a caller bracket the dominant kernel with
 * its own events on `stream`. */
int psg_plan_run_stage(psg_plan* plan, int stage, void* stream);
/* Synchronises the plan's last run and returns per-push matched counts,
 * jobs in order, pushes in order (sum of npush entries). */
int psg_plan_matched(psg_plan* plan, uint64_t* matched);
/* The aggregate kernel a plan runs (its form, chosen at creation from the
 * shape of the jobs or by the PSG_FORM_* flags): */
#define PSG_KERNEL_TILE 0    /* partition + push-uniform rounds, 1024-slot tiles */
#define PSG_KERNEL_TILE64 1  /* partition + push-uniform rounds, 64-push groups */
#define PSG_KERNEL_PACKED 2  /* partition + rounds packing several pushes */
#define PSG_KERNEL_DENSE 3   /* contiguous slices: no key reads */
#define PSG_KERNEL_CURSOR 4  /* no partition: per-push cursors across tile chunks */
#define PSG_KERNEL_PACKED_CURSOR 5  /* no partition: packed rounds, cursors across tile chunks */
int psg_plan_form(psg_plan* plan, int* form);
/* Algorithmic HBM bytes of one run (SURVEY.md 8d general form). */
int psg_plan_bytes(psg_plan* plan, uint64_t* bytes, uint64_t* kv_pairs);
/* The plan's resident bucket index (absent: 0 bytes): its size, 4 bits per
 * server slot of every tile, and the tiles whose table is not stored (a
 * bucket of more than 14 keys), which the kernels build on every run. */
int psg_plan_index_info(psg_plan* plan, uint64_t* index_bytes, uint64_t* marked_tiles);
/* How the search partition's waves stand after the plan's last run
 * (synchronises it): counts[0] waves whose last run searched and whose next
 * run tests the cuts it left, counts[1] waves that search without testing
 * (most of their cuts failed the test; they test again once a search returns
 * the old cuts), counts[2] waves whose last run kept every cut, counts[3]
 * waves that have not run.  All zero for a plan without hints (PSG_NO_HINTS,
 * no search-mode job). */
int psg_plan_hint_state(psg_plan* plan, uint64_t counts[4]);
int psg_plan_destroy(psg_plan* plan);

/* Device-resident gather (pull reply) over resident keys/values. */
int psg_gather_dev(int dtype, const uint64_t* dkeys, uint64_t nd,
                   const void* dvals, const uint64_t* req, uint64_t nreq,
                   void* out, unsigned long long* matched, void* stream);

/* Device-resident key union: out = a U b (both strictly increasing, else
 * PSG_ERR_UNSORTED, with nothing stored past out[na+nb)); out must hold na+nb; *nout (host) receives |a U b|.
 * The N-way merge of psg_nway_* with two pushes.  Synchronises. */
int psg_key_union_dev(const uint64_t* a, uint64_t na, const uint64_t* b,
                      uint64_t nb, uint64_t* out, uint64_t* nout,
                      void* stream);

/* ------------------------------------------------------------------ */
/* N-way merge of sorted pushes into their merged key set  */
/* ------------------------------------------------------------------ */
/* out_keys = the union of the npush pushes' keys (SArray::setUnion applied
 * push after push, shared_array_inl.h:155-162), sorted; with m > 0 value
 * arrays, out_vals[i][j] = the sum over the pushes holding out_keys[j] in
 * arrival order -- KVVector::serialSetValue / parallelSetValue over that
 * key set (kv_vector.h:84-204; flags PSG_SERIAL_MATCH / PSG_PARALLEL_MATCH).
 * Empty pushes are ignored (kv_vector.h:90,177); at most psg_nway_max_push()
 * non-empty pushes and < 2^32 keys in total.  All pointers are device
 * pointers except the host arrays keys[npush], n[npush], vals[npush * m]
 * and out_vals[m]; out_keys / out_vals hold sum(n) entries.  The pushes'
 * buffers are read again by every run (a prepared merge, like psg_plan).
 * Run: no host wait, capturable; the merged count is a device word
 * (psg_nway_count_dev).  psg_nway_result synchronises and returns
 * PSG_ERR_UNSORTED if a push was not strictly increasing (the reference's
 * std::set_union precondition; the output is then unspecified, but no
 * entry at or past sum(n) of out_keys / out_vals is written).  A merge of
 * disordered pushes can overflow a tile of the kernels: that is
 * PSG_ERR_UNSORTED too, decided by a check of the pushes' order on the error
 * path; PSG_ERR_DEVICE is left for an overflow with strictly increasing
 * pushes and for a look-back timeout. */
typedef struct psg_nway psg_nway;
int psg_nway_max_push(void);
int psg_nway_create(int device, int dtype, int m, unsigned flags, int npush,
                    const uint64_t* const* keys, const uint64_t* n, const void* const* vals,
                    uint64_t* out_keys, void* const* out_vals, psg_nway** out);
/* A batch of nmerge independent merges run as one pipeline (one launch per
 * stage over all of them: e.g. the 64 aggregates of a bench step).  Merge j
 * has npush[j] pushes; keys / n / vals list the merges' pushes back to back
 * (vals: m per push); out_keys[j] and out_vals[j * m + i] are merge j's
 * outputs.  psg_nway_create is the batch of one. */
int psg_nway_create_batch(int device, int dtype, int m, unsigned flags, int nmerge,
                          const int* npush, const uint64_t* const* keys, const uint64_t* n,
                          const void* const* vals, uint64_t* const* out_keys,
                          void* const* out_vals, psg_nway** out);
int psg_nway_run(psg_nway* u, void* stream);
/* the first merge's merged-count word (device) */
int psg_nway_count_dev(psg_nway* u, unsigned long long** nout);
/* nout (host, nullable): one merged count per merge */
int psg_nway_result(psg_nway* u, uint64_t* nout);
/* Algorithmic bytes read by a run (sum(n) * (8 + m s_V)) and keys read;
 * the merged output adds |union| * (8 + m s_V). */
int psg_nway_bytes(psg_nway* u, uint64_t* bytes, uint64_t* kv_pairs);
int psg_nway_destroy(psg_nway* u);
/* Read-outs of the planner and of a run, for tests.
 * psg_nway_shape: the plan psg_nway_create_batch would make for these push
 * lengths (npush / n as there; empty pushes are dropped the same way): per
 * merge shape[j * 5 ..] = K (non-empty pushes), s (sample stride), cw (rank
 * bucket width), B (buckets = splitters), T (tiles); *rank_form = the rank
 * kernel's candidates per thread (16, 4 or 1), *round_robin = 1 if the tile
 * tickets go round-robin over the merges (both nullable).  Host arithmetic
 * only: needs no device.
 * psg_nway_splitters: synchronises and copies the B splitter keys of merge j
 * of the last run to out (host). */
int psg_nway_shape(int nmerge, const int* npush, const uint64_t* n, uint32_t* shape,
                   int* rank_form, int* round_robin);
int psg_nway_splitters(psg_nway* u, int j, uint64_t* out);

/* ------------------------------------------------------------------ */
/* Shard exchange over RCCL ("unsliced" ingress)          */
/* ------------------------------------------------------------------ */
/* One communicator per rank and GPU (RCCL = NCCL API over xGMI).  Rank 0
 * makes the id and the caller broadcasts it (any channel). */
#define PSG_COMM_ID_BYTES 128
typedef struct psg_comm psg_comm;
int psg_comm_unique_id(uint8_t* id);
int psg_comm_init(int device, int nranks, const uint8_t* id, int rank,
                  psg_comm** out);
int psg_comm_destroy(psg_comm* comm);
/* nranks loopback communicators of ONE process on one device (out[r] is
 * rank r): the exchange's collective rounds run with the same pairing rule
 * as RCCL's grouped send/recv, each matched pair a device copy.  Each rank
 * must call the collective functions from its own host thread, all ranks
 * concurrently (as RCCL ranks do from their own processes); a rank whose
 * peers do not join within 120 s gets PSG_ERR_DEVICE.  For tests of the
 * multi-rank path on one GPU (RCCL refuses two ranks on one device).
 * Destroy every rank's communicator. */
int psg_comm_init_loopback(int device, int nranks, psg_comm** out);

/* RNode::submit's slice-and-send (remote_node.cc:39-60: KVVector::slice ->
 * sliceKeyOrderedMsg, message.h:89-123) for a batch of npush sorted
 * device-resident pushes held by this rank, at the server ranges
 * Range<uint64>::all().evenDivide(nranks, s) (linear_method.cc:137-145).
 * Every rank passes the same npush, dtype and m.  Create (synchronous,
 * collective): cut positions, piece counts exchanged, buffers sized.
 * Run (collective, enqueued on `stream`): pack + one grouped send/recv per
 * peer.  Afterwards psg_exchange_recv gives the received keys / m value
 * arrays (device) and recv_cnt[src * npush + p] (host, may be NULL): the
 * piece of push p of rank src starts after all earlier (src, p) pieces;
 * *nsent = keys this rank sends to the other ranks (its own pieces are
 * packed straight into its receive buffers and never cross the transport). */
typedef struct psg_exchange psg_exchange;
int psg_exchange_create(psg_comm* comm, int dtype, int m, int npush,
                        const uint64_t* const* push_keys, const uint64_t* push_n,
                        const void* const* push_vals, psg_exchange** out);
int psg_exchange_run(psg_exchange* x, void* stream);
int psg_exchange_recv(psg_exchange* x, const uint64_t** keys, void** vals,
                      uint64_t* nrecv, uint64_t* recv_cnt, uint64_t* nsent);
int psg_exchange_destroy(psg_exchange* x);
/* The layout is fixed at create (the pushes' device buffers are read again
 * by every run, like a psg_plan's).  Each run also redoes the cut on the
 * device and counts the positions that differ from the layout (pushes whose
 * keys changed since create); psg_exchange_status synchronises the last
 * run's stream and returns PSG_ERR_SIZE (*changed = that count) if any run
 * saw one.  The run's pieces are then those of the create-time cut. */
int psg_exchange_status(psg_exchange* x, uint64_t* changed);
/* Direct mode (on != 0; communicator exchanges only): a run sends every
 * peer-bound piece straight from the push arrays (one send per piece and
 * array, the receiver posts the matching receives in the same order) instead
 * of packing them into the send buffer first; own pieces are still packed
 * into the receive buffers.  Same received layout and bytes either way. */
int psg_exchange_set_direct(psg_exchange* x, int on);
/* The same slice-and-pack for nshards virtual shards on one device with no
 * communicator ("8 shards on 1 device"): a run re-cuts and packs
 * only; psg_exchange_send_layout gives the packed buffers (device) and
 * send_cnt[s * npush + p] (host, may be NULL): shard s's piece of push p
 * starts after all earlier (s, p) pieces.  Works on either kind. */
int psg_exchange_create_local(int device, int nshards, int dtype, int m, int npush,
                              const uint64_t* const* push_keys, const uint64_t* push_n,
                              const void* const* push_vals, psg_exchange** out);
int psg_exchange_send_layout(psg_exchange* x, const uint64_t** keys, void** vals,
                             uint64_t* send_cnt);

/* Server shard boundaries: Range<uint64>::all().evenDivide(n, i)
 * (range.h:75-98, linear_method.cc:137-145); bounds[n+1]. */
int psg_shard_bounds(size_t n, uint64_t* bounds);
/* sliceKeyOrderedMsg positions (message.h:89-123) of a device-resident
 * sorted push: pos[nsep] device array, computed on `stream`. */
int psg_slice_dev(const uint64_t* keys, uint64_t n, uint64_t kb, uint64_t ke,
                  const uint64_t* sep, int nsep, uint64_t* pos, void* stream);

/* ------------------------------------------------------------------ */
/* Server model update fused on the resident aggregate (Darling, L1-LR */
/* block coordinate descent; src/linear_method/darling.cc)             */
/* ------------------------------------------------------------------ */
typedef struct psg_darling_param {
  double eta;                  /* conf_.learning_rate().eta() */
  double lambda;               /* conf_.penalty().lambda(0) */
  double kkt_filter_threshold; /* Darling::KKT_filter_threshold_ */
  double delta_max;            /* conf_.darling().delta_max_value() */
} psg_darling_param;

/* Darling::preprocessData server state of channel grp (darling.cc:
 * 111-117): active_set all true, delta = delta_init, sized to key(chl).
 * Requires a PSG_F64 context (KVVector<Key,double>). */
int psg_darling_init(psg_ctx* ctx, int chl, double delta_init);
/* kkt_filter_reset: active_set.fill(true) (darling.cc:167-169). */
int psg_darling_reset_active(psg_ctx* ctx, int chl);
/* The server's UPDATE_MODEL step (darling.cc:251-262): received(time) must
 * hold m = 2 aggregates (G, U) of channel chl; updateWeight
 * (darling.cc:437-477) runs on the device over value(chl), delta and the
 * active set at the aggregate's positions, and the aggregate is erased.
 * Nothing crosses PCIe but *violation = max vio of this block (the caller
 * folds it into violation_ with std::max).  PSG_ERR_UNMATCHED leaves the
 * model untouched. */
int psg_darling_update(psg_ctx* ctx, int chl, int time, const psg_darling_param* p,
                       double* violation);
/* The same step (darling.cc:251-262, updateWeight :437-477) with no host
 * wait: the same argument checks, fold and kernel, and the aggregate of
 * `time` is erased.  The block's violation is max-accumulated into a device
 * word of the channel -- violation_ = std::max(violation_, vio) across
 * blocks, darling.cc:466 -- which psg_darling_progress reads.  A block whose
 * pushes did not all match leaves the model untouched and sets the deferred
 * PSG_ERR_UNMATCHED (see "Deferred errors" at psg_push_dev; the ordering rule
 * stated there holds here). */
int psg_darling_update_dev(psg_ctx* ctx, int chl, int time, const psg_darling_param* p);
/* The server branch of Darling::evaluateProgress (darling.cc:538-555) for one
 * channel: *nnz_w = the weights that are neither inactive nor zero, *objv =
 * lambda * sum |w| over them, *violation = the word psg_darling_update_dev
 * accumulates (reset_violation != 0 zeroes it after reading: violation_ = 0,
 * darling.cc:163-166), *nnz_active = active_set.nnz().  Any output may be
 * NULL.  Synchronises, and reports and clears the deferred error like
 * psg_dev_status.  Needs psg_darling_init.  inactive(w) is w != w
 * (darling.h): every NaN is inactive, whatever its bits; -0.0 is zero.
 * Defined deviation: sum |w| is not the serial chain of darling.cc:543-547
 * but a fixed-order device reduction (a tree over each 256 weights, then
 * over those sums): the same bits on every run of the same values, within
 * n * 2^-53 * (the exact sum) of it; nnz_w and nnz_active are exact. */
int psg_darling_progress(psg_ctx* ctx, int chl, double lambda, int reset_violation,
                         size_t* nnz_w, double* objv, double* violation, size_t* nnz_active);
/* Copies of delta[off, off+n) and the active bits (one byte each, 0/1);
 * *nnz_active = active_set.nnz() (darling.cc:549).  Any output may be NULL. */
int psg_darling_state(psg_ctx* ctx, int chl, size_t off, size_t n, double* delta,
                      uint8_t* active, size_t* nnz_active);

/* ------------------------------------------------------------------ */
/* Tail-feature filter: FreqencyFilter<uint64> of channel chl          */
/* (SharedParameter::key_filter_, shared_parameter.h:82,114-133) over  */
/* CountMin<uint64, uint8> (src/base/countmin.h), resident in HBM.     */
/* ------------------------------------------------------------------ */
/* CountMin::resize (countmin.h:14-19): n_ = max(n, 64) byte counters,
 * k_ = min(30, max(1, k)) probes, all zero. */
int psg_freq_resize(psg_ctx* ctx, int chl, int n, int k);
int psg_freq_clear(psg_ctx* ctx, int chl);                 /* clear() */
int psg_freq_empty(psg_ctx* ctx, int chl, int* empty);     /* empty() */
/* insertKeys (frequency_filter.h:36-43): counts[i] is added as uint8 to
 * every probe of keys[i] (byte arithmetic wraps).  Host arrays; async. */
int psg_freq_insert(psg_ctx* ctx, int chl, const uint64_t* keys,
                    const uint32_t* counts, size_t n);
/* queryKeys (frequency_filter.h:27-34): out[0, *nout) = the keys whose
 * count estimate is > freq, in input order (out holds n).  freq < 255. */
int psg_freq_query(psg_ctx* ctx, int chl, const uint64_t* keys, size_t n,
                   int freq, uint64_t* out, size_t* nout);
/* Device-resident forms on `stream`: *nout is a device word; scratch holds
 * psg_freq_query_scratch_bytes(n) device bytes (the binned query's records:
 * about 50 B per key up to 8 M keys, then constant -- longer queries take
 * several chunks).  A filter's operations run in call order whatever streams
 * they are enqueued on (each waits for the previous one's event). */
int psg_freq_insert_dev(psg_ctx* ctx, int chl, const uint64_t* keys,
                        const uint32_t* counts, size_t n, void* stream);
size_t psg_freq_query_scratch_bytes(size_t n);
int psg_freq_query_dev(psg_ctx* ctx, int chl, const uint64_t* keys, size_t n,
                       int freq, uint64_t* out, unsigned long long* nout,
                       void* scratch, void* stream);
/* The n_ counters as CountMin's uint8 data_ (tests, checkpoints). */
int psg_freq_table(psg_ctx* ctx, int chl, uint8_t* out, size_t n);
/* The inverse of psg_freq_table (restoring a checkpoint): table[n] becomes
 * CountMin's data_, in the filter's call order.  n must be the filter's n_
 * (PSG_ERR_SIZE otherwise); k_ is psg_freq_resize's.  Host array, free on
 * return. */
int psg_freq_table_assign(psg_ctx* ctx, int chl, const uint8_t* table, size_t n);

/* ------------------------------------------------------------------ */
/* Online server model: FTRLModel<uint64, double>                      */
/* (src/linear_method/ftrl_model.h, driven by linear_method/ftrl.cc),  */
/* a hash map from key to {uint64 pos, uint64 neg, double w, double z} */
/* resident in the HBM of the context's device.                        */
/* ------------------------------------------------------------------ */
/* One model per context; it needs a PSG_F64 context (V = double,
 * ftrl.h:26; PSG_ERR_ARG otherwise) and every call before psg_ftrl_init is
 * PSG_ERR_ARG.  Every uint64 is a legal key.  Messages are applied one after
 * another in call order, whatever streams the device forms are given.
 * Defined deviations from the reference:
 *  - a pull does not insert: getValue's operator[] (ftrl_model.h:76) adds a
 *    default entry there, which nothing observes but the map's size; here
 *    `entries` counts the keys touched by a push;
 *  - norm1 / norm2 are not running sums (ftrl_model.h:104-105, a serial
 *    chain in key order) but a fixed-order device reduction over the table,
 *    computed by psg_ftrl_status: sum |w| and sum w^2, each within
 *    entries * 2^-53 * (the exact sum) of it; nnz is exact;
 *  - a pushed message must be strictly increasing (the reference's callers
 *    send countUniqIndex's sorted unique keys, ftrl.cc:93-96,143, and the
 *    model does not check).  One that is not is rejected whole by a device
 *    check that runs ahead of the update, reported once as PSG_ERR_UNSORTED
 *    by the next psg_ftrl_pull, psg_ftrl_status, psg_ftrl_export or
 *    psg_ftrl_export_state, and then cleared; later messages apply normally.  psg_ftrl_lookup is a probe
 *    for tests and checkpoints and neither reports nor clears it;
 *  - psg_ftrl_export's order is unspecified (as writeToFile's is, the
 *    reference's map order); the Python and C++ mirrors sort by key. */
typedef struct psg_ftrl_param {
  double alpha, beta;      /* setLearningRate, ftrl_model.h:15-18 */
  double lambda1, lambda2; /* setPenalty, ftrl_model.h:19-22 */
} psg_ftrl_param;
/* A fresh, empty model (ftrl_model.h:47-68) sized for capacity_hint entries
 * (0: a default; any value is legal, the table grows by rehash). */
int psg_ftrl_init(psg_ctx* ctx, const psg_ftrl_param* p, size_t capacity_hint);
/* Room for `entries` entries: pushes allocate nothing and read no device
 * count until the keys pushed could number more than that. */
int psg_ftrl_reserve(psg_ctx* ctx, size_t entries);
/* setValue(msg) (ftrl_model.h:80-112): msg->key = keys[n], msg->value =
 * {pos[n], neg[n], grad[n]}.  Host arrays, free on return; the update runs
 * asynchronously on the context's stream (PSG_HOLD_BUFFERS as for psg_push).
 * Thresholded weights are -0.0, as the reference's are. */
int psg_ftrl_push(psg_ctx* ctx, const uint64_t* keys, size_t n, const uint32_t* pos,
                  const uint32_t* neg, const double* grad);
/* The same with device arrays, enqueued on `stream`; allocates nothing and
 * waits for nothing while the model has room (psg_ftrl_reserve). */
int psg_ftrl_push_dev(psg_ctx* ctx, const uint64_t* keys, size_t n, const uint32_t* pos,
                      const uint32_t* neg, const double* grad, void* stream);
/* getValue(msg) (ftrl_model.h:72-78): out[i] = w of keys[i], +0.0 for a key
 * never pushed.  Keys in any order, repeats allowed. */
int psg_ftrl_pull(psg_ctx* ctx, const uint64_t* keys, size_t n, double* out);
int psg_ftrl_pull_dev(psg_ctx* ctx, const uint64_t* keys, size_t n, double* out, void* stream);
/* nnz() (ftrl_model.h:32) and the terms of objv() (:31) = norm1 * lambda1 +
 * .5 * lambda2 * sqrt(norm2); entries = model_.size().  Any output may be
 * NULL.  Synchronises. */
int psg_ftrl_status(psg_ctx* ctx, size_t* entries, size_t* nnz, double* norm1, double* norm2);
/* writeToFile's content (ftrl_model.h:24-29): (key, w) of every entry with
 * w != 0, order unspecified.  *n = their count; PSG_ERR_SIZE (nothing
 * copied) if that exceeds cap. */
int psg_ftrl_export(psg_ctx* ctx, uint64_t* keys, double* w, size_t cap, size_t* n);
/* Whole entries (tests, checkpoints): found[i] = 1 and the entry of keys[i],
 * or 0 and zeros.  Any output may be NULL. */
int psg_ftrl_lookup(psg_ctx* ctx, const uint64_t* keys, size_t n, uint64_t* pos, uint64_t* neg,
                    double* w, double* z, uint8_t* found);
/* Checkpoint and restore.  The reference declares the hooks and leaves them
 * empty (setReplica / getReplica / recoverFrom, ftrl_model.h:41-44); these
 * are what they would carry: whole entries {pos, neg, w, z} by key.
 *
 * psg_ftrl_import: recoverFrom / setReplica.  An upsert of n whole entries:
 * a key already present has its entry replaced (the last one wins, as
 * weight[k] = v does across model files, model_evaluation.h:25), an absent
 * one is inserted.  Every bit is stored as given (-0.0, NaN payloads, counts
 * past 2^32); entries and nnz stay exact (nnz by ftrl_model.h:106-110's
 * comparisons: -0.0 is zero, a NaN weight is not).  Host arrays, free on
 * return; asynchronous on the context's stream and in the model's call
 * order, like psg_ftrl_push; the table grows by rehash when n needs it.
 * pos == neg == z == NULL is the weights-only form, the load of `key w`
 * model files (model_evaluation.h:16-27): the entries become
 * (0, 0, w, +0.0) and the model is frozen (below; an empty model file too:
 * n == 0 with w given).  Any other partly NULL
 * combination is PSG_ERR_ARG.
 * Defined deviations:
 *  - sorted import only: the message must be strictly increasing, and one
 *    that is not applies nothing and is reported once as PSG_ERR_UNSORTED by
 *    the next synchronising call, exactly as for a push;
 *  - after a restore the model equals the saved one entry for entry, and
 *    entries and nnz are exact, but norm1 / norm2 of psg_ftrl_status are a
 *    reduction in table order: they agree with the saved model's within the
 *    bound above (entries * 2^-53 * the sum), not bit for bit. */
int psg_ftrl_import(psg_ctx* ctx, const uint64_t* keys, size_t n, const uint64_t* pos,
                    const uint64_t* neg, const double* w, const double* z);
/* The same with device arrays, enqueued on `stream`; allocates nothing and
 * waits for nothing while the model has room (psg_ftrl_reserve). */
int psg_ftrl_import_dev(psg_ctx* ctx, const uint64_t* keys, size_t n, const uint64_t* pos,
                        const uint64_t* neg, const double* w, const double* z, void* stream);
/* getReplica(Range<Key>) (ftrl_model.h:42): every entry (those with w == +-0
 * and the entry of key 0 included) whose key lies in the closed interval
 * range[0] <= key <= range[1] (closed, so that key 2^64 - 1 can be named;
 * NULL: every key; range[0] > range[1]: PSG_ERR_ARG), sorted by key on the
 * device.  The image of a given model is the same bytes on every run,
 * whatever the table's size and slot order.  *n = the count; PSG_ERR_SIZE
 * (nothing copied) if that exceeds cap, or 2^32 - 1.  Any output array may be
 * NULL.  Synchronises, and reports a rejected message as psg_ftrl_status
 * does. */
int psg_ftrl_export_state(psg_ctx* ctx, const uint64_t* range, uint64_t* keys, uint64_t* pos,
                          uint64_t* neg, double* w, double* z, size_t cap, size_t* n);
/* The same into device arrays of cap entries on `stream`; *n_dev (a device
 * word) = the count.  The host waits once for that count (it shapes the
 * sort's launches) and takes its work blocks from the context's pool. */
int psg_ftrl_export_state_dev(psg_ctx* ctx, const uint64_t* range, uint64_t* keys, uint64_t* pos,
                              uint64_t* neg, double* w, double* z, size_t cap,
                              unsigned long long* n_dev, void* stream);
/* *frozen = 1 after a weights-only import: the model is evaluation-only (z
 * is unknown, and a push would recompute w from it).  psg_ftrl_push and
 * psg_ftrl_push_dev then return PSG_ERR_ARG; pulls, status, exports, lookups
 * and imports work.  The flag is host state, set by the weights-only call
 * itself (also one whose message the device check then rejects).
 * psg_ftrl_init makes a fresh, unfrozen model. */
int psg_ftrl_frozen(psg_ctx* ctx, int* frozen);

/* ------------------------------------------------------------------ */
/* Online worker step: FTRL::updateModel's minibatch loop              */
/* (src/linear_method/ftrl.cc:88-151) on a minibatch resident in HBM:  */
/* Localizer (src/base/localizer.h), FTRL::countKeys, Xw = Z * w,      */
/* LogitLoss (src/linear_method/loss.h:73-85) and grad = Z' * (-y tau).*/
/* ------------------------------------------------------------------ */
/* A minibatch is a row-major CSR with global feature ids: offset[rows+1],
 * index[nnz], value[nnz] (NULL: a binary matrix) and the labels y[rows].
 * The calls follow ftrl.cc's order: psg_mb_load, psg_mb_uniq (:96),
 * psg_mb_localize (:113-119), psg_mb_gradient (:128-138); a call ahead of
 * the one it needs is PSG_ERR_ARG.  A minibatch's calls run in call order
 * whatever streams they are given (each waits for the previous one's event);
 * stream == NULL is the context's stream.  Device pointers handed out stay
 * valid until the next psg_mb_load or psg_mb_destroy.  Buffers are reused
 * and only grow: after the first minibatch of a given size (and dictionary
 * of a given size) no call allocates.  The sums of psg_mb_times and
 * psg_mb_trans_times are the reference's, one rounded multiply and one
 * rounded add per entry in the reference's order (no float atomics, no
 * tree), so Xw and a gradient from given coefficients are bit for bit the
 * reference's.  Destroy a minibatch before its context.
 * Defined deviations from the reference:
 *  - a row with no surviving entry gets Xw = +0.0, so loss = log 2 and
 *    tau = 1/2; the reference skips the row and leaves Xw[i] unwritten
 *    (sparse_matrix.h:76 over the uninitialised SArray of ftrl.cc:128);
 *  - ndict == 0 is legal: Z is empty, Xw is all +0.0, and grad / pos / neg
 *    have length 0; the reference returns a null matrix (localizer.h:114)
 *    and dereferences it (ftrl.cc:115);
 *  - objv is a fixed-order device reduction of the per-row losses (a tree
 *    over each 256 rows, then over those sums): the same bits on every run
 *    of the same input, within rows * 2^-53 * objv of the exact sum; not
 *    Eigen's .sum() (loss.h:74), whose order its packet code decides;
 *  - a dictionary that is not strictly increasing is rejected by a device
 *    check and reported as PSG_ERR_UNSORTED by psg_mb_gradient or
 *    psg_mb_read, whichever synchronises next; psg_mb_localize must then be
 *    called again.  The reference assumes the order without checking
 *    (localizer.h:21);
 *  - only LossConfig::LOGIT is built; any other loss id is PSG_ERR_ARG;
 *  - exp and log are the device's (each within 1 ulp): tau is within 4 ulp
 *    of the host's and loss within 4 * 2^-52 * max(1, loss). */
typedef struct psg_minibatch psg_minibatch;
/* Needs a PSG_F64 context (Real = double, ftrl.h:26; PSG_ERR_ARG otherwise). */
int psg_mb_create(psg_ctx* ctx, psg_minibatch** mb);
void psg_mb_destroy(psg_minibatch* mb);
/* Host arrays, free on return; replaces the previous minibatch.  nnz =
 * offset[rows] >= 2^32 - 1 is PSG_ERR_SIZE (the CHECK_LT of localizer.h:54),
 * an offset array that does not start at 0 or decreases PSG_ERR_ARG. */
int psg_mb_load(psg_minibatch* mb, const uint64_t* offset, size_t rows, const uint64_t* index,
                const double* value, const double* y);
/* countUniqIndex (localizer.h:50-87): the sorted unique ids and how often
 * each occurs.  *n is written after a wait (the caller sizes its filter and
 * pull by it, as ftrl.cc:102 waits for the filter's reply). */
int psg_mb_uniq(psg_minibatch* mb, const uint64_t** keys_dev, const uint32_t** cnt_dev,
                size_t* n);
/* remapIndex (localizer.h:110-168) and countKeys (ftrl.cc:154-174) against
 * dict_dev[ndict], the keys the server kept: strictly increasing, and read
 * again by nothing after this call's kernels.  Enqueues only. */
int psg_mb_localize(psg_minibatch* mb, const uint64_t* dict_dev, size_t ndict,
                    const uint32_t** pos_dev, const uint32_t** neg_dev, void* stream);
/* xw[rows] = Z * x[ndict] (sparse_matrix.h:75-86) and g[ndict] = Z' * c[rows]
 * (matrix.h:57-58 over sparse_matrix.h:88-104).  Enqueue only. */
int psg_mb_times(psg_minibatch* mb, const double* x_dev, double* xw_dev, void* stream);
int psg_mb_trans_times(psg_minibatch* mb, const double* c_dev, double* g_dev, void* stream);
/* ftrl.cc:128-138: Xw = Z * w, objv = LogitLoss::evaluate (loss.h:74),
 * grad = Z' * (-y * tau) (loss.h:81-84).  *objv on the host; synchronises. */
#define PSG_LOSS_LOGIT 0
int psg_mb_gradient(psg_minibatch* mb, int loss, const double* w_dev, const double** grad_dev,
                    double* objv, void* stream);
/* Tests and checkpoints: one internal array to the host, after a wait.  *n =
 * its element count; PSG_ERR_SIZE (nothing copied) if cap_bytes is short. */
#define PSG_MB_SORTED_KEY 0  /* uint64[nnz]: the sorted pairs' keys */
#define PSG_MB_SORTED_POS 1  /* uint32[nnz]: ... and positions (Pair.i) */
#define PSG_MB_UNIQ_KEY 2    /* uint64[n_uniq] */
#define PSG_MB_KEY_CNT 3     /* uint32[n_uniq] */
#define PSG_MB_NEW_OFFSET 4  /* uint64[rows + 1]: Z */
#define PSG_MB_NEW_INDEX 5   /* uint32[matched] */
#define PSG_MB_NEW_VALUE 6   /* double[matched], none for a binary matrix */
#define PSG_MB_POS 7         /* uint32[ndict] */
#define PSG_MB_NEG 8         /* uint32[ndict] */
#define PSG_MB_XW 9          /* double[rows] */
#define PSG_MB_TAU 10        /* double[rows] */
#define PSG_MB_LOSS 11       /* double[rows] */
#define PSG_MB_GRAD 12       /* double[ndict] */
#define PSG_MB_RUN_START 13  /* uint32[n_uniq + 1]: each key's run of sorted pairs */
#define PSG_MB_REMAPPED 14   /* uint32[nnz]: remapped_idx of localizer.h:123 */
#define PSG_MB_ROW_OF 15     /* uint32[nnz]: the row of every position */
#define PSG_MB_SCRATCH 16    /* + slot: uint64[bytes / 8] of psg_mb_scratch */
int psg_mb_read(psg_minibatch* mb, int what, void* out, size_t cap_bytes, size_t* n);
/* Device blocks that live and grow with the minibatch, for what a worker
 * keeps between these calls (the kept keys, the pulled weights, the
 * filter's scratch): slot 0..3, at least `bytes` bytes. */
int psg_mb_scratch(psg_minibatch* mb, int slot, size_t bytes, void** dev);
/* Measurement aid (tools/bench_worker.py): with profiling on, a pair of HIP
 * timing events is recorded around each stage's launches; psg_mb_stage_ms
 * waits and writes the last run's time of each of the PSG_MB_STAGES stages
 * in milliseconds (-1: the stage has not run since profiling went on). */
#define PSG_MB_STAGE_SORT 0        /* (a) the radix passes */
#define PSG_MB_STAGE_RUNS 1        /* (b) run heads: count, scan, emit */
#define PSG_MB_STAGE_LOCALIZE 2    /* (c) order check, search, scatter, compaction */
#define PSG_MB_STAGE_COUNT_KEYS 3  /* (d) */
#define PSG_MB_STAGE_TIMES 4       /* (e) Xw = Z * w */
#define PSG_MB_STAGE_LOGIT 5       /* (f) with the objv reduction */
#define PSG_MB_STAGE_TRANS_TIMES 6 /* (e) grad */
#define PSG_MB_STAGES 7
int psg_mb_profile(psg_minibatch* mb, int on);
int psg_mb_stage_ms(psg_minibatch* mb, double* ms);
/* The context's stream, which stream == NULL above stands for: what a caller
 * hands to the psg_ftrl_*_dev and psg_freq_*_dev forms (whose NULL is the
 * device's default stream) to keep a whole worker step on one stream. */
int psg_mb_stream(psg_minibatch* mb, void** stream);
/* Pairs per workgroup of the sort (tests pick their sizes around it). */
size_t psg_mb_sort_tile(void);

/* ------------------------------------------------------------------ */
/* Text ingest: LIBSVM / ADFEA lines to a resident minibatch           */
/* (StreamReader::readMatricesFromText, src/data/stream_reader.h:50-122,*/
/* over ExampleParser::parseLibsvm / parseAdfea,                       */
/* src/data/example_parser.cc:84-160), in the configuration ftrl.cc:80 */
/* requires: ignore_feature_group = true, one label vector and one     */
/* sparse matrix.                                                      */
/* ------------------------------------------------------------------ */
/* The result is what psg_mb_load would have been given: offset / index /
 * value / y, so every later psg_mb_* call works unchanged.
 * Lines are what fgets returns: bytes up to and including '\n'; a last line
 * without '\n' counts only when final != 0 (the buffer ends the data).  At
 * most max_rows lines are taken.
 * PSG_TEXT_LIBSVM: tokens split at " \t\r\n".  Token 0 is the label by
 * strtof, y = (double)label.  Every further token is idx:val, split at its
 * first ':'; idx by strtoull (base 10), val by strtof, both consumed to the
 * end; idx must not decrease within the line (equal is allowed).  The matrix
 * is valued: value = (double)(float)val.
 * PSG_TEXT_ADFEA: tokens split at " :" only, so '\n', '\r' and '\t' are
 * token bytes.  Tokens 0 and 1 are skipped, token 2 is the label by strtol
 * (truncated to int32), y = label > 0 ? 1 : -1; after it odd tokens are keys
 * (strtoull) and even tokens slot ids, which are not parsed; a key is
 * appended when its slot token arrives.  The matrix is binary.  What follows
 * from that is kept: a trailing slot token may carry "\r\n"; a line whose
 * last token is the label or a key is rejected (the token ends in '\n'); a
 * last key with no slot token on a final line without '\n' is dropped.
 * A rejected line ends the minibatch (readOneLineFromText returning false,
 * stream_reader.h:95): the rows before it are loaded, the line is consumed
 * and reported in bad_line.
 * Defined deviations from the reference, each a rejected line:
 *  - a LIBSVM line with no token (the reference calls strtof(NULL)) and an
 *    ADFEA line with fewer than three tokens (no label value: the CHECK_EQ of
 *    stream_reader.h:104);
 *  - a line of kMaxLineLength_ - 1 = 61439 bytes or more, its '\n' counted
 *    (the reference splits it in two);
 *  - a line that holds a NUL byte.
 * The fast grammar.  A token is converted where it is parsed (on the device
 * in psg_mb_load_text) only if it matches:
 *  - key / idx: 1..20 decimal digits; a value past 2^64 - 1 saturates;
 *  - ADFEA label: an optional '-' and 1..9 digits;
 *  - val / LIBSVM label: an optional '-', digits, an optional '.' digits, at
 *    most 64 bytes, whose decimal significand w (leading zeros and trailing
 *    fraction zeros dropped) is <= 2^24 with k <= 10 fraction digits; the
 *    result is (float)((double)w / 10^k), which is strtof's; "-0" is -0.0f.
 * Every other token (signs, blanks, empty digit strings, exponents, hex
 * floats, inf / nan, more digits, '\n' inside an ADFEA token, ...) is a slow
 * token: the host calls the reference's own libc function on a NUL-terminated
 * copy and the result, or the line's rejection, is patched in.  Results do
 * not depend on how many tokens are slow.  A LIBSVM idx:val token counts as
 * one token and is slow if either half is.
 * Out of scope: TERAFEA, files, gzip, the protobuf and binary formats, text
 * that is already on the device.  ignore_feature_group = false is
 * psg_mb_load_text_groups, below. */
#define PSG_TEXT_ADFEA 4   /* DataConfig::ADFEA */
#define PSG_TEXT_LIBSVM 5  /* DataConfig::LIBSVM */
typedef struct psg_text_result {
  uint64_t rows;        /* rows loaded */
  uint64_t nnz;         /* entries loaded */
  uint64_t consumed;    /* bytes of text used up, the rejected line included */
  int64_t bad_line;     /* the rejected line (0-based; == rows), -1: none */
  uint64_t slow_tokens; /* tokens that went to libc.  psg_mb_load_text counts
                         * those of all the lines it took (up to max_rows);
                         * psg_text_parse_host stops at the rejected line */
  double parse_ms;      /* psg_mb_load_text with psg_mb_profile on: its
                         * kernels' time by HIP events (the slow tokens' host
                         * time included), else -1 */
} psg_text_result;
/* Text in host memory, free on return; replaces the previous minibatch and
 * leaves it as psg_mb_load does.  All of [0, nbytes) is copied to the device
 * and counted, so hand it about a minibatch of text, not a whole file.
 * PSG_ERR_ARG: a null argument, an unknown format.  PSG_ERR_SIZE: nbytes or
 * the entries >= 2^32 - 1.  One host wait more than psg_mb_load (the sizes);
 * two more when there are slow tokens; three when a line is rejected. */
int psg_mb_load_text(psg_minibatch* mb, const char* text, size_t nbytes, int format,
                     size_t max_rows, int final, psg_text_result* result);
/* The same parse, serially on the host, for callers without a device.  Two
 * calls: with offset == NULL it only fills *result (rows, nnz: the sizes);
 * then offset[rows + 1], index[nnz], value[nnz] (LIBSVM; may be NULL, and is
 * not written for ADFEA) and y[rows], with rows <= rows_cap and nnz <=
 * nnz_cap, or PSG_ERR_SIZE (the arrays then hold a part of the result).  One
 * call does when the arrays are known to be large enough. */
int psg_text_parse_host(const char* text, size_t nbytes, int format, size_t max_rows, int final,
                        uint64_t* offset, uint64_t* index, double* value, double* y,
                        size_t rows_cap, size_t nnz_cap, psg_text_result* result);
/* Bytes of text per workgroup of the ingest kernels (tests place tokens and
 * newlines around its multiples). */
size_t psg_text_chunk(void);
/* psg_mb_read ids of the loaded CSR (after either load) */
#define PSG_MB_OFFSET 24 /* uint64[rows + 1] */
#define PSG_MB_INDEX 25  /* uint64[nnz] */
#define PSG_MB_VALUE 26  /* double[nnz], none for a binary matrix */
#define PSG_MB_Y 27      /* double[rows] */

/* ------------------------------------------------------------------ */
/* Text ingest by feature group: SlotReader::read                      */
/* (src/data/slot_reader.cc:35-232) with ignore_feature_group = false: */
/* the slot id of every entry, the ExampleInfo of the load             */
/* (ExampleParser::toProto / info, example_parser.cc:38-82) and one    */
/* resident matrix per group.                                          */
/* ------------------------------------------------------------------ */
/* The grouped parse is the parse above with two differences.
 * (1) The line rule is FileLineReader's (util/filelinereader.cc:34-42), not
 * fgets': a line is the bytes up to '\n' (a last line without '\n' counts
 * only when final != 0); the terminating '\n' and then at most one '\r'
 * directly before it are chopped before the line is tokenised (on a final
 * line without '\n', at most one trailing '\r').  Every other byte is a token
 * byte as above, any other '\r' and an ADFEA '\t' included: such a token is
 * slow and libc decides (strtol("7\r") rejects, "\t7" is accepted).  What
 * follows from the chop is kept: "id 1 1\n" is a valid ADFEA row with no
 * entry, and "id 1 1 5:2 9\n" parses the key 9 and drops it, because no slot
 * token follows.  The 61439-byte rule (the '\n' and '\r' counted), the NUL
 * rule and "fewer than three ADFEA tokens" stay as they are.
 * (2) The slot tokens are read.  ADFEA: after the label, even tokens are slot
 * ids by strtoi32: strtol base 10 truncated to int32 and consumed to the
 * end, so "4294967297" is slot 1.  The fast grammar is 1..4 decimal digits;
 * every other slot token is a slow token.  LIBSVM: every entry has slot 1.
 * Defined deviation, a rejected line: a line holding a slot id outside
 * [1, 4095].  In the reference id 0 as a line's first group appends its keys
 * to the label slot, a negative id indexes SlotReader's vslots out of bounds,
 * and an id >= 4096 makes toProto return false after it has updated a part of
 * its slot_info_.
 * A rejected line ends the parse exactly as above: the rows before it are
 * kept, the line is consumed and reported in bad_line.  (SlotReader itself
 * skips such a line and goes on, slot_reader.cc:148; a caller does that by
 * cutting the line out and parsing again.)
 * psg_mb_load_text_groups is psg_mb_load_text with that rule: it leaves the
 * minibatch as psg_mb_load_text would (offset / index / value / y, loaded)
 * plus the resident slot array, one uint16 per entry, which
 * psg_mb_read(PSG_MB_SLOT) reads and psg_mb_groups works on.  A slow slot
 * token goes the way of every slow token (the host's libc call, patched in)
 * and is counted in slow_tokens.  Same errors and host waits.
 * psg_text_parse_groups_host is psg_text_parse_host with that rule and one
 * more output, slot[nnz] (may be NULL when offset is NULL).  Its arrays are
 * what psg_mb_load and psg_mb_set_slots take. */
int psg_mb_load_text_groups(psg_minibatch* mb, const char* text, size_t nbytes, int format,
                            size_t max_rows, int final, psg_text_result* result);
int psg_text_parse_groups_host(const char* text, size_t nbytes, int format, size_t max_rows,
                               int final, uint64_t* offset, uint64_t* index, double* value,
                               double* y, uint16_t* slot, size_t rows_cap, size_t nnz_cap,
                               psg_text_result* result);
#define PSG_MB_SLOT 28   /* uint16[nnz]: the slot id of every entry (after psg_mb_load_text_groups
                          * or psg_mb_set_slots) */

/* The slot ids of the loaded minibatch's entries: slot[n], a host array free
 * on return, n == nnz (PSG_ERR_SIZE otherwise); after psg_mb_load /
 * psg_mb_load_text and before psg_mb_uniq (PSG_ERR_ARG otherwise).  The ids
 * are checked by psg_mb_groups, not here. */
int psg_mb_set_slots(psg_minibatch* mb, const uint16_t* slot, size_t n);
/* SlotInfo (proto/example.proto) */
#define PSG_SLOT_DENSE 1
#define PSG_SLOT_SPARSE 2
#define PSG_SLOT_SPARSE_BINARY 3
typedef struct psg_slot_info {
  int32_t id;
  int32_t format;
  uint64_t min_key, max_key, nnz_ele, nnz_ex;
} psg_slot_info;
/* toProto's bookkeeping (example_parser.cc:43-55) and info() (:59-82) for the
 * whole load, in ascending id order.  The label slot 0 first (dropped when
 * rows == 0): PSG_SLOT_DENSE, min_key 0, max_key 1, nnz_ex = nnz_ele = rows.
 * Then every feature slot with an entry: PSG_SLOT_SPARSE for a valued matrix
 * (LIBSVM), PSG_SLOT_SPARSE_BINARY for a binary one (ADFEA); min_key the
 * smallest key; max_key the largest key + 1 as written, in uint64, so key
 * 2^64 - 1 contributes 0; nnz_ele its entries; nnz_ex the rows that hold it,
 * and for a valued matrix `rows` (parseLibsvm adds slot 1 to every example).
 * *n = the slots; PSG_ERR_SIZE with *n set (nothing written) when cap is
 * short; info may be NULL then.
 * The format's contract is "same group_ids should appear together"
 * (example_parser.cc:127): a row in which a slot id occurs in two separate
 * runs makes the reference push two row_siz entries for one example and lose
 * the row alignment of that slot.  Defined deviation: such a row, or a row
 * holding a slot id outside [1, 4095], is reported in *bad_row (the smallest
 * such row; -1: none), the call returns PSG_ERR_ARG and psg_mb_group_extract
 * is refused.  Equal ids at the end of row r and the start of row r + 1 are
 * legal.
 * A stable radix sort of (slot, position) over the digits in which the ids
 * differ, then integer counts, minima and maxima per slot: the same input
 * gives the same bytes on every run.  One host wait (the slots and the
 * verdict).  Needs psg_mb_set_slots; PSG_ERR_ARG after psg_mb_uniq. */
int psg_mb_groups(psg_minibatch* mb, psg_slot_info* info, size_t cap, size_t* n,
                  int64_t* bad_row);
/* SlotReader::index(g) / offset(g) / value(g) (slot_reader.cc:234-290) of
 * slot `slot_id` as the loaded minibatch `dst` (of the same context): all of
 * src's rows (a row without the group is empty: row_siz's zero padding), the
 * group's entries in their original order, y copied.  An absent slot gives
 * `rows` empty rows.  Device to device; dst is left as psg_mb_load leaves it
 * (one host wait).  PSG_ERR_ARG: before psg_mb_groups on src or after a
 * psg_mb_groups that reported a bad row, after psg_mb_uniq on src (it reuses
 * the sort's blocks), src == dst, a slot id outside [1, 4095], two contexts. */
int psg_mb_group_extract(psg_minibatch* src, int slot_id, psg_minibatch* dst);
/* Range<Key>(begin, end).evenDivide(n, i) for every i (range.h:85-98), which
 * cuts a slot's [min_key, max_key) into feature blocks
 * (batch_solver.cc:61-65): bounds[n + 1], block i is [bounds[i], bounds[i +
 * 1]), in long double as written.  Host arithmetic.  PSG_ERR_ARG: n == 0,
 * end < begin (the reference CHECKs both). */
int psg_even_divide(uint64_t begin, uint64_t end, size_t n, uint64_t* bounds);

/* ------------------------------------------------------------------ */
/* SlotReader's cache arrays (src/data/slot_reader.cc:86-141,208-290): */
/* per (file, slot) a .colidx (uint64), a .rowsiz (uint16) and a       */
/* .value (float) file, each a sequence of snappy streams              */
/* ("partitions") that a .partition file lists as start / size pairs.  */
/* DESIGN.md 4.11c.                                                    */
/* ------------------------------------------------------------------ */
#define PSG_CACHE_COLIDX 0  /* uint64[nnz]:  the minibatch's index                      */
#define PSG_CACHE_ROWSIZ 1  /* uint16[rows]: offset[r+1] - offset[r]                    */
#define PSG_CACHE_VALUE  2  /* float[nnz]:   (float)value; PSG_ERR_ARG for a binary mb  */
#define PSG_CACHE_LABEL  3  /* float[rows]:  (float)y  (slot 0's .value)                */
/* A raw array of raw_bytes cut into partitions of part_bytes raw bytes, the
 * last one shorter; part_bytes == 0: one partition; not a multiple of 8:
 * PSG_ERR_ARG.  *nparts = the partitions (0 for an empty array), *cap = the
 * sum of psg_snappy_max_compressed_length over them.  Host arithmetic. */
int psg_cache_pack_bound(size_t raw_bytes, size_t part_bytes, size_t* cap, size_t* nparts);
/* One cache array of a loaded minibatch (after any load or
 * psg_mb_group_extract; whenever psg_mb_read(PSG_MB_INDEX) is served), cut
 * as above, every partition compressed on the device in one call of the
 * compressor (so stream i is psg_snappy_compress_host of partition i's raw
 * bytes) and the streams copied back to back into host `out`: *len their
 * bytes, parts[2i] the start and parts[2i + 1] the size of stream i, *nparts
 * their count.  cap and parts_cap below psg_cache_pack_bound's are
 * PSG_ERR_SIZE, as is a partition of 4 GiB or more.  An empty array gives
 * len = 0 and nparts = 0 (compressTo of an empty array).
 * Defined deviation: the reference's pushBack into SArray<uint16> wraps a
 * row of more than 65535 entries silently; here PSG_CACHE_ROWSIZ reports the
 * smallest such row in *bad_row (-1: none) and returns PSG_ERR_RANGE with
 * nothing written.  One host wait. */
int psg_mb_cache_pack(psg_minibatch* mb, int what, size_t part_bytes, void* out, size_t cap,
                      size_t* len, uint64_t* parts /* (start, size) pairs */, size_t parts_cap,
                      size_t* nparts, int64_t* bad_row);

typedef struct psg_cache_array {   /* one array of one file; host memory, free on return */
  const void* data; size_t nbytes;          /* the file's bytes                            */
  const uint64_t* parts; size_t nparts;     /* (start, size) pairs; nparts == 0: the whole */
} psg_cache_array;                          /* file is one stream (no .partition file)     */
typedef struct psg_cache_file {
  psg_cache_array colidx, rowsiz, value, label;
  uint64_t num_ex;                          /* the file's .info num_ex                     */
} psg_cache_file;
typedef struct psg_cache_result {
  uint64_t rows, nnz; int64_t bad_file; int32_t bad_what; int32_t bad_part;
} psg_cache_result;
/* SlotReader::index / offset / value over `nfiles` files (:234-290) as the
 * loaded minibatch mb, left exactly as psg_mb_load leaves it: the rows are
 * the files' rows in the order given, offset the running sum of every rowsiz,
 * index the concatenated colidx, value (double) of the floats (not read, and
 * none, when valued == 0), y (double) of the labels.  All partitions of all
 * arrays of all files are decoded in one decoder launch; one host wait.
 * The reference's CHECKs: a partition outside its file, a partition whose
 * declared length is no multiple of the element size, and for a file f
 * sum rowsiz(f) != the colidx count, value count != colidx count (valued),
 * rowsiz count, label count and num_ex not all equal, or a total of
 * 2^32 - 1 entries or more are PSG_ERR_SIZE; a corrupt stream is
 * PSG_ERR_ARG.  bad_file / bad_what (a PSG_CACHE_* id) / bad_part name the
 * file, array and partition (-1: not applicable).  A partition of size 0
 * decodes to nothing.  After any error the minibatch is empty (as created)
 * and the next load works.
 * Defined deviation: a file whose colidx, rowsiz and value are all empty
 * (the slot is absent from that file) contributes num_ex empty rows; the
 * reference's offset() fails its CHECK_EQ(os.size(), num_ex + 1) there. */
int psg_mb_load_cache(psg_minibatch* mb, const psg_cache_file* files, size_t nfiles,
                      int valued, psg_cache_result* result);
/* Rows per workgroup of the load's scan of the row sizes (tests sit on its
 * multiples). */
size_t psg_cache_scan_tile(void);

/* ------------------------------------------------------------------ */
/* Batch worker step: the worker half of Darling::updateModel          */
/* (src/linear_method/darling.cc:196-250) on a localized minibatch:    */
/* computeGradients (:306-356), updateDual (:358-435), the worker's    */
/* lines of preprocessData (:110-117) and evaluateProgress (:506).     */
/* ------------------------------------------------------------------ */
/* The minibatch is the worker's data of one feature group, the dictionary of
 * psg_mb_localize is w_->key(grp), and the dictionary positions [cb, ce) are
 * what seg_pos / col_range are in the reference: column k of the column-major
 * matrix Darling reads (SparseMatrix::alterStorage, sparse_matrix.h:186-241,
 * fills each column in row-major scan order) is key k's entries in ascending
 * position.  Every call needs psg_mb_darling_init after psg_mb_localize;
 * psg_mb_load and psg_mb_localize invalidate the state; a call ahead of the
 * one it needs, cb > ce or ce > ndict is PSG_ERR_ARG.  Streams and buffers as
 * for the calls above.  Every operator of darling.cc:342-350,375-376,432 is
 * one rounded operation in the order written, std::min is b < a ? b : a (a
 * NaN first argument stays), and every sum and product runs in the
 * reference's order (no float atomics, no tree): G, cur_w, delta, delta_w and
 * the active set are bit for bit the reference's from the same state.
 * Defined deviations from the reference:
 *  - exp and log are the device's (each within 1 ulp), so U, dual and objv
 *    are within the bounds derived in tests/test_darling_worker_gpu.py of the
 *    host's;
 *  - objv is the fixed-order device reduction of psg_mb_gradient (a tree over
 *    each 256 rows, then over those sums): the same bits on every run, within
 *    rows * 2^-53 * objv of the exact sum; not Eigen's .sum() (darling.cc:506);
 *  - a dictionary key absent from the data is a column with no entry (G = U =
 *    +0.0), and a row with no surviving entry has dual = exp(y * +0.0) = 1;
 *  - the active set is kept as one byte per key, not a Bitmap. */
/* preprocessData (:110-117): dual[rows] = exp(y .* (Z * w)), the worker's
 * copy cur_w[ndict] = w (w_dev NULL: zero, and every dual exactly 1.0),
 * delta[ndict] = delta_init, active all true.  Also builds the rows' lists
 * that psg_mb_darling_update_dual walks (a stable sort of the surviving
 * sorted pairs by row) and reads each column's range of sorted pairs to the
 * host: synchronises, and reports an unsorted dictionary as psg_mb_gradient
 * does. */
int psg_mb_darling_init(psg_minibatch* mb, double delta_init, const double* w_dev, void* stream);
/* kkt_filter_reset: active_set.fill(true) (:167-169).  Enqueues only. */
int psg_mb_darling_reset_active(psg_minibatch* mb, void* stream);
/* computeGradients (:306-356) over columns [cb, ce): g_dev[j], u_dev[j] are
 * column cb + j's.  An inactive column gets the all-ones NaN in both
 * (kInactiveValue_, :15,334); both branches (binary, valued) are built.
 * Enqueues only. */
int psg_mb_darling_gradients(psg_minibatch* mb, size_t cb, size_t ce, double* g_dev,
                             double* u_dev, void* stream);
/* updateDual (:358-435): new_w_dev[j] is column cb + j's pulled weight.  The
 * columns' state first (:364-378; delta_max = conf_.darling().
 * delta_max_value() of newDelta, darling.h:31-33), then every row's dual
 * (:420-434), its factors multiplied in ascending column and, within a
 * column, ascending position.  A row that only columns with delta_w == 0 or
 * a cleared active bit touch is not written.  Enqueues only. */
int psg_mb_darling_update_dual(psg_minibatch* mb, size_t cb, size_t ce, const double* new_w_dev,
                               double delta_max, void* stream);
/* evaluateProgress (:506): *objv = sum log(1 + 1 / dual), on the host;
 * synchronises. */
int psg_mb_darling_objv(psg_minibatch* mb, double* objv, void* stream);
/* Tests and checkpoints: host arrays dual[rows], cur_w[ndict], delta[ndict],
 * active[ndict] (bytes 0 / 1; anything else PSG_ERR_ARG); any may be NULL.
 * Waits for the minibatch's work first. */
int psg_mb_darling_set_state(psg_minibatch* mb, const double* dual, const double* cur_w,
                             const double* delta, const uint8_t* active);
/* psg_mb_read ids of the state (PSG_ERR_ARG before psg_mb_darling_init) */
#define PSG_MB_DARLING_DUAL 32     /* double[rows] */
#define PSG_MB_DARLING_CUR_W 33    /* double[ndict] */
#define PSG_MB_DARLING_DELTA 34    /* double[ndict] */
#define PSG_MB_DARLING_ACTIVE 35   /* uint8[ndict], 0 / 1 */
#define PSG_MB_DARLING_DELTA_W 36  /* double[ce - cb] of the last psg_mb_darling_update_dual */
/* One dual for the feature groups of a worker: in the reference dual_ is one
 * vector over the rows, created once (batch_solver.cc:344-349) and updated by
 * every group's updateDual (darling.cc:358-435).  After this call, made
 * before psg_mb_darling_init(mb), every Darling call on `mb` reads and writes
 * `owner`'s dual block: gradients, update_dual, objv, set_state and
 * psg_mb_read(PSG_MB_DARLING_DUAL).  psg_mb_darling_init of a sharer needs
 * w_dev == NULL (PSG_ERR_ARG otherwise) and does not touch the dual: the
 * reference starts from zero weights (its init_w branch is under #if 0), so
 * every dual is 1, which the owner's own init wrote.  PSG_ERR_ARG: the row
 * counts or contexts differ, mb == owner, the owner has not had
 * psg_mb_darling_init, the owner shares someone else's dual, mb's own dual is
 * shared.  A load or the destruction of the owner invalidates its sharers
 * (their Darling calls are PSG_ERR_ARG until they share and init again), and
 * while the owner has no Darling state (after its psg_mb_localize, until its
 * next psg_mb_darling_init) they are PSG_ERR_ARG too.  A load of the sharer
 * ends its sharing; so does owner == NULL.
 * A minibatch's own calls run in call order whatever streams they are given,
 * but nothing orders the calls of two minibatches: the order in which the
 * groups touch the shared dual is the caller's, by passing ONE stream (e.g.
 * psg_mb_stream's) to every Darling call of the owner and its sharers. */
int psg_mb_darling_share_dual(psg_minibatch* mb, psg_minibatch* owner);

/* ------------------------------------------------------------------ */
/* Model evaluation: the distributed AUC (src/base/auc.h:8-103) and    */
/* the exact rank AUC (src/base/evaluation.h:17-44)                    */
/* ------------------------------------------------------------------ */
/* The label array of the loaded minibatch and its own Xw array, both valid
 * until the next psg_mb_load (PSG_ERR_ARG before the first).  xw_dev holds
 * values only after psg_mb_times has been run into it or psg_mb_gradient has
 * run; once psg_mb_times has run into it, psg_mb_read(PSG_MB_XW) reads it.
 * Scoring without training (ModelEvaluation::run, model_evaluation.h:48-57)
 * is load, uniq, psg_ftrl_pull_dev of the unique keys, localize against
 * them and psg_mb_times into xw_dev.  Defined deviation: a key the model
 * lacks adds +0.0 * v to its row where the reference skips the entry; the
 * bits are the same unless v is an infinity or a NaN. */
int psg_mb_labels(psg_minibatch* mb, const double** y_dev, const double** xw_dev);

/* A psg_auc is the root's two maps (auc.h:101) as one histogram resident in
 * HBM: the distinct keys in ascending signed order, a uint64 positive and a
 * uint64 negative count per key.  A handle's calls run in call order whatever
 * stream they are given; stream == NULL is the context's stream.  The arrays
 * only grow.  The host keeps an upper bound of the distinct keys (every add
 * raises it by its item count) and reads the device's true count only when
 * that bound passes the capacity; while there is room an add allocates
 * nothing.  Every count is an integer and every device sum an integer sum:
 * the histogram after any sequence of adds and merges is the one that a
 * single compute over all the examples gives.  Destroy a handle before its
 * context.
 * Defined deviations from the reference:
 *  - a product predict * goodness that is NaN or of magnitude >= 2^63 has no
 *    defined conversion in C++; it gets the key INT64_MIN, which is what the
 *    reference's x86-64 build produces (recorded from it, one prediction
 *    at a time, in tests/golden/reference_pin/auc.npz);
 *  - n == 0 is a legal no-op (the reference CHECKs it, auc.h:71);
 *    n >= 2^32 - 1 is PSG_ERR_SIZE (positions are uint32);
 *  - psg_auc_merge drops entries whose count is 0.  The reference's map keeps
 *    the key with a count of 0, which adds 0 to every sum and changes no
 *    accuracy, and no evaluate but one: a side that holds zero counts only is
 *    not empty() there, so its evaluate (auc.h:43) goes on to 0 / 0 = NaN
 *    where this one returns .5, as for a side with no entry;
 *  - an add reads the batch's smallest and largest key (16 bytes) back before
 *    it sorts, to choose the radix digits: it waits for its own key kernel,
 *    as psg_mb_load waits for its OR / AND reduction;
 *  - evaluate() as written (auc.h:49) advances over the positives while their
 *    COUNT is at most the negative's count, where it means their KEY: with
 *    all keys distinct (every count 1) it returns 1.0 whatever the data.
 *    PSG_AUC_BY_KEY is auc.h:42-59 with that one condition read as
 *    `tp_it->first <= fp_it.first`; PSG_AUC_AS_WRITTEN is the loop verbatim,
 *    for comparing numbers with a reference run.  On 2,000 examples: as
 *    written 0.783, 0.597, 1.0 at goodness 10, 1000, 100000; by key 0.862,
 *    0.8704, 0.8705; the exact rank AUC 0.8705. */
typedef struct psg_auc psg_auc;
#define PSG_AUC_BY_KEY 0
#define PSG_AUC_AS_WRITTEN 1
int psg_auc_create(psg_ctx* ctx, int64_t goodness, psg_auc** h);
void psg_auc_destroy(psg_auc* h);
/* clear() (auc.h:62): an empty histogram; the arrays are kept.  Enqueues. */
int psg_auc_clear(psg_auc* h);
/* setGoodness (auc.h:10); PSG_ERR_ARG unless the histogram is empty (keys of
 * two goodnesses do not mix). */
int psg_auc_set_goodness(psg_auc* h, int64_t goodness);
/* compute (auc.h:69-80) fused with merge (:14-22): example i adds one to key
 * (int64)(predict[i] * (double)goodness) -- one rounded multiply, truncation
 * toward zero -- as a positive iff y[i] > 0 (0, -0.0 and NaN are negatives). */
int psg_auc_add_dev(psg_auc* h, const double* y_dev, const double* predict_dev, size_t n,
                    void* stream);
/* The same with host arrays, free on return. */
int psg_auc_add(psg_auc* h, const double* y, const double* predict, size_t n);
/* merge (auc.h:14-22) of another worker's AUCData: host arrays, keys in any
 * order, repeats add up (the map's +=).  Takes add's device path with each
 * entry's count as its weight. */
int psg_auc_merge(psg_auc* h, const int64_t* tp_key, const uint64_t* tp_count, size_t ntp,
                  const int64_t* fp_key, const uint64_t* fp_count, size_t nfp);
/* The AUCData compute writes (auc.h:85-97): the keys with a positive count
 * and those counts, then the same for the negatives, each list in ascending
 * signed key order.  *ntp / *nfp = the lists' lengths; PSG_ERR_SIZE (nothing
 * copied) if either exceeds its capacity.  Synchronises. */
int psg_auc_data(psg_auc* h, int64_t* tp_key, uint64_t* tp_count, size_t tp_cap, size_t* ntp,
                 int64_t* fp_key, uint64_t* fp_count, size_t fp_cap, size_t* nfp);
/* accuracy (auc.h:26-39) over an AUCData whose lists ascend by key: pure host
 * code, every double the reference's (x = threshold * goodness, (double)key
 * >= x, correct and total summed as doubles, positives first).  An empty
 * AUCData gives 0 / 0 = NaN. */
int psg_auc_accuracy_data(int64_t goodness, const int64_t* tp_key, const uint64_t* tp_count,
                          size_t ntp, const int64_t* fp_key, const uint64_t* fp_count, size_t nfp,
                          double threshold, double* out);
/* evaluate (auc.h:42-59) over such an AUCData, mode PSG_AUC_BY_KEY or
 * PSG_AUC_AS_WRITTEN (above); pure host code, serial, in the reference's
 * order; .5 when either list is empty. */
int psg_auc_evaluate_data(const int64_t* tp_key, const uint64_t* tp_count, size_t ntp,
                          const int64_t* fp_key, const uint64_t* fp_count, size_t nfp, int mode,
                          double* out);
/* psg_auc_data, then the function above.  Synchronise. */
int psg_auc_accuracy(psg_auc* h, double threshold, double* v);
int psg_auc_evaluate(psg_auc* h, int mode, double* v);
/* Evaluation<double>::auc (evaluation.h:17-44) on device arrays: a stable sort
 * by prediction, A = the sum over the negatives (y <= 0 or NaN) of the
 * positives sorted before them, in uint64 (exact), then area = (double)A /
 * ((double)P * (double)(n - P)) and area < 0.5 ? 1 - area : area.  One class
 * absent or n == 0 gives 0 / 0: NaN is returned, as the reference would.
 * Synchronises.  Defined deviations: a NaN prediction is PSG_ERR_ARG (counted
 * on the device; the reference's comparator is then no strict weak order and
 * std::sort undefined); equal predictions keep their input order (std::sort
 * leaves it open); -0.0 and +0.0 are equal, as under the comparator; only
 * V = double is built (ModelEvaluation's float stops counting at 2^24);
 * n >= 2^32 - 1 is PSG_ERR_SIZE. */
int psg_auc_exact_dev(psg_ctx* ctx, const double* y_dev, const double* predict_dev, size_t n,
                      double* auc, void* stream);
int psg_auc_exact(psg_ctx* ctx, const double* y, const double* predict, size_t n, double* auc);

/* ------------------------------------------------------------------ */
/* Wire ingress: key signatures of the key cache                       */
/* ------------------------------------------------------------------ */
/* CRC-32C of device-resident byte segments: out[i] = crc32c::Extend(
 * init ? init[i] : 0, data + off[i], min(off[i+1] - off[i], max_len))
 * (src/util/crc32c.cc:283-330; crc32c::Value = init 0).  The key signature
 * of RNode::cacheKeySender/cacheKeyRecver (src/system/remote_node.cc:108,
 * 163) is max_len = PSG_MAX_SIG_LEN over the key bytes.  off[nseg+1], init
 * (nullable) and out[nseg] are device arrays; enqueued on `stream`. */
#define PSG_MAX_SIG_LEN 2048 /* RNode::max_sig_len_, remote_node.h:96 */

/* snappy raw-format decompression of device-resident message parts: what
 * Van::recv does per key/value part (van.cc:204-214,
 * SArray::uncompressFrom, shared_array_inl.h:232-240), for nmsg parts in
 * one launch.  Part i is src[soff[i], soff[i+1]) and decompresses into
 * dst[doff[i], doff[i+1]), which must be its declared length
 * (snappy::GetUncompressedLength; psg_snappy_uncompressed_length reads it
 * from a host copy of the first bytes).  status[i] = 0, PSG_ERR_SIZE (the
 * declared length differs) or PSG_ERR_ARG (corrupt stream: the reference's
 * CHECK).  soff, doff, status: device arrays; enqueued on `stream`. */
int psg_snappy_uncompress_dev(const uint8_t* src, const uint64_t* soff, uint64_t nmsg,
                              uint8_t* dst, const uint64_t* doff, int32_t* status,
                              void* stream);
int psg_snappy_uncompressed_length(const void* src, size_t n, size_t* len);

/* snappy raw-format compression of device-resident message parts: what
 * Van::send does per key and value part (van.cc:121-131,
 * SArray::compressTo, shared_array_inl.h:244-256), for nparts parts in one
 * call.  Part i is src[soff[i], soff[i+1]); its stream is written
 * contiguously from dst + doff[i] and its length to clen[i].  The stream is a
 * pure function of the part's bytes (the rule of DESIGN.md 4.12: 64 KB
 * fragments, literal / copy-1 / copy-2 elements, never a copy-4), whatever
 * the launch holds besides; it is a valid snappy stream, not libsnappy's own.
 * It never exceeds psg_snappy_max_compressed_length(part bytes) =
 * 32 + n + n / 6 (snappy::MaxCompressedLength): providing that much room at
 * doff[i] is the caller's duty (the sizes are on the device, so the host
 * cannot check it), and nothing is written past the stream's end.  A part of
 * 4 GiB or more gets clen[i] = 0 and no stream (the preamble is a 32-bit
 * varint).  soff[nparts + 1], doff[nparts] and clen[nparts] are device arrays;
 * `scratch` is device memory of psg_snappy_compress_scratch_bytes(the parts'
 * total bytes, nparts) bytes, 256-byte aligned, free again once the call's
 * work on `stream` has run.  Enqueued on `stream`: waits for nothing and
 * allocates nothing.
 * psg_snappy_compress_host is the same rule in plain C++ on host memory and
 * gives the same stream byte for byte; cap below the maximum length is
 * PSG_ERR_SIZE. */
size_t psg_snappy_max_compressed_length(size_t n);
size_t psg_snappy_compress_scratch_bytes(size_t total_src_bytes, uint64_t nparts);
int psg_snappy_compress_dev(const uint8_t* src, const uint64_t* soff, uint64_t nparts,
                            uint8_t* dst, const uint64_t* doff, uint64_t* clen, void* scratch,
                            void* stream);
int psg_snappy_compress_host(const void* src, size_t n, void* dst, size_t cap, size_t* len);
int psg_crc32c_dev(const void* data, const uint64_t* off, uint64_t nseg,
                   uint64_t max_len, const uint32_t* init, uint32_t* out,
                   void* stream);

#ifdef __cplusplus
}
#endif
#endif /* PSG_H_ */
