// TEST INFRASTRUCTURE ONLY.  C entry points onto the reference's own match,
// oldMatch and sliceKeyOrderedMsg (reference src/system/message.h:89-267) and
// Range<uint64>::evenDivide (src/base/range.h:85-98), compiled in place from
// the reference tree by oracle/Makefile into oracle/_ref/, with
// src/util/threadpool.cc for match's per-call ThreadPool.  oracle/standin/
// supplies the containers, message structs, CHECK macros and flags those
// headers ask for.  Used by tools/record_reference.py and
// tests/test_reference_pin.py to pin oracle/psg_oracle.c's restatements.
//
// PINNED here: match, oldMatch, sliceKeyOrderedMsg, evenDivide.
// OURS, not pinned: the per-push loops of ref_aggregate_* below.  They follow
// KVVector::parallelSetValue (parameter/kv_vector.h:106-132: the first push
// is matched with ASSIGN, later ones with ADD) and serialSetValue
// (:185-201: oldMatch, the first aligned array kept, later ones added
// elementwise; Eigen's array += is one IEEE add per element), and
// serialGetValue (:216-227) in ref_gather_*: they do what those loops do and
// are written here, not taken from there.  So are the SArray members
// (findRange, segment) of oracle/standin/base/shared_array.h.
#include "system/message.h"

int FLAGS_num_threads = 1;

using namespace PS;

namespace {

template <typename T> SArray<T> copy_in(const T* p, size_t n) {
  SArray<T> a(n);
  if (n) memcpy(a.data(), p, n * sizeof(T));
  return a;
}

template <typename V>
size_t do_match(int threads, size_t lo, size_t hi, const uint64* dk, size_t nd,
                V* dv, const uint64* sk, const V* sv, size_t ns, int add) {
  FLAGS_num_threads = threads;
  SArray<uint64> D = copy_in(dk, nd), S = copy_in(sk, ns);
  SArray<V> val = copy_in(sv, ns), out = copy_in(dv, hi - lo);
  size_t matched = 0;
  match<uint64, V>(SizeR(lo, hi), D, out, S, val, &matched,
                   add ? MatchOperation::ADD : MatchOperation::ASSIGN);
  if (hi > lo) memcpy(dv, out.data(), (hi - lo) * sizeof(V));
  return matched;
}

template <typename V>
int do_old_match(const uint64* dk, size_t nd, const uint64* sk, size_t ns,
                 const V* sv, uint64 kb, uint64 ke, V* out, size_t* lo,
                 size_t* hi, size_t* matched) {
  SArray<uint64> D = copy_in(dk, nd), S = copy_in(sk, ns);
  SArray<V> val = copy_in(sv, ns);
  auto r = oldMatch<uint64, V>(D, S, val.data(), Range<uint64>(kb, ke), matched);
  *lo = r.first.begin();
  *hi = r.first.end();
  if (r.second.size()) memcpy(out, r.second.data(), r.second.size() * sizeof(V));
  return 0;
}

// The fold of one time's pushes, in arrival order.  What the loop does is
// KVVector's (parallelSetValue, kv_vector.h:84-137: the first non-empty push
// is matched with ASSIGN into fresh sums, every later one with ADD;
// serialSetValue, :171-204: each push is spread by oldMatch, the first spread
// is kept and later ones are added element by element); how it is written is
// ours.  sums[i] holds value array i's aggregate over the server slots.
template <typename V>
int do_aggregate(const uint64* Dk, size_t nD, uint64 kb, uint64 ke, int npush,
                 const uint64* const* keys, const size_t* n, int m,
                 const V* const* vals, int parallel, int nthreads,
                 V* const* out, size_t* lo, size_t* hi, size_t* matched) {
  FLAGS_num_threads = nthreads;
  *lo = *hi = 0;
  const SArray<uint64> server = copy_in(Dk, nD);
  const Range<uint64> owned(kb, ke);
  SizeR slots;                  // server positions of `owned`
  std::vector<SArray<V>> sums;  // empty until the first non-empty push
  for (int p = 0; p < npush; ++p) {
    matched[p] = 0;
    if (n[p] == 0) continue;  // an empty push is dropped before any of this
    if (nD == 0) return -1;
    const SArray<uint64> pushed = copy_in(keys[p], n[p]);
    const bool first = sums.empty();
    if (first) slots = server.findRange(owned);
    for (int i = 0; i < m; ++i) {
      const SArray<V> values = copy_in(vals[(size_t)p * m + i], n[p]);
      size_t hit = 0;
      if (parallel) {
        if (first) sums.push_back(SArray<V>(slots.size()));
        match(slots, server, sums[i], pushed, values, &hit,
              first ? MatchOperation::ASSIGN : MatchOperation::ADD);
      } else {
        AlignedArray<V> spread =
            oldMatch(server, pushed, values.data(), owned, &hit);
        if (!(spread.first == slots)) return -2;
        if (first) {
          sums.push_back(spread.second);
        } else {
          V* acc = sums[i].data();
          const V* term = spread.second.data();
          for (size_t j = 0; j < slots.size(); ++j) acc[j] += term[j];
        }
      }
      matched[p] = hit;
    }
  }
  if (!sums.empty()) {
    *lo = slots.begin();
    *hi = slots.end();
    for (int i = 0; i < m; ++i)
      if (slots.size()) memcpy(out[i], sums[i].data(), slots.size() * sizeof(V));
  }
  return 0;
}

// A pull: the server's values spread onto the request's keys, zero where the
// server lacks the key.  As KVVector::serialGetValue (kv_vector.h:216-227)
// this is oldMatch with the request as destination over a key range that
// covers both key lists; the range is worked out here from the end keys.
template <typename V>
void do_gather(const uint64* Dk, size_t nD, const V* W, const uint64* req,
               size_t nreq, V* out, size_t* matched) {
  *matched = 0;
  if (nreq) memset(out, 0, nreq * sizeof(V));
  if (nreq == 0 || nD == 0) return;
  const SArray<uint64> server = copy_in(Dk, nD), wanted = copy_in(req, nreq);
  const SArray<V> weights = copy_in(W, nD);
  const uint64 low = std::min(req[0], Dk[0]);
  const uint64 high = std::max(req[nreq - 1], Dk[nD - 1]);
  AlignedArray<V> got = oldMatch(wanted, server, weights.data(),
                                 Range<uint64>(low, high + 1), matched);
  if (got.second.size())
    memcpy(out, got.second.data(), got.second.size() * sizeof(V));
}

}  // namespace

extern "C" {

size_t ref_match_f32(int threads, size_t lo, size_t hi, const uint64* dk,
                     size_t nd, float* dv, const uint64* sk, const float* sv,
                     size_t ns, int add) {
  return do_match<float>(threads, lo, hi, dk, nd, dv, sk, sv, ns, add);
}
size_t ref_match_f64(int threads, size_t lo, size_t hi, const uint64* dk,
                     size_t nd, double* dv, const uint64* sk, const double* sv,
                     size_t ns, int add) {
  return do_match<double>(threads, lo, hi, dk, nd, dv, sk, sv, ns, add);
}

int ref_old_match_f32(const uint64* dk, size_t nd, const uint64* sk, size_t ns,
                      const float* sv, uint64 kb, uint64 ke, float* out,
                      size_t* lo, size_t* hi, size_t* matched) {
  return do_old_match<float>(dk, nd, sk, ns, sv, kb, ke, out, lo, hi, matched);
}
int ref_old_match_f64(const uint64* dk, size_t nd, const uint64* sk, size_t ns,
                      const double* sv, uint64 kb, uint64 ke, double* out,
                      size_t* lo, size_t* hi, size_t* matched) {
  return do_old_match<double>(dk, nd, sk, ns, sv, kb, ke, out, lo, hi, matched);
}

int ref_aggregate_f32(const uint64* D, size_t nD, uint64 kb, uint64 ke,
                      int npush, const uint64* const* keys, const size_t* n,
                      int m, const float* const* vals, int parallel,
                      int nthreads, float* const* out, size_t* lo, size_t* hi,
                      size_t* matched) {
  return do_aggregate<float>(D, nD, kb, ke, npush, keys, n, m, vals, parallel,
                             nthreads, out, lo, hi, matched);
}
int ref_aggregate_f64(const uint64* D, size_t nD, uint64 kb, uint64 ke,
                      int npush, const uint64* const* keys, const size_t* n,
                      int m, const double* const* vals, int parallel,
                      int nthreads, double* const* out, size_t* lo, size_t* hi,
                      size_t* matched) {
  return do_aggregate<double>(D, nD, kb, ke, npush, keys, n, m, vals, parallel,
                              nthreads, out, lo, hi, matched);
}

void ref_gather_f32(const uint64* D, size_t nD, const float* W,
                    const uint64* req, size_t nreq, float* out,
                    size_t* matched) {
  do_gather<float>(D, nD, W, req, nreq, out, matched);
}
void ref_gather_f64(const uint64* D, size_t nD, const double* W,
                    const uint64* req, size_t nreq, double* out,
                    size_t* matched) {
  do_gather<double>(D, nD, W, req, nreq, out, matched);
}

// sliceKeyOrderedMsg<uint64> over a message of n keys and one uint32 value
// per key.  For piece i: valid[i]; a valid piece's key segment as positions
// [begin[i], end[i]) of the message's keys, and vbegin[i], the position its
// value segment starts at.  An invalid piece leaves -1 in all three.
void ref_slice_key_ordered(const uint64* keys, size_t n, uint64 rb, uint64 re,
                           const uint64* sep, size_t nsep, long long* begin,
                           long long* end, long long* vbegin, int* valid) {
  MessagePtr msg(new Message());
  msg->task.mutable_key_range()->set_begin(rb);
  msg->task.mutable_key_range()->set_end(re);
  SArray<uint64> k = copy_in(keys, n);
  SArray<uint32> v(n);
  msg->key = SArray<char>(k);
  msg->addValue(v);
  KeyList s(sep, sep + nsep);
  MessagePtrList pieces = sliceKeyOrderedMsg<uint64>(msg, s);
  for (size_t i = 0; i < pieces.size(); ++i) {
    valid[i] = pieces[i]->valid ? 1 : 0;
    begin[i] = end[i] = vbegin[i] = -1;
    if (!pieces[i]->valid) continue;
    SArray<uint64> pk(pieces[i]->key);
    begin[i] = n ? pk.data() - k.data() : 0;
    end[i] = begin[i] + (long long)pk.size();
    vbegin[i] = 0;
    if (n && !pieces[i]->value.empty())
      vbegin[i] = SArray<uint32>(pieces[i]->value[0]).data() - v.data();
  }
}

void ref_even_divide_u64(uint64 b, uint64 e, size_t n, size_t i, uint64* ob,
                         uint64* oe) {
  Range<uint64> r = Range<uint64>(b, e).evenDivide(n, i);
  *ob = r.begin();
  *oe = r.end();
}

// Range<uint64>::all() (range.h:75-78)
void ref_range_all_u64(uint64* ob, uint64* oe) {
  Range<uint64> r = Range<uint64>::all();
  *ob = r.begin();
  *oe = r.end();
}

}  // extern "C"
