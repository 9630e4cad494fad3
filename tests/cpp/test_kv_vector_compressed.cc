// KVVector::getValueCompressed (parameter_server_amd/csrc/kv_vector.h) built
// with plain g++ against libpsg.so, the way a reference server links it at
// Van::send: the reply's stream decodes (by the oracle) to exactly getValue's
// values, is the host twin's stream of them, and is shorter than they are.
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../oracle/psg_oracle.h"
#include "../../parameter_server_amd/csrc/kv_vector.h"

using psg::Key;
using psg::KVVector;
using psg::Message;
using psg::MessagePtr;

static int failures = 0;
#define EXPECT(c)                                                  \
  do {                                                             \
    if (!(c)) {                                                    \
      std::fprintf(stderr, "%s:%d: EXPECT(%s)\n", __FILE__, __LINE__, #c); \
      ++failures;                                                  \
    }                                                              \
  } while (0)

static MessagePtr key_msg(const std::vector<Key>& k) {
  MessagePtr m(new Message());
  m->task.key_channel = 0;
  m->key = k;
  return m;
}

template <typename V>
static void pull(size_t nreq) {
  // 30,000 server keys 3 i + 7, values in eighths; every third request key
  // is not a server key
  std::vector<Key> D(30000);
  std::vector<V> W(D.size());
  for (size_t i = 0; i < D.size(); ++i) {
    D[i] = 3 * i + 7;
    W[i] = (V)((int)((i * 2654435761u) >> 26) - 32) / 8;
  }
  KVVector<V> kv(0, false);
  kv.setValue(key_msg(D));
  kv.setValueArray(0, W);
  std::vector<Key> req(nreq);
  for (size_t i = 0; i < nreq; ++i) req[i] = 7 + 4 * i + (i % 3 == 2);
  MessagePtr plain = key_msg(req), comp = key_msg(req);
  kv.getValue(plain);
  const std::vector<V> want = nreq ? plain->valueAs<V>(0) : std::vector<V>();
  size_t matched = 12345;
  const std::vector<char> s = kv.getValueCompressed(comp, &matched);
  const size_t raw = nreq * sizeof(V);
  size_t declared = 0;
  EXPECT(orc_snappy_uncompressed_length((const uint8_t*)s.data(), s.size(), &declared) >= 0);
  EXPECT(declared == raw);
  std::vector<V> got(nreq);
  EXPECT(orc_snappy_uncompress((const uint8_t*)s.data(), s.size(), (uint8_t*)got.data(), raw) == 0);
  EXPECT(got.size() == want.size() && (raw == 0 || std::memcmp(got.data(), want.data(), raw) == 0));
  size_t hits = 0;
  for (size_t i = 0; i < nreq; ++i) hits += (req[i] - 7) % 3 == 0 && (req[i] - 7) / 3 < D.size();
  EXPECT(matched == hits);
  // the twin's stream of the same values
  std::vector<char> twin(psg_snappy_max_compressed_length(raw));
  size_t tl = 0;
  EXPECT(psg_snappy_compress_host(want.data(), raw, twin.data(), twin.size(), &tl) == PSG_OK);
  EXPECT(tl == s.size() && std::memcmp(twin.data(), s.data(), tl) == 0);
  if (nreq >= 1000) EXPECT(s.size() < raw);
}

int main() {
  pull<float>(20000);
  pull<double>(20000);
  pull<float>(1);
  pull<float>(0);
  if (failures) {
    std::fprintf(stderr, "%d failure(s)\n", failures);
    return 1;
  }
  std::printf("test_kv_vector_compressed: ok\n");
  return 0;
}
