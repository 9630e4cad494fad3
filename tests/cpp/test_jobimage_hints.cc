// The job-table planner's part in the hinted search partition
// (psg_jobimage.cc fill, JobImage::hints): a hinted image holds zeroes in the
// seg of every search-mode job that is searched on the device and one state
// word per partition item after the plain image, and nothing else changes.
// Addresses are made up and never dereferenced.
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../include/psg.h"
#include "../../parameter_server_amd/csrc/psg_host.h"
#include "../../parameter_server_amd/csrc/psg_jobimage.h"

using namespace psg;

int psg::fail(int code, const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vprintf(fmt, ap);
  va_end(ap);
  printf("\n");
  return code;
}

static int g_bad = 0;
#define CHECK(c)                                                \
  do {                                                          \
    if (!(c) && ++g_bad < 40) printf("line %d: %s\n", __LINE__, #c); \
  } while (0)

static const unsigned char kPoison = 0xA5;
static char* const kBase = (char*)0x7f0000000000ull;

static JobSpec make_job(size_t j, uint64_t nslots, const std::vector<uint64_t>& pn) {
  JobSpec s;
  s.keys = (const uint64_t*)(0x500000000000ull + ((uint64_t)j << 36));
  s.nslots = nslots;
  s.flags = 0;
  for (size_t p = 0; p < pn.size(); ++p) {
    s.pkeys.push_back((const uint64_t*)(0x100000000000ull + ((uint64_t)j << 32 | (uint64_t)p << 16)));
    s.pvals.push_back((const void*)(0x200000000000ull + ((uint64_t)j << 32 | (uint64_t)p << 16)));
    s.pn.push_back(pn[p]);
  }
  s.out.push_back((void*)(0x300000000000ull + ((uint64_t)j << 32)));
  return s;
}

static std::vector<unsigned char> image(JobImage& G, const std::vector<JobSpec>& jobs, bool index) {
  CHECK(G.plan(jobs.data(), jobs.size(), PSG_F32, 1, index) == PSG_OK);
  G.layout(jobs.data(), 128);
  std::vector<unsigned char> img(G.lay.total, kPoison);
  CHECK(G.fill(jobs.data(), (char*)img.data(), kBase, false) == PSG_OK);
  return img;
}

int main() {
  // job 0: long pieces (search mode), 3 tiles + 17 slots, one empty push;
  // job 1: short pieces (stream mode); job 2: no server keys
  std::vector<JobSpec> jobs = {make_job(0, 3 * 1024 + 17, {5000, 0, 4000}),
                               make_job(1, 8 * 1024, {40, 50, 60}),
                               make_job(2, 0, {10})};
  for (int index = 0; index < 2; ++index) {
    JobImage plain, hinted;
    plain.knob_pack = hinted.knob_pack = 0;  // uniform rounds, 1024-slot tiles
    hinted.hints = true;
    const std::vector<unsigned char> a = image(plain, jobs, index != 0);
    const std::vector<unsigned char> b = image(hinted, jobs, index != 0);
    // the hinted image is the plain one plus the waves' state words at its end
    const JobLayout& L = hinted.lay;
    CHECK(L.hstate == a.size() && b.size() == L.hstate + 256);
    CHECK(hinted.nitems == 2 + 3);  // job 0: 2 pushes x 1 group; job 1: 3 one-chunk pushes
    for (uint32_t i = 0; i < hinted.nitems; ++i)
      CHECK(((const uint32_t*)(b.data() + L.hstate))[i] == kHintFresh);
    CHECK(plain.lay.hstate == plain.lay.total);
    CHECK(plain.h[0].mode == kSearch && plain.h[1].mode == kStream);
    CHECK(!hinted.all_search);
    const size_t seg0 = L.job[0].seg, len0 = 4 * (size_t)(4 + 1) * 2;  // 4 tiles, 2 kept pushes
    CHECK(hinted.info[0].ntiles == 4 && hinted.info[0].np == 2);
    CHECK(seg0 + len0 <= b.size());
    for (size_t i = 0; i < a.size() && i < b.size(); ++i) {
      const bool in_seg0 = i >= seg0 && i < seg0 + len0;
      if (in_seg0) {
        CHECK(a[i] == kPoison);  // unhinted: left to the kernel
        CHECK(b[i] == 0);
      } else {
        CHECK(a[i] == b[i]);     // the stream job's seg included
      }
    }
    // the stream job's seg is not written by the host in either image
    const size_t seg1 = L.job[1].seg;
    CHECK(b[seg1] == kPoison && b[seg1 + 4 * 9 * 3 - 1] == kPoison);
  }
  // a dense job's seg is the host's own (not zeroed over)
  {
    std::vector<JobSpec> d = {make_job(0, 2048, {100})};
    d[0].dense = true;
    d[0].dpos = {1000};
    JobImage G;
    G.hints = true;
    const std::vector<unsigned char> img = image(G, d, true);
    const uint32_t* seg = (const uint32_t*)(img.data() + G.lay.job[0].seg);
    CHECK(G.dense && seg[0] == 0 && seg[1] == 24 && seg[2] == 100);
  }
  if (g_bad) printf("%d checks failed\n", g_bad);
  return g_bad ? 1 : 0;
}
