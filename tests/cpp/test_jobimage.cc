// The job-table planner (parameter_server_amd/csrc/psg_jobimage.cc) on the
// CPU: form, counts, layout, shape key and image of a batch of merge jobs.
// Push, key and device addresses are made up and never dereferenced.  Every
// expectation is recomputed here from a plain description of the job (loops
// and divisions written out), not with the module's helpers.
#include <algorithm>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/psg.h"
#include "../../parameter_server_amd/csrc/psg_host.h"
#include "../../parameter_server_amd/csrc/psg_jobimage.h"

using namespace psg;

// the library's error recorder (psg_runtime.hip there)
static std::string g_err;
int psg::fail(int code, const char* fmt, ...) {
  char buf[512];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof(buf), fmt, ap);
  va_end(ap);
  g_err = buf;
  return code;
}

static int g_bad = 0;
static const char* g_case = "";
#define CHECK(c)                                                          \
  do {                                                                    \
    if (!(c)) {                                                           \
      if (++g_bad < 40) printf("%s: line %d: %s\n", g_case, __LINE__, #c); \
    }                                                                     \
  } while (0)
#define CHECK_EQ(a, b)                                                              \
  do {                                                                              \
    const unsigned long long _a = (unsigned long long)(a), _b = (unsigned long long)(b); \
    if (_a != _b) {                                                                 \
      if (++g_bad < 40)                                                             \
        printf("%s: line %d: %s = %llu, want %s = %llu\n", g_case, __LINE__, #a, _a, #b, _b); \
    }                                                                               \
  } while (0)

static const uint64_t kKeys = 0x500000000000ull;  // D of job j at kKeys + j << 36
static const uint64_t kPush = 0x100000000000ull;  // push p of job j: + (j << 32 | p << 20)
static const uint64_t kVals = 0x200000000000ull;
static const uint64_t kOut = 0x300000000000ull;
static char* const kBase = (char*)0x7f0000000000ull;  // the device image
static const unsigned char kPoison = 0xA5;

static JobSpec make_job(size_t j, uint64_t nslots, const std::vector<uint64_t>& pn, int m,
                        uint32_t flags = 0, uint64_t gen = 0) {
  JobSpec s;
  s.keys = (const uint64_t*)(kKeys + ((uint64_t)j << 36));
  s.nslots = nslots;
  s.flags = flags;
  for (size_t p = 0; p < pn.size(); ++p) {
    const uint64_t a = ((uint64_t)j << 32 | (uint64_t)p << 16) + gen * 4096;
    s.pkeys.push_back((const uint64_t*)(kPush + a));
    for (int i = 0; i < m; ++i) s.pvals.push_back((const void*)(kVals + a + 256 * i));
    s.pn.push_back(pn[p]);
  }
  for (int i = 0; i < m; ++i) s.out.push_back((void*)(kOut + ((uint64_t)j << 32) + 256 * i));
  return s;
}

struct Case {
  const char* name;
  std::vector<JobSpec> jobs;
  int m = 1, dtype = PSG_F32;
  bool index = false;
  int part = -1, pack = -1, wide = -1, cursor = -1;
  // expected form
  uint32_t tile = 1024;
  bool xpack = false, xwide = false, xdense = false, xcursor = false, xpcursor = false;
};

static size_t up(size_t x, size_t a) {
  while (x % a) ++x;
  return x;
}

struct Region {
  const char* name;
  size_t off, size, pad;
  bool zeroed;
};

// Plans, lays out and fills the case into a poisoned image, and checks
// everything that holds for every image.  Returns the image.
static std::vector<unsigned char> run_case(const Case& c, JobImage& G, bool expect_same = false) {
  g_case = c.name;
  const std::vector<JobSpec>& jobs = c.jobs;
  const size_t nj = jobs.size();
  const int m = c.m;
  G.knob_part = c.part;
  G.knob_pack = c.pack;
  G.knob_wide = c.wide;
  G.knob_cursor = c.cursor;
  CHECK_EQ(G.plan(jobs.data(), nj, c.dtype, m, c.index), PSG_OK);
  CHECK_EQ(G.tile, c.tile);
  CHECK_EQ(G.pack, c.xpack);
  CHECK_EQ(G.wide, c.xwide);
  CHECK_EQ(G.dense, c.xdense);
  CHECK_EQ(G.cursor, c.xcursor);
  CHECK_EQ(G.pcursor, c.xpcursor);
  const uint32_t tile = c.tile, iw = tile / 8;  // 4 bits per slot
  const bool use_index = c.index && !c.xdense, chunked = c.xcursor || c.xpcursor;

  // ---- the naive description of every job ----
  struct Want {
    std::vector<uint64_t> pn;
    std::vector<uint32_t> slot;
    uint32_t nt = 0, mode = kSearch, segq = 1, segb = 0, split_begin = 0;
    bool split = false;
    std::vector<uint64_t> items;
    uint32_t nsplit = 0, nch = 0, ch0 = 0;
  };
  std::vector<Want> W(nj);
  std::vector<uint64_t> items;
  std::vector<uint32_t> sitems;
  uint64_t tiles = 0, npall = 0;
  bool all_search = true;
  for (size_t j = 0; j < nj; ++j) {
    const JobSpec& s = jobs[j];
    Want& w = W[j];
    uint64_t kv = 0;
    for (size_t p = 0; p < s.pn.size(); ++p)
      if (s.pn[p]) {
        w.pn.push_back(s.pn[p]);
        w.slot.push_back((uint32_t)p);
        kv += s.pn[p];
      }
    const size_t np = w.pn.size();
    w.nt = (uint32_t)(s.nslots / tile + (s.nslots % tile != 0));
    const uint64_t nt1 = s.nslots / 1024 + (s.nslots % 1024 != 0);
    const bool stream = !s.dense && (c.part >= 0 ? c.part == (int)kStream
                                                 : np && nt1 && (double)kv / (double)(np * nt1) < 24.0);
    w.mode = stream ? kStream : kSearch;
    all_search = all_search && !stream;
    w.segq = stream ? w.nt + 1 : 1;
    w.segb = stream ? 1 : (uint32_t)np;
    const bool work = w.nt && np && !s.dense;
    w.split = stream || (c.index && work);
    if (work && w.split) {
      w.split_begin = (uint32_t)sitems.size();
      const uint64_t span = std::max<uint64_t>(w.nt + 1, np);
      for (uint64_t b = 0; b * 256 < span; ++b) sitems.push_back((uint32_t)j), ++w.nsplit;
    }
    if (work && !stream)  // one item per push per group of 64 boundaries 0..nt
      for (uint64_t g = 0; g * 64 <= w.nt; ++g)
        for (size_t p = 0; p < np; ++p) w.items.push_back((uint64_t)j << 37 | (uint64_t)p << 24 | g);
    if (work && stream)  // one item per push per chunk of 512 keys
      for (size_t p = 0; p < np; ++p)
        for (uint64_t ch = 0; ch * 512 < w.pn[p]; ++ch)
          w.items.push_back((uint64_t)j << 37 | (uint64_t)p << 24 | ch);
    items.insert(items.end(), w.items.begin(), w.items.end());
    tiles += w.nt;
    npall += np;
  }
  uint32_t nchunks = 0;
  if (chunked) {
    const uint64_t target = c.xcursor ? 2048 : 1024;
    uint64_t per = 1;
    while (per * target < tiles) ++per;
    for (Want& w : W) {
      w.ch0 = nchunks;
      for (uint64_t t = 0; t < w.nt; t += per) ++w.nch;
      nchunks += w.nch;
    }
  }
  const uint32_t bxs = c.xpcursor ? 256 : 32;

  // ---- plan ----
  CHECK_EQ(G.ntiles, tiles);
  CHECK_EQ(G.nitems, items.size());
  CHECK_EQ(G.nsplit, sitems.size());
  CHECK_EQ(G.nchunks, nchunks);
  CHECK_EQ(G.bxs, bxs);
  CHECK_EQ(G.all_search, all_search);
  CHECK_EQ(G.h.size(), nj);
  CHECK_EQ(G.info.size(), nj);
  for (size_t j = 0; j < nj; ++j) {
    const Want& w = W[j];
    const JobInfo& I = G.info[j];
    const JobDev& d = G.h[j];
    CHECK_EQ(I.np, w.pn.size());
    CHECK_EQ(I.ncaller, jobs[j].pn.size());
    CHECK(I.pn == w.pn);
    CHECK(I.slot == w.slot);
    CHECK_EQ(I.ntiles, w.nt);
    CHECK_EQ(I.segq, w.segq);
    CHECK_EQ(I.nitems, w.items.size());
    CHECK_EQ(I.nsplit, w.nsplit);
    CHECK_EQ(I.has_split, w.split);
    CHECK_EQ(I.nch, w.nch);
    if (chunked) CHECK_EQ(I.ch0, w.ch0);
    CHECK_EQ(d.nslots, jobs[j].nslots);
    CHECK_EQ(d.npush, w.pn.size());
    CHECK_EQ(d.ntiles, w.nt);
    CHECK_EQ(d.tile, tile);
    CHECK_EQ(d.mode, w.mode);
    CHECK_EQ(d.segq, w.segq);
    CHECK_EQ(d.segb, w.segb);
    if (w.nsplit) CHECK_EQ(d.split_begin, w.split_begin);
  }

  // ---- layout: the regions in image order, each padded to `pad` ----
  G.layout(jobs.data(), iw);
  const JobLayout& L = G.lay;
  CHECK_EQ(L.iw, iw);
  CHECK_EQ(L.job.size(), nj);
  std::vector<Region> R;
  R.push_back({"jobs", JobLayout::jobs, sizeof(JobDev) * nj, 256, false});
  R.push_back({"tiles", L.tiles, sizeof(TileDesc) * tiles, 256, false});
  R.push_back({"index", L.index, use_index ? 4 * (size_t)iw * tiles : 0, 256, false});
  R.push_back({"marked", L.marked, use_index ? 256u : 0u, 256, false});
  R.push_back({"sitems", L.sitems, 4 * sitems.size(), 256, false});
  R.push_back({"items", L.items, 8 * items.size(), 256, false});
  R.push_back({"cjobs", L.cjobs, c.xcursor ? sizeof(CursorJob) * nj : 0, 256, false});
  R.push_back({"chunks", L.chunks, chunked ? sizeof(CursorChunk) * nchunks : 0, 256, false});
  R.push_back({"fail", L.zero, 8 * npall, 256, true});
  R.push_back({"bx", L.bx, chunked ? 4 * (size_t)bxs * (nchunks + 1) : 0, 256, true});
  const size_t nlead = R.size();
  for (size_t j = 0; j < nj; ++j) {
    const JobLayout::Job& o = L.job[j];
    const size_t np = W[j].pn.size(), nt = W[j].nt;
    R.push_back({"pk", o.pk, 8 * np, 64, false});
    R.push_back({"pv", o.pv, 8 * np * m, 64, false});
    R.push_back({"pn", o.pn, 8 * np, 64, false});
    R.push_back({"out", o.out, 8 * (size_t)m, 64, false});
    R.push_back({"seg", o.seg, 4 * (nt + 1) * np, 256, false});
    R.push_back({"split", o.split, W[j].split ? 8 * (nt + 1) : 0, 256, false});
    R.push_back({"dpos", o.dpos, jobs[j].dense ? 8 * np : 0, 256, false});
  }
  size_t want_off = 0;
  for (size_t r = 0; r < R.size(); ++r) {
    if (R[r].off != want_off)
      printf("%s: region %zu (%s) at %zu, want %zu\n", c.name, r, R[r].name, R[r].off, want_off), ++g_bad;
    CHECK(R[r].off + R[r].size <= L.total);
    const bool a64 = r >= nlead && (!strcmp(R[r].name, "pv") || !strcmp(R[r].name, "pn") ||
                                    !strcmp(R[r].name, "out") || !strcmp(R[r].name, "seg"));
    CHECK_EQ(R[r].off % (a64 ? 64 : 256), 0);
    for (size_t q = 0; q < r; ++q) CHECK(R[q].off + R[q].size <= R[r].off);  // pairwise disjoint
    want_off = up(R[r].off + R[r].size, R[r].pad);
  }
  CHECK_EQ(L.total, want_off);
  CHECK_EQ(L.zero_end, nj ? L.job[0].pk : L.total);
  // the zero region holds the fail counters and the boundary words, no more
  for (const Region& r : R) {
    const bool inside = r.off >= L.zero && r.off + r.size <= L.zero_end;
    const bool outside = r.off + r.size <= L.zero || r.off >= L.zero_end;
    if (r.size) CHECK(r.zeroed ? inside : outside);
  }
  size_t fail_off = L.zero;
  for (size_t j = 0; j < nj; ++j) {  // the fail counters: packed, in job order
    CHECK_EQ(L.job[j].fail, fail_off);
    fail_off += 8 * W[j].pn.size();
  }
  CHECK(fail_off <= L.bx);

  // ---- shape key and fill ----
  const bool same = G.same_shape(jobs.data(), kBase);
  CHECK_EQ(same, expect_same);
  std::vector<unsigned char> img(L.total, kPoison);
  CHECK_EQ(G.fill(jobs.data(), (char*)img.data(), kBase, same), PSG_OK);
  G.keep_shape();
  for (size_t b = 0; b < L.total; ++b) {  // zeroed: the zero region and the marked word only
    const bool z = (b >= L.zero && b < L.zero_end) || (use_index && b >= L.marked && b < L.marked + 8);
    if (z && img[b] != 0) {
      CHECK(!"zero region not zeroed");
      break;
    }
  }
  if (use_index) CHECK_EQ(img[L.marked + 8], kPoison);
  const JobDev* hj = (const JobDev*)img.data();
  const TileDesc* ht = (const TileDesc*)(img.data() + L.tiles);
  uint64_t tcur = 0;
  for (size_t j = 0; j < nj; ++j) {
    const JobSpec& s = jobs[j];
    const Want& w = W[j];
    const JobLayout::Job& o = L.job[j];
    const size_t np = w.pn.size();
    const JobDev& d = hj[j];
    CHECK(memcmp(&d, &G.h[j], sizeof(JobDev)) == 0);
    CHECK(d.dkeys == s.keys);
    CHECK((char*)d.pkeys == kBase + o.pk);
    CHECK((char*)d.pn == kBase + o.pn);
    CHECK((char*)d.seg == kBase + o.seg);
    CHECK((char*)d.fail == kBase + o.fail);
    CHECK((char*)d.split == (w.split ? kBase + o.split : nullptr));
    CHECK(G.info[j].seg == d.seg);
    CHECK(G.info[j].fail == d.fail);
    const uint64_t* hk = (const uint64_t*)(img.data() + o.pk);
    const uint64_t* hv = (const uint64_t*)(img.data() + o.pv);
    const uint64_t* hn = (const uint64_t*)(img.data() + o.pn);
    const uint64_t* ho = (const uint64_t*)(img.data() + o.out);
    for (size_t p = 0; p < np; ++p) {
      CHECK_EQ(hk[p], (uint64_t)s.pkeys[w.slot[p]]);
      CHECK_EQ(hn[p], w.pn[p]);
      for (int i = 0; i < m; ++i) CHECK_EQ(hv[p * m + i], (uint64_t)s.pvals[w.slot[p] * m + i]);
    }
    for (int i = 0; i < m; ++i) CHECK_EQ(ho[i], (uint64_t)s.out[i]);
    if (s.dense) {
      const uint64_t* hd = (const uint64_t*)(img.data() + o.dpos);
      const uint32_t* hs = (const uint32_t*)(img.data() + o.seg);
      for (size_t p = 0; p < np; ++p) {
        const uint64_t dp = s.dpos[w.slot[p]];
        CHECK_EQ(hd[p], dp);
        for (uint64_t t = 0; t <= w.nt; ++t) {  // clamp(t * tile - dpos, 0, n), tile-major
          long long v = (long long)(t * tile) - (long long)dp;
          v = v < 0 ? 0 : v > (long long)w.pn[p] ? (long long)w.pn[p] : v;
          CHECK_EQ(hs[t * np + p], v);
        }
      }
    }
    for (uint32_t t = 0; t < w.nt && !same; ++t, ++tcur) {
      const TileDesc& T = ht[tcur];
      const uint64_t slot0 = (uint64_t)t * tile;
      const bool last = slot0 + tile >= s.nslots;
      CHECK(T.dk == s.keys + slot0);
      CHECK((char*)T.seg == kBase + o.seg + 4 * (size_t)t * w.segb);
      CHECK((char*)T.pkeys == kBase + o.pk);
      CHECK((char*)T.pvals == kBase + o.pv);
      CHECK((char*)T.pn == kBase + o.pn);
      CHECK((char*)T.out == kBase + o.out);
      CHECK((char*)T.fail == kBase + o.fail);
      CHECK_EQ(T.slot0, slot0);
      CHECK_EQ(T.nt, last ? s.nslots - slot0 : tile);
      CHECK_EQ(T.np, np);
      CHECK_EQ(T.stride, w.segq);
      CHECK_EQ(T.segb, w.segb);
      CHECK_EQ(T.flags, s.flags | (last ? kFlagLastTile : 0u));
      CHECK((char*)T.dpos == (s.dense ? kBase + o.dpos : nullptr));
      CHECK((char*)T.bt == (use_index ? kBase + L.index + 4 * (size_t)iw * tcur : nullptr));
    }
  }
  if (!same) {
    CHECK(std::equal(items.begin(), items.end(), (const uint64_t*)(img.data() + L.items)));
    CHECK(std::equal(sitems.begin(), sitems.end(), (const uint32_t*)(img.data() + L.sitems)));
  } else {  // descriptors, index and items stay as they are on the device
    for (size_t b = L.tiles; b < L.zero; ++b)
      if (img[b] != kPoison) {
        CHECK(!"same shape: tile or item region rewritten");
        break;
      }
  }

  // ---- cursor tables ----
  if (chunked) {
    const CursorJob* cj = (const CursorJob*)(img.data() + L.cjobs);
    const CursorChunk* ch = (const CursorChunk*)(img.data() + L.chunks);
    uint64_t tbase = 0;
    uint32_t k = 0;
    for (size_t j = 0; j < nj; ++j) {
      const Want& w = W[j];
      // the job's chunks tile [0, ntiles) (packed: its tile descriptors) in order
      uint64_t next = c.xpcursor ? tbase : 0;
      for (uint32_t i = 0; i < w.nch; ++i, ++k) {
        CHECK_EQ(ch[k].job, j);
        CHECK_EQ(ch[k].t0, next);
        CHECK(ch[k].t1 > ch[k].t0);
        next = ch[k].t1;
      }
      CHECK_EQ(next, (c.xpcursor ? tbase : 0) + w.nt);
      if (c.xcursor) {
        const CursorJob& J = cj[j];
        const JobLayout::Job& o = L.job[j];
        CHECK(J.dkeys == jobs[j].keys);
        CHECK_EQ(J.nslots, jobs[j].nslots);
        CHECK((char*)J.pkeys == kBase + o.pk);
        CHECK((char*)J.pvals == kBase + o.pv);
        CHECK((char*)J.pn == kBase + o.pn);
        CHECK((char*)J.out == kBase + o.out);
        CHECK((char*)J.fail == kBase + o.fail);
        CHECK((char*)J.seg == kBase + o.seg);
        CHECK((char*)J.bt == kBase + L.index + 4 * (size_t)iw * tbase);
        CHECK_EQ(J.np, w.pn.size());
        CHECK_EQ(J.ntiles, w.nt);
        CHECK_EQ(J.flags, jobs[j].flags);
        CHECK_EQ(J.kr, G.ckr);
        CHECK_EQ(G.info[j].kr, G.ckr);
      }
      tbase += w.nt;
    }
    CHECK_EQ(k, nchunks);
  }
  return img;
}

static Case one_job(const char* name, uint64_t nslots, const std::vector<uint64_t>& pn, int m = 1) {
  Case c;
  c.name = name;
  c.m = m;
  c.jobs.push_back(make_job(0, nslots, pn, m));
  return c;
}

static void tile_edges() {
  for (uint64_t n : {0ull, 1ull, 1024ull, 1025ull, 2049ull}) {
    JobImage G;
    Case c = one_job("tile edges", n, {3000});
    run_case(c, G);
    CHECK_EQ(G.ntiles, n == 0 ? 0 : n <= 1024 ? 1 : n == 1025 ? 2 : 3);
  }
}

static void tile_size() {
  for (int np : {32, 33}) {  // long pieces: the uniform kernel, groups of 32 or 64 pushes
    JobImage G;
    Case c = one_job("tile size", 4096, std::vector<uint64_t>(np, 4000));
    c.jobs[0].pn.push_back(0);  // an empty push does not count
    c.jobs[0].pkeys.push_back(nullptr);
    c.jobs[0].pvals.push_back(nullptr);
    c.tile = np == 32 ? 1024 : 2048;
    c.xwide = np == 33;
    run_case(c, G);
  }
  // 40 short pushes are packed and wide by themselves, 2 long ones neither
  struct { bool small; int pack, wide; bool xpack, xwide; uint32_t tile; } forced[] = {
      {true, 0, 0, false, false, 1024},   {true, 0, -1, false, true, 2048},
      {true, -1, 0, true, false, 2048},   {false, 1, -1, true, false, 2048},
      {false, -1, 1, false, true, 2048},  {false, -1, -1, false, false, 1024}};
  for (auto f : forced) {
    JobImage G;
    Case c = one_job("forced form", 5000, f.small ? std::vector<uint64_t>(40, 20)
                                                  : std::vector<uint64_t>(2, 4000));
    c.pack = f.pack;
    c.wide = f.wide;
    c.xpack = f.xpack;
    c.xwide = f.xwide;
    c.tile = f.tile;
    run_case(c, G);
  }
  JobImage G;
  Case c = one_job("packed by itself", 5000, std::vector<uint64_t>(4, 70));  // 70 / 5 tiles < 16
  c.xpack = true;
  c.tile = 2048;
  run_case(c, G);
}

static void empty_pushes() {
  JobImage G;
  Case c = one_job("empty pushes", 3000, {2000, 0, 2000}, 2);
  c.jobs.push_back(make_job(1, 3000, {0, 0}, 2));
  c.jobs.push_back(make_job(2, 0, {5}, 2));
  run_case(c, G);
  CHECK_EQ(G.info[0].np, 2);
  CHECK_EQ(G.info[0].slot[1], 2);
  CHECK_EQ(G.info[0].ncaller, 3);
  CHECK_EQ(G.info[1].np, 0);
  CHECK_EQ(G.info[1].ncaller, 2);
  CHECK_EQ(G.info[1].nitems, 0);
  CHECK_EQ(G.info[2].ntiles, 0);
  Case none;
  none.name = "no jobs";
  run_case(none, G);
  CHECK_EQ(G.lay.total, 0);
}

static void search_items() {
  for (uint32_t nt : {63u, 64u}) {  // (nt + 64) / 64 goes 1 -> 2
    for (bool index : {false, true}) {
      JobImage G;
      Case c = one_job("search items", (uint64_t)nt * 1024 - 5, {100000, 0, 90000, 80000});
      c.index = index;
      run_case(c, G);
      CHECK_EQ(G.h[0].mode, kSearch);
      CHECK_EQ(G.nitems, (nt == 63 ? 1 : 2) * 3);
      CHECK_EQ(G.nsplit, index ? 1 : 0);
    }
  }
}

static void stream_mode() {
  {  // mean piece 23.95 and 24 keys per push per 1024 slots: streams below 24
    JobImage G;
    Case c = one_job("stream threshold", 10 * 1024, {240, 239});
    c.jobs.push_back(make_job(1, 10 * 1024, {240, 240}, 1));
    c.pack = 0;
    run_case(c, G);
    CHECK_EQ(G.h[0].mode, kStream);
    CHECK_EQ(G.h[1].mode, kSearch);
    CHECK_EQ(G.h[0].segq, 11);  // push-major
    CHECK_EQ(G.h[0].segb, 1);
    CHECK_EQ(G.h[1].segq, 1);  // tile-major
    CHECK_EQ(G.h[1].segb, 2);
  }
  {
    JobImage G;
    Case c = one_job("stream chunks", 64 * 1024, {512, 513, 1});
    c.pack = 0;
    run_case(c, G);
    CHECK_EQ(G.h[0].mode, kStream);
    CHECK_EQ(G.nitems, 1 + 2 + 1);
  }
  for (int part : {(int)kSearch, (int)kStream}) {  // PSG_PART_*
    JobImage G;
    Case c = one_job("forced partition", 64 * 1024, {512, 60000});
    c.part = part;
    run_case(c, G);
    CHECK_EQ(G.h[0].mode, part);
  }
}

static void splitter_items() {
  for (uint32_t nt : {255u, 256u}) {  // max(nt + 1, np) of 256 and 257
    JobImage G;
    Case c = one_job("splitter items", (uint64_t)nt * 1024, {100, 200});
    c.pack = 0;
    run_case(c, G);
    CHECK_EQ(G.h[0].mode, kStream);
    CHECK_EQ(G.nsplit, nt == 255 ? 1 : 2);
  }
  for (int np : {256, 257}) {  // np > nt + 1
    JobImage G;
    Case c = one_job("splitter items by pushes", 2048, std::vector<uint64_t>(np, 3));
    c.pack = 0;
    c.wide = 1;
    c.xwide = true;
    c.tile = 2048;
    run_case(c, G);
    CHECK_EQ(G.h[0].mode, kStream);
    CHECK_EQ(G.nsplit, np == 256 ? 1 : 2);
  }
}

static void dense_job() {
  for (bool index : {false, true}) {
    JobImage G;
    // slices at 0, mid-tile and ending at nslots; an empty push between
    Case c = one_job("dense", 5000, {1500, 0, 2000, 700}, 2);
    c.index = index;
    c.jobs[0].dense = true;
    c.jobs[0].dpos = {0, 0, 1500, 4300};
    c.xdense = true;
    run_case(c, G);
    CHECK_EQ(G.nitems, 0);
    CHECK_EQ(G.nsplit, 0);
    CHECK_EQ(G.h[0].mode, kSearch);
  }
  JobImage G;  // one job not dense: the batch takes the general kernels
  Case c = one_job("dense mixed", 5000, {1500, 2000}, 1);
  c.jobs[0].dense = true;
  c.jobs[0].dpos = {100, 3000};
  c.jobs.push_back(make_job(1, 5000, {1500, 2000}, 1));
  run_case(c, G);
  CHECK_EQ(G.info[0].nitems, 0);
  CHECK(G.info[1].nitems > 0);
}

static void cursor_forms() {
  {  // 2049 tiles: just above the 2048-chunk target, 2 tiles per chunk
    JobImage G;
    Case c = one_job("cursor", 1500 * 1024, {150000, 0, 120000});
    c.jobs.push_back(make_job(1, 549 * 1024 - 7, {60000}, 1, kFlagParallel));
    c.index = true;
    c.cursor = 1;
    c.xcursor = true;
    run_case(c, G);
    CHECK_EQ(G.nchunks, 750 + 275);
    // pieces of 90 and ~109 keys: 90 + 4 sqrt(90) + 1 = 129 -> 3 rounds of 64
    CHECK_EQ(G.ckr, 3);
  }
  {  // short pieces: one round
    JobImage G;
    Case c = one_job("cursor kr 1", 4 * 1024, {100, 120});
    c.index = true;
    c.cursor = 1;
    c.part = kSearch;
    c.pack = 0;
    c.xcursor = true;
    run_case(c, G);
    CHECK_EQ(G.ckr, 1);
  }
  {  // not a plan, more than 32 pushes or a stream job: no cursor form
    JobImage G;
    Case c = one_job("cursor off: flush", 4 * 1024, {4000, 4000});
    c.cursor = 1;
    run_case(c, G);
    Case d = one_job("cursor off: stream", 4 * 1024, {4000, 4000});
    d.cursor = 1;
    d.index = true;
    d.part = kStream;
    run_case(d, G);
  }
  {  // packed: 1025 tiles of 2048 slots, chunks index the tile descriptors
    JobImage G;
    Case c = one_job("packed cursor", 600 * 2048, std::vector<uint64_t>(40, 900), 2);
    c.jobs.push_back(make_job(1, 425 * 2048 - 100, std::vector<uint64_t>(3, 500), 2));
    c.index = true;
    c.cursor = 1;
    c.xpack = true;
    c.xwide = true;
    c.xpcursor = true;
    c.tile = 2048;
    run_case(c, G);
    CHECK_EQ(G.nchunks, 300 + 213);
    // a pointer that uses its top 16 bits (the kernel keeps a length there)
    for (int which = 0; which < 2; ++which) {
      Case d = c;
      d.name = "packed cursor off: high pointer";
      if (which) d.jobs[1].pvals[3] = (const void*)((uint64_t)d.jobs[1].pvals[3] | 1ull << 48);
      else d.jobs[0].pkeys[7] = (const uint64_t*)((uint64_t)d.jobs[0].pkeys[7] | 1ull << 63);
      d.xpcursor = false;
      run_case(d, G);
    }
  }
}

static void same_shape() {
  JobImage G;
  auto batch = [](uint64_t gen, uint64_t n1, uint32_t flags) {
    Case c;
    c.name = "same shape";
    c.m = 2;
    c.pack = 0;
    c.jobs.push_back(make_job(0, 70 * 1024, {50000, 0, 60000}, 2, flags, gen));  // search
    c.jobs.push_back(make_job(1, 9 * 1024, {200, n1}, 2, 0, gen));                 // stream
    return c;
  };
  run_case(batch(0, 200, 0), G, false);
  CHECK_EQ(G.h[1].mode, kStream);
  run_case(batch(1, 200, 0), G, true);   // other push pointers only
  run_case(batch(2, 200, 0), G, true);
  run_case(batch(2, 201, 0), G, false);  // a stream job's items follow its pn
  run_case(batch(3, 201, 0), G, true);
  run_case(batch(3, 201, kFlagCont), G, false);
  run_case(batch(3, 201, kFlagCont), G, true);
  {  // a search job's pn is not in its descriptors
    Case c = batch(4, 201, kFlagCont);
    c.jobs[0].pn[0] = 50001;
    run_case(c, G, true);
  }
  {  // another image address
    Case c = batch(4, 201, kFlagCont);
    g_case = c.name;
    CHECK_EQ(G.plan(c.jobs.data(), c.jobs.size(), c.dtype, c.m, false), PSG_OK);
    G.layout(c.jobs.data(), 128);
    CHECK(!G.same_shape(c.jobs.data(), kBase + 4096));
    CHECK(G.same_shape(c.jobs.data(), kBase));
  }
  // plans and cursor forms are never the same shape
  Case p = batch(0, 200, 0);
  p.index = true;
  run_case(p, G, false);
  run_case(p, G, false);
  JobImage H;
  Case c = one_job("cursor never same", 4 * 1024, {4000, 4000});
  c.index = true;
  c.cursor = 1;
  c.xcursor = true;
  run_case(c, H, false);
  run_case(c, H, false);
}

// The splitter items have a 2^31 limit too, but a job adds at most
// (its tiles + its pushes) / 256 + 2 of them, and at least one item per
// push: the tile, item or job limit is always passed first, so no input
// reaches it.
static void limits() {
  g_case = "limits";
  JobImage G;
  JobSpec one = make_job(0, 1024, {10}, 1);
  CHECK_EQ(G.plan(&one, 1, PSG_F32, 1, false), PSG_OK);
  {  // more than kMaxPush pushes (empty ones count)
    JobSpec s = make_job(0, 1024, std::vector<uint64_t>(4096, 0), 1);
    CHECK_EQ(G.plan(&s, 1, PSG_F32, 1, false), PSG_OK);
    s = make_job(0, 1024, std::vector<uint64_t>(4097, 0), 1);
    CHECK_EQ(G.plan(&s, 1, PSG_F32, 1, false), PSG_ERR_ARG);
  }
  {  // a push of 2^32 keys
    JobSpec s = make_job(0, 1024, {(1ull << 32) - 1}, 1);
    CHECK_EQ(G.plan(&s, 1, PSG_F32, 1, false), PSG_OK);
    s = make_job(0, 1024, {1ull << 32}, 1);
    CHECK_EQ(G.plan(&s, 1, PSG_F32, 1, false), PSG_ERR_ARG);
  }
  {  // 2^31 tiles, in one job and summed over two
    JobSpec s = make_job(0, ((1ull << 31) - 1) * 1024, {1ull << 31}, 1);
    G.knob_pack = 0;
    CHECK_EQ(G.plan(&s, 1, PSG_F32, 1, false), PSG_OK);
    CHECK_EQ(G.ntiles, (1ull << 31) - 1);
    s.nslots += 1;
    CHECK_EQ(G.plan(&s, 1, PSG_F32, 1, false), PSG_ERR_ARG);
    std::vector<JobSpec> two = {make_job(0, (1ull << 30) * 1024, {1ull << 31}, 1),
                                make_job(1, (1ull << 30) * 1024, {1ull << 31}, 1)};
    CHECK_EQ(G.plan(two.data(), 2, PSG_F32, 1, false), PSG_ERR_ARG);
  }
  {  // 2^31 items: 2^25 groups of 64 boundaries x 64 pushes
    JobSpec s = make_job(0, ((1ull << 31) - 64) * 1024, std::vector<uint64_t>(64, 1ull << 31), 1);
    G.knob_wide = 0;
    G.knob_part = kSearch;
    CHECK_EQ(G.plan(&s, 1, PSG_F32, 1, false), PSG_ERR_ARG);
    s = make_job(0, ((1ull << 31) - 64) * 1024, std::vector<uint64_t>(63, 1ull << 31), 1);
    CHECK_EQ(G.plan(&s, 1, PSG_F32, 1, false), PSG_OK);
  }
  // more than 2^27 jobs (an item holds the job in 27 bits): refused by the
  // count alone, before a job is read
  CHECK_EQ(G.plan(&one, (1ull << 27) + 1, PSG_F32, 1, false), PSG_ERR_ARG);
  CHECK(!g_err.empty());
}

int main() {
  tile_edges();
  tile_size();
  empty_pushes();
  search_items();
  stream_mode();
  splitter_items();
  dense_job();
  cursor_forms();
  same_shape();
  limits();
  if (g_bad) {
    printf("test_jobimage: %d check(s) failed\n", g_bad);
    return 1;
  }
  printf("test_jobimage ok\n");
  return 0;
}
