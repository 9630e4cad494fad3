// psg_jobimage.cc -- see psg_jobimage.h.  Host code only.
#include "psg_jobimage.h"

#include <algorithm>
#include <cmath>
#include <cstring>

#include "psg_host.h"

namespace psg {
namespace {

// Mean piece length (keys per push per tile) below which a job's partition
// streams the push keys instead of searching every tile boundary
// (DESIGN.md 4.1): a bracketed boundary search reads ~3.5 random lines
// (~450 B), the stream 8 B per key, but the stream's chunks wait on more
// dependent round trips; measured on cfg3 (29.7 keys per piece) the search
// is 8 % faster, so the switch sits below it.
constexpr double kStreamBelow = 24.0;
// Mean piece length below which the aggregate kernel packs several pushes'
// pieces into one 64-lane round; above it rounds are
// push-uniform, which is faster while most rounds are full anyway.
constexpr double kPackBelow = 16.0;

// Kernel-form overrides come from explicit flags (psg.h PSG_FORM_*,
// PSG_PART_*, PSG_GROUP*, PSG_NO_DENSE, PSG_NO_ZERO_COPY), never from the
// environment: tests and A/B measurements pass them to psg_plan_create /
// psg_create; results are bit-identical either way.

// The work items of a job's partition (launch_partition): a search item
// covers 64 tile boundaries of one push, a stream item kStreamChunk keys of
// one push, a splitter item 256 splitters (or fail counters) of the job.
uint64_t search_groups(uint64_t nt) { return (nt + 64) / 64; }
uint64_t stream_chunks(uint64_t n) { return (n + kStreamChunk - 1) / kStreamChunk; }
uint64_t split_blocks(uint64_t nt, uint64_t np) { return (std::max(nt + 1, np) + 255) / 256; }

}  // namespace

int JobImage::plan(const JobSpec* jobs, size_t njobs, int dt, int mm, bool idx) {
  if (njobs > (1ull << 27)) return fail(PSG_ERR_ARG, "too many jobs");
  dtype = dt;
  m = mm;
  index = idx;
  const int forced = knob_part;
  h.assign(njobs, JobDev{});
  info.assign(njobs, JobInfo{});
  uint64_t tiles = 0, items = 0, sitems = 0;
  dense = njobs != 0;
  for (size_t j = 0; j < njobs; ++j) dense = dense && jobs[j].dense;
  // the round form first (mean keys per push per 1024-slot tile) and the
  // push-group size: they fix the tile size, 2048 slots for the packed
  // kernel and for the tile kernel's 64-push form
  {
    const uint64_t t1 = kTileSlots;
    double kv_all = 0, pieces_all = 0;
    uint32_t maxnp = 0;
    for (size_t j = 0; j < njobs; ++j) {
      const JobSpec& s = jobs[j];
      uint32_t np = 0;
      for (uint64_t n : s.pn) {
        kv_all += (double)n;
        np += n != 0;
      }
      maxnp = std::max(maxnp, np);
      pieces_all += (double)np * (double)((s.nslots + t1 - 1) / t1);
    }
    pack = knob_pack >= 0 ? knob_pack == 1 : (pieces_all > 0 && kv_all / pieces_all < kPackBelow);
    wide = knob_wide >= 0 ? knob_wide == 1 : maxnp > 32;
  }
  tile = dense ? kTileSlots : pack ? kPackTileSlots : wide ? kWideSlots : kTileSlots;
  all_search = true;
  for (size_t j = 0; j < njobs; ++j) {
    const JobSpec& s = jobs[j];
    JobInfo& I = info[j];
    I.ncaller = (uint32_t)s.pn.size();
    if (s.pn.size() > (size_t)kMaxPush)
      return fail(PSG_ERR_ARG, "job %zu: %zu pushes > max %d", j, s.pn.size(), kMaxPush);
    uint64_t kv = 0;
    for (size_t p = 0; p < s.pn.size(); ++p) {
      if (s.pn[p] >= (1ull << 32))
        return fail(PSG_ERR_ARG, "push of %llu keys >= 2^32", (unsigned long long)s.pn[p]);
      // an empty push is ignored (kv_vector.h:90,177): the first NON-empty
      // push is the one that assigns
      if (s.pn[p] == 0) continue;
      I.pn.push_back(s.pn[p]);
      I.slot.push_back((uint32_t)p);
      kv += s.pn[p];
    }
    I.np = (uint32_t)I.pn.size();
    // no server keys: nothing can match (every pushed key is reported unmatched)
    I.ntiles = s.nslots ? (uint32_t)((s.nslots + tile - 1) / tile) : 0u;
    JobDev& d = h[j];
    d.nslots = s.nslots;
    d.npush = I.np;
    d.ntiles = I.ntiles;
    d.tile = tile;
    // keys per push per 1024 slots (the partition modes' calibration unit)
    const uint64_t nt1 = (s.nslots + kTileSlots - 1) / kTileSlots;
    const double piece = I.np && nt1 ? (double)kv / ((double)I.np * nt1) : 1e9;
    d.mode = s.dense ? kSearch
                     : forced >= 0 ? (uint32_t)forced
                                   : (piece < kStreamBelow ? kStream : kSearch);
    all_search = all_search && d.mode == kSearch;
    d.segq = d.mode == kStream ? I.ntiles + 1 : 1u;
    d.segb = d.mode == kStream ? 1u : I.np;
    I.segq = d.segq;
    tiles += I.ntiles;
    // a dense job's seg is filled on the host: nothing to search.  Stream
    // jobs map keys through their splitter array; search-mode jobs of plans
    // read their boundary keys from one too, written once (64 consecutive
    // boundaries: one coalesced read per wave instead of one line of D per
    // boundary)
    const bool work = I.ntiles && I.np && !s.dense;
    I.has_split = d.mode == kStream || (index && work);
    uint64_t ni = 0, ns = 0;
    if (work) {
      if (d.mode == kSearch) ni = search_groups(I.ntiles) * I.np;
      else for (uint64_t n : I.pn) ni += stream_chunks(n);
      if (I.has_split) ns = split_blocks(I.ntiles, I.np);
    }
    if (ns) d.split_begin = (uint32_t)sitems;
    items += ni;
    sitems += ns;
    if (tiles >= (1ull << 31) || items >= (1ull << 31) || sitems >= (1ull << 31))
      return fail(PSG_ERR_ARG, "batch too large (%llu tiles)", (unsigned long long)tiles);
    I.nitems = (uint32_t)ni;
    I.nsplit = (uint32_t)ns;
  }
  ntiles = (uint32_t)tiles;
  nitems = (uint32_t)items;
  nsplit = (uint32_t)sitems;
  // the cursor form: plans (resident index) of search-mode jobs of at most
  // kCursorPushes pushes; kr = the rounds of 64 keys loaded per push per
  // tile (mean + 4 sigma keys, at most 3: longer pieces finish round by
  // round in the fold step).  Opt-in only (PSG_FORM_CURSOR), with no size
  // gate: measured slower than partition + tile kernel on cfg2 (0.509 vs
  // 0.437 ms per step)
  cursor = index && !dense && !pack && !wide && knob_cursor == 1 && tiles > 0;
  for (size_t j = 0; cursor && j < njobs; ++j) {
    JobInfo& I = info[j];
    if (jobs[j].dense || h[j].mode != kSearch || I.np > (uint32_t)kCursorPushes) {
      cursor = false;
      break;
    }
    double kv = 0;
    for (uint64_t n : I.pn) kv += (double)n;
    const double piece = I.np && I.ntiles ? kv / ((double)I.np * I.ntiles) : 0.0;
    const double need = piece + 4.0 * std::sqrt(piece) + 1.0;
    I.kr = (uint32_t)std::min(3.0, std::max(1.0, std::ceil(need / 64.0)));
  }
  if (cursor) {  // one kernel instance: the jobs' largest round count
    ckr = 1;
    for (const JobInfo& I : info) ckr = std::max(ckr, I.kr);
    for (JobInfo& I : info) I.kr = ckr;
  }
  // the packed cursor form: plans (resident index) of packed-round jobs of
  // at most 256 pushes whose pointers leave the top 16 bits free (the
  // kernel keeps a piece's length there); tiles whose elements overflow one
  // pass take more groups.  Opt-in only (PSG_FORM_CURSOR), with no size
  // gate: measured slower than partition + packed kernel on cfg5 (1.34 vs
  // 0.77 ms per step)
  pcursor = index && !dense && pack && knob_cursor == 1 && tiles > 0;
  for (size_t j = 0; pcursor && j < njobs; ++j) {
    const JobSpec& s = jobs[j];
    if (s.dense || info[j].np > (uint32_t)kPackCursorPushes) {
      pcursor = false;
      break;
    }
    for (size_t p = 0; p < s.pkeys.size(); ++p) {
      bool hi = ((uint64_t)s.pkeys[p] >> 48) != 0;
      for (int i = 0; i < m; ++i) hi |= ((uint64_t)s.pvals[p * m + i] >> 48) != 0;
      if (hi) pcursor = false;
    }
  }
  bxs = pcursor ? (uint32_t)kPackCursorPushes : 32u;
  nchunks = 0;
  if (cursor || pcursor) {
    // about one chunk per workgroup slot of the chip (256 CUs x 8
    // workgroups of the cursor kernel, x 4 of the packed one)
    const uint64_t kChunkTarget = cursor ? 2048 : 1024;
    const uint64_t per = std::max<uint64_t>(1, (tiles + kChunkTarget - 1) / kChunkTarget);
    for (JobInfo& I : info) {
      I.nch = (uint32_t)((I.ntiles + per - 1) / per);
      I.ch0 = nchunks;
      nchunks += I.nch;
    }
  }
  return PSG_OK;
}

void JobImage::layout(const JobSpec* jobs, uint32_t iw) {
  JobLayout& L = lay;
  const size_t njobs = h.size();
  const bool chunked = cursor || pcursor;
  L.iw = iw;
  size_t off = align_up(sizeof(JobDev) * njobs, 256);
  L.tiles = off;
  off = align_up(off + sizeof(TileDesc) * ntiles, 256);
  // one bucket per slot in every kernel (the same bucket map): the index
  // depends only on D and the tile size
  L.index = off;
  if (use_index()) off = align_up(off + 4 * (size_t)iw * ntiles, 256);
  L.marked = off;
  if (use_index()) off += 256;
  L.sitems = off;
  off = align_up(off + 4 * (size_t)nsplit, 256);
  L.items = off;
  off = align_up(off + 8 * (size_t)nitems, 256);
  L.cjobs = off;
  if (cursor) off = align_up(off + sizeof(CursorJob) * njobs, 256);
  L.chunks = off;
  if (chunked) off = align_up(off + sizeof(CursorChunk) * nchunks, 256);
  L.zero = off;
  size_t fail_cur = off;
  uint64_t npall = 0;
  for (const JobInfo& I : info) npall += I.np;
  off = align_up(off + 8 * npall, 256);
  L.bx = off;
  if (chunked) off = align_up(off + 4 * (size_t)bxs * ((size_t)nchunks + 1), 256);
  L.zero_end = off;
  L.job.resize(njobs);
  for (size_t j = 0; j < njobs; ++j) {
    const size_t np = info[j].np, nt = info[j].ntiles;
    JobLayout::Job& o = L.job[j];
    o.pk = off; off = align_up(off + 8 * np, 64);
    o.pv = off; off = align_up(off + 8 * np * m, 64);
    o.pn = off; off = align_up(off + 8 * np, 64);
    o.out = off; off = align_up(off + 8 * m, 64);
    o.fail = fail_cur; fail_cur += 8 * np;
    o.seg = off; off = align_up(off + 4 * (nt + 1) * np, 256);
    o.split = off;
    if (info[j].has_split) off = align_up(off + 8 * (nt + 1), 256);
    o.dpos = off;
    if (jobs[j].dense) off = align_up(off + 8 * np, 256);
  }
  L.hstate = off;
  if (hints) off = align_up(off + 4 * (size_t)nitems, 256);
  L.total = off;
}

// everything the tile descriptors and work items depend on (their pointers
// into the image follow from the offsets)
bool JobImage::same_shape(const JobSpec* jobs, const void* base) {
  shape.clear();
  if (index || cursor || pcursor) return false;
  const JobLayout& L = lay;
  shape.insert(shape.end(), {(uint64_t)h.size(), tile, (uint64_t)m, (uint64_t)dtype,
                             (uint64_t)pack, (uint64_t)wide, (uint64_t)(uintptr_t)base, L.total,
                             L.tiles, L.zero, nitems, nsplit, ntiles});
  for (size_t j = 0; j < h.size(); ++j) {
    const JobSpec& s = jobs[j];
    const JobDev& d = h[j];
    const JobLayout::Job& o = L.job[j];
    shape.insert(shape.end(), {(uint64_t)info[j].np, s.nslots, (uint64_t)(uintptr_t)s.keys,
                               (uint64_t)s.flags, (uint64_t)s.dense, (uint64_t)d.mode,
                               (uint64_t)d.segq, (uint64_t)d.segb, o.pk, o.pv, o.pn, o.out,
                               o.fail, o.seg, o.split, o.dpos});
    if (d.mode == kStream) shape.insert(shape.end(), info[j].pn.begin(), info[j].pn.end());
  }
  return shape == last_shape;
}

void JobImage::keep_shape() {
  last_shape.swap(shape);  // empty for a build that is not cacheable
  shape.clear();
}

int JobImage::fill(const JobSpec* jobs, char* img, const void* dev, bool same) {
  const JobLayout& L = lay;
  char* base = (char*)dev;
  const size_t njobs = h.size();
  // only the region the kernels expect zeroed (fail counters, cursor
  // boundary words): every other field of the image is written below, or
  // (seg, splitters, bucket index) by a kernel before any read -- but for
  // the seg of a hinted plan's search-mode jobs, which the first run reads
  // as the cuts to try (zeroed per job below, once per plan).  Zeroing
  // the whole image cost ~0.1 ms per flush of a 16.8 M-slot aggregate
  if (L.zero_end > L.zero) memset(img + L.zero, 0, L.zero_end - L.zero);
  if (use_index()) memset(img + L.marked, 0, 8);
  if (hints)
    for (uint32_t i = 0; i < nitems; ++i) ((uint32_t*)(img + L.hstate))[i] = kHintFresh;
  TileDesc* htiles = (TileDesc*)(img + L.tiles);
  uint32_t* hsitems = (uint32_t*)(img + L.sitems);
  uint64_t* hitems = (uint64_t*)(img + L.items);
  const uint32_t* bt = use_index() ? (const uint32_t*)(base + L.index) : nullptr;
  uint64_t tcur = 0, icur = 0, scur = 0;
  for (size_t j = 0; j < njobs; ++j) {
    const JobSpec& s = jobs[j];
    JobInfo& I = info[j];
    const JobLayout::Job& o = L.job[j];
    const uint32_t np = I.np, nt = I.ntiles;
    uint64_t* hk = (uint64_t*)(img + o.pk);
    uint64_t* hv = (uint64_t*)(img + o.pv);
    for (uint32_t p = 0; p < np; ++p) {
      const uint32_t c = I.slot[p];
      hk[p] = (uint64_t)s.pkeys[c];
      for (int i = 0; i < m; ++i) hv[(size_t)p * m + i] = (uint64_t)s.pvals[(size_t)c * m + i];
    }
    if (np) memcpy(img + o.pn, I.pn.data(), 8 * np);
    if (s.dense) {
      // seg(p, t) = clamp(t * tile - dpos[p], 0, n_p), tile-major (segq 1, segb np)
      uint64_t* hd = (uint64_t*)(img + o.dpos);
      uint32_t* hs = (uint32_t*)(img + o.seg);
      for (uint32_t p = 0; p < np; ++p) {
        const uint64_t dp = s.dpos[I.slot[p]], n = I.pn[p];
        hd[p] = dp;
        for (uint32_t t = 0; t <= nt; ++t) {
          const uint64_t edge = (uint64_t)t * tile;
          const uint64_t v = edge <= dp ? 0 : std::min<uint64_t>(edge - dp, n);
          hs[(size_t)t * np + p] = (uint32_t)v;
        }
      }
    }
    memcpy(img + o.out, s.out.data(), 8 * m);
    JobDev& d = h[j];
    if (hints && nt && !s.dense && d.mode == kSearch)
      memset(img + o.seg, 0, 4 * ((size_t)nt + 1) * np);
    d.dkeys = s.keys;
    d.pkeys = (const uint64_t* const*)(base + o.pk);
    d.pn = (const uint64_t*)(base + o.pn);
    d.seg = (uint32_t*)(base + o.seg);
    d.fail = (unsigned long long*)(base + o.fail);
    d.split = I.has_split ? (uint64_t*)(base + o.split) : nullptr;
    I.seg = d.seg;
    I.fail = d.fail;
    if (same) continue;  // descriptors and items already on the device
    for (uint32_t b = 0; b < I.nsplit; ++b) hsitems[scur++] = (uint32_t)j;
    if (I.nitems && d.mode == kSearch) {
      const uint64_t ng = search_groups(nt);
      for (uint64_t g = 0; g < ng; ++g)  // group-major: a boundary group's pushes adjacent
        for (uint32_t p = 0; p < np; ++p)
          hitems[icur++] = (uint64_t)j << 37 | (uint64_t)p << 24 | g;
    } else if (I.nitems) {
      for (uint32_t p = 0; p < np; ++p) {
        const uint64_t nc = stream_chunks(I.pn[p]);
        for (uint64_t c = 0; c < nc; ++c)
          hitems[icur++] = (uint64_t)j << 37 | (uint64_t)p << 24 | c;
      }
    }
    for (uint32_t t = 0; t < nt; ++t) {
      TileDesc& T = htiles[tcur];
      const uint64_t slot0 = (uint64_t)t * tile;
      T.dk = s.keys + slot0;
      T.seg = d.seg + (size_t)t * d.segb;
      T.pkeys = d.pkeys;
      T.pvals = (const void* const*)(base + o.pv);
      T.pn = d.pn;
      T.out = (void* const*)(base + o.out);
      T.fail = d.fail;
      T.slot0 = slot0;
      T.nt = (uint32_t)std::min<uint64_t>(tile, s.nslots - slot0);
      T.np = np;
      T.stride = d.segq;
      T.segb = d.segb;
      T.flags = s.flags | (t + 1 == nt ? kFlagLastTile : 0u);
      T.dpos = s.dense ? (const uint64_t*)(base + o.dpos) : nullptr;
      T.bt = bt ? bt + (size_t)tcur * L.iw : nullptr;
      ++tcur;
    }
  }
  // the counts are the plan's own, so the regions (packed back to back)
  // cannot overflow: a mismatch is a bug, never launched
  if (!same && (icur != nitems || scur != nsplit || tcur != ntiles))
    return fail(PSG_ERR_DEVICE, "job table: %llu/%u items, %llu/%u split items, %llu/%u tiles",
                (unsigned long long)icur, nitems, (unsigned long long)scur, nsplit,
                (unsigned long long)tcur, ntiles);
  if (cursor || pcursor) {
    CursorJob* hcj = (CursorJob*)(img + L.cjobs);
    CursorChunk* hch = (CursorChunk*)(img + L.chunks);
    uint64_t tbase = 0;
    for (size_t j = 0; j < njobs; ++j) {
      const JobInfo& I = info[j];
      const JobDev& d = h[j];
      if (cursor) {
        CursorJob& c = hcj[j];
        c.dkeys = jobs[j].keys;
        c.nslots = jobs[j].nslots;
        c.pkeys = d.pkeys;
        c.pvals = (const void* const*)(base + L.job[j].pv);
        c.pn = d.pn;
        c.out = (void* const*)(base + L.job[j].out);
        c.fail = d.fail;
        c.seg = d.seg;
        c.bt = bt + (size_t)tbase * L.iw;
        c.np = I.np;
        c.ntiles = I.ntiles;
        c.flags = jobs[j].flags;
        c.kr = I.kr;
      }
      // the cursor kernel's chunks count a job's tiles from 0, the packed
      // kernel's index the tile descriptors
      const uint64_t t0 = cursor ? 0 : tbase;
      for (uint32_t k = 0; k < I.nch; ++k) {
        CursorChunk& ch = hch[I.ch0 + k];
        ch.job = (uint32_t)j;
        ch.t0 = (uint32_t)(t0 + (uint64_t)k * I.ntiles / I.nch);
        ch.t1 = (uint32_t)(t0 + (uint64_t)(k + 1) * I.ntiles / I.nch);
      }
      tbase += I.ntiles;
    }
  }
  if (njobs) memcpy(img, h.data(), sizeof(JobDev) * njobs);
  return PSG_OK;
}

}  // namespace psg
