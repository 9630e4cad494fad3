// psg_nway_plan.h -- the N-way merge's planner (psg_nway.hip): the shape of
// each merge of a batch -- sample stride, bucket width, candidates, buckets,
// tiles -- and the batch's choices that follow from the shapes: the rank
// kernel's form and the ticket order of the tile stage.  Host arithmetic on
// the pushes' lengths only (no HIP call: psg_nway_shape reads it out with no
// device); NwLayout (psg_nway.hip) lays the device scratch out from it.
#pragma once

#include <stdint.h>

#include <algorithm>
#include <vector>

namespace psg {

constexpr int kNwThreads = 256;                  // threads per tile workgroup
constexpr int kNwPer = 8;                        // merged elements per thread
constexpr int kNwCap = kNwThreads * kNwPer;      // elements per tile (LDS)
constexpr int kNwMaxRuns = 64;                   // pushes per merge (runs per tile)

// One merge's shape: sample stride s and bucket width C' (psg_nway.hip's
// header: a tile holds <= C' + 2 K s - K elements), candidates, buckets,
// tiles.
struct NwShape {
  uint32_t K = 0, s = 1, cw = 1, B = 1, T = 2;
  uint64_t ncand = 0;
  uint64_t ntot = 0;  // keys over the merge's pushes: what its outputs hold
  std::vector<uint64_t> cbase;
  void plan(uint32_t k, const uint64_t* pn) {
    K = k;
    ntot = 0;
    for (uint32_t q = 0; q < K; ++q) ntot += pn[q];
    s = std::max<uint32_t>(1, kNwCap / (8 * std::max<uint32_t>(K, 1)));
    cw = kNwCap - 2 * K * s;
    cbase.assign(K + 1, 0);
    for (uint32_t q = 0; q < K; ++q) cbase[q + 1] = cbase[q] + pn[q] / s;
    ncand = cbase[K];
    B = (uint32_t)(ntot / cw + 1);
    T = B + 1;
    if (K == 0) B = T = 0;  // no pushes: no work, the merged count stays 0
  }
  // rank workgroups at `per` candidates per thread
  uint64_t waves(uint32_t per) const { return (ncand + 256u * per - 1) / (256u * per); }
};

#ifndef PSG_NW_RR
#define PSG_NW_RR 1
#endif

// A batch's shapes and what the stages' launches are sized by.
struct NwPlan {
  uint32_t nm = 0;
  std::vector<NwShape> sh;
  uint64_t nwaves = 0, ncand = 0, nseg = 0, ntiles = 0;
  uint64_t maxT = 0;  // the most tiles of one merge (round-robin tickets: maxT * nm)
  uint32_t rk_per = 16;  // rank-stage candidates per thread (16, 4 or 1)

  // pn: the merges' push lengths back to back, npush[j] per merge (empty
  // pushes already dropped: nway_keep)
  void plan_shapes(uint32_t nmerge, const uint32_t* npush, const uint64_t* pn) {
    nm = nmerge;
    sh.assign(nm, NwShape{});
    size_t pcur = 0;
    for (uint32_t j = 0; j < nm; ++j) {
      sh[j].plan(npush[j], pn + pcur);
      pcur += npush[j];
    }
    nwaves = ncand = nseg = ntiles = maxT = 0;
    // the fewest candidates per thread that still gives >= 512 rank workgroups
    uint64_t w16 = 0, w4 = 0;
    for (const NwShape& x : sh) {
      w16 += x.waves(16);
      w4 += x.waves(4);
    }
    rk_per = w16 >= 512 ? 16u : (w4 >= 512 ? 4u : 1u);
    for (const NwShape& x : sh) {
      nwaves += x.waves(rk_per);
      ncand += x.ncand;
      nseg += (uint64_t)(x.T + 1) * x.K;
      ntiles += x.T;
      maxT = std::max<uint64_t>(maxT, x.T);
    }
  }
  // round-robin tickets run maxT * nm workgroups: only where that stays
  // within a small factor of the tiles (a skewed batch -- one large merge and
  // many one-tile merges -- would launch mostly idle workgroups)
  bool rr() const { return PSG_NW_RR && nm > 1 && maxT * nm <= 2 * ntiles; }
  uint64_t tickets() const { return rr() ? maxT * nm : ntiles; }
};

// Empty pushes are ignored (kv_vector.h:90,177): push 0 of a merge is its
// first non-empty one.  kept[j] = merge j's non-empty pushes, idx = their
// positions in the caller's back-to-back list, in order.
inline void nway_keep(int nmerge, const int* npush, const uint64_t* n,
                      std::vector<uint32_t>& kept, std::vector<size_t>& idx) {
  kept.assign((size_t)nmerge, 0);
  idx.clear();
  size_t p = 0;
  for (int j = 0; j < nmerge; ++j)
    for (int e = 0; e < npush[j]; ++e, ++p)
      if (n[p] != 0) {
        idx.push_back(p);
        ++kept[j];
      }
}

}  // namespace psg
