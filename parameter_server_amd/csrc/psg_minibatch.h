// psg_minibatch.h -- the minibatch handle of psg_worker.hip, shared with
// psg_text.hip, which fills its CSR blocks from text, and the two halves of a
// load that both loads go through.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <vector>

#include "../../include/psg.h"
#include "psg_blocks.h"

enum BufId {
  B_OFFSET, B_INDEX, B_VALUE, B_Y, B_KEY_A, B_KEY_B, B_POS_A, B_POS_B, B_COUNTS, B_TILE_SUM,
  B_UNIQ_KEY, B_KEY_CNT, B_RUN_START, B_RUN_OF, B_ROW_OF, B_RUN_RANK, B_REMAPPED, B_BEFORE,
  B_NEW_OFFSET, B_NEW_INDEX, B_NEW_VALUE, B_DICT_RUN, B_CNT_POS, B_CNT_NEG, B_XW, B_TAU, B_C,
  B_LOSS, B_PARTIAL, B_GRAD, B_TERM, B_LONG_LIST, B_SCRATCH0, B_SCRATCH1, B_SCRATCH2, B_SCRATCH3,
  // (g): the Darling worker's state, its second term array and the rows' lists
  B_DUAL, B_CUR_W, B_DELTA, B_ACTIVE, B_DELTA_W, B_EXP_DELTA, B_TERM2, B_RKEY_A, B_RKEY_B,
  B_RPOS_A, B_RPOS_B, B_ROW_START, B_COL_RANGE,
  // psg_text.hip: the text, the chunks' counts and bases, the lanes' counts,
  // the lines' ends, the slow tokens and their patches, the control words
  B_TEXT, B_TX_CHUNK, B_TX_LANE, B_TX_LINE_END, B_TX_SLOW, B_TX_PATCH, B_TX_WORDS,
  // psg_groups.hip: the entries' slot ids; two control words and the slots' statistics
  B_SLOT, B_GRP,
  // psg_cache.hip: a raw cache array (pack) or the files' bytes (load); the
  // streams (pack) or the staged rowsiz / value / label (load); the
  // partitions' tables and the verdicts; the compressor's or decoder's scratch
  B_CA_RAW, B_CA_OUT, B_CA_TAB, B_CA_SCR,
  B_COUNT
};

// device words: [0] OR of the keys, [1] AND, [2] dictionary order violations,
// [3] objv, [4] as two u32: n_uniq, survivors, [5] as u32: long runs; then
// the 256 digit totals
constexpr size_t kSmallBytes = 6 * 8 + 256 * 4;

enum State { S_NEW = 0, S_LOADED, S_UNIQ, S_LOCAL, S_GRAD };

struct psg_minibatch : psg::DeviceBlocks<B_COUNT> {
  int state = S_NEW;
  size_t rows = 0, nnz = 0, n_uniq = 0, ndict = 0;
  bool binary = false;
  uint64_t differ = 0;  // the key bits that differ between some two keys
  const uint64_t* skey = nullptr;  // the sorted pairs (one side of the ping-pong)
  const uint32_t* spos = nullptr;
  // (g): set by psg_mb_darling_init, cleared by psg_mb_load and psg_mb_localize
  bool darling = false;
  bool xw_own = false;  // psg_mb_times has run into the minibatch's own Xw (psg_mb_labels)
  const uint32_t* row_pair = nullptr;  // the rows' lists (one side of their ping-pong)
  // host: pair_lo[k] = the first sorted pair of the first of keys k, k + 1, ...
  // that has a run (nnz: none); pair_hi[k] = the end of the last run among
  // keys 0 .. k - 1 (0: none).  Block [cb, ce) is pairs [pair_lo[cb], pair_hi[ce]).
  std::vector<uint32_t> pair_lo, pair_hi;
  size_t n_long = 0;  // the length of the long-run list, read at psg_mb_darling_init
  size_t last_cb = 0, last_ce = 0;  // the columns of the last psg_mb_darling_update_dual
  size_t scratch_len[4] = {0, 0, 0, 0};
  // psg_mb_profile: a pair of timing events around each stage's launches;
  // the last pair is psg_mb_load_text's
  bool prof = false;
  hipEvent_t tev[2 * PSG_MB_STAGES + 2] = {};
  bool tset[2 * PSG_MB_STAGES + 2] = {};
  void tick(int stage, int end, hipStream_t s) {
    const int i = 2 * stage + end;
    if (prof && tev[i] && hipEventRecord(tev[i], s) == hipSuccess) tset[i] = true;
  }
  // psg_text.hip: pinned words the sizes and the verdict are read into, and a
  // pinned stage for the slow tokens and their patches
  uint32_t* h_text = nullptr;
  void* h_slow = nullptr;
  size_t h_slow_cap = 0;

  // psg_groups.hip: psg_mb_set_slots has run since the load, with the bits in
  // which its ids differ; psg_mb_groups has run and found no bad row, with
  // every slot's segment of the sorted pairs (ascending id)
  bool has_slots = false;
  uint64_t slot_differ = 0;
  bool groups_ok = false;
  struct Group {
    uint32_t id, start, end;
  };
  std::vector<Group> groups;
  // psg_mb_darling_share_dual: whose dual block this minibatch's Darling calls
  // use (null: its own), and who uses this one's
  psg_minibatch* dual_owner = nullptr;
  std::vector<psg_minibatch*> sharers;
  double* dual() const { return (dual_owner ? dual_owner : this)->at<double>(B_DUAL); }

  uint32_t* d_u32(int word) const { return (uint32_t*)(d_small + 4) + word; }
  uint32_t* d_dtotal() const { return (uint32_t*)(d_small + 6); }
};

namespace psg {
// The first half of a load, after the caller's own checks: waits for the
// previous minibatch's work, drops its state and sizes every block of a
// minibatch of `rows` rows and `nnz` entries.
int mb_load_begin(psg_minibatch* mb, size_t rows, size_t nnz, bool valued);
// The second half, with offset / index / value / y in their blocks (or being
// written there by work enqueued on the minibatch's stream): the row of every
// position, the OR / AND of the keys, one wait, and the state S_LOADED.
int mb_load_finish(psg_minibatch* mb, size_t rows, size_t nnz, bool valued);
// mb's dual block is about to go (a load, its destruction): its sharers lose
// their Darling state, and mb stops sharing another's
void mb_drop_sharing(psg_minibatch* mb);
}  // namespace psg
