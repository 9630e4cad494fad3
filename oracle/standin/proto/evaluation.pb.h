// TEST INFRASTRUCTURE ONLY.  Stand-in for the protobuf-generated AUCData
// (four repeated fields with their accessors), written for
// oracle/ref_auc_shim.cc from what the reference's base/auc.h calls.  It also
// brings in <map>, which the reference's util/common.h supplies and the
// stand-in one does not.  It holds no arithmetic or control flow of a pinned
// function.
#pragma once
#include <map>

#include "util/common.h"

namespace PS {
struct AUCData {
  std::vector<int64> tp_key_, fp_key_;
  std::vector<uint64> tp_count_, fp_count_;

  int tp_key_size() const { return (int)tp_key_.size(); }
  int tp_count_size() const { return (int)tp_count_.size(); }
  int fp_key_size() const { return (int)fp_key_.size(); }
  int fp_count_size() const { return (int)fp_count_.size(); }
  int64 tp_key(int i) const { return tp_key_[i]; }
  uint64 tp_count(int i) const { return tp_count_[i]; }
  int64 fp_key(int i) const { return fp_key_[i]; }
  uint64 fp_count(int i) const { return fp_count_[i]; }
  void add_tp_key(int64 v) { tp_key_.push_back(v); }
  void add_tp_count(uint64 v) { tp_count_.push_back(v); }
  void add_fp_key(int64 v) { fp_key_.push_back(v); }
  void add_fp_count(uint64 v) { fp_count_.push_back(v); }
  void clear_tp_key() { tp_key_.clear(); }
  void clear_tp_count() { tp_count_.clear(); }
  void clear_fp_key() { fp_key_.clear(); }
  void clear_fp_count() { fp_count_.clear(); }
};
}  // namespace PS
