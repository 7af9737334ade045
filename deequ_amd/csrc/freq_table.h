// freq_table.h -- the frequency table of the hash group-by (freq.hip has the overview), shared by
// the translation units that work on one.  Internal: nothing here is part of the C ABI.
//   freq_device.h      the group-by's constants and the device helpers more than one unit uses
//                      (wave / block sums and scans, the 128-bit fixed-point sums, entropy_term);
//                      it knows nothing of the table
//   freq_table.h       record / group layouts, the table (dq::freq_table, which the C ABI's opaque
//                      dq_freq is), the small host helpers and the prototypes of the host functions
//                      that cross files
//   freq.hip           phases A, B and C, the table's C ABI and the consumers of a finalized table
//   freq_mi.hip        marginals and MutualInformation
//   key_partition.hip  the raw-key repartition (it uses only the codec and the device helpers)
#pragma once
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <array>
#include <map>
#include <mutex>
#include <vector>

#include "freq_device.h"
#include "kernels.h"
#include "stream_load.h"

namespace dq {

// C_MAXCNT: an upper bound of the count any phase-A record carries (packed phase-C slots at
// fewer than kMaxSubBits sub-bits need every record count below 2^(s-3); merges add the bounds)
// C_NAN_FOLDED: keyed rows of a Histogram-mode floating-point table whose NaN payload was folded
// into the canonical NaN (zero: the table's groups are also the grouping's, dq_freq_folded_nan_rows)
enum Counter { C_NULL_ROWS = 0, C_NULL_GROUP, C_COLLISIONS, C_DBG_NOTREADY, C_DBG_DIFF, C_DBG_FULL, C_DBG_BYPASS,
               C_MAXCNT, C_NAN_FOLDED, C_N };

template <bool HASHED>
struct FM;
template <>
struct FM<false> {
  static constexpr int kTile = 8192;    // rows (and at most records) per phase-A chunk
  static constexpr int kRB = 8;         // bytes per record
  static constexpr int kTableC = 4096;  // phase-C LDS table slots (two workgroups per CU)
  static constexpr int kTarget = 2000;  // records per final partition the sizing aims at
  // records per partition of a table one level shallower that stays packed (finalize_b)
  static constexpr uint64_t kTargetPk = 3700;
};
template <>
struct FM<true> {
  static constexpr int kTile = 2048;
  static constexpr int kRB = 16;
  static constexpr int kTableC = 2560;
  // (freq_phaseC_h takes up to 4096 records and 3584 groups per partition: ~1900-record partitions
  // halve its per-item costs against ~950, configs[4] 176.3 -> 171.5 ms)
  static constexpr int kTarget = 2400;
};
// records per phase-B unit (whole chunk segments of one bucket): hashed two tiles (~32 records per
// partition run); exact one (8192 records: the whole-unit scatter then stages 64 KB and two
// workgroups share a CU, configs[2] 26.3 -> 25.0 ms)
constexpr int kUnitTilesH = 2, kUnitTilesX = 1;

struct RecIn {  // == dq_freq_record
  uint64_t key;
  uint64_t count;
  uint64_t enc_off;
};

struct Group {  // one materialised group
  uint64_t h;
  uint64_t count;
  uint64_t rep;  // hashed: arena offset of the encoded key
};

struct FEntry {  // phase-C work item of a recount: partition p, hash subset v of 2^f
  uint32_t p, f, v, pad;
};

struct PartTypes {
  int32_t types[kMaxKeys];
  int32_t n_keys;
  int32_t exact;
  uint32_t parts;
  uint32_t pad;
};

// 8-byte page-locked words (the small-key phase A's give-up flag) carved from shared 4 KB blocks
// kept to process exit: a hipHostMalloc + hipHostFree per table cost ~0.1-0.2 ms each at every
// string Histogram job's boundary.
struct PinnedWords {
  std::mutex m;
  std::vector<unsigned long long*> free_words;
};
inline PinnedWords& pinned_words() {
  static PinnedWords* w = new PinnedWords;
  return *w;
}
inline hipError_t pinned_word_get(unsigned long long** out) {
  PinnedWords& w = pinned_words();
  std::lock_guard<std::mutex> lock(w.m);
  if (w.free_words.empty()) {
    void* blk = nullptr;
    hipError_t e = hipHostMalloc(&blk, 4096, hipHostMallocDefault);
    if (e != hipSuccess) return e;
    for (int i = 0; i < 512; ++i) w.free_words.push_back(static_cast<unsigned long long*>(blk) + i);
  }
  *out = w.free_words.back();
  w.free_words.pop_back();
  return hipSuccess;
}
// The caller has synchronized the stream of the last copy into the word (dq_freq_destroy), so
// no copy can still land in it; no device-wide barrier (it would wait for other tables' streams).
inline void pinned_word_put(unsigned long long* p) {
  PinnedWords& w = pinned_words();
  std::lock_guard<std::mutex> lock(w.m);
  w.free_words.push_back(p);
}

// The table.  The C ABI's opaque `dq_freq` (global scope, end of this file) is this struct.
struct freq_table {
  int device = 0;
  int n_keys = 0;
  // key types as the caller declared them, and the physical layout the group-by runs on
  // (freq_phys_type: dates / timestamps as their integers, decimals as their unscaled long or
  // 16-byte string); every kernel sees only `types`
  std::vector<int32_t> logical;
  std::vector<int32_t> types;
  bool relabel = false;  // some logical type differs from its physical one
  DevBuf<int64_t> dec_long[kMaxKeys];  // decimal(p <= 18) keys narrowed to their unscaled long
  DevBuf<int32_t> dec_off;             // decimal(p > 18) keys: offsets 0, 16, 32, ... (shared)
  bool exact = false;
  int mode_null_as_group = -1;  // fixed by the first add
  int tile = 0, rb = 0;
  // the table: bucket-sorted chunk regions (phase A output) + their histograms
  DevBuf<uint8_t> recs;
  DevBuf<uint16_t> hist;
  int64_t n_chunks = 0;
  // exact rows: batch regions written bucket-major (freq_prepass_x), one piece row per phase-A
  // workgroup: piece (r, b) = records [pbase[r] + pstart[r][b], + plen[r][b]) of `recs`
  DevBuf<uint32_t> pstart, plen;
  std::vector<unsigned long long> h_pbase;
  int64_t n_prow = 0;
  int64_t n_empty_chunks = 0;  // chunk rows known empty (bucket-piece batches): finalize skips them
  DevBuf<uint32_t> ph, ptot;  // the pre-pass's per-workgroup bucket counts (scratch)
  DevBuf<unsigned long long> pbase;
  DevBuf<uint8_t> arena;                 // hashed: encoded keys
  DevBuf<unsigned long long> dev_words;  // counters[C_N], then the arena cursor
  DevBuf<unsigned long long> batch_tab;  // freq_phaseA_small's cross-workgroup group table
  uint64_t h_counters[C_N] = {0};
  uint64_t arena_used = 0;
  uint64_t rec_var_base = 0;  // arena offset of the last dq_freq_add_records_device's var bytes
  // a table built from another table's records may read that table's arena in place instead of
  // a copy (MutualInformation's marginals, which die before their joint table): then the keys live
  // here and the table takes no further adds
  const uint8_t* arena_view = nullptr;
  // phase A launches leave the device counters and arena cursor ahead of the host copies: they
  // are read back only when needed (finalize, merge, arena growth), so batches queue back to back
  bool counters_stale = false;
  uint64_t arena_hi = 0;  // upper bound of the arena bytes in use (arena_used at the last read-back
                          // + the worst case of every batch added since)
  int64_t num_rows = 0;
  hipStream_t stream = nullptr;
  // the small-key phase A (freq_phaseA_small): the epoch of its last attempt, and a pinned copy of
  // the epoch it last gave up (copied back asynchronously: a table it gave up on stops trying)
  uint64_t fast_epoch = 0;
  bool fast_off = false;
  // every batch went through freq_phaseA_xp, which counts C_NAN_FOLDED (records, merges and the
  // other phase-A kernels do not)
  bool nan_counted = true;
  struct PinnedWord {
    unsigned long long* p = nullptr;
    hipStream_t last_copy = nullptr;  // the stream of the last copy into *p
    // Before a copy into *p is queued on `st`: a copy still queued on another stream could land
    // after it (and after dq_freq_destroy synced only `st`, recycling the word to another table),
    // so that stream is waited for first.  Same stream: stream order already holds.
    hipError_t before_copy(hipStream_t st) {
      hipError_t e = hipSuccess;
      if (last_copy && last_copy != st) e = hipStreamSynchronize(last_copy);
      last_copy = st;
      return e;
    }
    ~PinnedWord() {
      if (p) pinned_word_put(p);
    }
  } fast_seen;
  // the dense integer path (freq_dense_count / _emit): its device words (AArgs::dense_words), the
  // epoch of its last attempt, the counting workgroups' counters, and a pinned copy of the epoch
  // it last declined (a table it declined stops trying)
  DevBuf<unsigned long long> dense_words;
  DevBuf<uint32_t> dense_part;
  uint64_t dense_epoch = 0;
  bool dense_off = false;
  PinnedWord dense_seen;
  // recorded behind the first tried batch's decline-word copy (ahead of its phase A): the second
  // batch waits for that answer instead of trying again (a fresh table per run -- the runner's
  // Histogram tables -- ran the range pre-pass on three or four batches of a wide column)
  hipEvent_t dense_ev = nullptr;
  bool dense_waited = false;
  // finalize cache (phase B)
  bool b_valid = false;
  int s_bits = 0;
  uint64_t R = 0;
  uint32_t n_units = 0;
  std::vector<unsigned long long> h_bucket_base = std::vector<unsigned long long>(kBuckets + 1, 0);
  std::vector<uint32_t> h_unit_start = std::vector<uint32_t>(kBuckets + 1, 0);
  DevBuf<unsigned long long> segS;         // phase B's segments per bucket (freq_seg_scan)
  DevBuf<uint32_t> segP, nseg;
  DevBuf<uint32_t> chunk_id;               // the non-empty chunks (finalize over those only)
  DevBuf<unsigned long long> chunk_boff, scan_tmp;
  DevBuf<uint32_t> unit_start, unit_c0, uhist;
  DevBuf<uint16_t> unit_b;
  DevBuf<unsigned long long> totals, part_base;
  // Capacity layout (exact tables, finalize_b): partition p's records are [part_base[p],
  // part_end[p]) inside a fixed capacity, filled through atomic cursors (no count pass).  The
  // counted layout's ends are part_base + 1.  Rcap: the records region's size in records.
  DevBuf<unsigned long long> part_end, cap_words;  // cap_words: bucket bases [kBuckets + 1], caps
  DevBuf<unsigned int> b_ovf;
  std::vector<unsigned long long> h_cap_words;
  const unsigned long long* part_end_ptr = nullptr;
  uint64_t Rcap = 0;
  bool cap_failed = false;  // a capacity layout overflowed: this table counts from now on
  DevBuf<uint8_t> recsB;
  // (phase C)
  bool c_valid = false, c_groups = false, c_cand = false;
  double c_num_rows = -1.0;
  DevBuf<unsigned long long> part_groups, part_unique, part_off;
  DevBuf<unsigned long long> part_entropy;  // (lo, hi) fixed-point sum per partition
  DevBuf<Group> cand, groups, compact;
  int64_t n_compact = -1;
  DevBuf<FEntry> ovf_a, ovf_b;
  DevBuf<unsigned int> ovf_n;
  DevBuf<unsigned long long> red;
  uint64_t st_groups = 0, st_unique = 0;
  double st_entropy = 0.0;
  fix128 st_entropy_fix = 0;  // the same sum, before its rounding to fp64
  uint64_t st_literal = 0;  // Histogram on a string: count of the "NullValue" string group
  bool recounted = false;
  // last top-k (dq_freq_topk is called twice: sizes, then data)
  int topk_k = -1;
  std::vector<int64_t> topk_counts, topk_offs;
  std::vector<uint8_t> topk_bytes;
};

inline unsigned grid_for(uint64_t n, unsigned cap = 4096) {
  uint64_t g = (n + 255) / 256;
  if (g < 1) g = 1;
  if (g > cap) g = cap;
  return (unsigned)g;
}

// A Histogram table over one string column: its NULL rows are kept apart from a "NullValue"
// string group that phase C probes for.
inline bool has_null_literal(const freq_table* f) {
  return !f->exact && f->n_keys == 1 && f->types[0] == DQ_UTF8 && f->mode_null_as_group > 0;
}

inline void invalidate(freq_table* f) {
  f->b_valid = false;
  f->c_valid = f->c_groups = f->c_cand = false;
  f->n_compact = -1;
  f->topk_k = -1;
}

// Grows `b` to at least `need` elements keeping the first `used` (stream-ordered copy).
template <typename T>
inline hipError_t grow_keep(DevBuf<T>& b, size_t used, size_t need, hipStream_t st) {
  if (need <= b.n && b.p) return hipSuccess;
  DevBuf<T> nb;
  hipError_t e = nb.ensure(std::max(need, b.n * 2));
  if (e != hipSuccess) return e;
  if (used) {
    e = hipMemcpyAsync(nb.p, b.p, used * sizeof(T), hipMemcpyDeviceToDevice, st);
    if (e != hipSuccess) return e;
    e = hipStreamSynchronize(st);
    if (e != hipSuccess) return e;
  }
  b.swap(nb);
  return hipSuccess;
}

inline dq_status ensure_chunks(freq_table* f, int64_t add) {
  const int64_t need = f->n_chunks + add;
  HIP_TRY(grow_keep(f->recs, (size_t)f->n_chunks * f->tile * f->rb, (size_t)need * f->tile * f->rb,
                    f->stream));
  HIP_TRY(grow_keep(f->hist, (size_t)f->n_chunks * kHistRow, (size_t)need * kHistRow, f->stream));
  return DQ_OK;
}

// the counters and the arena cursor as read back (dev_words: C_N counters + the cursor)
inline void apply_counters(freq_table* f, const unsigned long long* w) {
  for (int k = 0; k < C_N; ++k) f->h_counters[k] = w[k];
  f->arena_used = w[C_N];
  f->arena_hi = f->arena_used;
  f->counters_stale = false;
}
inline dq_status pull_counters(freq_table* f) {  // (d2h is ordered after the stream's work)
  unsigned long long w[C_N + 1];
  HIP_TRY(d2h(w, f->dev_words.p, sizeof(w), f->stream));
  apply_counters(f, w);
  return DQ_OK;
}
inline dq_status sync_counters(freq_table* f) { return f->counters_stale ? pull_counters(f) : DQ_OK; }

inline dq_status push_counters(freq_table* f) {
  HIP_TRY(hipStreamSynchronize(f->stream));
  unsigned long long w[C_N + 1];
  for (int k = 0; k < C_N; ++k) w[k] = f->h_counters[k];
  w[C_N] = f->arena_used;
  HIP_TRY(hipMemcpy(f->dev_words.p, w, sizeof(w), hipMemcpyHostToDevice));
  f->arena_hi = f->arena_used;
  f->counters_stale = false;
  return DQ_OK;
}

inline const uint8_t* arena_of(const freq_table* f) { return f->arena_view ? f->arena_view : f->arena.p; }

inline PartTypes part_types(const freq_table* f, int parts) {
  PartTypes t;
  memset(&t, 0, sizeof(t));
  for (int k = 0; k < f->n_keys; ++k) t.types[k] = f->types[k];
  t.n_keys = f->n_keys;
  t.exact = f->exact ? 1 : 0;
  t.parts = (uint32_t)parts;
  return t;
}

// DQ_FREQ_DEBUG, read once.  level (0 when unset): 1 times the records and MutualInformation
// steps (synchronising), 2 also stamps workgroup 0's phases in phase A and phase C; set: finalize_b
// prints the table's shape whenever the variable is set, at 0 too.
struct FreqDebug {
  bool set;
  int level;
};
inline const FreqDebug& freq_debug() {
  static const FreqDebug d = [] {
    const char* e = getenv("DQ_FREQ_DEBUG");
    return FreqDebug{e != nullptr, e ? atoi(e) : 0};
  }();
  return d;
}
inline int freq_debug_level() { return freq_debug().level; }

// ---- the host functions that cross files (defined in freq.hip, used by freq_mi.hip too) ----
dq_status add_records(dq_freq* f, const dq_freq_record* records, const uint8_t* var, int n_src,
                      const int64_t* src_records, const int64_t* src_var_bytes, int64_t num_rows,
                      const int64_t* special, int null_as_group, void* hip_stream, bool borrow);
// Phases B and C, unless the table's cached results already answer (groups materialised,
// Histogram candidates kept); fills f->st_* and the per-partition statistics.
dq_status finalize_c(dq_freq* f, bool want_groups, bool want_cand);
// The materialised groups, compacted: f->compact[0 .. f->n_compact).
dq_status compact_groups(dq_freq* f);

}  // namespace dq

struct dq_freq : dq::freq_table {};
