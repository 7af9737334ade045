// freq_device.h -- the group-by's constants and the device helpers that more than one of its
// translation units uses (freq_table.h has the file map); nothing here knows the table.
// Every function is DQ_DEV (force-inlined) except entropy_term.
#pragma once
#include <hip/hip_runtime.h>

#include <type_traits>

#include "engine.h"
#include "freq_codec.h"

namespace dq {

#define DQ_DEV __device__ __forceinline__

constexpr int kBucketBits = 9;
constexpr int kBuckets = 1 << kBucketBits;
constexpr int kHistRow = kBuckets + 1;  // u16 exclusive bucket prefix of a chunk + its total
constexpr int kThreads = 1024;
constexpr int kMaxSubBits = 10;
constexpr int kMinPkSubBits = 7;  // packed phase-C slots need a partition of >= 9 + 7 fixed bits
constexpr int kFilterShift = 32;        // hash bits that split an overflowing partition
constexpr int kCand = 4;                // top groups kept per partition for Histogram
constexpr int kSmallCounts = 64;        // phase C histograms group counts below this
constexpr int kMaxParts = 64;
constexpr uint64_t kEmptyKey = ~0ULL;
constexpr uint64_t kNotReady = ~0ULL;

struct SrcSegs {
  int64_t rec_start[kMaxParts + 1];
  int64_t var_base[kMaxParts];
  int32_t n_src;
};
using fix128 = __int128;

DQ_DEV uint64_t lds_load(const uint64_t* p) {
  return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
}
DQ_DEV void lds_store(uint64_t* p, uint64_t v) {
  __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
}

// ockl wavefront reductions / scans: DPP row and broadcast steps, no LDS round trips (the
// __shfl_* forms are ds_bpermute, a few hundred cycles for a 6-step 64-bit chain)
extern "C" __device__ uint32_t __ockl_wfred_add_u32(uint32_t);
extern "C" __device__ uint64_t __ockl_wfred_add_u64(uint64_t);
extern "C" __device__ double __ockl_wfred_add_f64(double);
extern "C" __device__ uint64_t __ockl_wfred_max_u64(uint64_t);
extern "C" __device__ uint32_t __ockl_wfscan_add_u32(uint32_t, bool);

// Exclusive scan of one u32 per thread over the workgroup; returns the thread's prefix and sets
// `total`.  Every thread of the block must call it.
DQ_DEV uint32_t block_excl_scan(uint32_t v, uint32_t* s_wave, uint32_t& total) {
  const int lane = __lane_id(), wave = threadIdx.x >> 6, nw = blockDim.x >> 6;
  const uint32_t x = __ockl_wfscan_add_u32(v, true);
  if (lane == 63) s_wave[wave] = x;
  __syncthreads();
  if (wave == 0) {
    const uint32_t w = __ockl_wfscan_add_u32(lane < nw ? s_wave[lane] : 0u, true);
    if (lane < nw) s_wave[lane] = w;
  }
  __syncthreads();
  const uint32_t base = wave ? s_wave[wave - 1] : 0u;
  total = s_wave[nw - 1];
  __syncthreads();
  return base + x - v;
}

template <typename T>
DQ_DEV T wave_sum(T v) {
  if constexpr (std::is_same_v<T, double>) return __ockl_wfred_add_f64(v);
  else if constexpr (sizeof(T) == 8) return (T)__ockl_wfred_add_u64((uint64_t)v);
  else return (T)__ockl_wfred_add_u32((uint32_t)v);
}

// Fixed-order block sums (every thread calls; the result is valid in every thread).
DQ_DEV uint64_t block_sum_u64(uint64_t v, uint64_t* s) {
  v = wave_sum(v);
  const int wave = threadIdx.x >> 6, nw = blockDim.x >> 6;
  if (__lane_id() == 0) s[wave] = v;
  __syncthreads();
  uint64_t t = 0;
  for (int w = 0; w < nw; ++w) t += s[w];
  __syncthreads();
  return t;
}
DQ_DEV double block_sum_f64(double v, double* s) {
  v = wave_sum(v);
  const int wave = threadIdx.x >> 6, nw = blockDim.x >> 6;
  if (__lane_id() == 0) s[wave] = v;
  __syncthreads();
  double t = 0.0;
  for (int w = 0; w < nw; ++w) t += s[w];
  __syncthreads();
  return t;
}

// Sum over the wave, added to a table counter by lane 0 (counters are single addresses).
DQ_DEV void wave_count(unsigned long long* counter, unsigned long long v) {
  v = wave_sum(v);
  if (__lane_id() == 0 && v) atomicAdd(counter, v);
}
// A workgroup's largest record count into an LDS word, only when it could bar packed slots
// (>= 16 = 2^(7-3)); the workgroup then makes one global atomic (one per wave on one address
// serialised phase A over records: 9.4 -> 50 ms per configs[4] run)
DQ_DEV void wave_max_lds(unsigned long long* s_slot, uint64_t v) {
  v = __ockl_wfred_max_u64(v);
  if (__lane_id() == 0 && v >= 16) atomicMax(s_slot, (unsigned long long)v);
}

// last index j in [0, n) with pos[j] <= x (pos non-decreasing, pos[0] = 0 <= x)
DQ_DEV uint32_t seg_of(const uint32_t* pos, uint32_t n, uint32_t x) {
  uint32_t lo = 0, hi = n;  // answer in [lo, hi)
  while (hi - lo > 1) {
    const uint32_t mid = (lo + hi) >> 1;
    if (pos[mid] <= x) lo = mid;
    else hi = mid;
  }
  return lo;
}

DQ_DEV int64_t seg_var_base(const SrcSegs& s, int64_t i) {
  int j = 0;
  while (j + 1 < s.n_src && i >= s.rec_start[j + 1]) ++j;
  return s.var_base[j];
}

template <typename F>
DQ_DEV void for_digits(uint64_t c, F&& f) {
  for (uint32_t e = 0; c; c >>= 2, ++e)
    if (c & 3) f((e << 2) | (uint32_t)(c & 3));
}

DQ_DEV uint32_t bucket_of(uint64_t h) { return (uint32_t)(h >> (64 - kBucketBits)); }
// sub-bucket (the s hash bits below the bucket bits); x = h or the exact record >> 8 (both hold
// hash bits 54..0 in place)
DQ_DEV uint32_t sub_of(uint64_t x, int s) {
  return s ? (uint32_t)((x >> (64 - kBucketBits - s)) & ((1u << s) - 1u)) : 0u;
}
DQ_DEV uint64_t xrec_h(uint64_t rec, uint32_t b) {
  return ((uint64_t)b << 55) | ((rec >> 8) & ((1ULL << 55) - 1));
}

// -(c/n) ln(c/n), out of line: the statistics pass calls it from every unrolled slot, and inlined
// copies of log() there made phase C several times larger than the instruction cache holds.
// Defined here and nowhere else: freq.hip (phase C) and freq_mi.hip (freq_slots_entropy) each compile
// their own out-of-line copy from this one text, which is why a small marginal's entropy has the
// bits of a table's.
__device__ __attribute__((noinline)) double entropy_term(uint64_t c, double n) {
  const double pr = (double)c / n;
  return -pr * log(pr);
}

// ---- Exact sums of fp64 terms (Entropy's -p ln p, MutualInformation's p ln(p / (px py))) ----
// A term enters as a signed 128-bit fixed-point integer at 2^-112 (exact for every term of
// magnitude >= 2^-60, cut below 2^-112), so a sum is the same integer in ANY order: the table's
// entropy is the sum of its groups' terms whatever the phase-C insert order, the partition depth,
// the recount subsets or the order partial sums meet in -- bit-stable from run to run.  Terms are
// bounded (|term| <= ln(rows) < 2^6), sums stay far inside 2^15.
constexpr double kFixUlp = 0x1p-112;
DQ_HD fix128 fix_of(double x) {
  const uint64_t b = __builtin_bit_cast(uint64_t, x);
  const int ex = (int)((b >> 52) & 0x7ff);
  if (ex == 0) return 0;  // zero (and subnormals, < 2^-1022: cut)
  const uint64_t m = (b & ((1ULL << 52) - 1)) | (1ULL << 52);
  const int sh = ex - 1075 + 112;  // x = m 2^(ex - 1075); fixed = m 2^(ex - 1075 + 112)
  const fix128 v = sh >= 0 ? ((fix128)m << sh) : (sh > -64 ? (fix128)(m >> -sh) : (fix128)0);
  return (b >> 63) ? -v : v;
}
// (a fixed sequence of roundings: deterministic, within 2 ulp)
DQ_HD double fix_to_f64(fix128 v) {
  const int64_t hi = (int64_t)(v >> 64);
  const uint64_t lo = (uint64_t)v;
  return ((double)hi * 18446744073709551616.0 + (double)lo) * kFixUlp;
}
DQ_DEV fix128 wave_sum_fix(fix128 v) {
#pragma unroll
  for (int o = 32; o; o >>= 1) {
    const uint64_t lo = __shfl_xor((unsigned long long)(uint64_t)v, o);
    const uint64_t hi = __shfl_xor((unsigned long long)(uint64_t)(v >> 64), o);
    v += (fix128)(((unsigned __int128)hi << 64) | lo);
  }
  return v;
}
// p[0..1] += v (lo, hi words): the carry of each lo add goes with that add's hi, so the total is
// exact whatever order the adds land in
DQ_DEV void atomic_add_fix(unsigned long long* p, fix128 v) {
  const uint64_t lo = (uint64_t)v, hi = (uint64_t)(v >> 64);
  const uint64_t old = atomicAdd(p, (unsigned long long)lo);
  const uint64_t up = hi + (old + lo < old ? 1u : 0u);
  if (up) atomicAdd(p + 1, (unsigned long long)up);
}
DQ_DEV void store_fix(unsigned long long* p, fix128 v) {
  p[0] = (uint64_t)v;
  p[1] = (uint64_t)(v >> 64);
}

}  // namespace dq
