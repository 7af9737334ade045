// split.hip -- the random row split behind Table.random_split (the device side of
// ConstraintSuggestionRunner.scala:80-92, `data.randomSplit(...)`).
//
// A row's split is a pure function of (seed, table-global row index): a SplitMix64 step at counter
// r + 1 gives 53 uniform bits u in [0, 1), and the row goes to the first split whose cumulative
// weight bound exceeds u.  Nothing depends on the batch a row arrives in.
//
// One lane takes one row, so a wave's ballot of `split == k` is word w of split k's bitmap: lane 0
// stores it with one 64-bit store, no two waves share a word, and the bitmap needs no atomics.  A
// lane past `rows` votes in no ballot, which leaves the padding bits of the last word zero.  The
// popcounts of the ballots are summed per wave in registers, per block through LDS, and reach the
// device counters as one atomic add per block and split.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "device_util.h"
#include "engine.h"
#include "kernels.h"

namespace dq {
namespace {

constexpr int kSplitBlock = kBlock;       // threads per block: 4 waves, 4 bitmap words per pass
constexpr int kSplitMaxBlocks = 2048;     // the grid is capped here; blocks stride over the words
constexpr int kSplitWaves = kSplitBlock / 64;
constexpr int64_t kMaxRows = 2147483647;

struct SplitArgs {
  uint64_t* bitmap[DQ_SPLIT_MAX];
  double bound[DQ_SPLIT_MAX];  // entries at and after n_splits - 1 are never compared
  int32_t n_splits, pad;
};

// u(seed, r): SplitMix64's output function at state seed + (r + 1) * gamma, top 53 bits.
DQ_HD double split_draw(uint64_t seed, uint64_t r) {
  uint64_t z = seed + (r + 1) * 0x9E3779B97F4A7C15ULL;
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ULL;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBULL;
  z = z ^ (z >> 31);
  return (double)(z >> 11) * 0x1.0p-53;
}

__global__ void __launch_bounds__(kSplitBlock)
split_rows_kernel(const SplitArgs a, int64_t rows, uint64_t row_base, uint64_t seed,
                  unsigned long long* __restrict__ counts) {
  __shared__ uint32_t lds[kSplitWaves][DQ_SPLIT_MAX];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int64_t wave = (int64_t)blockIdx.x * kSplitWaves + wv;
  const int64_t n_waves = (int64_t)gridDim.x * kSplitWaves;
  const int64_t n_words = (rows + 63) >> 6;
  uint32_t cnt[DQ_SPLIT_MAX];
#pragma unroll
  for (int k = 0; k < DQ_SPLIT_MAX; ++k) cnt[k] = 0;
  for (int64_t w = wave; w < n_words; w += n_waves) {  // wave-uniform
    const int64_t i = w * 64 + lane;
    int split = -1;
    if (i < rows) {
      const double u = split_draw(seed, row_base + (uint64_t)i);
      // bounds are non-decreasing and the last is 1 > u: the first k with u < bound[k] is the
      // number of bounds before the last that u has reached
      split = 0;
#pragma unroll
      for (int k = 0; k < DQ_SPLIT_MAX - 1; ++k)
        if (k < a.n_splits - 1) split += u >= a.bound[k];
    }
#pragma unroll
    for (int k = 0; k < DQ_SPLIT_MAX; ++k) {
      if (k < a.n_splits) {  // uniform
        const uint64_t word = __ballot(split == k);
        if (lane == 0) a.bitmap[k][w] = word;
        cnt[k] += (uint32_t)__popcll(word);
      }
    }
  }
  if (lane == 0) {
#pragma unroll
    for (int k = 0; k < DQ_SPLIT_MAX; ++k) lds[wv][k] = cnt[k];
  }
  __syncthreads();
  if (threadIdx.x < a.n_splits) {
    uint32_t sum = 0;
    for (int j = 0; j < kSplitWaves; ++j) sum += lds[j][threadIdx.x];
    if (sum) atomicAdd(counts + threadIdx.x, (unsigned long long)sum);
  }
}

}  // namespace
}  // namespace dq

using namespace dq;

extern "C" dq_status dq_split_rows(int64_t rows, int64_t row_base, uint64_t seed, const double* bounds,
                                   int n_splits, uint64_t* const* bitmaps, int64_t* counts,
                                   void* hip_stream) {
  if (rows < 0 || row_base < 0 || !bounds || !bitmaps || !counts)
    return fail(DQ_ERR_INVALID_ARGUMENT, "dq_split_rows: null or negative argument");
  if (n_splits < 1 || n_splits > DQ_SPLIT_MAX)
    return fail(DQ_ERR_INVALID_ARGUMENT, "dq_split_rows: %d splits (1 .. %d)", n_splits, DQ_SPLIT_MAX);
  double prev = 0.0;
  for (int k = 0; k < n_splits; ++k) {
    const double b = bounds[k];
    // (a NaN fails every comparison)
    if (!(b > 0.0 && b <= 1.0 && b >= prev))
      return fail(DQ_ERR_INVALID_ARGUMENT, "dq_split_rows: bound %d = %g is not non-decreasing in (0, 1]",
                  k, b);
    prev = b;
  }
  if (prev != 1.0) return fail(DQ_ERR_INVALID_ARGUMENT, "dq_split_rows: the last bound is %g, not 1", prev);
  if (rows > kMaxRows)
    return fail(DQ_ERR_UNSUPPORTED, "dq_split_rows: a batch of %lld rows (at most 2^31-1)", (long long)rows);
  for (int k = 0; k < n_splits; ++k)
    if (rows && !bitmaps[k]) return fail(DQ_ERR_INVALID_ARGUMENT, "dq_split_rows: null bitmap %d", k);
  for (int k = 0; k < n_splits; ++k) counts[k] = 0;
  if (rows == 0) return DQ_OK;
  SplitArgs a;
  for (int k = 0; k < DQ_SPLIT_MAX; ++k) {
    a.bitmap[k] = k < n_splits ? bitmaps[k] : nullptr;
    a.bound[k] = k < n_splits ? bounds[k] : 1.0;
  }
  a.n_splits = n_splits;
  a.pad = 0;
  hipStream_t st = reinterpret_cast<hipStream_t>(hip_stream);
  DevBuf<unsigned long long> cnt;
  HIP_TRY(cnt.ensure(DQ_SPLIT_MAX));
  HIP_TRY(hipMemsetAsync(cnt.p, 0, DQ_SPLIT_MAX * sizeof(unsigned long long), st));
  const int64_t n_words = (rows + 63) / 64;
  const unsigned grid =
      (unsigned)std::min<int64_t>((n_words + kSplitWaves - 1) / kSplitWaves, kSplitMaxBlocks);
  hipLaunchKernelGGL(split_rows_kernel, dim3(grid), dim3(kSplitBlock), 0, st, a, rows,
                     (uint64_t)row_base, seed, cnt.p);
  HIP_TRY(hipGetLastError());
  unsigned long long h[DQ_SPLIT_MAX];
  HIP_TRY(d2h(h, cnt.p, sizeof(h), st));
  for (int k = 0; k < n_splits; ++k) counts[k] = (int64_t)h[k];
  return DQ_OK;
}
