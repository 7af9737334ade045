// cast.hip -- Spark 2.2 Cast(StringType -> LongType | DoubleType) of a utf8 column on the device:
// the ColumnProfiler's second pass casts the string columns its first pass inferred Integral or
// Fractional (ColumnProfiler.scala:311-320 castColumn, 389-405 castNumericStringColumns) before
// Minimum / Maximum / Mean / StandardDeviation / Sum / ApproxQuantiles run over them.
//
// One thread per 8 rows, so every thread writes one whole validity byte (LSB-first, the bits past
// the last row zero).  A row's value is 0 wherever its validity bit is 0; a NULL input row stays
// NULL and its bytes are never read.  The per-string parsers are cast_parse.h's (shared with the
// host entry point dq_cast_parse_utf8):
//   LongType:   UTF8String.toLong; never counted in *n_unsupported.
//   DoubleType: java.lang.Double.parseDouble.  Every plain decimal, of any length and magnitude,
//               becomes the correctly rounded double (+-Infinity above the range, +-0.0 below); a
//               string parseDouble rejects is NULL; a non-plain form parseDouble reads (an
//               exponent, "NaN", "Infinity", hex, a 'd'/'f' suffix) is NULL and counted in
//               *n_unsupported, and the caller fails loudly on a non-zero count.
//
// The double cast runs in two passes so that the common rows do not pay for the rare ones.
// cast_utf8_kernel runs only the register-resident conversions (the exact window and Eisel-Lemire,
// parse_double.h).  A row they cannot decide stays NULL for the moment, and the thread appends one
// entry for its validity byte -- the byte's index and the mask of its undecided rows -- to a device
// list through an atomic cursor.  The cursor comes back in the read that returns n_unsupported, and
// only when it is non-zero does cast_exact_kernel run: one thread per entry, the exact multi-word
// fallback (dec_exact, which lives in scratch memory) for each flagged row, then the validity byte
// re-emitted with those bits set.  The byte has one owner in each pass -- in the second the only
// entry that names it -- and the second pass follows the first in stream order, so neither an
// atomic nor an aligned-word access that would touch neighbouring bytes is needed.
#include <hip/hip_runtime.h>

#include <atomic>

#include "cast_parse.h"
#include "engine.h"
#include "kernels.h"

namespace dq {
namespace {

using castp::java_parse_double;
using castp::java_parse_double_fast;
using castp::spark_to_long;

constexpr int kCastThreads = 256;
constexpr int kExactThreads = 64;  // (every thread of the second pass holds two multi-word integers)

// counters[0] = rows counted unsupported, counters[1] = the cursor of `undecided`, which holds one
// entry (byte index << 8 | mask of undecided rows) per validity byte at most: (n + 7) / 8 entries
__global__ void __launch_bounds__(kCastThreads) cast_utf8_kernel(
    const int32_t* __restrict__ off, const uint8_t* __restrict__ data,
    const uint8_t* __restrict__ valid, int64_t n, int to_type, void* __restrict__ values,
    uint8_t* __restrict__ validity_out, unsigned long long* __restrict__ counters,
    unsigned long long* __restrict__ undecided) {
  const int64_t byte = (int64_t)blockIdx.x * kCastThreads + threadIdx.x;
  const int64_t r0 = byte * 8;
  if (r0 >= n) return;
  uint32_t vbits = 0, bad = 0, later = 0;
  for (int k = 0; k < 8 && r0 + k < n; ++k) {
    const int64_t r = r0 + k;
    bool ok = false;
    if (!valid || ((valid[r >> 3] >> (r & 7)) & 1u)) {
      const int32_t s = off[r], len = off[r + 1] - s;
      if (to_type == DQ_INT64) {
        int64_t v = 0;
        ok = spark_to_long(data + s, len, v);
        static_cast<int64_t*>(values)[r] = ok ? v : 0;
      } else {
        double v = 0.0;
        const int res = java_parse_double_fast(data + s, len, v);
        ok = res == 1;
        bad += res == 2;
        later |= (res == 3 ? 1u : 0u) << k;
        static_cast<double*>(values)[r] = ok ? v : 0.0;
      }
    } else if (to_type == DQ_INT64) {
      static_cast<int64_t*>(values)[r] = 0;
    } else {
      static_cast<double*>(values)[r] = 0.0;
    }
    vbits |= (ok ? 1u : 0u) << k;
  }
  validity_out[byte] = (uint8_t)vbits;
  if (bad) atomicAdd(&counters[0], (unsigned long long)bad);
  if (later) undecided[atomicAdd(&counters[1], 1ULL)] = ((unsigned long long)byte << 8) | later;
}

// The second pass of the double cast: one thread per entry of `undecided`.  Every flagged row is a
// non-NULL plain decimal, so the complete parser gives it a value.
__global__ void __launch_bounds__(kExactThreads) cast_exact_kernel(
    const int32_t* __restrict__ off, const uint8_t* __restrict__ data, int64_t n,
    const unsigned long long* __restrict__ undecided, int64_t n_entries,
    double* __restrict__ values, uint8_t* __restrict__ validity_out) {
  const int64_t i = (int64_t)blockIdx.x * kExactThreads + threadIdx.x;
  if (i >= n_entries) return;
  const unsigned long long entry = undecided[i];
  const int64_t byte = (int64_t)(entry >> 8);
  const uint32_t mask = (uint32_t)(entry & 0xFF);
  uint32_t done = 0;
  for (int k = 0; k < 8; ++k) {
    const int64_t r = byte * 8 + k;
    if (!((mask >> k) & 1u) || r >= n) continue;
    const int32_t s = off[r], len = off[r + 1] - s;
    double v = 0.0;
    if (java_parse_double(data + s, len, v) == 1) {
      values[r] = v;
      done |= 1u << k;
    }
  }
  validity_out[byte] = (uint8_t)(validity_out[byte] | done);
}

// Arrow bitmap at bit offset `bit` -> LSB-first bitmap at bit 0 (one thread per output byte).
// Reads only bytes that hold bits of rows [bit, bit + rows).
__global__ void __launch_bounds__(kCastThreads)
bitmap_rebase_kernel(const uint8_t* __restrict__ src, int64_t bit, int64_t rows,
                     uint8_t* __restrict__ dst) {
  const int64_t i = (int64_t)blockIdx.x * kCastThreads + threadIdx.x;
  const int64_t n_out = (rows + 7) / 8;
  if (i >= n_out) return;
  const int64_t last_src = (bit + rows - 1) / 8;  // last source byte holding a row's bit
  const int64_t j = bit / 8 + i;
  const uint32_t sh = (uint32_t)(bit & 7);
  uint32_t v = src[j] >> sh;
  if (sh && j + 1 <= last_src) v |= (uint32_t)src[j + 1] << (8 - sh);
  dst[i] = (uint8_t)v;
}

}  // namespace

hipError_t launch_bitmap_rebase(const uint8_t* src, int64_t bit, int64_t rows, uint8_t* dst,
                                hipStream_t stream) {
  const int64_t n_out = (rows + 7) / 8;
  if (n_out <= 0) return hipSuccess;
  hipLaunchKernelGGL(bitmap_rebase_kernel, dim3((unsigned)((n_out + kCastThreads - 1) / kCastThreads)),
                     dim3(kCastThreads), 0, stream, src, bit, rows, dst);
  return hipGetLastError();
}

}  // namespace dq

using namespace dq;

extern "C" dq_status dq_cast_utf8(const dq_column* in, int to_type, void* values_out,
                                  uint8_t* validity_out, int64_t* n_unsupported, void* hip_stream) {
  if (!in || !n_unsupported) return fail(DQ_ERR_INVALID_ARGUMENT, "null argument");
  if (in->type != DQ_UTF8) return fail(DQ_ERR_WRONG_TYPE, "dq_cast_utf8 casts a utf8 column");
  if (to_type != DQ_INT64 && to_type != DQ_FLOAT64)
    return fail(DQ_ERR_UNSUPPORTED, "dq_cast_utf8 casts to int64 or float64 only");
  *n_unsupported = 0;
  if (in->length == 0) return DQ_OK;
  if (!in->values || !in->data || !values_out || !validity_out)
    return fail(DQ_ERR_INVALID_ARGUMENT, "null column buffers");
  hipStream_t st = reinterpret_cast<hipStream_t>(hip_stream);
  const int64_t bytes = (in->length + 7) / 8;
  // one stream-ordered block: the two counters, then (double casts only) the undecided list
  const size_t words = 2 + (to_type == DQ_FLOAT64 ? (size_t)bytes : 0);
  unsigned long long* cnt = nullptr;
  HIP_TRY(hipMallocAsync(reinterpret_cast<void**>(&cnt), words * sizeof(*cnt), st));
  HIP_TRY(hipMemsetAsync(cnt, 0, 2 * sizeof(*cnt), st));
  unsigned long long* undecided = cnt + 2;
  const auto* off = static_cast<const int32_t*>(in->values);
  const unsigned grid = (unsigned)((bytes + kCastThreads - 1) / kCastThreads);
  hipLaunchKernelGGL(cast_utf8_kernel, dim3(grid), dim3(kCastThreads), 0, st, off, in->data,
                     in->validity, in->length, to_type, values_out, validity_out, cnt, undecided);
  HIP_TRY(hipGetLastError());
  unsigned long long h[2] = {0, 0};
  HIP_TRY(hipMemcpyAsync(h, cnt, sizeof(h), hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  if (h[1]) {  // (at most `bytes` entries: one per thread of the first pass)
    const int64_t n_entries = (int64_t)h[1];
    const unsigned grid2 = (unsigned)((n_entries + kExactThreads - 1) / kExactThreads);
    hipLaunchKernelGGL(cast_exact_kernel, dim3(grid2), dim3(kExactThreads), 0, st, off, in->data,
                       in->length, undecided, n_entries, static_cast<double*>(values_out),
                       validity_out);
    HIP_TRY(hipGetLastError());
  }
  HIP_TRY(hipFreeAsync(cnt, st));
  if (h[1]) HIP_TRY(hipStreamSynchronize(st));
  *n_unsupported = (int64_t)h[0];
  return DQ_OK;
}

extern "C" int dq_cast_parse_utf8(const uint8_t* s, int32_t n, int to_type, int64_t* long_out,
                                  double* double_out) {
  if (to_type == DQ_INT64) {
    int64_t v = 0;
    const bool ok = castp::spark_to_long(s, n, v);
    *long_out = ok ? v : 0;
    return ok ? 1 : 0;
  }
  double v = 0.0;
  const int res = castp::java_parse_double(s, n, v);
  *double_out = res == 1 ? v : 0.0;
  return res;
}

namespace {
std::atomic<int64_t> g_exact_fallbacks{0};
}

extern "C" int dq_parse_double_utf8(const uint8_t* s, int32_t n, double* out) {
  double v = 0.0;
  int flags = 0;
  const bool ok = castp::parse_double(s, n, v, flags);
  if (flags & castp::kPdFallback) g_exact_fallbacks.fetch_add(1, std::memory_order_relaxed);
  *out = ok ? v : 0.0;
  return ok ? 1 : 0;
}

extern "C" int64_t dq_parse_double_fallbacks(void) {
  return g_exact_fallbacks.load(std::memory_order_relaxed);
}
