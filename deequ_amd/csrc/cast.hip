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
//   DoubleType: java.lang.Double.parseDouble.  Plain decimals inside the exact window (digits
//               without leading and trailing zeros <= 2^53, the matching power of ten within
//               +-22 or brought there by an exact rescale) are converted with one correctly
//               rounded fp64 multiply or divide; a string parseDouble rejects is NULL; a string
//               parseDouble reads but this path does not convert (exponents, "NaN", "Infinity",
//               hex, a 'd'/'f' suffix, more digits) is NULL and counted in *n_unsupported, and the
//               caller fails loudly on a non-zero count rather than guess.
#include <hip/hip_runtime.h>

#include "cast_parse.h"
#include "engine.h"
#include "kernels.h"

namespace dq {
namespace {

using castp::java_parse_double;
using castp::spark_to_long;

constexpr int kCastThreads = 256;

__global__ void __launch_bounds__(kCastThreads) cast_utf8_kernel(
    const int32_t* __restrict__ off, const uint8_t* __restrict__ data,
    const uint8_t* __restrict__ valid, int64_t n, int to_type, void* __restrict__ values,
    uint8_t* __restrict__ validity_out, unsigned long long* __restrict__ n_unsupported) {
  const int64_t byte = (int64_t)blockIdx.x * kCastThreads + threadIdx.x;
  const int64_t r0 = byte * 8;
  if (r0 >= n) return;
  uint32_t vbits = 0, bad = 0;
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
        const int res = java_parse_double(data + s, len, v);
        ok = res == 1;
        bad += res == 2;
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
  if (bad) atomicAdd(n_unsupported, (unsigned long long)bad);
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
  unsigned long long* cnt = nullptr;
  HIP_TRY(hipMallocAsync(reinterpret_cast<void**>(&cnt), sizeof(*cnt), st));
  HIP_TRY(hipMemsetAsync(cnt, 0, sizeof(*cnt), st));
  const int64_t bytes = (in->length + 7) / 8;
  const unsigned grid = (unsigned)((bytes + kCastThreads - 1) / kCastThreads);
  hipLaunchKernelGGL(cast_utf8_kernel, dim3(grid), dim3(kCastThreads), 0, st,
                     static_cast<const int32_t*>(in->values), in->data, in->validity, in->length,
                     to_type, values_out, validity_out, cnt);
  HIP_TRY(hipGetLastError());
  unsigned long long h = 0;
  HIP_TRY(hipMemcpyAsync(&h, cnt, sizeof(h), hipMemcpyDeviceToHost, st));
  HIP_TRY(hipFreeAsync(cnt, st));
  HIP_TRY(hipStreamSynchronize(st));
  *n_unsupported = (int64_t)h;
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
