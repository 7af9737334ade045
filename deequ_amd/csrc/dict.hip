// dict.hip -- dictionary-encoded Arrow columns (dictionary<I, V>) on the device.
//
// A dictionary column is a small array of distinct values (the dictionary, an ordinary dq_column)
// and one integer per row that names an entry.  Two things happen to it here:
//   * dq_dict_decode: the decoded column, in the layout Table.from_arrow gives the decoded array,
//     so every operator that reads a ColumnBatch runs unchanged;
//   * launch_dict_count: rows per dictionary entry, the first half of dq_freq_add_dict_device
//     (freq.hip): the group-by of a one-key table then hashes and encodes every used ENTRY once
//     instead of every row.
//
// A row is NULL when its index is NULL or the entry it names is NULL.  A valid index outside
// [0, entries) is counted as bad and written as NULL / zero / empty: every kernel compares the index
// with the bounds before it forms an address from it.
//
// Decode, fixed-width V: one launch, one thread per 8 rows (one whole validity byte per thread, as
// cast.hip).  Decode, utf8 V: three launches over tiles of kDictTile rows, no workgroup waits for
// another:
//   1. dict_len_kernel   per-row length (into the output offsets) and validity, per-tile totals;
//   2. the single-block scan of the tile totals (rowschema.hip's, launch_tile_scan);
//   3. dict_copy_kernel  the tile's lengths scanned into offsets in place, then the bytes.
// The copy has two shapes.  Short entries (a few bytes, thousands of rows per workgroup): when the
// dictionary's offsets and bytes fit kDictLdsBytes they are staged in LDS once per workgroup and
// every row reads its entry from there, not from L2.  Long entries (>= kDictLongLen bytes): the
// wave copies the row together, lane-strided, so one lane's byte loop never holds the other 63.
// Every string loop is bounded by a length computed from the dictionary's offsets.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "engine.h"
#include "kernels.h"

namespace dq {
namespace {

constexpr int kDictThreads = 256;
constexpr int kDictPerThread = 8;                           // rows per thread (one validity byte)
constexpr int kDictTile = kDictThreads * kDictPerThread;    // rows per workgroup of the utf8 decode
constexpr int kDictLongLen = 64;                            // bytes from which a wave copies a row together
// LDS a copy workgroup may spend on the dictionary: 16 KiB leaves 160 / 16 = 10 workgroups of LDS
// room per CU, more than the 8 the wave slots allow, so staging never costs occupancy.
constexpr int kDictLdsBytes = 16384;
constexpr int64_t kDictMaxRows = 2147483647;

// Count kernel regimes by dictionary size: registers, LDS counters (replicated per
// wave while 4 copies stay within 16 KiB), global atomics.
constexpr int64_t kDictRegMax = 8;
constexpr int64_t kDictWaveMax = 1024;
constexpr int64_t kDictLdsMax = 16384;  // 64 KiB of u32 counters: two workgroups per CU
constexpr int kCountRows = 16;           // rows per thread and step (one 128-bit load of int8 indices)

struct B16 {
  uint64_t a, b;
};

__device__ inline uint32_t vbit(const uint8_t* bm, int64_t r) {
  return bm ? ((bm[r >> 3] >> (r & 7)) & 1u) : 1u;
}

// What row r names: 0 = NULL index, 1 = entry e in [0, entries), 2 = a bad index (e is not set to
// anything an address may be formed from).  An unsigned 64-bit index >= 2^63 reads negative: bad.
template <typename T>
__device__ inline int resolve(const T* __restrict__ idx, const uint8_t* __restrict__ valid, int64_t r,
                              int64_t entries, int64_t& e) {
  e = 0;
  if (!vbit(valid, r)) return 0;
  const int64_t v = (int64_t)idx[r];
  if (v < 0 || v >= entries) return 2;
  e = v;
  return 1;
}

__device__ inline unsigned long long wave_sum_u64(unsigned long long v) {
  for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d);
  return v;
}

// Exclusive prefix of v over the block's threads and the block's total; every thread calls it.
__device__ inline uint32_t block_scan(uint32_t v, uint32_t* lds /* kDictThreads / 64 */, uint32_t& total) {
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  uint32_t inc = v;
  for (int d = 1; d < 64; d <<= 1) {
    const uint32_t t = __shfl_up(inc, d);
    if (lane >= d) inc += t;
  }
  if (lane == 63) lds[wv] = inc;
  __syncthreads();
  uint32_t base = 0;
  total = 0;
  for (int k = 0; k < kDictThreads / 64; ++k) {
    const uint32_t x = lds[k];
    if (k < wv) base += x;
    total += x;
  }
  __syncthreads();
  return base + inc - v;
}

// ------------------------------------------------------------------------------------------------
// Decode, fixed-width and boolean values
// ------------------------------------------------------------------------------------------------
template <typename T, typename V>
__global__ void __launch_bounds__(kDictThreads)
dict_decode_fixed(const T* __restrict__ idx, const uint8_t* __restrict__ ivalid, int64_t n,
                  const V* __restrict__ dvals, const uint8_t* __restrict__ dvalid, int64_t entries,
                  V* __restrict__ out, uint8_t* __restrict__ ovalid,
                  unsigned long long* __restrict__ words) {
  const int64_t byte = (int64_t)blockIdx.x * kDictThreads + threadIdx.x;
  const int64_t r0 = byte * 8;
  if (r0 >= n) return;
  uint32_t vbits = 0, bad = 0;
  for (int k = 0; k < 8 && r0 + k < n; ++k) {
    const int64_t r = r0 + k;
    int64_t e;
    const int s = resolve(idx, ivalid, r, entries, e);
    bad += s == 2;
    const bool ok = s == 1 && vbit(dvalid, e);
    out[r] = ok ? dvals[e] : V{};
    vbits |= (ok ? 1u : 0u) << k;
  }
  if (ovalid) ovalid[byte] = (uint8_t)vbits;
  if (bad) atomicAdd(words, (unsigned long long)bad);
}

template <typename T>
__global__ void __launch_bounds__(kDictThreads)
dict_decode_bool(const T* __restrict__ idx, const uint8_t* __restrict__ ivalid, int64_t n,
                 const uint8_t* __restrict__ dvals, const uint8_t* __restrict__ dvalid, int64_t entries,
                 uint8_t* __restrict__ out, uint8_t* __restrict__ ovalid,
                 unsigned long long* __restrict__ words) {
  const int64_t byte = (int64_t)blockIdx.x * kDictThreads + threadIdx.x;
  const int64_t r0 = byte * 8;
  if (r0 >= n) return;
  uint32_t vbits = 0, bits = 0, bad = 0;
  for (int k = 0; k < 8 && r0 + k < n; ++k) {
    int64_t e;
    const int s = resolve(idx, ivalid, r0 + k, entries, e);
    bad += s == 2;
    const bool ok = s == 1 && vbit(dvalid, e);
    vbits |= (ok ? 1u : 0u) << k;
    bits |= (ok ? vbit(dvals, e) : 0u) << k;
  }
  out[byte] = (uint8_t)bits;
  if (ovalid) ovalid[byte] = (uint8_t)vbits;
  if (bad) atomicAdd(words, (unsigned long long)bad);
}

// ------------------------------------------------------------------------------------------------
// Decode, utf8 values
// ------------------------------------------------------------------------------------------------
// Length of row r (0 for a NULL or bad row) and whether it is valid.
template <typename T>
__device__ inline uint32_t row_len(const T* __restrict__ idx, const uint8_t* __restrict__ ivalid, int64_t r,
                                   const int32_t* __restrict__ doff, const uint8_t* __restrict__ dvalid,
                                   int64_t entries, bool& ok, uint32_t& bad) {
  int64_t e;
  const int s = resolve(idx, ivalid, r, entries, e);
  bad += s == 2;
  ok = s == 1 && vbit(dvalid, e);
  if (!ok) return 0;
  const int32_t len = doff[e + 1] - doff[e];
  return len > 0 ? (uint32_t)len : 0u;
}

// lens / ovalid / tiles may be NULL (a sizing call wants words[1] only).
// words[0] += bad indices, words[1] += string bytes.
template <typename T>
__global__ void __launch_bounds__(kDictThreads)
dict_len_kernel(const T* __restrict__ idx, const uint8_t* __restrict__ ivalid, int64_t n,
                const int32_t* __restrict__ doff, const uint8_t* __restrict__ dvalid, int64_t entries,
                int32_t* __restrict__ lens, uint8_t* __restrict__ ovalid, uint32_t* __restrict__ tiles,
                unsigned long long* __restrict__ words) {
  __shared__ unsigned long long s_sum[kDictThreads / 64];
  const int64_t i0 = (int64_t)blockIdx.x * kDictTile + (int64_t)threadIdx.x * kDictPerThread;
  unsigned long long sum = 0;
  uint32_t vbits = 0, bad = 0;
  for (int k = 0; k < kDictPerThread && i0 + k < n; ++k) {
    bool ok;
    const uint32_t len = row_len(idx, ivalid, i0 + k, doff, dvalid, entries, ok, bad);
    if (lens) lens[i0 + k] = (int32_t)len;
    vbits |= (ok ? 1u : 0u) << k;
    sum += len;
  }
  if (ovalid && i0 < n) ovalid[i0 >> 3] = (uint8_t)vbits;
  sum = wave_sum_u64(sum);
  const unsigned long long wbad = wave_sum_u64(bad);
  if ((threadIdx.x & 63) == 0) {
    s_sum[threadIdx.x >> 6] = sum;
    if (wbad) atomicAdd(words, wbad);
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    unsigned long long t = 0;
    for (int k = 0; k < kDictThreads / 64; ++k) t += s_sum[k];
    // (a tile of >= 2^32 bytes: the caller refuses the batch from words[1] before any offset is used)
    if (tiles) tiles[blockIdx.x] = t < 0xFFFFFFFFull ? (uint32_t)t : 0xFFFFFFFFu;
    if (t) atomicAdd(words + 1, t);
  }
}

// off_out[r] holds row r's length on entry (dict_len_kernel) and its offset on return; a block
// reads and writes the entries of its own tile only.  lds_cap > 0: dynamic LDS of that many bytes.
template <typename T>
__global__ void __launch_bounds__(kDictThreads)
dict_copy_kernel(const T* __restrict__ idx, const uint8_t* __restrict__ ivalid, int64_t n,
                 const int32_t* __restrict__ doff, const uint8_t* __restrict__ ddata,
                 const uint8_t* __restrict__ dvalid, int64_t entries,
                 const uint32_t* __restrict__ tile_off, int64_t n_tiles, int32_t* __restrict__ off_out,
                 uint8_t* __restrict__ data_out, int lds_cap) {
  __shared__ uint32_t s_wave[kDictThreads / 64];
  extern __shared__ uint4 s_dict4[];
  uint8_t* const s_dict = reinterpret_cast<uint8_t*>(s_dict4);
  // the dictionary in LDS: offsets re-based to its first byte, then the bytes from the aligned dword
  // that holds that byte (every dword read holds a byte of the dictionary)
  bool staged = false;
  const int32_t* s_off = reinterpret_cast<const int32_t*>(s_dict);
  const uint8_t* s_bytes = nullptr;
  if (lds_cap > 0 && entries > 0) {
    const int64_t first = doff[0], nbytes = (int64_t)doff[entries] - first;
    const int64_t off_bytes = ((entries + 1) * 4 + 15) & ~(int64_t)15;
    const uint32_t sh = (uint32_t)(reinterpret_cast<uintptr_t>(ddata + first) & 3u);
    const int64_t n_words = nbytes > 0 ? (sh + nbytes + 3) >> 2 : 0;
    if (nbytes >= 0 && off_bytes + 4 * n_words <= lds_cap) {  // (block-uniform)
      int32_t* so = reinterpret_cast<int32_t*>(s_dict);
      for (int64_t i = threadIdx.x; i <= entries; i += kDictThreads) so[i] = doff[i] - (int32_t)first;
      const uint32_t* src = reinterpret_cast<const uint32_t*>(ddata + first - sh);
      uint32_t* sw = reinterpret_cast<uint32_t*>(s_dict + off_bytes);
      for (int64_t i = threadIdx.x; i < n_words; i += kDictThreads) sw[i] = src[i];
      s_bytes = s_dict + off_bytes + sh;
      staged = true;
      __syncthreads();
    }
  }
  const int64_t i0 = (int64_t)blockIdx.x * kDictTile + (int64_t)threadIdx.x * kDictPerThread;
  uint32_t len[kDictPerThread], sum = 0;
  for (int k = 0; k < kDictPerThread; ++k) {
    len[k] = i0 + k < n ? (uint32_t)off_out[i0 + k] : 0u;
    sum += len[k];
  }
  uint32_t total;
  uint32_t at = tile_off[blockIdx.x] + block_scan(sum, s_wave, total);
  const int lane = threadIdx.x & 63;
  for (int k = 0; k < kDictPerThread; ++k) {
    const int64_t r = i0 + k;
    int64_t e = 0;
    if (r < n) {
      off_out[r] = (int32_t)at;
      if (len[k]) resolve(idx, ivalid, r, entries, e);  // (a row with bytes named a valid entry)
    }
    const uint32_t L = len[k];
    const int32_t src_off = L ? doff[e] : 0;
    if (L && L < (uint32_t)kDictLongLen) {
      uint8_t* dst = data_out + at;
      if (staged) {
        const uint8_t* src = s_bytes + s_off[e];
        for (uint32_t b = 0; b < L; ++b) dst[b] = src[b];
      } else {
        const uint8_t* src = ddata + src_off;
        for (uint32_t b = 0; b < L; ++b) dst[b] = src[b];
      }
    }
    // long rows of this round: the wave copies each together (every lane reaches the ballot)
    unsigned long long m = __ballot(L >= (uint32_t)kDictLongLen);
    while (m) {
      const int l = __ffsll((long long)m) - 1;
      m &= m - 1;
      const uint32_t wl = (uint32_t)__shfl((int)L, l);
      const uint32_t wat = (uint32_t)__shfl((int)at, l);
      const int32_t wsrc = __shfl(src_off, l);
      const uint8_t* src = ddata + wsrc;
      uint8_t* dst = data_out + wat;
      for (uint32_t b = lane; b < wl; b += 64) dst[b] = src[b];
    }
    at += L;
  }
  if (blockIdx.x == 0 && threadIdx.x == 0) off_out[n] = (int32_t)tile_off[n_tiles];
}

// ------------------------------------------------------------------------------------------------
// Rows per dictionary entry
// ------------------------------------------------------------------------------------------------
// MODE 0: entries <= kDictRegMax, per-lane register counters (every lane of a wave hits the same
//         few entries: no atomics until the wave's sums at the end);
// MODE 1: u32 counters in LDS, `copies` replicas (one per wave while they fit), LDS atomics, one
//         global atomic per non-zero counter at the end of the block;
// MODE 2: 64-bit global atomics on counts.
// words[0] += bad indices, words[1] += NULL indices.
template <typename T, int MODE>
__global__ void __launch_bounds__(kDictThreads)
dict_count_kernel(const T* __restrict__ idx, const uint8_t* __restrict__ valid, int64_t rows,
                  int64_t entries, int copies, unsigned long long* __restrict__ counts,
                  unsigned long long* __restrict__ words) {
  extern __shared__ uint4 s_cnt4[];
  uint32_t* const s_cnt = reinterpret_cast<uint32_t*>(s_cnt4);
  uint32_t* mine = s_cnt;
  if (MODE == 1) {
    for (int64_t i = threadIdx.x; i < entries * copies; i += kDictThreads) s_cnt[i] = 0;
    __syncthreads();
    mine = s_cnt + (int64_t)((threadIdx.x >> 6) % copies) * entries;
  }
  uint32_t reg[kDictRegMax];
#pragma unroll
  for (int j = 0; j < (int)kDictRegMax; ++j) reg[j] = 0;
  unsigned long long bad = 0, nulls = 0;
  const bool vec = (reinterpret_cast<uintptr_t>(idx) & 15u) == 0;
  const int64_t step = (int64_t)gridDim.x * kDictThreads * kCountRows;
  for (int64_t r0 = ((int64_t)blockIdx.x * kDictThreads + threadIdx.x) * kCountRows; r0 < rows; r0 += step) {
    const int m = rows - r0 < kCountRows ? (int)(rows - r0) : kCountRows;
    T v[kCountRows];
    if (vec && m == kCountRows) {  // sizeof(T) 128-bit loads
      uint4 q[sizeof(T)];
      const uint4* src = reinterpret_cast<const uint4*>(idx + r0);
#pragma unroll
      for (int j = 0; j < (int)sizeof(T); ++j) q[j] = src[j];
      __builtin_memcpy(v, q, sizeof(v));
    } else {
#pragma unroll
      for (int k = 0; k < kCountRows; ++k) v[k] = k < m ? idx[r0 + k] : T(0);
    }
    uint32_t vb = 0xFFFFu;
    if (valid) {  // r0 is a multiple of 16: its rows' bits are bytes r0 / 8 and r0 / 8 + 1
      vb = valid[r0 >> 3];
      if (m > 8) vb |= (uint32_t)valid[(r0 >> 3) + 1] << 8;
    }
#pragma unroll
    for (int k = 0; k < kCountRows; ++k) {
      if (k >= m) continue;
      if (!((vb >> k) & 1u)) {
        ++nulls;
        continue;
      }
      const int64_t e = (int64_t)v[k];
      if (e < 0 || e >= entries) {
        ++bad;
        continue;
      }
      if (MODE == 0) {
#pragma unroll
        for (int j = 0; j < (int)kDictRegMax; ++j) reg[j] += e == j ? 1u : 0u;
      } else if (MODE == 1) {
        atomicAdd(&mine[e], 1u);
      } else {
        atomicAdd(&counts[e], 1ull);
      }
    }
  }
  if (MODE == 0) {
#pragma unroll
    for (int j = 0; j < (int)kDictRegMax; ++j) {
      const unsigned long long s = wave_sum_u64(reg[j]);
      if ((threadIdx.x & 63) == 0 && s && j < entries) atomicAdd(&counts[j], s);
    }
  }
  if (MODE == 1) {
    __syncthreads();
    for (int64_t i = threadIdx.x; i < entries; i += kDictThreads) {
      unsigned long long s = 0;
      for (int c = 0; c < copies; ++c) s += s_cnt[(int64_t)c * entries + i];
      if (s) atomicAdd(&counts[i], s);
    }
  }
  bad = wave_sum_u64(bad);
  nulls = wave_sum_u64(nulls);
  if ((threadIdx.x & 63) == 0) {
    if (bad) atomicAdd(words, bad);
    if (nulls) atomicAdd(words + 1, nulls);
  }
}

unsigned blocks_for(int64_t n, int64_t per_block) { return (unsigned)((n + per_block - 1) / per_block); }

int fixed_width(int32_t type) {
  switch (DQ_TYPE_ID(type)) {
    case DQ_INT8: return 1;
    case DQ_INT16: return 2;
    case DQ_INT32: case DQ_FLOAT32: case DQ_DATE32: return 4;
    case DQ_INT64: case DQ_FLOAT64: case DQ_TIMESTAMP_US: return 8;
    case DQ_DECIMAL128: return 16;
    default: return 0;
  }
}

template <typename T>
hipError_t count_typed(const void* indices, const uint8_t* valid, int64_t rows, int64_t entries,
                       unsigned long long* counts, unsigned long long* words, hipStream_t st) {
  const T* idx = static_cast<const T*>(indices);
  const int64_t per_block = (int64_t)kDictThreads * kCountRows;
  const int64_t full = std::min<int64_t>((rows + per_block - 1) / per_block, 2048);
  if (entries <= kDictRegMax) {
    hipLaunchKernelGGL((dict_count_kernel<T, 0>), dim3((unsigned)full), dim3(kDictThreads), 0, st, idx,
                       valid, rows, entries, 1, counts, words);
  } else if (entries <= kDictLdsMax) {
    const int copies = entries <= kDictWaveMax ? kDictThreads / 64 : 1;
    // (a block clears and flushes entries x copies counters: give it at least 8x as many rows)
    const int64_t grid = std::max<int64_t>(1, std::min<int64_t>(full, rows / (8 * entries * copies)));
    hipLaunchKernelGGL((dict_count_kernel<T, 1>), dim3((unsigned)grid), dim3(kDictThreads),
                       (size_t)entries * copies * sizeof(uint32_t), st, idx, valid, rows, entries, copies,
                       counts, words);
  } else {
    hipLaunchKernelGGL((dict_count_kernel<T, 2>), dim3((unsigned)full), dim3(kDictThreads), 0, st, idx,
                       valid, rows, entries, 1, counts, words);
  }
  return hipGetLastError();
}

template <typename T>
dq_status decode_typed(const dq_column* in, const dq_column* dict, dq_column* out, bool sizing,
                       int64_t capacity, int64_t* n_bad, hipStream_t st) {
  const T* idx = static_cast<const T*>(in->values);
  const int64_t n = in->length, entries = dict->length;
  const int tid = DQ_TYPE_ID(dict->type), width = fixed_width(dict->type);
  uint8_t* ovalid = const_cast<uint8_t*>(out->validity);
  DevBuf<unsigned long long> words;
  HIP_TRY(words.ensure(2));
  HIP_TRY(hipMemsetAsync(words.p, 0, 2 * sizeof(unsigned long long), st));
  unsigned long long h[2] = {0, 0};
  if (tid != DQ_UTF8) {
    const unsigned grid = blocks_for((n + 7) / 8, kDictThreads);
    void* ov = const_cast<void*>(out->values);
#define DQ_DECODE_FIXED(V)                                                                        \
  hipLaunchKernelGGL((dict_decode_fixed<T, V>), dim3(grid), dim3(kDictThreads), 0, st, idx,       \
                     in->validity, n, static_cast<const V*>(dict->values), dict->validity, entries, \
                     static_cast<V*>(ov), ovalid, words.p)
    if (tid == DQ_BOOL) {
      hipLaunchKernelGGL((dict_decode_bool<T>), dim3(grid), dim3(kDictThreads), 0, st, idx, in->validity, n,
                         static_cast<const uint8_t*>(dict->values), dict->validity, entries,
                         static_cast<uint8_t*>(ov), ovalid, words.p);
    } else if (width == 1) {
      DQ_DECODE_FIXED(uint8_t);
    } else if (width == 2) {
      DQ_DECODE_FIXED(uint16_t);
    } else if (width == 4) {
      DQ_DECODE_FIXED(uint32_t);
    } else if (width == 8) {
      DQ_DECODE_FIXED(uint64_t);
    } else {
      DQ_DECODE_FIXED(B16);
    }
#undef DQ_DECODE_FIXED
    HIP_TRY(hipGetLastError());
    HIP_TRY(d2h(h, words.p, sizeof(h), st));
    *n_bad = (int64_t)h[0];
    return DQ_OK;
  }
  const int32_t* doff = static_cast<const int32_t*>(dict->values);
  int32_t* off_out = static_cast<int32_t*>(const_cast<void*>(out->values));
  const int64_t n_tiles = (n + kDictTile - 1) / kDictTile;
  DevBuf<uint32_t> tiles;
  HIP_TRY(tiles.ensure((size_t)n_tiles + 1));
  hipLaunchKernelGGL((dict_len_kernel<T>), dim3((unsigned)n_tiles), dim3(kDictThreads), 0, st, idx,
                     in->validity, n, doff, dict->validity, entries, sizing ? nullptr : off_out,
                     sizing ? nullptr : ovalid, tiles.p, words.p);
  HIP_TRY(hipGetLastError());
  HIP_TRY(d2h(h, words.p, sizeof(h), st));
  *n_bad = (int64_t)h[0];
  if (h[1] >= (1ull << 31))
    return fail(DQ_ERR_UNSUPPORTED, "dq_dict_decode: the %lld rows decode to %llu string bytes (int32 "
                "offsets hold fewer than 2^31: import the column in smaller batches)", (long long)n, h[1]);
  if (sizing) {
    out->data_bytes = (int32_t)h[1];
    return DQ_OK;
  }
  if ((int64_t)h[1] > capacity)
    return fail(DQ_ERR_INVALID_ARGUMENT, "dq_dict_decode: %llu string bytes, out->data holds %lld", h[1],
                (long long)capacity);
  HIP_TRY(launch_tile_scan(tiles.p, n_tiles, st));
  // LDS staging when the dictionary can fit: its offsets, its bytes (data_bytes bounds them) and
  // the alignment slack; the kernel decides from the offsets themselves
  int lds = 0;
  if (entries > 0 && dict->data_bytes > 0 &&
      (((entries + 1) * 4 + 15) & ~(int64_t)15) <= kDictLdsBytes - 8)
    lds = kDictLdsBytes;
  hipLaunchKernelGGL((dict_copy_kernel<T>), dim3((unsigned)n_tiles), dim3(kDictThreads), (size_t)lds, st, idx,
                     in->validity, n, doff, dict->data, dict->validity, entries, tiles.p, n_tiles, off_out,
                     const_cast<uint8_t*>(out->data), lds);
  HIP_TRY(hipGetLastError());
  out->data_bytes = (int32_t)h[1];
  HIP_TRY(hipStreamSynchronize(st));
  return DQ_OK;
}

}  // namespace

bool dict_index_type_ok(int index_type) { return index_type >= DQ_INDEX_INT8 && index_type <= DQ_INDEX_UINT64; }

hipError_t launch_dict_count(const void* indices, int index_type, const uint8_t* valid, int64_t rows,
                             int64_t entries, unsigned long long* counts, unsigned long long* words,
                             hipStream_t st) {
  if (rows <= 0) return hipSuccess;
  switch (index_type) {
    case DQ_INDEX_INT8: return count_typed<int8_t>(indices, valid, rows, entries, counts, words, st);
    case DQ_INDEX_UINT8: return count_typed<uint8_t>(indices, valid, rows, entries, counts, words, st);
    case DQ_INDEX_INT16: return count_typed<int16_t>(indices, valid, rows, entries, counts, words, st);
    case DQ_INDEX_UINT16: return count_typed<uint16_t>(indices, valid, rows, entries, counts, words, st);
    case DQ_INDEX_INT32: return count_typed<int32_t>(indices, valid, rows, entries, counts, words, st);
    case DQ_INDEX_UINT32: return count_typed<uint32_t>(indices, valid, rows, entries, counts, words, st);
    case DQ_INDEX_INT64: return count_typed<int64_t>(indices, valid, rows, entries, counts, words, st);
    case DQ_INDEX_UINT64: return count_typed<uint64_t>(indices, valid, rows, entries, counts, words, st);
    default: return hipErrorInvalidValue;
  }
}

}  // namespace dq

using namespace dq;

extern "C" dq_status dq_dict_decode(const dq_column* indices, int index_type, const dq_column* dictionary,
                                    dq_column* out, int64_t* n_bad_index, void* hip_stream) {
  if (!indices || !dictionary || !out || !n_bad_index)
    return fail(DQ_ERR_INVALID_ARGUMENT, "dq_dict_decode: null argument");
  *n_bad_index = 0;
  if (!dict_index_type_ok(index_type))
    return fail(DQ_ERR_INVALID_ARGUMENT, "dq_dict_decode: index type %d", index_type);
  const int64_t n = indices->length, entries = dictionary->length;
  if (n < 0 || entries < 0) return fail(DQ_ERR_INVALID_ARGUMENT, "dq_dict_decode: negative length");
  if (n > kDictMaxRows || entries > kDictMaxRows)
    return fail(DQ_ERR_UNSUPPORTED, "dq_dict_decode: more than 2^31-1 rows or entries");
  const int tid = DQ_TYPE_ID(dictionary->type);
  if (!fixed_width(dictionary->type) && tid != DQ_BOOL && tid != DQ_UTF8)
    return fail(DQ_ERR_WRONG_TYPE, "dq_dict_decode: dictionary type %d", dictionary->type);
  if (out->type != dictionary->type)
    return fail(DQ_ERR_WRONG_TYPE, "dq_dict_decode: out is of another type than the dictionary");
  const bool sizing = tid == DQ_UTF8 && !out->data;
  if (!sizing && !out->values) return fail(DQ_ERR_INVALID_ARGUMENT, "dq_dict_decode: null output buffers");
  if (!sizing && !out->validity && (indices->validity || dictionary->validity))
    return fail(DQ_ERR_INVALID_ARGUMENT, "dq_dict_decode: out needs a validity buffer when the indices "
                                         "or the dictionary have one");
  if (n && !indices->values) return fail(DQ_ERR_INVALID_ARGUMENT, "dq_dict_decode: null indices");
  if (entries && (!dictionary->values || (tid == DQ_UTF8 && !dictionary->data)))
    return fail(DQ_ERR_INVALID_ARGUMENT, "dq_dict_decode: null dictionary buffers");
  hipStream_t st = reinterpret_cast<hipStream_t>(hip_stream);
  const int64_t capacity = out->data_bytes;
  out->length = n;
  out->data_bytes = 0;
  if (n == 0) {
    if (tid == DQ_UTF8 && !sizing) HIP_TRY(hipMemsetAsync(const_cast<void*>(out->values), 0, sizeof(int32_t), st));
    HIP_TRY(hipStreamSynchronize(st));
    return DQ_OK;
  }
  switch (index_type) {
    case DQ_INDEX_INT8: return decode_typed<int8_t>(indices, dictionary, out, sizing, capacity, n_bad_index, st);
    case DQ_INDEX_UINT8: return decode_typed<uint8_t>(indices, dictionary, out, sizing, capacity, n_bad_index, st);
    case DQ_INDEX_INT16: return decode_typed<int16_t>(indices, dictionary, out, sizing, capacity, n_bad_index, st);
    case DQ_INDEX_UINT16: return decode_typed<uint16_t>(indices, dictionary, out, sizing, capacity, n_bad_index, st);
    case DQ_INDEX_INT32: return decode_typed<int32_t>(indices, dictionary, out, sizing, capacity, n_bad_index, st);
    case DQ_INDEX_UINT32: return decode_typed<uint32_t>(indices, dictionary, out, sizing, capacity, n_bad_index, st);
    case DQ_INDEX_INT64: return decode_typed<int64_t>(indices, dictionary, out, sizing, capacity, n_bad_index, st);
    default: return decode_typed<uint64_t>(indices, dictionary, out, sizing, capacity, n_bad_index, st);
  }
}
