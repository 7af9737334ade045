// rowschema.hip -- RowLevelSchemaValidator on the device (schema/RowLevelSchemaValidator.scala:
// validate 183-206, extractAndCastValidRows 208-223, toCNF 225-281) and the row selection it needs.
//
// Evaluate: one launch per declared column, one lane per row.  A launch ORs the column's clauses
// into two row bitmaps (any clause FALSE, any clause NULL; one uint64 word per 64 rows, built with a
// ballot, so the launches of one call -- stream-ordered -- need no atomics) and writes the column's
// cast (Spark 2.2 Cast of a string to IntegerType / DecimalType(p, s), unix_timestamp(v, mask) cast
// to TimestampType) and its validity for every row, so a string is parsed once.  The regex clause
// of a string column reuses launch_regex (expr.hip) and its fused automaton table.  A last launch
// turns the two bitmaps into the Kleene verdict: valid = ~(false | null), invalid = false.
//
// Select (dq_select_plan): per-tile popcounts of a keep bitmap, an exclusive scan of the tile
// counts, then the stable index list src_row[out_pos].  Gather (dq_gather_column): one lane per
// output row reading through the index list; bit-packed buffers are balloted per output word, utf8
// offsets come from the same three-phase scan over the gathered lengths.  The scans are three
// separate launches (count, scan of counts, write): no workgroup ever waits on another.
#include <hip/hip_runtime.h>
#include <string.h>

#include <algorithm>
#include <string>
#include <vector>

#include "device_util.h"
#include "engine.h"
#include "kernels.h"

namespace dq {
namespace {

constexpr int kTileWords = DQ_SELECT_TILE_ROWS / 64;  // one bitmap word per thread of a block
static_assert(kTileWords == kBlock, "a selection tile is one bitmap word per thread");
constexpr int kLenPerThread = 8;                      // utf8 offsets: rows per thread ...
constexpr int kLenTile = kBlock * kLenPerThread;      // ... and per block
constexpr int kMaskTokMax = 48;
constexpr int64_t kMaxRows = 2147483647;

// ------------------------------------------------------------------------------------------------
// Per-value semantics
// ------------------------------------------------------------------------------------------------
DQ_HD bool is_digit(uint8_t b) { return b >= '0' && b <= '9'; }

// Spark 2.2 UTF8String.toInt: the int32 sibling of spark_to_long (cast.hip).  Optional sign, digits,
// optionally '.' and digits (truncated); no trimming; overflow, "", a lone sign or any other byte
// -> false (NULL).
DQ_HD bool spark_to_int(const uint8_t* s, int32_t n, int32_t& out) {
  if (n == 0) return false;
  int32_t i = 0;
  const bool neg = s[0] == '-';
  if (neg || s[0] == '+') {
    if (n == 1) return false;
    i = 1;
  }
  const int64_t stop = INT32_MIN / 10;
  int64_t r = 0;  // accumulated negatively, in 64 bits: below INT32_MIN is Java's wrapped `result > 0`
  for (; i < n; ++i) {
    const uint8_t b = s[i];
    if (b == '.') {
      ++i;
      break;
    }
    if (!is_digit(b)) return false;
    if (r < stop) return false;
    r = r * 10 - (int64_t)(b - '0');
    if (r < INT32_MIN) return false;
  }
  for (; i < n; ++i)
    if (!is_digit(s[i])) return false;
  if (!neg) {
    if (r == INT32_MIN) return false;
    r = -r;
  }
  out = (int32_t)r;
  return true;
}

// new java.math.BigDecimal(s) then Decimal.changePrecision(p, sc) with ROUND_HALF_UP (Spark 2.2
// Cast.castToDecimal): [+-]? (digits [. digits?] | . digits) ([eE] [+-]? digits)?, ASCII digits only.
// 0 = NULL (outside the grammar, or the rounded |unscaled| >= 10^p), 1 = value, 2 = not decided here
// (a byte >= 0x80: Java reads Unicode digits; an exponent field of more than 4 digits).
DQ_HD int java_to_decimal(const uint8_t* s, int32_t n, int p, int sc, uint64_t& lo, int64_t& hi) {
  for (int32_t j = 0; j < n; ++j)
    if (s[j] >= 0x80) return 2;
  int32_t i = 0;
  bool neg = false;
  if (i < n && (s[i] == '+' || s[i] == '-')) {
    neg = s[i] == '-';
    ++i;
  }
  const int32_t m0 = i;
  int32_t nint = 0, nfrac = 0;
  for (; i < n && is_digit(s[i]); ++i) ++nint;
  if (i < n && s[i] == '.') {
    ++i;
    for (; i < n && is_digit(s[i]); ++i) ++nfrac;
  }
  if (nint + nfrac == 0) return 0;
  const int32_t m1 = i;
  int64_t e = 0;
  if (i < n) {
    if (s[i] != 'e' && s[i] != 'E') return 0;
    ++i;
    bool eneg = false;
    if (i < n && (s[i] == '+' || s[i] == '-')) {
      eneg = s[i] == '-';
      ++i;
    }
    int32_t ne = 0;
    for (; i < n && is_digit(s[i]); ++i) {
      ++ne;
      if (ne <= 4) e = e * 10 + (s[i] - '0');
    }
    if (ne == 0 || i < n) return 0;
    if (ne > 4) return 2;
    if (eneg) e = -e;
  }
  // significant digits d_0 .. d_(m-1): the mantissa's digits from its first non-zero one
  int32_t first = m0;
  while (first < m1 && (s[first] == '0' || s[first] == '.')) ++first;
  int64_t m = 0;
  for (int32_t j = first; j < m1; ++j) m += s[j] != '.';
  lo = 0;
  hi = 0;
  if (m == 0) return 1;
  // unscaled = d_0 .. d_(m-1) x 10^k: its integer part has ni = m + k digits, d_ni rounds it
  const int64_t k = e - nfrac + sc;
  const int64_t ni = m + k;
  if (ni > 38) return 0;  // >= 10^38 >= 10^p
  unsigned __int128 u = 0;
  int round_digit = 0;
  int64_t t = 0;
  for (int32_t j = first; j < m1 && t <= ni; ++j) {
    if (s[j] == '.') continue;
    if (t < ni) u = u * 10 + (unsigned)(s[j] - '0');
    else round_digit = s[j] - '0';
    ++t;
  }
  for (int64_t z = m; z < ni; ++z) u *= 10;
  if (round_digit >= 5) u += 1;
  unsigned __int128 bound = 1;
  for (int z = 0; z < p; ++z) bound *= 10;
  if (u >= bound) return 0;
  if (neg) u = (unsigned __int128)0 - u;
  lo = (uint64_t)u;
  hi = (int64_t)(uint64_t)(u >> 64);
  return 1;
}

// Proleptic Gregorian day count since 1970-01-01 (civil_from_days' inverse, decimal.h).
DQ_HD int64_t days_from_civil(int64_t y, int m, int d) {
  y -= m <= 2;
  const int64_t era = (y >= 0 ? y : y - 399) / 400;
  const int64_t yoe = y - era * 400;
  const int64_t doy = (153 * (m + (m > 2 ? -3 : 9)) + 2) / 5 + d - 1;
  const int64_t doe = yoe * 365 + yoe / 4 - yoe / 100 + doy;
  return era * 146097 + doe - 719468;
}

// unix_timestamp(v, mask).cast(TimestampType) over a compiled mask: tok[2 t] = 0 for a literal byte
// tok[2 t + 1], or 1..6 for the field yyyy MM dd HH mm ss of width tok[2 t + 1].
// 1 = strict form, converted (UTC); 0 = SimpleDateFormat's lenient parse must fail too; 2 = a form
// the lenient parse may read (short / long digit runs, rolled-over fields, trailing text, signs,
// blanks, years before 1583): not decided here.  The walk goes on while the lenient parser's
// position is known (every field so far had exactly its width in digits), so a later definite
// failure still gives 0; out-of-range fields are judged after it.
DQ_HD int parse_timestamp(const uint8_t* s, int32_t n, const uint8_t* tok, int n_tok,
                          int64_t& micros) {
  int32_t pos = 0;
  int32_t yy = 1970, mo = 1, dd = 1, hh = 0, mi = 0, ss = 0;
  for (int t = 0; t < n_tok; ++t) {
    const int ty = tok[2 * t], v = tok[2 * t + 1];
    if (pos >= n) return 0;
    const uint8_t b = s[pos];
    if (ty == 0) {
      if (b != v) return (b == ' ' || b == '\t' || v == ' ' || v == '\t') ? 2 : 0;
      ++pos;
      continue;
    }
    if (!is_digit(b)) return (b == '+' || b == '-' || b == ' ' || b == '\t' || b >= 0x80) ? 2 : 0;
    int32_t val = 0;
    for (int k = 0; k < v; ++k) {
      if (pos + k >= n || !is_digit(s[pos + k])) return 2;
      val = val * 10 + (s[pos + k] - '0');
    }
    pos += v;
    const bool abuts = t + 1 < n_tok && tok[2 * (t + 1)] != 0;
    if (!abuts && pos < n && is_digit(s[pos])) return 2;
    switch (ty) {
      case 1: yy = val; break;
      case 2: mo = val; break;
      case 3: dd = val; break;
      case 4: hh = val; break;
      case 5: mi = val; break;
      default: ss = val; break;
    }
  }
  if (pos < n) return 2;
  if (yy < 1583 || yy > 9999 || mo < 1 || mo > 12 || dd < 1 || hh > 23 || mi > 59 || ss > 59) return 2;
  const bool leap = (yy % 4 == 0 && yy % 100 != 0) || yy % 400 == 0;
  const int dim = mo == 2 ? (leap ? 29 : 28) : ((mo == 4 || mo == 6 || mo == 9 || mo == 11) ? 30 : 31);
  if (dd > dim) return 2;
  micros = ((days_from_civil(yy, mo, dd) * 24 + hh) * 60 + mi) * 60 * 1000000LL + ss * 1000000LL;
  return 1;
}

// Spark's length(): characters = bytes that are not UTF-8 continuation bytes (0x80-0xBF).
DQ_HD int32_t utf8_chars(const uint8_t* s, int32_t n) {
  int32_t c = 0;
  for (int32_t j = 0; j < n; ++j) c += (s[j] & 0xC0) != 0x80;
  return c;
}

// ------------------------------------------------------------------------------------------------
// Evaluate
// ------------------------------------------------------------------------------------------------
struct EvalArgs {
  int32_t kind, nullable, has_min, has_max, min, max, precision, scale;
  const uint8_t* valid;
  const int32_t* off;
  const uint8_t* data;
  const uint64_t* rx_val;  // string column with a regex: launch_regex's truth words, else nullptr
  void* cast_values;
  uint64_t* cast_valid;
  int32_t n_tok, pad;
  uint8_t tok[2 * kMaskTokMax];
};

__global__ void __launch_bounds__(kBlock)
schema_eval_kernel(const EvalArgs a, int64_t rows, uint64_t* __restrict__ any_null,
                   uint64_t* __restrict__ any_false, unsigned long long* __restrict__ n_bad) {
  const int lane = threadIdx.x & 63;
  const int64_t wave = ((int64_t)blockIdx.x * kBlock + threadIdx.x) >> 6;
  const int64_t n_waves = ((int64_t)gridDim.x * kBlock) >> 6;
  const int64_t n_words = (rows + 63) >> 6;
  for (int64_t w = wave; w < n_words; w += n_waves) {
    const int64_t r = w * 64 + lane;
    bool f = false, nl = false, cv = false, bad = false;
    if (r < rows) {
      const bool isnull = !bit1(a.valid, r);
      if (!a.nullable && isnull) f = true;  // toCNF :230-232
      const int32_t s = isnull ? 0 : a.off[r], len = isnull ? 0 : a.off[r + 1] - s;
      const uint8_t* p = a.data + s;
      switch (a.kind) {
        case DQ_SCHEMA_INT: {  // :238-251
          int32_t v = 0;
          if (!isnull) {
            cv = spark_to_int(p, len, v);
            if (!cv) f = true;
            else if ((a.has_max && v > a.max) || (a.has_min && v < a.min)) f = true;
          } else if (a.has_min) {
            nl = true;  // :246 `colIsNull.isNull` is always false: false OR (NULL >= min) = NULL
          }
          static_cast<int32_t*>(a.cast_values)[r] = cv ? v : 0;
          break;
        }
        case DQ_SCHEMA_DECIMAL: {  // :253-256
          uint64_t lo = 0;
          int64_t hi = 0;
          if (!isnull) {
            const int res = java_to_decimal(p, len, a.precision, a.scale, lo, hi);
            cv = res == 1;
            bad = res == 2;
            if (!cv) f = true;
          }
          uint64_t* o = static_cast<uint64_t*>(a.cast_values) + 2 * r;
          o[0] = cv ? lo : 0;
          o[1] = cv ? (uint64_t)hi : 0;
          break;
        }
        case DQ_SCHEMA_TIMESTAMP: {  // :273-276
          int64_t us = 0;
          if (!isnull) {
            const int res = parse_timestamp(p, len, a.tok, a.n_tok, us);
            cv = res == 1;
            bad = res == 2;
            if (!cv) f = true;
          }
          static_cast<int64_t*>(a.cast_values)[r] = cv ? us : 0;
          break;
        }
        default: {  // DQ_SCHEMA_STRING :258-271
          if (!isnull) {
            if (a.has_min || a.has_max) {
              const int32_t c = utf8_chars(p, len);
              if ((a.has_min && c < a.min) || (a.has_max && c > a.max)) f = true;
            }
            if (a.rx_val && !((a.rx_val[w] >> lane) & 1ull)) f = true;
          }
          break;
        }
      }
    }
    const uint64_t bf = __ballot(f), bn = __ballot(nl), bc = __ballot(cv), bb = __ballot(bad);
    if (lane == 0) {
      if (bf) any_false[w] |= bf;
      if (bn) any_null[w] |= bn;
      if (a.cast_valid) a.cast_valid[w] = bc;
      if (bb) atomicAdd(n_bad, (unsigned long long)__popcll(bb));
    }
  }
}

DQ_DEV uint64_t tail_mask(int64_t w, int64_t rows) {  // the bits of word w that are rows
  const int64_t left = rows - w * 64;
  return left >= 64 ? ~0ull : (left <= 0 ? 0ull : ((1ull << left) - 1));
}

DQ_DEV uint32_t wave_sum(uint32_t v) {
  for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d);
  return v;
}

// in: valid = any clause NULL, invalid = any clause FALSE.  out: the verdicts; counts[0..1] += rows.
__global__ void __launch_bounds__(kBlock)
schema_verdict_kernel(uint64_t* __restrict__ valid, uint64_t* __restrict__ invalid, int64_t rows,
                      unsigned long long* __restrict__ counts) {
  const int64_t w = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  const int64_t n_words = (rows + 63) >> 6;
  uint64_t v = 0, f = 0;
  if (w < n_words) {
    const uint64_t m = tail_mask(w, rows);
    f = invalid[w] & m;
    v = ~(f | valid[w]) & m;
    valid[w] = v;
    invalid[w] = f;
  }
  const uint32_t cv = wave_sum((uint32_t)__popcll(v)), cf = wave_sum((uint32_t)__popcll(f));
  if ((threadIdx.x & 63) == 0) {
    if (cv) atomicAdd(counts, (unsigned long long)cv);
    if (cf) atomicAdd(counts + 1, (unsigned long long)cf);
  }
}

// ------------------------------------------------------------------------------------------------
// Three-phase exclusive scan: per-tile counts, this single-block scan of them, then a write launch
// ------------------------------------------------------------------------------------------------
// Exclusive prefix of v over the block's threads and the block's total; every thread calls it.
DQ_DEV uint32_t block_excl_scan(uint32_t v, uint32_t* lds /* kBlock / 64 words */, uint32_t& total) {
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
  for (int k = 0; k < kBlock / 64; ++k) {
    const uint32_t x = lds[k];
    if (k < wv) base += x;
    total += x;
  }
  __syncthreads();
  return base + inc - v;
}

// tiles[0 .. n) counts -> exclusive offsets in place, tiles[n] = the total.  One block.
__global__ void __launch_bounds__(kBlock) tile_scan_kernel(uint32_t* __restrict__ tiles, int64_t n) {
  __shared__ uint32_t lds[kBlock / 64];
  uint32_t carry = 0;
  for (int64_t base = 0; base < n; base += kBlock) {
    const int64_t i = base + threadIdx.x;
    const uint32_t v = i < n ? tiles[i] : 0;
    uint32_t total;
    const uint32_t ex = block_excl_scan(v, lds, total);
    if (i < n) tiles[i] = carry + ex;
    carry += total;
  }
  if (threadIdx.x == 0) tiles[n] = carry;
}

// ------------------------------------------------------------------------------------------------
// Select
// ------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(kBlock)
select_count_kernel(const uint64_t* __restrict__ bitmap, int64_t rows, uint32_t* __restrict__ tiles) {
  __shared__ uint32_t lds[kBlock / 64];
  const int64_t w = (int64_t)blockIdx.x * kTileWords + threadIdx.x;
  const int64_t n_words = (rows + 63) >> 6;
  const uint64_t word = w < n_words ? bitmap[w] & tail_mask(w, rows) : 0;
  uint32_t total;
  block_excl_scan((uint32_t)__popcll(word), lds, total);
  if (threadIdx.x == 0) tiles[blockIdx.x] = total;
}

__global__ void __launch_bounds__(kBlock)
select_write_kernel(const uint64_t* __restrict__ bitmap, int64_t rows,
                    const uint32_t* __restrict__ tile_off, int32_t* __restrict__ index) {
  __shared__ uint32_t lds[kBlock / 64];
  __shared__ uint64_t words[kTileWords];
  __shared__ uint32_t base[kTileWords];
  const int64_t w0 = (int64_t)blockIdx.x * kTileWords;
  const int64_t n_words = (rows + 63) >> 6;
  const int64_t w = w0 + threadIdx.x;
  const uint64_t word = w < n_words ? bitmap[w] & tail_mask(w, rows) : 0;
  uint32_t total;
  const uint32_t ex = block_excl_scan((uint32_t)__popcll(word), lds, total);
  words[threadIdx.x] = word;
  base[threadIdx.x] = ex;
  __syncthreads();
  const int lane = threadIdx.x & 63;
  const int64_t out0 = tile_off[blockIdx.x];
  for (int j = threadIdx.x >> 6; j < kTileWords; j += kBlock / 64) {
    const uint64_t x = words[j];
    if (!((x >> lane) & 1ull)) continue;
    const int rank = __popcll(x & ((1ull << lane) - 1));  // set bits of the lanes below
    index[out0 + base[j] + rank] = (int32_t)((w0 + j) * 64 + lane);
  }
}

// Σ of the selected rows' byte lengths of one utf8 column.
__global__ void __launch_bounds__(kBlock)
select_bytes_kernel(const int32_t* __restrict__ off, int64_t in_rows, const int32_t* __restrict__ index,
                    int64_t n, unsigned long long* __restrict__ total) {
  unsigned long long sum = 0;
  for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += (int64_t)gridDim.x * kBlock) {
    const int64_t s = index[i];
    if (s >= 0 && s < in_rows) sum += (unsigned long long)(off[s + 1] - off[s]);
  }
  for (int d = 32; d >= 1; d >>= 1) sum += __shfl_xor(sum, d);
  if ((threadIdx.x & 63) == 0 && sum) atomicAdd(total, sum);
}

// ------------------------------------------------------------------------------------------------
// Gather (an index outside [0, in_rows) reads nothing and yields zero / NULL / the empty string)
// ------------------------------------------------------------------------------------------------
struct B16 {
  uint64_t a, b;
};

template <typename T>
__global__ void __launch_bounds__(kBlock)
gather_fixed_kernel(const T* __restrict__ in, int64_t in_rows, const int32_t* __restrict__ index,
                    int64_t n, T* __restrict__ out) {
  const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (i >= n) return;
  const int64_t s = index[i];
  out[i] = s >= 0 && s < in_rows ? in[s] : T{};
}

// Bit-packed source (validity, boolean values): the bit of each output row, balloted into the
// output word -- no two waves share an output word.
__global__ void __launch_bounds__(kBlock)
gather_bits_kernel(const uint8_t* __restrict__ in, int64_t in_rows, const int32_t* __restrict__ index,
                   int64_t n, uint64_t* __restrict__ out) {
  const int lane = threadIdx.x & 63;
  const int64_t w = ((int64_t)blockIdx.x * kBlock + threadIdx.x) >> 6;
  if (w >= (n + 63) >> 6) return;  // wave-uniform
  const int64_t i = w * 64 + lane;
  bool b = false;
  if (i < n) {
    const int64_t s = index[i];
    b = s >= 0 && s < in_rows && ((in[s >> 3] >> (s & 7)) & 1u);
  }
  const uint64_t word = __ballot(b);
  if (lane == 0) out[w] = word;
}

DQ_DEV uint32_t gathered_len(const int32_t* off, int64_t in_rows, const int32_t* index, int64_t i,
                             int64_t n) {
  if (i >= n) return 0;
  const int64_t s = index[i];
  return s >= 0 && s < in_rows ? (uint32_t)(off[s + 1] - off[s]) : 0u;
}

__global__ void __launch_bounds__(kBlock)
utf8_count_kernel(const int32_t* __restrict__ off, int64_t in_rows, const int32_t* __restrict__ index,
                  int64_t n, uint32_t* __restrict__ tiles) {
  __shared__ uint32_t lds[kBlock / 64];
  const int64_t i0 = (int64_t)blockIdx.x * kLenTile + (int64_t)threadIdx.x * kLenPerThread;
  uint32_t sum = 0;
  for (int k = 0; k < kLenPerThread; ++k) sum += gathered_len(off, in_rows, index, i0 + k, n);
  uint32_t total;
  block_excl_scan(sum, lds, total);
  if (threadIdx.x == 0) tiles[blockIdx.x] = total;
}

__global__ void __launch_bounds__(kBlock)
utf8_offsets_kernel(const int32_t* __restrict__ off, int64_t in_rows, const int32_t* __restrict__ index,
                    int64_t n, const uint32_t* __restrict__ tile_off, int64_t n_tiles,
                    int32_t* __restrict__ off_out) {
  __shared__ uint32_t lds[kBlock / 64];
  const int64_t i0 = (int64_t)blockIdx.x * kLenTile + (int64_t)threadIdx.x * kLenPerThread;
  uint32_t len[kLenPerThread], sum = 0;
  for (int k = 0; k < kLenPerThread; ++k) {
    len[k] = gathered_len(off, in_rows, index, i0 + k, n);
    sum += len[k];
  }
  uint32_t total;
  uint32_t at = tile_off[blockIdx.x] + block_excl_scan(sum, lds, total);
  for (int k = 0; k < kLenPerThread; ++k) {
    if (i0 + k < n) off_out[i0 + k] = (int32_t)at;
    at += len[k];
  }
  if (blockIdx.x == 0 && threadIdx.x == 0) off_out[n] = (int32_t)tile_off[n_tiles];
}

__global__ void __launch_bounds__(kBlock)
utf8_copy_kernel(const int32_t* __restrict__ off, const uint8_t* __restrict__ data, int64_t in_rows,
                 const int32_t* __restrict__ index, int64_t n, const int32_t* __restrict__ off_out,
                 uint8_t* __restrict__ data_out) {
  const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (i >= n) return;
  const int64_t s = index[i];
  if (s < 0 || s >= in_rows) return;
  const uint8_t* src = data + off[s];
  uint8_t* dst = data_out + off_out[i];
  const int32_t len = off_out[i + 1] - off_out[i];
  for (int32_t k = 0; k < len; ++k) dst[k] = src[k];
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

}  // namespace

hipError_t launch_tile_scan(uint32_t* tiles, int64_t n, hipStream_t stream) {
  hipLaunchKernelGGL(tile_scan_kernel, dim3(1), dim3(kBlock), 0, stream, tiles, n);
  return hipGetLastError();
}

}  // namespace dq

using namespace dq;

extern "C" dq_status dq_schema_evaluate(const dq_schema_column* defs, int n_defs, const dq_column* cols,
                                        int n_cols, int64_t rows, uint64_t* valid_bitmap,
                                        uint64_t* invalid_bitmap, int64_t* n_valid, int64_t* n_invalid,
                                        int64_t* n_unsupported, void* hip_stream) {
  if (n_defs < 0 || n_cols < 0 || rows < 0 || (n_defs && (!defs || !n_unsupported)) ||
      (n_cols && !cols) || !n_valid || !n_invalid)
    return fail(DQ_ERR_INVALID_ARGUMENT, "dq_schema_evaluate: null or negative argument");
  if (rows > kMaxRows)
    return fail(DQ_ERR_UNSUPPORTED, "dq_schema_evaluate: a batch of %lld rows (at most 2^31-1)",
                (long long)rows);
  *n_valid = *n_invalid = 0;
  std::vector<EvalArgs> args((size_t)n_defs);
  struct Rx {
    std::vector<uint8_t> tab;
    int ns = 0, start = 0;
  };
  std::vector<Rx> rx((size_t)n_defs);
  std::vector<char> seen((size_t)n_cols, 0);
  for (int d = 0; d < n_defs; ++d) {
    const dq_schema_column& c = defs[d];
    n_unsupported[d] = 0;
    if (c.kind < DQ_SCHEMA_STRING || c.kind > DQ_SCHEMA_TIMESTAMP)
      return fail(DQ_ERR_INVALID_ARGUMENT, "schema column %d: kind %d", d, c.kind);
    if (c.column < 0 || c.column >= n_cols)
      return fail(DQ_ERR_NO_SUCH_COLUMN, "schema column %d: no input column %d", d, c.column);
    if (seen[c.column]++)
      return fail(DQ_ERR_INVALID_ARGUMENT, "input column %d is declared twice", c.column);
    const dq_column& in = cols[c.column];
    if (in.type != DQ_UTF8)
      return fail(DQ_ERR_WRONG_TYPE, "schema column %d: input column %d is not utf8", d, c.column);
    if (in.length != rows)
      return fail(DQ_ERR_INVALID_ARGUMENT, "schema column %d: input column %d has %lld rows, not %lld",
                  d, c.column, (long long)in.length, (long long)rows);
    if (rows && (!in.values || !in.data))
      return fail(DQ_ERR_INVALID_ARGUMENT, "schema column %d: null column buffers", d);
    EvalArgs& a = args[d];
    memset(&a, 0, sizeof(a));
    a.kind = c.kind;
    a.nullable = c.is_nullable != 0;
    a.valid = in.validity;
    a.off = static_cast<const int32_t*>(in.values);
    a.data = in.data;
    if (c.kind == DQ_SCHEMA_STRING || c.kind == DQ_SCHEMA_INT) {
      a.has_min = c.has_min != 0;
      a.has_max = c.has_max != 0;
      a.min = c.min_value;
      a.max = c.max_value;
    }
    if (c.kind == DQ_SCHEMA_DECIMAL) {
      if (c.precision < 1 || c.precision > 38 || c.scale < 0 || c.scale > c.precision)
        return fail(DQ_ERR_INVALID_ARGUMENT, "schema column %d: decimal(%d,%d)", d, c.precision, c.scale);
      a.precision = c.precision;
      a.scale = c.scale;
    }
    if (c.kind == DQ_SCHEMA_TIMESTAMP) {
      if (!c.mask || c.mask_tokens < 1 || c.mask_tokens > kMaskTokMax)
        return fail(DQ_ERR_INVALID_ARGUMENT, "schema column %d: a mask of 1 .. %d tokens", d, kMaskTokMax);
      uint32_t fields = 0;
      for (int t = 0; t < c.mask_tokens; ++t) {
        const int ty = c.mask[2 * t], v = c.mask[2 * t + 1];
        const int width = ty == 1 ? 4 : 2;
        if (ty > 6 || (ty && (v != width || (fields >> ty) & 1u)) ||
            (!ty && (v >= 0x80 || is_digit((uint8_t)v))))
          return fail(DQ_ERR_INVALID_ARGUMENT, "schema column %d: mask token %d", d, t);
        if (ty) fields |= 1u << ty;
      }
      a.n_tok = c.mask_tokens;
      memcpy(a.tok, c.mask, 2 * (size_t)c.mask_tokens);
    }
    if (c.kind != DQ_SCHEMA_STRING) {
      if (rows && (!c.cast_values || !c.cast_validity))
        return fail(DQ_ERR_INVALID_ARGUMENT, "schema column %d: null cast staging", d);
      a.cast_values = c.cast_values;
      a.cast_valid = c.cast_validity;
    } else if (c.regex) {
      if (c.regex_bytes < 16 + 256)
        return fail(DQ_ERR_INVALID_ARGUMENT, "schema column %d: truncated automaton", d);
      int32_t ns = 0;
      memcpy(&ns, c.regex, 4);
      if (ns > kRegexMaxStates)
        return fail(DQ_ERR_UNSUPPORTED, "schema column %d: an automaton of %d states (at most %d)", d, ns,
                    kRegexMaxStates);
      const std::string blob(reinterpret_cast<const char*>(c.regex), (size_t)c.regex_bytes);
      if (!build_regex_table(blob, 0, rx[d].tab, &rx[d].ns, &rx[d].start))
        return fail(DQ_ERR_INVALID_ARGUMENT, "schema column %d: malformed automaton", d);
      rx[d].tab.resize((rx[d].tab.size() + 15) / 16 * 16, 0);
    }
  }
  if (rows == 0) return DQ_OK;
  if (!valid_bitmap || !invalid_bitmap)
    return fail(DQ_ERR_INVALID_ARGUMENT, "dq_schema_evaluate: null bitmaps");
  hipStream_t st = reinterpret_cast<hipStream_t>(hip_stream);
  const int64_t n_words = (rows + 63) / 64;
  HIP_TRY(hipMemsetAsync(valid_bitmap, 0, (size_t)n_words * 8, st));
  HIP_TRY(hipMemsetAsync(invalid_bitmap, 0, (size_t)n_words * 8, st));
  DevBuf<unsigned long long> cnt;
  HIP_TRY(cnt.ensure((size_t)n_defs + 2));
  HIP_TRY(hipMemsetAsync(cnt.p, 0, ((size_t)n_defs + 2) * sizeof(unsigned long long), st));
  DevBuf<uint64_t> rx_bits;  // truth words, validity words
  std::vector<DevBuf<uint8_t>> rx_tab((size_t)n_defs);
  const unsigned grid = (unsigned)std::min<int64_t>((n_words + 3) / 4, 4096);
  for (int d = 0; d < n_defs; ++d) {
    EvalArgs& a = args[d];
    if (!rx[d].tab.empty()) {
      HIP_TRY(rx_bits.ensure(2 * (size_t)n_words));
      HIP_TRY(rx_tab[d].ensure(rx[d].tab.size()));
      HIP_TRY(hipMemcpyAsync(rx_tab[d].p, rx[d].tab.data(), rx[d].tab.size(), hipMemcpyHostToDevice, st));
      HIP_TRY(launch_regex(a.valid, a.off, a.data, rows, rx_tab[d].p, rx[d].ns, rx[d].start, 0,
                           rx_bits.p, rx_bits.p + n_words, st));
      a.rx_val = rx_bits.p;
    }
    hipLaunchKernelGGL(schema_eval_kernel, dim3(grid), dim3(kBlock), 0, st, a, rows, valid_bitmap,
                       invalid_bitmap, cnt.p + 2 + d);
    HIP_TRY(hipGetLastError());
  }
  hipLaunchKernelGGL(schema_verdict_kernel, dim3(blocks_for(n_words, kBlock)), dim3(kBlock), 0, st,
                     valid_bitmap, invalid_bitmap, rows, cnt.p);
  HIP_TRY(hipGetLastError());
  std::vector<unsigned long long> h((size_t)n_defs + 2);
  HIP_TRY(d2h(h.data(), cnt.p, h.size() * sizeof(unsigned long long), st));
  *n_valid = (int64_t)h[0];
  *n_invalid = (int64_t)h[1];
  for (int d = 0; d < n_defs; ++d) n_unsupported[d] = (int64_t)h[2 + d];
  return DQ_OK;
}

extern "C" dq_status dq_select_plan(const uint64_t* bitmap, int64_t rows, int32_t* index_out,
                                    int64_t index_capacity, int64_t* n_selected,
                                    const dq_column* utf8_cols, int n_utf8, int64_t* utf8_bytes_out,
                                    void* hip_stream) {
  if (rows < 0 || index_capacity < 0 || !n_selected || n_utf8 < 0 ||
      (n_utf8 && (!utf8_cols || !utf8_bytes_out)))
    return fail(DQ_ERR_INVALID_ARGUMENT, "dq_select_plan: null or negative argument");
  if (rows > kMaxRows)
    return fail(DQ_ERR_UNSUPPORTED, "dq_select_plan: a batch of %lld rows (at most 2^31-1)", (long long)rows);
  *n_selected = 0;
  for (int c = 0; c < n_utf8; ++c) {
    utf8_bytes_out[c] = 0;
    if (utf8_cols[c].type != DQ_UTF8) return fail(DQ_ERR_WRONG_TYPE, "dq_select_plan: column %d is not utf8", c);
    if (utf8_cols[c].length != rows || (rows && !utf8_cols[c].values))
      return fail(DQ_ERR_INVALID_ARGUMENT, "dq_select_plan: column %d does not have %lld rows", c, (long long)rows);
  }
  if (rows == 0) return DQ_OK;
  if (!bitmap) return fail(DQ_ERR_INVALID_ARGUMENT, "dq_select_plan: null bitmap");
  hipStream_t st = reinterpret_cast<hipStream_t>(hip_stream);
  const int64_t n_tiles = (rows + DQ_SELECT_TILE_ROWS - 1) / DQ_SELECT_TILE_ROWS;
  DevBuf<uint32_t> tiles;
  HIP_TRY(tiles.ensure((size_t)n_tiles + 1));
  hipLaunchKernelGGL(select_count_kernel, dim3((unsigned)n_tiles), dim3(kBlock), 0, st, bitmap, rows, tiles.p);
  HIP_TRY(hipGetLastError());
  hipLaunchKernelGGL(tile_scan_kernel, dim3(1), dim3(kBlock), 0, st, tiles.p, n_tiles);
  HIP_TRY(hipGetLastError());
  uint32_t total = 0;
  HIP_TRY(d2h(&total, tiles.p + n_tiles, sizeof(total), st));
  *n_selected = (int64_t)total;
  if ((int64_t)total > index_capacity)
    return fail(DQ_ERR_INVALID_ARGUMENT, "dq_select_plan: %lld rows selected, index_out holds %lld",
                (long long)total, (long long)index_capacity);
  if (total == 0) return DQ_OK;
  if (!index_out) return fail(DQ_ERR_INVALID_ARGUMENT, "dq_select_plan: null index_out");
  hipLaunchKernelGGL(select_write_kernel, dim3((unsigned)n_tiles), dim3(kBlock), 0, st, bitmap, rows,
                     tiles.p, index_out);
  HIP_TRY(hipGetLastError());
  if (n_utf8) {
    DevBuf<unsigned long long> sums;
    HIP_TRY(sums.ensure((size_t)n_utf8));
    HIP_TRY(hipMemsetAsync(sums.p, 0, (size_t)n_utf8 * sizeof(unsigned long long), st));
    const unsigned grid = (unsigned)std::min<int64_t>(blocks_for(total, kBlock), 4096);
    for (int c = 0; c < n_utf8; ++c) {
      hipLaunchKernelGGL(select_bytes_kernel, dim3(grid), dim3(kBlock), 0, st,
                         static_cast<const int32_t*>(utf8_cols[c].values), rows, index_out, (int64_t)total,
                         sums.p + c);
      HIP_TRY(hipGetLastError());
    }
    std::vector<unsigned long long> h((size_t)n_utf8);
    HIP_TRY(d2h(h.data(), sums.p, h.size() * sizeof(unsigned long long), st));
    for (int c = 0; c < n_utf8; ++c) utf8_bytes_out[c] = (int64_t)h[c];
  } else {
    HIP_TRY(hipStreamSynchronize(st));
  }
  return DQ_OK;
}

extern "C" dq_status dq_gather_column(const dq_column* in, const int32_t* index, int64_t n_out,
                                      dq_column* out, void* hip_stream) {
  if (!in || !out || n_out < 0) return fail(DQ_ERR_INVALID_ARGUMENT, "dq_gather_column: null or negative argument");
  if (n_out > kMaxRows || in->length > kMaxRows || in->length < 0)
    return fail(DQ_ERR_UNSUPPORTED, "dq_gather_column: more than 2^31-1 rows");
  const int tid = DQ_TYPE_ID(in->type);
  const int width = fixed_width(in->type);
  if (!width && tid != DQ_BOOL && tid != DQ_UTF8)
    return fail(DQ_ERR_WRONG_TYPE, "dq_gather_column: type %d", in->type);
  if (out->type != in->type) return fail(DQ_ERR_WRONG_TYPE, "dq_gather_column: out is of another type");
  if ((in->validity != nullptr) != (out->validity != nullptr))
    return fail(DQ_ERR_INVALID_ARGUMENT, "dq_gather_column: out has a validity buffer iff in has one");
  if (!out->values || (tid == DQ_UTF8 && !out->data))
    return fail(DQ_ERR_INVALID_ARGUMENT, "dq_gather_column: null output buffers");
  if (n_out && (!index || !in->values || (tid == DQ_UTF8 && !in->data)))
    return fail(DQ_ERR_INVALID_ARGUMENT, "dq_gather_column: null input buffers");
  hipStream_t st = reinterpret_cast<hipStream_t>(hip_stream);
  const int64_t capacity = out->data_bytes;
  out->length = n_out;
  out->data_bytes = 0;
  if (n_out == 0) {
    if (tid == DQ_UTF8) HIP_TRY(hipMemsetAsync(const_cast<void*>(out->values), 0, sizeof(int32_t), st));
    HIP_TRY(hipStreamSynchronize(st));
    return DQ_OK;
  }
  const int64_t in_rows = in->length;
  const unsigned row_grid = blocks_for(n_out, kBlock), word_grid = blocks_for((n_out + 63) / 64, kBlock / 64);
  if (in->validity) {
    hipLaunchKernelGGL(gather_bits_kernel, dim3(word_grid), dim3(kBlock), 0, st, in->validity, in_rows,
                       index, n_out, reinterpret_cast<uint64_t*>(const_cast<uint8_t*>(out->validity)));
    HIP_TRY(hipGetLastError());
  }
  void* ov = const_cast<void*>(out->values);
#define DQ_GATHER_FIXED(T)                                                                     \
  hipLaunchKernelGGL(gather_fixed_kernel<T>, dim3(row_grid), dim3(kBlock), 0, st,              \
                     static_cast<const T*>(in->values), in_rows, index, n_out, static_cast<T*>(ov))
  if (tid == DQ_BOOL) {
    hipLaunchKernelGGL(gather_bits_kernel, dim3(word_grid), dim3(kBlock), 0, st,
                       static_cast<const uint8_t*>(in->values), in_rows, index, n_out,
                       static_cast<uint64_t*>(ov));
  } else if (width == 1) {
    DQ_GATHER_FIXED(uint8_t);
  } else if (width == 2) {
    DQ_GATHER_FIXED(uint16_t);
  } else if (width == 4) {
    DQ_GATHER_FIXED(uint32_t);
  } else if (width == 8) {
    DQ_GATHER_FIXED(uint64_t);
  } else if (width == 16) {
    DQ_GATHER_FIXED(B16);
  }
#undef DQ_GATHER_FIXED
  HIP_TRY(hipGetLastError());
  if (tid == DQ_UTF8) {
    const int32_t* off = static_cast<const int32_t*>(in->values);
    int32_t* off_out = static_cast<int32_t*>(ov);
    const int64_t n_tiles = (n_out + kLenTile - 1) / kLenTile;
    DevBuf<uint32_t> tiles;
    HIP_TRY(tiles.ensure((size_t)n_tiles + 1));
    hipLaunchKernelGGL(utf8_count_kernel, dim3((unsigned)n_tiles), dim3(kBlock), 0, st, off, in_rows, index,
                       n_out, tiles.p);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(tile_scan_kernel, dim3(1), dim3(kBlock), 0, st, tiles.p, n_tiles);
    HIP_TRY(hipGetLastError());
    uint32_t total = 0;
    HIP_TRY(d2h(&total, tiles.p + n_tiles, sizeof(total), st));
    if ((int64_t)total > capacity)
      return fail(DQ_ERR_INVALID_ARGUMENT, "dq_gather_column: %lld string bytes, out->data holds %lld",
                  (long long)total, (long long)capacity);
    hipLaunchKernelGGL(utf8_offsets_kernel, dim3((unsigned)n_tiles), dim3(kBlock), 0, st, off, in_rows, index,
                       n_out, tiles.p, n_tiles, off_out);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(utf8_copy_kernel, dim3(row_grid), dim3(kBlock), 0, st, off, in->data, in_rows, index,
                       n_out, off_out, const_cast<uint8_t*>(out->data));
    HIP_TRY(hipGetLastError());
    out->data_bytes = (int32_t)total;
  }
  HIP_TRY(hipStreamSynchronize(st));
  return DQ_OK;
}
