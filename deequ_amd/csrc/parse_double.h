// parse_double.h -- java.lang.Double.parseDouble for host and device code: for every byte string
// either the double Java returns, bit for bit, or "NumberFormatException".  cast_parse.h wraps it
// for the string cast (cast.hip), expr.hip calls it for CAST(s AS DOUBLE) and every
// `string <op> number` comparison, and dq_parse_double_utf8 runs it on the host.
//
// Grammar (Double.valueOf's documentation; java_float_form below): bytes <= 0x20 trimmed at both
// ends, an optional sign, then NaN | Infinity | a decimal with an optional e/E exponent and an
// optional f F d D suffix | a hex significand with its mandatory p/P exponent and an optional suffix.
//
// Decimal forms, in three steps (each one returns the correctly rounded double or declines):
//   1. the exact window: at most 19 digits, none dropped, w <= 2^53 and |q| <= 22 (after moving
//      trailing zeros between w and q): one correctly rounded multiply or divide of exact doubles;
//   2. Eisel-Lemire (D. Lemire, "Number parsing at a gigabyte per second", SPE 51(8), 2021): the
//      first 19 significant digits w and the power of ten q, one 64x128-bit multiply by the
//      truncated power of five of pow5_128.h.  When digits were dropped, the result stands only if
//      w and w + 1 round to the same double; the algorithm's own ambiguous case (all-ones low
//      product word outside q in [-27, 55]) declines too;
//   3. dec_exact: the decimal against the midpoint of the two candidate doubles in multi-word
//      integers.  Not inlined, and never called by the cast's first kernel.
// Hex forms: 64 significand bits and a sticky bit, the binary exponent, one rounding to 53 bits
// (ties to even), subnormals and overflow included.
// Out of range follows Java: +-Infinity above, +-0.0 below; the sign of zero is kept.
//
// Bytes are read with plain byte loads at offsets in [0, n) only, so nothing outside the string
// is touched (the aligned-dword reader DevBytes exists for wide loads; a byte load at the same
// offset returns the same byte).
#pragma once

#include <stdint.h>

#include "pow5_128.h"

#ifndef DQ_HD
#define DQ_HD __host__ __device__ __forceinline__
#endif
#ifndef DQ_HD_NOINLINE
#define DQ_HD_NOINLINE __host__ __device__ inline __attribute__((noinline))
#endif

namespace dq {
namespace castp {

DQ_HD bool is_digit(uint8_t c) { return c >= '0' && c <= '9'; }
DQ_HD bool is_hex_digit(uint8_t c) {
  return is_digit(c) || (c >= 'a' && c <= 'f') || (c >= 'A' && c <= 'F');
}

DQ_HD double pow10_exact(int e) {  // 10^e, exact in fp64 for 0 <= e <= 22
  double p = 1.0;
  for (int k = 0; k < e; ++k) p *= 10.0;
  return p;
}

// Whether s[a, b) -- a trimmed string after its optional sign -- is one of the forms Double.valueOf
// documents:  NaN | Infinity | HexSignificand BinaryExponent [fFdD] | decimal [ExponentPart] [fFdD]
//   decimal:        Digits [.] [Digits] | . Digits
//   ExponentPart:   (e|E) [+-] Digits
//   HexSignificand: 0(x|X) HexDigits [.] | 0(x|X) [HexDigits] . HexDigits
//   BinaryExponent: (p|P) [+-] Digits      (mandatory after a hex significand)
DQ_HD bool java_float_form(const uint8_t* s, int32_t a, int32_t b) {
  const int32_t n = b - a;
  if (n == 3 && s[a] == 'N' && s[a + 1] == 'a' && s[a + 2] == 'N') return true;
  if (n == 8 && s[a] == 'I' && s[a + 1] == 'n' && s[a + 2] == 'f' && s[a + 3] == 'i' &&
      s[a + 4] == 'n' && s[a + 5] == 'i' && s[a + 6] == 't' && s[a + 7] == 'y')
    return true;
  int32_t i = a;
  const bool hex = n >= 2 && s[a] == '0' && (s[a + 1] == 'x' || s[a + 1] == 'X');
  if (hex) i += 2;
  int32_t nd = 0;  // significand digits on both sides of the point
  for (; i < b && (hex ? is_hex_digit(s[i]) : is_digit(s[i])); ++i) ++nd;
  if (i < b && s[i] == '.') {
    ++i;
    for (; i < b && (hex ? is_hex_digit(s[i]) : is_digit(s[i])); ++i) ++nd;
  }
  if (nd == 0) return false;
  const bool exp = i < b && (hex ? (s[i] == 'p' || s[i] == 'P') : (s[i] == 'e' || s[i] == 'E'));
  if (exp) {
    ++i;
    if (i < b && (s[i] == '+' || s[i] == '-')) ++i;
    int32_t ne = 0;
    for (; i < b && is_digit(s[i]); ++i) ++ne;
    if (ne == 0) return false;
  } else if (hex) {
    return false;
  }
  if (i < b && (s[i] == 'f' || s[i] == 'F' || s[i] == 'd' || s[i] == 'D')) ++i;
  return i == b;
}

// ------------------------------------------------------------------------------------------------
// The double with 53-bit significand m (m < 2^52 only at e = -1074) and value m * 2^e
// ------------------------------------------------------------------------------------------------
DQ_HD double assemble(uint64_t m, int e, bool neg) {
  if (m >> 53) {  // a rounding carried out of 53 bits
    m >>= 1;
    ++e;
  }
  uint64_t bits;
  if (m < (1ULL << 52)) bits = m;  // subnormal or zero
  else if (e + 1075 >= 0x7FF) bits = 0x7FFULL << 52;  // above DBL_MAX: Infinity
  else bits = ((uint64_t)(e + 1075) << 52) | (m & ((1ULL << 52) - 1));
  if (neg) bits |= 1ULL << 63;
  return __builtin_bit_cast(double, bits);
}

DQ_HD double infinity(bool neg) {
  return __builtin_bit_cast(double, (0x7FFULL << 52) | ((uint64_t)neg << 63));
}

DQ_HD int clz64(uint64_t x) { return __builtin_clzll(x); }  // x != 0

// ------------------------------------------------------------------------------------------------
// Eisel-Lemire
// ------------------------------------------------------------------------------------------------
struct ElProduct {
  uint64_t hi, lo;  // the top 128 bits of (w << lz) * 5^q's table entry: a truncation
  int power2;       // the biased exponent that goes with a 53-bit significand taken from hi
  int shift;        // hi >> shift is that significand with one more bit below it
};

// w != 0, kPow10Min <= q <= kPow10Max
DQ_HD ElProduct el_product(uint64_t w, int q) {
  const int lz = clz64(w);
  w <<= lz;
  const uint64_t t_hi = kPow5_128[q - kPow10Min][0], t_lo = kPow5_128[q - kPow10Min][1];
  unsigned __int128 first = (unsigned __int128)w * t_hi;
  ElProduct p;
  p.hi = (uint64_t)(first >> 64);
  p.lo = (uint64_t)first;
  if ((p.hi & 0x1FF) == 0x1FF) {  // the 9 bits below the 55 that matter: the second word may carry
    const uint64_t second_hi = (uint64_t)(((unsigned __int128)w * t_lo) >> 64);
    p.lo += second_hi;
    if (second_hi > p.lo) ++p.hi;
  }
  const int upper = (int)(p.hi >> 63);
  p.shift = upper + 9;
  // floor(log2(10^q)) + 63 = ((217706 * q) >> 16) + 63 on this range of q
  p.power2 = (int)(((int64_t)217706 * q) >> 16) + 63 + upper - lz + 1023;
  return p;
}

// w * 10^q rounded to nearest even; false when the truncated product cannot decide
DQ_HD bool eisel_lemire(uint64_t w, int q, bool neg, double& out) {
  const ElProduct p = el_product(w, q);
  if (p.lo == ~0ULL && (q < -27 || q > 55)) return false;
  uint64_t m = p.hi >> p.shift;  // 54 bits: the significand and a rounding bit
  if (p.power2 <= 0) {           // subnormal, or below
    if (-p.power2 + 1 >= 64) {
      out = neg ? -0.0 : 0.0;
      return true;
    }
    m >>= -p.power2 + 1;
    m += m & 1;
    out = assemble(m >> 1, -1074, neg);
    return true;
  }
  // exactly halfway (possible only for small |q|): ties to even, here down
  if (p.lo <= 1 && q >= -4 && q <= 23 && (m & 3) == 1 && (m << p.shift) == p.hi) m &= ~1ULL;
  m += m & 1;
  out = assemble(m >> 1, p.power2 - 1075, neg);
  return true;
}

// ------------------------------------------------------------------------------------------------
// The exact fallback.
//
// The decimal is D = d * 10^E, d the first kMaxDigits significant digits and `sticky` whether a
// later one is non-zero.  A midpoint between two doubles has at most 768 significant digits
// ((2^54 - 1) * 2^-1075 has them) and lies within a factor of four of D, so it is a multiple of
// the unit of D's 769th digit: where the 769-digit prefix differs from the midpoint it decides,
// and where it equals the midpoint the sticky flag does.
//
// The candidate m * 2^e (m the 53-bit truncation of the Eisel-Lemire product, off from D by far
// less than 2^e) gives the midpoint (2m + 1) * 2^(e - 1).  Both sides are scaled to integers:
//   E >= 0:  d * 5^E * 2^(E - e + 1)  against  2m + 1
//   E <  0:  d * 2^(E - e + 1)        against  (2m + 1) * 5^-E
// with a negative power of two moved to the other side.  Sizes: d < 10^769 < 2^2555.  The callers
// pass 19 digits with -342 <= q <= 308, so -E <= 342 + 750 = 1092 and 5^1092 < 2^2536, and
// 2m + 1 < 2^55.  The two sides are within a factor of four of each other, so each is below
// 4 * max(2^2555, 2^55 * 2^2536) = 2^2593: kBigWords = 41 words of 64 bits (2624).  For E >= 0,
// d * 5^E <= D < 10^328 is far below that.  Every operation also clamps at kBigWords.
// ------------------------------------------------------------------------------------------------
constexpr int kMaxDigits = 769;
constexpr int kBigWords = 41;

struct Big {
  uint64_t w[kBigWords];
  int n;  // words in use; w[n - 1] != 0
};

DQ_HD void big_mul_add(Big& x, uint64_t mul, uint64_t add) {
  uint64_t carry = add;
  for (int i = 0; i < x.n; ++i) {
    const unsigned __int128 t = (unsigned __int128)x.w[i] * mul + carry;
    x.w[i] = (uint64_t)t;
    carry = (uint64_t)(t >> 64);
  }
  if (carry && x.n < kBigWords) x.w[x.n++] = carry;
}

DQ_HD void big_mul_pow5(Big& x, int k) {
  for (; k >= 27; k -= 27) big_mul_add(x, 7450580596923828125ULL, 0);  // 5^27 < 2^63
  uint64_t p = 1;
  for (; k > 0; --k) p *= 5;
  big_mul_add(x, p, 0);
}

DQ_HD void big_shl(Big& x, int s) {
  if (s <= 0 || x.n == 0) return;
  const int ws = s >> 6, bs = s & 63;
  int nn = x.n + ws + 1;
  if (nn > kBigWords) nn = kBigWords;
  for (int i = nn - 1; i >= 0; --i) {  // downwards: reads only words at or below i
    const int j = i - ws;
    const uint64_t a = j >= 0 && j < x.n ? x.w[j] : 0;
    const uint64_t b = j >= 1 && j - 1 < x.n ? x.w[j - 1] : 0;
    x.w[i] = bs ? (a << bs) | (b >> (64 - bs)) : a;
  }
  x.n = nn;
  while (x.n > 0 && x.w[x.n - 1] == 0) --x.n;
}

DQ_HD int big_cmp(const Big& a, const Big& b) {
  if (a.n != b.n) return a.n < b.n ? -1 : 1;
  for (int i = a.n - 1; i >= 0; --i)
    if (a.w[i] != b.w[i]) return a.w[i] < b.w[i] ? -1 : 1;
  return 0;
}

// s[a, b): the significand's digits with at most one '.'; exp: the explicit exponent (saturated);
// w, q: its first 19 significant digits and their power of ten, kPow10Min <= q <= kPow10Max.
DQ_HD_NOINLINE double dec_exact(const uint8_t* s, int32_t a, int32_t b, int64_t exp, uint64_t w,
                                int q, bool neg) {
  Big d;
  d.n = 0;
  uint64_t chunk = 0;
  int in_chunk = 0, nd = 0;
  bool dot = false, sticky = false;
  int64_t E = exp;
  for (int32_t i = a; i < b; ++i) {
    const uint8_t c = s[i];
    if (c == '.') {
      dot = true;
      continue;
    }
    if (nd == 0 && c == '0') {
      if (dot) --E;
      continue;
    }
    if (nd < kMaxDigits) {
      chunk = chunk * 10 + (uint64_t)(c - '0');
      ++nd;
      if (dot) --E;
      if (++in_chunk == 19) {
        big_mul_add(d, 10000000000000000000ULL, chunk);
        chunk = 0;
        in_chunk = 0;
      }
    } else {
      if (c != '0') sticky = true;
      if (!dot) ++E;
    }
  }
  if (in_chunk) {
    uint64_t p = 1;
    for (int k = 0; k < in_chunk; ++k) p *= 10;
    big_mul_add(d, p, chunk);
  }
  if (E > kPow10Max) E = kPow10Max;  // (the callers' bounds; clamped so that a slip stays in range)
  if (E < kPow10Min - (kMaxDigits - 19)) E = kPow10Min - (kMaxDigits - 19);

  const ElProduct p = el_product(w, q);
  uint64_t m;
  int e;
  if (p.power2 > 0) {
    m = p.hi >> (p.shift + 1);
    e = p.power2 - 1075;
  } else {
    const int sh = p.shift + 2 - p.power2;
    m = sh < 64 ? p.hi >> sh : 0;
    e = -1074;
  }
  Big mid;
  mid.n = 1;
  mid.w[0] = 2 * m + 1;
  const int e10 = (int)E;
  if (e10 >= 0) big_mul_pow5(d, e10);
  else big_mul_pow5(mid, -e10);
  const int two = e10 - e + 1;
  if (two >= 0) big_shl(d, two);
  else big_shl(mid, -two);
  const int c = big_cmp(d, mid);
  if (c > 0 || (c == 0 && (sticky || (m & 1)))) ++m;
  return assemble(m, e, neg);
}

// ------------------------------------------------------------------------------------------------
// Decimal and hex significands
// ------------------------------------------------------------------------------------------------
struct DecScan {
  uint64_t w;    // the first 19 significant digits
  int64_t e10;   // the power of ten that goes with w (before an explicit exponent)
  int32_t end;   // the first byte that is neither a digit nor the first '.'
  int32_t digits;
  bool lost;     // a digit after the 19th is non-zero
};

DQ_HD DecScan scan_decimal(const uint8_t* s, int32_t a, int32_t b) {
  DecScan r{0, 0, a, 0, false};
  int sig = 0;
  bool dot = false;
  int32_t i = a;
  for (; i < b; ++i) {
    const uint8_t c = s[i];
    if (c == '.') {
      if (dot) break;
      dot = true;
      continue;
    }
    if (!is_digit(c)) break;
    ++r.digits;
    if (r.w == 0 && c == '0') {  // leading zeros: only the exponent moves
      if (dot) --r.e10;
      continue;
    }
    if (sig < 19) {
      r.w = r.w * 10 + (uint64_t)(c - '0');
      ++sig;
      if (dot) --r.e10;
    } else {
      if (c != '0') r.lost = true;  // a digit beyond 19 significant ones
      if (!dot) ++r.e10;
    }
  }
  r.end = i;
  return r;
}

// Steps 1 and 2 for w * 10^e10 (+ dropped digits when lost).  true: out holds the double; false:
// only dec_exact decides (then kPow10Min <= e10 <= kPow10Max).
DQ_HD bool dec_fast(uint64_t w, int64_t e10, bool lost, bool neg, double& out) {
  // w + 1 <= 10^19, so below 10^kPow10Min the decimal is under 10^-323 * 10^-1 < 2^-1075: zero
  if (w == 0 || e10 < kPow10Min) {
    out = neg ? -0.0 : 0.0;
    return true;
  }
  if (e10 > kPow10Max) {  // w >= 1: at least 10^309
    out = infinity(neg);
    return true;
  }
  if (!lost) {
    // trailing zeros of w move into the exponent, whatever its sign ("1" and 20 zeros is
    // 1 * 10^20, not 10^18 * 10^2); a large exponent then moves back into w while w stays exact
    uint64_t x = w;
    int64_t e = e10;
    while (x % 10 == 0) {
      x /= 10;
      ++e;
    }
    while (e > 22 && x <= (1ULL << 53) / 10) {
      x *= 10;
      --e;
    }
    if (x <= (1ULL << 53) && e <= 22 && e >= -22) {
      const double v = e >= 0 ? (double)x * pow10_exact((int)e) : (double)x / pow10_exact((int)-e);
      out = neg ? -v : v;
      return true;
    }
  }
  const int q = (int)e10;
  double v0;
  if (!eisel_lemire(w, q, neg, v0)) return false;
  if (lost) {  // the decimal lies between w and w + 1: decided where both round alike
    double v1;
    if (!eisel_lemire(w + 1, q, neg, v1)) return false;
    if (__builtin_bit_cast(uint64_t, v0) != __builtin_bit_cast(uint64_t, v1)) return false;
  }
  out = v0;
  return true;
}

// [+-]digits after e/E or p/P from s[i, b), saturated at 10^9; i moves past them.  false: none.
DQ_HD bool scan_exponent(const uint8_t* s, int32_t& i, int32_t b, int64_t& exp) {
  bool eneg = false;
  if (i < b && (s[i] == '+' || s[i] == '-')) {
    eneg = s[i] == '-';
    ++i;
  }
  int64_t v = 0;
  int32_t ne = 0;
  for (; i < b && is_digit(s[i]); ++i, ++ne)
    if (v < 1000000000) v = v * 10 + (s[i] - '0');
  exp = eneg ? -v : v;
  return ne > 0;
}

// s[a, b) after "0x": hex digits with at most one '.', the p exponent, an optional suffix
DQ_HD bool parse_hex(const uint8_t* s, int32_t a, int32_t b, bool neg, double& out) {
  uint64_t w = 0;
  int64_t e2 = 0;
  bool dot = false, sticky = false;
  int32_t i = a, nd = 0;
  for (; i < b; ++i) {
    const uint8_t c = s[i];
    if (c == '.') {
      if (dot) return false;
      dot = true;
      continue;
    }
    if (!is_hex_digit(c)) break;
    ++nd;
    const uint64_t v = is_digit(c) ? c - '0' : (c | 0x20) - 'a' + 10;
    if (w >> 60) {  // 64 bits are full: the rest is sticky
      sticky |= v != 0;
      if (!dot) e2 += 4;
    } else {
      w = (w << 4) | v;
      if (dot) e2 -= 4;
    }
  }
  if (nd == 0 || i >= b || (s[i] != 'p' && s[i] != 'P')) return false;
  ++i;
  int64_t exp;
  if (!scan_exponent(s, i, b, exp)) return false;
  if (i < b && (s[i] == 'f' || s[i] == 'F' || s[i] == 'd' || s[i] == 'D')) ++i;
  if (i != b) return false;
  if (w == 0) {
    out = neg ? -0.0 : 0.0;
    return true;
  }
  // (leading zero digits were shifted into w as zeros, so e2 already counts them)
  const int lz = clz64(w);
  w <<= lz;
  int64_t e = e2 + exp - lz + 11;  // value = (w >> 11) * 2^e, w in [2^63, 2^64)
  if (e > 2000) e = 2000;
  if (e < -3000) e = -3000;
  int64_t sh = 11;
  if (e < -1074) {
    sh += -1074 - e;
    e = -1074;
  }
  uint64_t m = 0;
  bool round = false;
  if (sh <= 64) {
    m = sh < 64 ? w >> sh : 0;
    round = (w >> (sh - 1)) & 1;
    sticky |= (w & ((1ULL << (sh - 1)) - 1)) != 0;
  } else {
    sticky = true;
  }
  if (round && (sticky || (m & 1))) ++m;
  out = assemble(m, (int)e, neg);
  return true;
}

constexpr int kPdPlain = 1;     // a plain decimal: no exponent, no suffix
constexpr int kPdFallback = 2;  // dec_exact decided

// The complete parser: true and the double, or false for NumberFormatException.
DQ_HD bool parse_double(const uint8_t* s, int32_t n, double& out, int& flags) {
  flags = 0;
  int32_t a = 0, b = n;
  while (a < b && s[a] <= ' ') ++a;
  while (b > a && s[b - 1] <= ' ') --b;
  if (a == b) return false;
  bool neg = false;
  if (s[a] == '-' || s[a] == '+') {
    neg = s[a] == '-';
    ++a;
  }
  const int32_t len = b - a;
  if (len == 3 && s[a] == 'N' && s[a + 1] == 'a' && s[a + 2] == 'N') {
    out = __builtin_nan("");
    return true;
  }
  if (len == 8 && s[a] == 'I' && s[a + 1] == 'n' && s[a + 2] == 'f' && s[a + 3] == 'i' &&
      s[a + 4] == 'n' && s[a + 5] == 'i' && s[a + 6] == 't' && s[a + 7] == 'y') {
    out = infinity(neg);
    return true;
  }
  if (len >= 2 && s[a] == '0' && (s[a + 1] == 'x' || s[a + 1] == 'X'))
    return parse_hex(s, a + 2, b, neg, out);
  const DecScan d = scan_decimal(s, a, b);
  if (d.digits == 0) return false;
  int32_t i = d.end;
  int64_t exp = 0;
  if (i == b) {
    flags |= kPdPlain;
  } else {
    if (s[i] == 'e' || s[i] == 'E') {
      ++i;
      if (!scan_exponent(s, i, b, exp)) return false;
    }
    if (i < b && (s[i] == 'f' || s[i] == 'F' || s[i] == 'd' || s[i] == 'D')) ++i;
    if (i != b) return false;
  }
  if (dec_fast(d.w, d.e10 + exp, d.lost, neg, out)) return true;
  out = dec_exact(s, a, d.end, exp, d.w, (int)(d.e10 + exp), neg);
  flags |= kPdFallback;
  return true;
}

}  // namespace castp
}  // namespace dq
