// cast_parse.h -- the per-string parsers of Spark 2.2's Cast(StringType -> LongType | DoubleType)
// for host and device code: cast.hip's kernel calls them once per row, and dq_cast_parse_utf8 runs
// the same functions on the host (tests/test_cast_cases.py).
//
//   spark_to_long:     UTF8String.toLong (Spark 2.2): optional sign, digits, optionally '.' and
//                      digits (truncated); no whitespace; overflow or any other byte -> NULL.
//   java_parse_double: java.lang.Double.parseDouble (Cast: `s.toString.toDouble`,
//                      NumberFormatException -> NULL).  Three results per string:
//                        1  a plain decimal (bytes <= ' ' trimmed at both ends, optional sign, digits
//                           with at most one '.', at least one digit) converted exactly: one
//                           correctly rounded multiply or divide by an exact power of ten.  With d
//                           the digits without leading and trailing zeros and e the power of ten
//                           that goes with them, that is every string with d <= 2^53 and either
//                           |e| <= 22, or e > 22 and d * 10^(e - 22) <= 2^53; zero in any spelling;
//                        0  NULL: parseDouble throws.  Decided by the grammar of Double.valueOf's
//                           documentation (java_float_form below), so "1e", "d", "0x1" and "1d2"
//                           are NULL like "abc";
//                        2  parseDouble reads the string but this path does not convert it: an
//                           exponent, "NaN", "Infinity", a hex form, an f/F/d/D suffix, or a plain
//                           decimal outside the window above.  The caller counts these rows and
//                           fails loudly rather than guess.
#pragma once

#include <stdint.h>

#ifndef DQ_HD
#define DQ_HD __host__ __device__ __forceinline__
#endif

namespace dq {
namespace castp {

DQ_HD bool is_digit(uint8_t c) { return c >= '0' && c <= '9'; }
DQ_HD bool is_hex_digit(uint8_t c) {
  return is_digit(c) || (c >= 'a' && c <= 'f') || (c >= 'A' && c <= 'F');
}

DQ_HD bool spark_to_long(const uint8_t* s, int32_t n, int64_t& out) {
  if (n == 0) return false;
  int32_t i = 0;
  const bool neg = s[0] == '-';
  if (neg || s[0] == '+') {
    if (n == 1) return false;
    i = 1;
  }
  const int64_t stop = INT64_MIN / 10;
  int64_t r = 0;  // accumulated negatively (INT64_MIN has no positive counterpart)
  for (; i < n; ++i) {
    const uint8_t b = s[i];
    if (b == '.') {
      ++i;
      break;
    }
    if (!is_digit(b)) return false;
    if (r < stop) return false;
    // (unsigned: the product may wrap, which the sign test below then reports)
    r = (int64_t)((uint64_t)r * 10u - (uint64_t)(b - '0'));
    if (r > 0) return false;
  }
  for (; i < n; ++i)
    if (!is_digit(s[i])) return false;
  if (!neg) {
    if (r == INT64_MIN) return false;
    r = -r;
  }
  out = r;
  return true;
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

// 0 = NULL (NumberFormatException), 1 = value, 2 = readable by parseDouble but not converted here
DQ_HD int java_parse_double(const uint8_t* s, int32_t n, double& out) {
  int32_t a = 0, b = n;
  while (a < b && s[a] <= ' ') ++a;
  while (b > a && s[b - 1] <= ' ') --b;
  if (a == b) return 0;
  bool neg = false;
  if (s[a] == '-' || s[a] == '+') {
    neg = s[a] == '-';
    ++a;
  }
  uint64_t w = 0;
  int sig = 0, e10 = 0, digits = 0;
  bool dot = false, lost = false;
  for (int32_t i = a; i < b; ++i) {
    const uint8_t c = s[i];
    if (c == '.') {
      if (dot) return 0;
      dot = true;
      continue;
    }
    if (is_digit(c)) {
      ++digits;
      if (w == 0 && c == '0') {  // leading zeros: only the exponent moves
        if (dot) --e10;
        continue;
      }
      if (sig < 19) {
        w = w * 10 + (uint64_t)(c - '0');
        ++sig;
        if (dot) --e10;
      } else {
        if (c != '0') lost = true;  // a digit beyond 19 significant ones
        if (!dot) ++e10;
      }
      continue;
    }
    // not a plain decimal: the other forms parseDouble accepts (exponent, NaN, Infinity, hex, type
    // suffix) are reported, everything else is a NumberFormatException
    return java_float_form(s, a, b) ? 2 : 0;
  }
  if (digits == 0) return 0;
  if (lost) return 2;
  if (w == 0) {
    out = neg ? -0.0 : 0.0;
    return 1;
  }
  // trailing zeros of w move into the exponent, whatever its sign ("1" and 20 zeros is 1 * 10^20,
  // not 10^18 * 10^2); a large exponent then moves back into w while w stays exact
  while (w % 10 == 0) {
    w /= 10;
    ++e10;
  }
  while (e10 > 22 && w <= (1ULL << 53) / 10) {
    w *= 10;
    --e10;
  }
  if (w > (1ULL << 53) || e10 > 22 || e10 < -22) return 2;
  const double x = (double)w;  // exact
  double v = e10 >= 0 ? x * pow10_exact(e10) : x / pow10_exact(-e10);
  out = neg ? -v : v;
  return 1;
}

}  // namespace castp
}  // namespace dq
