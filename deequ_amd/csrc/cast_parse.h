// cast_parse.h -- the per-string parsers of Spark 2.2's Cast(StringType -> LongType | DoubleType)
// for host and device code: cast.hip's kernels call them once per row, and dq_cast_parse_utf8 runs
// the same functions on the host (tests/test_cast_cases.py, tests/test_parse_double.py).
//
//   spark_to_long:     UTF8String.toLong (Spark 2.2): optional sign, digits, optionally '.' and
//                      digits (truncated); no whitespace; overflow or any other byte -> NULL.
//   java_parse_double: java.lang.Double.parseDouble (Cast: `s.toString.toDouble`,
//                      NumberFormatException -> NULL) as the string cast reports it.  Three results
//                      per string:
//                        1  a plain decimal (bytes <= ' ' trimmed at both ends, optional sign, digits
//                           with at most one '.', at least one digit) of any length and magnitude:
//                           the correctly rounded double of parse_double.h, +-Infinity above the
//                           range, +-0.0 below it;
//                        0  NULL: parseDouble throws.  Decided by the grammar of Double.valueOf's
//                           documentation (java_float_form), so "1e", "d", "0x1" and "1d2" are NULL
//                           like "abc";
//                        2  a non-plain form parseDouble reads: an exponent, "NaN", "Infinity", a
//                           hex form, an f/F/d/D suffix.  parse_double.h converts these too (the
//                           predicate interpreter uses it for them), but the cast keeps reporting
//                           them: DataType's regexes never infer Fractional for a column that holds
//                           one, so no public profiler path reaches them, and the profiler's loud
//                           failure on such a row ("1e5", "NaN") is pinned by its tests.  The caller
//                           counts these rows and fails loudly.
//   java_parse_double_fast: the same without the exact fallback, for the cast's first kernel: 3
//                           where only dec_exact decides (result 1 once it has run).
#pragma once

#include <stdint.h>

#include "parse_double.h"

namespace dq {
namespace castp {

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

// 0 = NULL, 1 = value, 2 = non-plain form (reported), 3 = plain, but only dec_exact decides
DQ_HD int java_parse_double_fast(const uint8_t* s, int32_t n, double& out) {
  int32_t a = 0, b = n;
  while (a < b && s[a] <= ' ') ++a;
  while (b > a && s[b - 1] <= ' ') --b;
  if (a == b) return 0;
  bool neg = false;
  if (s[a] == '-' || s[a] == '+') {
    neg = s[a] == '-';
    ++a;
  }
  const DecScan d = scan_decimal(s, a, b);
  // not a plain decimal: the other forms parseDouble accepts (exponent, NaN, Infinity, hex, type
  // suffix) are reported, everything else is a NumberFormatException
  if (d.end != b) return java_float_form(s, a, b) ? 2 : 0;
  if (d.digits == 0) return 0;
  return dec_fast(d.w, d.e10, d.lost, neg, out) ? 1 : 3;
}

// 0 = NULL (NumberFormatException), 1 = value, 2 = non-plain form (reported, not converted)
DQ_HD int java_parse_double(const uint8_t* s, int32_t n, double& out, int* flags = nullptr) {
  double v = 0.0;
  int f = 0;
  const bool ok = parse_double(s, n, v, f);
  if (flags) *flags = f;
  if (!ok) return 0;
  if (!(f & kPdPlain)) return 2;
  out = v;
  return 1;
}

}  // namespace castp
}  // namespace dq
