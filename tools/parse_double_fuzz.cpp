// Stand-alone check of deequ_amd/csrc/parse_double.h against the C library's strtod (correctly
// rounded in glibc), meant to be built with sanitizers on the host:
//
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all \
//       -I deequ_amd/csrc tools/parse_double_fuzz.cpp -o parse_double_fuzz && ./parse_double_fuzz 4000000
//
// Every string is copied into an exactly sized heap block, so a read outside [0, n) is reported.
// Prints the number of strings, how many reached the exact fallback, and fails on a mismatch.
// A mismatch on a hex string with a subnormal result wants a second opinion before it is blamed on
// the parser: glibc 2.35 rounds 0xF33.8E9c1604B24p-1036 down although the dropped part is 0.5625
// of a unit (exact rational arithmetic and Python's float.fromhex round it up, as the parser does).
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>
#include <vector>

#define DQ_HD inline
#define DQ_HD_NOINLINE inline __attribute__((noinline))
#include "parse_double.h"

namespace {

uint64_t g_state = 0x9E3779B97F4A7C15ULL;
uint64_t rnd() {  // xorshift64*
  g_state ^= g_state >> 12;
  g_state ^= g_state << 25;
  g_state ^= g_state >> 27;
  return g_state * 0x2545F4914F6CDD1DULL;
}
uint64_t below(uint64_t n) { return rnd() % n; }

long g_count = 0, g_fallback = 0, g_bad = 0;

uint64_t bits_of(double d) {
  uint64_t b;
  memcpy(&b, &d, 8);
  return b;
}

void check(const std::string& text) {
  uint8_t* p = static_cast<uint8_t*>(malloc(text.size() ? text.size() : 1));
  memcpy(p, text.data(), text.size());
  double got = 0;
  int flags = 0;
  const bool ok = dq::castp::parse_double(p, (int32_t)text.size(), got, flags);
  free(p);
  char* end = nullptr;
  const double want = strtod(text.c_str(), &end);
  ++g_count;
  g_fallback += (flags & dq::castp::kPdFallback) != 0;
  if (!ok || *end != 0 || bits_of(got) != bits_of(want)) {
    if (++g_bad <= 20) {
      const std::string head = text.substr(0, 80);
      printf("MISMATCH %s%s: ok=%d got=%a want=%a\n", head.c_str(), text.size() > 80 ? "..." : "",
             (int)ok, got, want);
    }
  }
}

std::string digits(int n) {
  std::string s;
  for (int i = 0; i < n; ++i) s.push_back((char)('0' + below(10)));
  return s;
}

std::string random_decimal() {
  const int kind = (int)below(8);
  int n = kind < 3 ? 1 + (int)below(19) : kind < 6 ? 17 + (int)below(24) : 1 + (int)below(60);
  if (below(400) == 0) n = 700 + (int)below(200);
  std::string d = digits(n);
  std::string s = below(2) ? "-" : "";
  const int point = (int)below((uint64_t)n + 2);
  if (point <= n) d.insert((size_t)point, ".");
  if (d == ".") d = "0.";
  s += d;
  if (below(3) == 0) return s;
  int e;
  switch (below(5)) {
    case 0: e = (int)below(60) - 30; break;
    case 1: e = -330 + (int)below(40) - n / 2; break;  // around the subnormals
    case 2: e = 290 + (int)below(30) - n / 2; break;   // around DBL_MAX
    default: e = (int)below(700) - 350; break;
  }
  return s + "e" + std::to_string(e);
}

// the exact midpoint above a random double (or its neighbours in the last digit), as a decimal
std::string near_halfway() {
  uint64_t b = rnd() & 0x7FEFFFFFFFFFFFFFULL;
  if (below(4) == 0) b &= 0x001FFFFFFFFFFFFFULL;  // subnormals and the first binades
  // (2m + 1) * 2^(e - 1) printed exactly: long multiplication / division in base 10^9
  uint64_t m = b & ((1ULL << 52) - 1);
  int e = (int)(b >> 52);
  if (e) m |= 1ULL << 52; else e = 1;
  e -= 1075;
  const uint64_t mid = 2 * m + 1;
  int e2 = e - 1;
  std::vector<uint32_t> num;  // little-endian base 10^9
  for (uint64_t v = mid; v; v /= 1000000000) num.push_back((uint32_t)(v % 1000000000));
  int frac_digits = 0;
  for (; e2 > 0; --e2) {
    uint64_t carry = 0;
    for (auto& w : num) {
      const uint64_t t = (uint64_t)w * 2 + carry;
      w = (uint32_t)(t % 1000000000);
      carry = t / 1000000000;
    }
    if (carry) num.push_back((uint32_t)carry);
  }
  for (; e2 < 0; ++e2) {  // x / 2 = x * 5 / 10
    uint64_t carry = 0;
    for (auto& w : num) {
      const uint64_t t = (uint64_t)w * 5 + carry;
      w = (uint32_t)(t % 1000000000);
      carry = t / 1000000000;
    }
    if (carry) num.push_back((uint32_t)carry);
    ++frac_digits;
  }
  std::string s;
  char buf[16];
  for (size_t i = num.size(); i-- > 0;) {
    snprintf(buf, sizeof buf, i + 1 == num.size() ? "%u" : "%09u", num[i]);
    s += buf;
  }
  const size_t exact_len = s.size();
  const int tweak = (int)below(5);
  if (tweak == 1 && s.back() != '9') s.back()++;
  if (tweak == 2 && s.back() != '0') s.back()--;
  if (tweak == 3) s += std::string(1 + below(60), '0');
  if (tweak == 4) s += std::string(780, '0') + "1";
  // value = s * 10^-frac_digits; appended digits are further fractional ones
  return s + "e-" + std::to_string(frac_digits + (int)(s.size() - exact_len));
}

std::string random_hex() {
  std::string s = below(2) ? "-0x" : "0x";
  const int n = 1 + (int)below(22);
  std::string d;
  for (int i = 0; i < n; ++i) d.push_back("0123456789abcdefABCDEF"[below(22)]);
  if (below(3) == 0) d = "1" + std::string(13, "08f"[below(3)]) + d;  // ties and near ties
  const int point = (int)below((uint64_t)d.size() + 2);
  if (point <= (int)d.size()) d.insert((size_t)point, ".");
  if (d == ".") d = "0.";
  int e = below(2) ? (int)below(120) - 60 : (int)below(2300) - 1150;
  return s + d + "p" + std::to_string(e);
}

}  // namespace

int main(int argc, char** argv) {
  const long total = argc > 1 ? atol(argv[1]) : 1000000;
  const char* hard[] = {
      "2.2250738585072011e-308", "2.2250738585072012e-308", "2.2250738585072014e-308",
      "1.7976931348623157e308", "1.7976931348623158e308", "1.7976931348623159e308", "1e309",
      "1e-324", "4.9e-324", "2.4703282292062327e-324", "2.4703282292062328e-324",
      "2.47032822920623272e-324", "1e99999999999999999999", "1e-99999999999999999999",
      "0e99999999999", "9007199254740993", "9007199254740992.5", "9007199254740993.0000000001",
      "0.30000000000000004", "8.41e21", "6.8e22", "1e23", "9e-265", "0x1p-1074", "0x1p-1075",
      "0x1.8p-1075", "0x1.fffffffffffff8p1023", "0x1.fffffffffffff7ffffp1023", "0x.8p1",
      "0x1.00000000000008p0", "0x1.00000000000018p0", "0x1.000000000000080000001p0",
      "0x0.0000000000000000000000001p100", "0x100000000000000000000000000p-100"};
  for (const char* h : hard) check(h);
  check("1" + std::string(400, '0'));
  check("0." + std::string(400, '0') + "1");
  for (long i = 0; i < total; ++i) {
    const uint64_t k = below(10);
    if (k < 6) check(random_decimal());
    else if (k < 8) check(near_halfway());
    else check(random_hex());
  }
  printf("%ld strings, %ld through the exact fallback, %ld mismatches\n", g_count, g_fallback, g_bad);
  return g_bad ? 1 : 0;
}
