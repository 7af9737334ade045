// date_fields_check.cpp -- stand-alone host check of the date helpers in csrc/decimal.h
// (date_field, ts_to_days), to be built with the sanitizers:
//
//   hipcc -x hip --offload-arch=gfx950 -O1 -g -Xarch_host -fsanitize=address,undefined \
//         -Xarch_host -fno-sanitize-recover=undefined tools/date_fields_check.cpp -o date_fields_check
//
// Every day from 1582-10-15 to 9999-12-31: year / month / dayofmonth must equal the fields a second
// formulation gives -- a calendar walked one day at a time with the Gregorian leap rule, and the
// digits date_format prints -- and days_of (the walk's inverse) must give the day back.  Then
// ts_to_days against a floor computed in 128 bits, at the edges of every day near the epoch, of
// the range and of int64.
#include <cstdint>
#include <cstdio>
#include <cstdlib>

#include "../deequ_amd/csrc/decimal.h"

using namespace dq;

static bool leap(int y) { return (y % 4 == 0 && y % 100 != 0) || y % 400 == 0; }
static int month_days(int y, int m) {
  static const int n[12] = {31, 28, 31, 30, 31, 30, 31, 31, 30, 31, 30, 31};
  return m == 2 && leap(y) ? 29 : n[m - 1];
}
static int digits(const char* p, int n) {
  int v = 0;
  for (int k = 0; k < n; ++k) v = v * 10 + (p[k] - '0');
  return v;
}

int main() {
  // 1582-10-15 is day -141427: 1970-01-01 is 0, and the walk below confirms it by arriving there
  int y = 1582, m = 10, d = 15;
  long checked = 0;
  bool saw_epoch = false;
  for (int64_t day = -141427;; ++day) {
    if (date_field(day, 0) != y || date_field(day, 1) != m || date_field(day, 2) != d) {
      fprintf(stderr, "day %lld: fields %d-%d-%d, expected %d-%d-%d\n", (long long)day, date_field(day, 0),
              date_field(day, 1), date_field(day, 2), y, m, d);
      return 1;
    }
    char buf[kFmtMax];
    const int n = date_format(day, buf);
    if (n != 10 || buf[4] != '-' || buf[7] != '-' || digits(buf, 4) != y || digits(buf + 5, 2) != m ||
        digits(buf + 8, 2) != d) {
      fprintf(stderr, "day %lld: text %.*s, expected %04d-%02d-%02d\n", (long long)day, n, buf, y, m, d);
      return 1;
    }
    // a timestamp anywhere inside the day belongs to it
    const int64_t us = 86400000000LL;
    if (ts_to_days(day * us) != day || ts_to_days(day * us + us - 1) != day || ts_to_days(day * us - 1) != day - 1) {
      fprintf(stderr, "day %lld: ts_to_days at its edges\n", (long long)day);
      return 1;
    }
    if (y == 1970 && m == 1 && d == 1) saw_epoch = day == 0;
    ++checked;
    if (y == 9999 && m == 12 && d == 31) break;
    if (++d > month_days(y, m)) {
      d = 1;
      if (++m > 12) {
        m = 1;
        ++y;
      }
    }
  }
  if (!saw_epoch || checked != 2932896 + 141427 + 1) {
    fprintf(stderr, "walked %ld days, epoch at day 0: %d\n", checked, (int)saw_epoch);
    return 1;
  }
  // floor division over the whole int64 range
  const int64_t probes[] = {0, -1, 1, 86399999999LL, 86400000000LL, -86400000000LL, -86400000001LL,
                            INT64_MAX, INT64_MIN, INT64_MIN + 1, INT64_MAX - 86400000000LL};
  for (int64_t p : probes) {
    __int128 q = (__int128)p / 86400000000LL;
    if ((__int128)p % 86400000000LL < 0) q -= 1;
    if ((__int128)ts_to_days(p) != q) {
      fprintf(stderr, "ts_to_days(%lld)\n", (long long)p);
      return 1;
    }
  }
  printf("date_fields_check: %ld days from 1582-10-15 to 9999-12-31 agree\n", checked);
  return 0;
}
