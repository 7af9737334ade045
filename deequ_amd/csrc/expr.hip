// expr.hip -- the generic predicate interpreter: materialises a `where` filter or a Compliance
// predicate that the planner could not fuse into a column task as two Arrow boolean bitmaps (value
// bits, validity bits), with Spark SQL three-valued logic (Analyzers.conditionalSelection,
// Analyzer.scala:385-408; Compliance.scala:37-53).
#include <hip/hip_runtime.h>

#include "device_util.h"
#include "kernels.h"
#include "jfmt.h"
#include "parse_double.h"

namespace dq {

// ------------------------------------------------------------------------------------------------
// Generic predicate evaluation (the slow path for expressions that the planner cannot fuse):
// a postfix program over typed values with Kleene logic; one lane per row, results ballot-packed
// into Arrow boolean bitmaps (value bits, validity bits).
// ------------------------------------------------------------------------------------------------
struct V {
  int32_t tag;  // 0 NULL, 1 BOOL, 2 I64, 3 F64, 4 STR, 5 DECIMAL (i = low word, d = high word's
                // bits, len = scale), 6 DATE (i = days), 7 TIMESTAMP (i = microseconds)
  int32_t len;
  int64_t i;
  double d;
  const uint8_t* p;
};

DQ_DEV int cmp_str(const uint8_t* a, int32_t la, const uint8_t* b, int32_t lb) {
  DevBytes ra{a}, rb{b};
  int32_t n = la < lb ? la : lb;
  for (int32_t k = 0; k < n; ++k) {
    int32_t d = (int32_t)ra.u8(k) - (int32_t)rb.u8(k);
    if (d) return d < 0 ? -1 : 1;
  }
  return la == lb ? 0 : (la < lb ? -1 : 1);
}

// three-way compare of two non-NULL values; returns 2 when incomparable.  kText: the interpreter
// instantiation that also compares dates (int days) and timestamps (int64 microseconds) with
// their own kind (dq_plan_create admits no other pairing: the host casts one side to string)
template <bool kText>
DQ_DEV int cmp_vals(const V& a, const V& b) {
  if constexpr (kText) {
    if (a.tag >= 6 || b.tag >= 6) return a.tag == b.tag ? cmp3_i64(a.i, b.i) : 2;
  }
  if (a.tag == 5 && b.tag == 5) {  // unscaled at one scale (the plan aligns a literal's scale)
    const int64_t ah = __builtin_bit_cast(int64_t, a.d), bh = __builtin_bit_cast(int64_t, b.d);
    if (ah != bh) return ah < bh ? -1 : 1;
    if (a.i == b.i) return 0;
    return (uint64_t)a.i < (uint64_t)b.i ? -1 : 1;
  }
  if (a.tag >= 5 || b.tag >= 5) return 2;  // (dq_plan_create admits no other pairing)
  if (a.tag == 4 && b.tag == 4) return cmp_str(a.p, a.len, b.p, b.len);
  if (a.tag == 4 || b.tag == 4) return 2;
  if (a.tag == 3 || b.tag == 3) {
    double x = a.tag == 3 ? a.d : (double)a.i, y = b.tag == 3 ? b.d : (double)b.i;
    return cmp3_f64(x, y);
  }
  return cmp3_i64(a.i, b.i);
}

// java.lang.Double.parseDouble (what Spark 2.2's Cast(StringType -> DoubleType) calls, and with it
// every `string <op> number` comparison through PromoteStrings): the complete parser of
// parse_double.h -- every form of Double.valueOf's grammar (decimal with exponent and suffix, NaN,
// Infinity, hex), correctly rounded, the exact multi-word fallback included.  Returns false where
// Java throws NumberFormatException -> NULL.  The parser reads s[0, len) with plain byte loads;
// DevBytes::u8(k) returns that same byte (it exists so that wider loads stay inside the
// allocation), so the two are equivalent here.
DQ_DEV bool parse_f64(const uint8_t* s, int32_t len, double& out) {
  int flags;
  return castp::parse_double(s, len, out, flags);
}

// ------------------------------------------------------------------------------------------------
// Arithmetic and scalar functions (DQ_X_ARITH / DQ_X_FUNC): Spark 2.2 semantics in the result type
// the host computed (numericPrecedence; Division: always double).  Operands are numbers by the
// host's typing (tag 2 or 3; a boolean counts as its integer); anything else gives NULL.
// ------------------------------------------------------------------------------------------------
constexpr V kNullV{0, 0, 0, 0.0, nullptr};

// an integral result at the width of its type: Java's wrap-around (a sign extension of the low bits)
DQ_DEV int64_t wrap_int(int64_t v, int rt) {
  switch (rt) {
    case DQ_INT8: return (int8_t)v;
    case DQ_INT16: return (int16_t)v;
    case DQ_INT32: return (int32_t)v;
    default: return v;
  }
}

// a numeric value in the type `rt` (Spark's Cast to the common type; never narrows an integer)
DQ_DEV V to_num_type(V a, int rt) {
  if (a.tag == 0) return kNullV;
  if (a.tag > 3) return kNullV;
  if (rt == DQ_FLOAT32) {
    const float f = a.tag == 3 ? (float)a.d : (float)a.i;  // (float)long: one rounding
    return V{3, 1, 0, (double)f, nullptr};
  }
  if (rt == DQ_FLOAT64) return V{3, 0, 0, a.tag == 3 ? a.d : (double)a.i, nullptr};
  return a.tag == 3 ? kNullV : V{2, 0, a.i, 0.0, nullptr};
}

DQ_DEV V arith_eval(const V& a, const V& b, int which, int rt) {
  const bool unary = which == DQ_AR_NEG;
  if (a.tag == 0 || a.tag > 3 || (!unary && (b.tag == 0 || b.tag > 3))) return kNullV;
  if (rt == DQ_FLOAT32) {
    const float x = a.tag == 3 ? (float)a.d : (float)a.i;
    const float y = unary ? 0.0f : (b.tag == 3 ? (float)b.d : (float)b.i);
    float r;
    switch (which) {
      case DQ_AR_ADD: r = x + y; break;
      case DQ_AR_SUB: r = x - y; break;
      case DQ_AR_MUL: r = x * y; break;
      case DQ_AR_MOD:
        if (y == 0.0f) return kNullV;
        r = fmodf(x, y);
        break;
      case DQ_AR_NEG: r = -x; break;
      default: return kNullV;  // (a division is always double: dq_plan_create)
    }
    return V{3, 1, 0, (double)r, nullptr};
  }
  if (rt == DQ_FLOAT64) {
    const double x = a.tag == 3 ? a.d : (double)a.i;
    const double y = unary ? 0.0 : (b.tag == 3 ? b.d : (double)b.i);
    double r;
    switch (which) {
      case DQ_AR_ADD: r = x + y; break;
      case DQ_AR_SUB: r = x - y; break;
      case DQ_AR_MUL: r = x * y; break;
      case DQ_AR_DIV:
        if (y == 0.0) return kNullV;
        r = x / y;
        break;
      case DQ_AR_MOD:
        if (y == 0.0) return kNullV;
        r = fmod(x, y);
        break;
      default: r = -x; break;
    }
    return V{3, 0, 0, r, nullptr};
  }
  if (a.tag == 3 || (!unary && b.tag == 3)) return kNullV;  // (an integral result of a double)
  const uint64_t x = (uint64_t)a.i, y = unary ? 0 : (uint64_t)b.i;
  uint64_t r;
  switch (which) {
    case DQ_AR_ADD: r = x + y; break;
    case DQ_AR_SUB: r = x - y; break;
    case DQ_AR_MUL: r = x * y; break;
    case DQ_AR_MOD:
      if (b.i == 0) return kNullV;
      r = b.i == -1 ? 0 : (uint64_t)(a.i % b.i);  // (MIN % -1 is 0 in Java; it traps in C++)
      break;
    case DQ_AR_NEG: r = 0 - x; break;
    default: return kNullV;
  }
  return V{2, 0, wrap_int((int64_t)r, rt), 0.0, nullptr};
}

// UTF8String.numChars: one per lead byte (a malformed sequence counts its stray bytes)
DQ_DEV int32_t utf8_chars(const uint8_t* p, int32_t len) {
  DevBytes rd{p};
  int32_t n = 0;
  for (int32_t k = 0; k < len; ++k) n += (rd.u8(k) & 0xC0u) != 0x80u;
  return n;
}

// ------------------------------------------------------------------------------------------------
// LIKE (DQ_X_LIKE): the host-compiled pattern program (LIT / ANY1 / ANYSEQ tokens, validated by
// dq_plan_create) against a row's bytes.  The shapes `lit`, `lit%`, `%lit`, `%lit%`, `lit%lit`
// (LikeShape, decided on the host) are loops over a byte range known on entry; everything else runs
// like_general.
// ------------------------------------------------------------------------------------------------
// text[at .. at + len) == lit[0 .. len): four bytes at a time (a dword read that starts inside the
// string never leaves the allocation: DevBytes), then the tail
DQ_DEV bool bytes_eq(DevBytes text, int32_t at, DevBytes lit, int32_t lit_at, int32_t len) {
  int32_t k = 0;
  for (; k + 4 <= len; k += 4)
    if (text.u32(at + k) != lit.u32(lit_at + k)) return false;
  for (; k < len; ++k)
    if (text.u8(at + k) != lit.u8(lit_at + k)) return false;
  return true;
}

// bytes of the UTF-8 sequence a lead byte starts (a stray continuation byte: 1)
DQ_DEV int32_t utf8_len(uint32_t b) { return b < 0xC0u ? 1 : (b < 0xE0u ? 2 : (b < 0xF0u ? 3 : 4)); }

// %lit%: the first byte of the literal is looked for one aligned dword of text at a time
DQ_DEV bool like_contains(DevBytes text, int32_t n, DevBytes prog, int32_t lit_at, int32_t m) {
  if (m > n) return false;
  const uint32_t c0 = prog.u8(lit_at);
  const int32_t last = n - m;  // last start position
  const uintptr_t a = reinterpret_cast<uintptr_t>(text.p);
  const int32_t lead = (int32_t)(a & 3);  // text.p[0] is byte `lead` of its dword
  const uint32_t* w = reinterpret_cast<const uint32_t*>(a - lead);
  const int32_t n_dw = (lead + last) / 4 + 1;  // dwords holding a start position
  for (int32_t q = 0; q < n_dw; ++q) {
    const uint32_t x = w[q];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int32_t s = q * 4 + j - lead;
      if (s >= 0 && s <= last && ((x >> (8 * j)) & 0xffu) == c0 && bytes_eq(text, s + 1, prog, lit_at + 1, m - 1))
        return true;
    }
  }
  return false;
}

// The general case: the wildcard matcher with one backtrack point (the latest ANYSEQ and the text
// position it is tried at, which moves on by one code point per retry).  Every retry moves that
// position forward and at most every token runs between two retries, so (n + 2) * (tokens + 2)
// steps decide every row; the loop counts them and has no other way to keep running.
DQ_DEV bool like_general(DevBytes text, int32_t n, DevBytes prog, int32_t nb) {
  int32_t ti = 0, pi = 0, star_pi = -1, star_ti = 0;
  const int64_t bound = ((int64_t)n + 2) * ((int64_t)nb + 2);
  for (int64_t step = 0; step < bound; ++step) {
    if (pi < nb) {
      const uint32_t kind = prog.u8(pi);
      if (kind == DQ_LIKE_ANYSEQ) {
        star_pi = ++pi;
        star_ti = ti;
        continue;
      }
      if (kind == DQ_LIKE_ANY1) {
        if (ti < n) {
          ti += utf8_len(text.u8(ti));
          if (ti > n) ti = n;
          ++pi;
          continue;
        }
      } else {
        const int32_t len = (int32_t)(prog.u8(pi + 1) | (prog.u8(pi + 2) << 8));
        if (len <= n - ti && bytes_eq(text, ti, prog, pi + 3, len)) {
          ti += len;
          pi += 3 + len;
          continue;
        }
      }
    } else if (ti == n) {
      return true;
    }
    // mismatch: retry the latest ANYSEQ one code point further on
    if (star_pi < 0 || star_ti >= n) return false;
    star_ti += utf8_len(text.u8(star_ti));
    if (star_ti > n) star_ti = n;
    ti = star_ti;
    pi = star_pi;
  }
  return false;
}

DQ_DEV bool like_match(const uint8_t* s, int32_t n, const uint8_t* program, int32_t nb, int shape) {
  const DevBytes text{s}, prog{program};
  if (shape == LK_GENERAL) return like_general(text, n, prog, nb);
  if (shape == LK_ALL) return true;
  // a fast shape's literals are whole LIT tokens [kind, u16 length, bytes]; the first one follows
  // the leading ANYSEQ of %lit and %lit% (the empty pattern has none: length 0)
  const int32_t t1 = shape == LK_SUFFIX || shape == LK_CONTAINS ? 1 : 0;
  const int32_t l1 = nb >= 3 ? (int32_t)(prog.u8(t1 + 1) | (prog.u8(t1 + 2) << 8)) : 0;
  switch (shape) {
    case LK_EQ: return n == l1 && bytes_eq(text, 0, prog, 3, l1);
    case LK_PREFIX: return n >= l1 && bytes_eq(text, 0, prog, 3, l1);
    case LK_SUFFIX: return n >= l1 && bytes_eq(text, n - l1, prog, 4, l1);
    case LK_CONTAINS: return like_contains(text, n, prog, 4, l1);
    case LK_ENDS: {
      const int32_t at2 = 3 + l1 + 1;  // the second LIT token, after the ANYSEQ
      const int32_t l2 = (int32_t)(prog.u8(at2 + 1) | (prog.u8(at2 + 2) << 8));
      return n >= l1 + l2 && bytes_eq(text, 0, prog, 3, l1) && bytes_eq(text, n - l2, prog, at2 + 3, l2);
    }
    default: return false;
  }
}

// Spark's Cast(x AS STRING) of a non-NULL, non-string value into buf (kFmtMax bytes hold every
// form: decimal.h); returns the length.  What XI_REGEX prints inline, for XI_CAST_STR.
DQ_DEV int32_t value_text(const V& a, char* buf) {
  if (a.tag == 5) return dec_format((uint64_t)a.i, __builtin_bit_cast(int64_t, a.d), a.len, buf);
  if (a.tag == 6) return date_format(a.i, buf);
  if (a.tag == 7) return ts_format(a.i, buf);
  if (a.tag == 3) return a.len ? jfmt::float_to_java((float)a.d, buf) : jfmt::double_to_java(a.d, buf);
  int nb = 0;
  if (a.tag == 1) {
    const char* t = a.i ? "true" : "false";
    for (; t[nb]; ++nb) buf[nb] = t[nb];
    return nb;
  }
  uint64_t m = a.i < 0 ? 0ULL - (uint64_t)a.i : (uint64_t)a.i;
  char tmp[20];
  int nd = 0;
  do {
    tmp[nd++] = (char)('0' + m % 10);
    m /= 10;
  } while (m);
  if (a.i < 0) buf[nb++] = '-';
  while (nd) buf[nb++] = tmp[--nd];
  return nb;
}

// The day count a date function reads: a date's own, a timestamp's day in UTC; false otherwise
// (NULL included)
DQ_DEV bool date_arg(const V& a, int64_t& days) {
  if (a.tag == 6) days = a.i;
  else if (a.tag == 7) days = ts_to_days(a.i);
  else return false;
  return true;
}

// The date functions of DQ_X_FUNC over the top of the stack (two-argument ones: a = the first
// argument, b = the second); NULL on a NULL argument
DQ_DEV V date_func(int which, const V& a, const V& b) {
  int64_t x, y;
  if (!date_arg(a, x)) return kNullV;
  switch (which) {
    case DQ_FN_YEAR: return V{2, 0, date_field(x, 0), 0.0, nullptr};
    case DQ_FN_MONTH: return V{2, 0, date_field(x, 1), 0.0, nullptr};
    case DQ_FN_DAYOFMONTH: return V{2, 0, date_field(x, 2), 0.0, nullptr};
    case DQ_FN_TO_DATE: return V{6, 0, x, 0.0, nullptr};
    case DQ_FN_DATEDIFF:
      if (!date_arg(b, y)) return kNullV;
      return V{2, 0, (int32_t)((uint64_t)x - (uint64_t)y), 0.0, nullptr};
    case DQ_FN_DATE_ADD:
    case DQ_FN_DATE_SUB: {  // Int addition: wraps at 32 bits
      if (b.tag != 2) return kNullV;
      const uint64_t n = (uint64_t)b.i;
      return V{6, 0, (int32_t)(which == DQ_FN_DATE_ADD ? (uint64_t)x + n : (uint64_t)x - n), 0.0, nullptr};
    }
    default: return kNullV;
  }
}

// The interpreter.  kText = false is the program set of every plan without a date / timestamp
// value or a cast to string; kText = true adds XI_CAST_STR, XI_DATE, XI_TIMESTAMP, the date
// functions and date / timestamp comparisons, with kTextSlots per-lane text slots in private
// memory for the printed values (kernels.h).  Two instantiations, so that the first keeps the
// registers and scratch it had before the second existed.
template <bool kText>
DQ_DEV void expr_body(const XInstr* __restrict__ prog, int n_instr, const DevCol* __restrict__ cols,
                      const uint8_t* __restrict__ pool, int64_t rows, uint64_t* __restrict__ out_val,
                      uint64_t* __restrict__ out_vld) {
  const int lane = threadIdx.x & 63;
  const int64_t wave = ((int64_t)blockIdx.x * kBlock + threadIdx.x) >> 6;
  const int64_t n_waves = ((int64_t)gridDim.x * kBlock) >> 6;
  const int64_t n_words = (rows + 63) >> 6;
  for (int64_t w = wave; w < n_words; w += n_waves) {
    const int64_t r = w * 64 + lane;
    V st[kMaxStack];
    // printed values: dword aligned and a whole number of dwords each, so that the aligned dword
    // loads of DevBytes (cmp_str, like_match, utf8_chars, the regex walk) stay inside a slot
    alignas(8) char text[kText ? kTextSlots : 1][kFmtMax];
    static_assert(kFmtMax % 8 == 0 && kFmtMax >= jfmt::kMaxChars, "a slot holds every printed value");
    int sp = 0;
    bool in_range = r < rows;
    if (in_range) {
      for (int pc = 0; pc < n_instr; ++pc) {
        const XInstr ins = prog[pc];
        switch (ins.op) {
          case XI_COL: {
            const DevCol& c = cols[ins.a];
            V v{};
            const int tid = DQ_TYPE_ID(c.type);
            if (!bit1(c.valid, r)) {
              v.tag = 0;
            } else if (tid == DQ_DECIMAL128) {
              const uint64_t* dv = reinterpret_cast<const uint64_t*>(c.values) + 2 * r;
              v.tag = 5;
              v.i = (int64_t)dv[0];
              v.d = __builtin_bit_cast(double, dv[1]);
              v.len = DQ_DECIMAL_SCALE(c.type);
            } else if (tid == DQ_DATE32) {
              v.tag = 6;
              v.i = reinterpret_cast<const int32_t*>(c.values)[r];
            } else if (tid == DQ_TIMESTAMP_US) {
              v.tag = 7;
              v.i = reinterpret_cast<const int64_t*>(c.values)[r];
            } else if (c.type == DQ_UTF8) {
              const int32_t* off = reinterpret_cast<const int32_t*>(c.values);
              v.tag = 4;
              v.p = c.data + off[r];
              v.len = off[r + 1] - off[r];
            } else if (c.type == DQ_BOOL) {
              v.tag = 1;
              v.i = bit1(reinterpret_cast<const uint8_t*>(c.values), r);
            } else if (is_float_type(c.type)) {
              v.tag = 3;
              v.len = c.type == DQ_FLOAT32;  // the cast to string prints a float as Float.toString
              v.d = load_f64(c.type, c.values, r);
            } else {
              v.tag = 2;
              v.i = load_i64(c.type, c.values, r);
            }
            st[sp++] = v;
            break;
          }
          case XI_NULL: st[sp++] = V{0, 0, 0, 0.0, nullptr}; break;
          case XI_BOOL: st[sp++] = V{1, 0, ins.imm, 0.0, nullptr}; break;
          case XI_I64: st[sp++] = V{2, 0, ins.imm, 0.0, nullptr}; break;
          case XI_F64: st[sp++] = V{3, 0, 0, __builtin_bit_cast(double, ins.imm), nullptr}; break;
          case XI_DEC128: st[sp++] = V{5, 0, ins.imm, 0.0, nullptr}; break;
          case XI_DEC128_HI: st[sp - 1].d = __builtin_bit_cast(double, ins.imm); break;
          case XI_STR: st[sp++] = V{4, ins.a, 0, 0.0, pool + ins.imm}; break;
          case XI_IS_NULL: st[sp - 1] = V{1, 0, st[sp - 1].tag == 0 ? 1 : 0, 0.0, nullptr}; break;
          case XI_IS_NOT_NULL: st[sp - 1] = V{1, 0, st[sp - 1].tag != 0 ? 1 : 0, 0.0, nullptr}; break;
          case XI_NOT:
            if (st[sp - 1].tag != 0) st[sp - 1].i = st[sp - 1].i ? 0 : 1;
            break;
          case XI_AND: {
            V b = st[--sp];
            V a = st[sp - 1];
            // Kleene: FALSE dominates, then NULL
            bool af = a.tag != 0 && !a.i, bf = b.tag != 0 && !b.i;
            if (af || bf) st[sp - 1] = V{1, 0, 0, 0.0, nullptr};
            else if (a.tag == 0 || b.tag == 0) st[sp - 1] = V{0, 0, 0, 0.0, nullptr};
            else st[sp - 1] = V{1, 0, 1, 0.0, nullptr};
            break;
          }
          case XI_OR: {
            V b = st[--sp];
            V a = st[sp - 1];
            bool at = a.tag != 0 && a.i, bt = b.tag != 0 && b.i;
            if (at || bt) st[sp - 1] = V{1, 0, 1, 0.0, nullptr};
            else if (a.tag == 0 || b.tag == 0) st[sp - 1] = V{0, 0, 0, 0.0, nullptr};
            else st[sp - 1] = V{1, 0, 0, 0.0, nullptr};
            break;
          }
          case XI_CMP: {
            V b = st[--sp];
            V a = st[sp - 1];
            if (ins.a == DQ_X_EQ_NULL_SAFE) {
              int eq;
              if (a.tag == 0 || b.tag == 0) eq = (a.tag == 0 && b.tag == 0);
              else eq = cmp_vals<kText>(a, b) == 0;
              st[sp - 1] = V{1, 0, eq, 0.0, nullptr};
            } else if (a.tag == 0 || b.tag == 0) {
              st[sp - 1] = V{0, 0, 0, 0.0, nullptr};
            } else {
              int c = cmp_vals<kText>(a, b);
              if (c == 2) st[sp - 1] = V{0, 0, 0, 0.0, nullptr};
              else st[sp - 1] = V{1, 0, (op_mask(ins.a) >> (c + 1)) & 1, 0.0, nullptr};
            }
            break;
          }
          case XI_IN: {
            const int n = ins.a;
            const int base = sp - n - 1;
            V x = st[base];
            V res{0, 0, 0, 0.0, nullptr};
            if (x.tag != 0) {
              bool found = false, saw_null = false;
              for (int q = 0; q < n; ++q) {
                const V& it = st[base + 1 + q];
                if (it.tag == 0) {
                  saw_null = true;
                } else if (cmp_vals<kText>(x, it) == 0) {
                  found = true;
                }
              }
              if (found) res = V{1, 0, 1, 0.0, nullptr};
              else if (!saw_null) res = V{1, 0, 0, 0.0, nullptr};
            }
            sp = base;
            st[sp++] = res;
            break;
          }
          case XI_CAST_F64: {  // ins.a = 1: CAST AS FLOAT (rounded to float, prints as Float.toString)
            V& a = st[sp - 1];
            const bool to_f32 = ins.a != 0;
            if (a.tag == 2 || a.tag == 1) {
              a.d = to_f32 ? (double)(float)a.i : (double)a.i;  // (float)long: one rounding
              a.tag = 3;
            } else if (a.tag == 5) {  // Decimal.toDouble: correctly rounded
              a.d = dec_to_double((uint64_t)a.i, __builtin_bit_cast(int64_t, a.d), a.len);
              a.tag = 3;
            } else if (a.tag == 4) {
              double d;
              if (parse_f64(a.p, a.len, d)) a = V{3, 0, 0, d, nullptr};
              else a = V{0, 0, 0, 0.0, nullptr};
            } else if (a.tag == 3 && to_f32) {
              a.d = (double)(float)a.d;
            }
            // the type of the result decides how a regex prints it (Double / Float.toString)
            if (a.tag == 3) a.len = to_f32 ? 1 : 0;
            break;
          }
          case XI_REGEX: {  // find() over x's text with a compiled automaton (regex.py)
            V& a = st[sp - 1];
            if (a.tag == 0) {  // NULL: null_mode 1 (PatternMatch's otherwise(0)) -> FALSE
              if (ins.a) a = V{1, 0, 0, 0.0, nullptr};
              else a = V{0, 0, 0, 0.0, nullptr};
              break;
            }
            const uint8_t* blob = pool + ins.imm;
            const int32_t ns = reinterpret_cast<const int32_t*>(blob)[0];
            const int32_t nc = reinterpret_cast<const int32_t*>(blob)[1];
            uint32_t q = (uint32_t)reinterpret_cast<const int32_t*>(blob)[2];
            const uint8_t* cls = blob + 16;
            const uint8_t* status = blob + 16 + 256;
            const uint16_t* nx = reinterpret_cast<const uint16_t*>(blob + 16 + 256 + ((ns + 3) & ~3));
            if (a.tag == 4) {
              DevBytes rd{a.p};
              for (int32_t k = 0; k < a.len && !status[q]; ++k) q = nx[q * nc + cls[rd.u8(k)]];
            } else {  // Spark's cast to string: decimal integer, true / false, Double.toString,
                      // BigDecimal.toString, yyyy-MM-dd [HH:mm:ss[.f]] (decimal.h)
              char buf[kFmtMax > jfmt::kMaxChars ? kFmtMax : jfmt::kMaxChars];
              int nb = 0;
              if (a.tag == 5) {
                nb = dec_format((uint64_t)a.i, __builtin_bit_cast(int64_t, a.d), a.len, buf);
              } else if (a.tag == 6) {
                nb = date_format(a.i, buf);
              } else if (a.tag == 7) {
                nb = ts_format(a.i, buf);
              } else if (a.tag == 3) {
                nb = a.len ? jfmt::float_to_java((float)a.d, buf) : jfmt::double_to_java(a.d, buf);
              } else if (a.tag == 1) {
                const char* t = a.i ? "true" : "false";
                for (; t[nb]; ++nb) buf[nb] = t[nb];
              } else {
                uint64_t m = a.i < 0 ? 0ULL - (uint64_t)a.i : (uint64_t)a.i;
                char tmp[20];
                int nd = 0;
                do {
                  tmp[nd++] = (char)('0' + m % 10);
                  m /= 10;
                } while (m);
                if (a.i < 0) buf[nb++] = '-';
                while (nd) buf[nb++] = tmp[--nd];
              }
              for (int k = 0; k < nb && !status[q]; ++k) q = nx[q * nc + cls[(uint8_t)buf[k]]];
            }
            if (!status[q]) q = nx[q * nc + nc - 1];  // end of text
            a = V{1, 0, status[q] == 1 ? 1 : 0, 0.0, nullptr};
            break;
          }
          case XI_LIKE: {  // a = program bytes | LikeShape << 16
            V& a = st[sp - 1];
            if (a.tag != 4) {  // NULL (or, past the host's typing, not a string): NULL
              a = kNullV;
              break;
            }
            const bool m = like_match(a.p, a.len, pool + ins.imm, ins.a & 0xffff, ins.a >> 16);
            a = V{1, 0, m ? 1 : 0, 0.0, nullptr};
            break;
          }
          case XI_ARITH: {  // a = dq_arith_op | result dq_type << 8
            const int which = ins.a & 0xff, rt = ins.a >> 8;
            if (which != DQ_AR_NEG) --sp;
            st[sp - 1] = arith_eval(st[sp - 1], st[which != DQ_AR_NEG ? sp : sp - 1], which, rt);
            break;
          }
          case XI_FUNC: {  // a = dq_func | result dq_type << 8, imm = number of arguments
            const int which = ins.a & 0xff, rt = ins.a >> 8;
            if constexpr (kText) {
              if (which >= DQ_FN_YEAR) {
                if (ins.imm == 2) --sp;
                st[sp - 1] = date_func(which, st[sp - 1], st[ins.imm == 2 ? sp : sp - 1]);
                break;
              }
            }
            V& a = st[sp - 1];
            if (which == DQ_FN_COALESCE) {  // the first non-NULL argument, in the common type
              const int n = (int)ins.imm;
              const int base = sp - n;
              V res = kNullV;
              for (int q = n - 1; q >= 0; --q)
                if (st[base + q].tag != 0) res = st[base + q];
              sp = base;
              st[sp++] = rt == DQ_UTF8 ? res : to_num_type(res, rt);
            } else if (which == DQ_FN_ISNAN) {  // FALSE, not NULL, on a NULL operand
              a = V{1, 0, a.tag == 3 && a.d != a.d ? 1 : 0, 0.0, nullptr};
            } else if (which == DQ_FN_LENGTH) {
              a = a.tag == 4 ? V{2, 0, utf8_chars(a.p, a.len), 0.0, nullptr} : kNullV;
            } else if (a.tag == 3) {  // DQ_FN_ABS
              a.d = __builtin_fabs(a.d);
            } else if (a.tag == 2) {
              a.i = wrap_int((int64_t)(a.i < 0 ? 0 - (uint64_t)a.i : (uint64_t)a.i), rt);
            } else {
              a = kNullV;
            }
            break;
          }
          case XI_CAST_STR:  // a = the text slot dq_plan_create assigned
            if constexpr (kText) {
              V& a = st[sp - 1];
              if (a.tag != 0 && a.tag != 4) {
                char* buf = text[ins.a & (kTextSlots - 1)];
                const int32_t nb = value_text(a, buf);
                a = V{4, nb, 0, 0.0, reinterpret_cast<const uint8_t*>(buf)};
              }
            }
            break;
          case XI_DATE:
            if constexpr (kText) st[sp++] = V{6, 0, ins.imm, 0.0, nullptr};
            break;
          case XI_TIMESTAMP:
            if constexpr (kText) st[sp++] = V{7, 0, ins.imm, 0.0, nullptr};
            break;
          default: break;
        }
      }
    }
    if constexpr (!kText) (void)text;
    const V& res = st[0];
    const bool valid = in_range && sp == 1 && res.tag != 0;
    const bool truth = valid && res.i != 0;
    const uint64_t bv = __ballot(truth);
    const uint64_t bn = __ballot(valid);
    if (lane == 0) {
      out_val[w] = bv;
      out_vld[w] = bn;
    }
  }
}

__global__ void __launch_bounds__(kBlock) expr_kernel(const XInstr* __restrict__ prog, int n_instr,
                                                      const DevCol* __restrict__ cols,
                                                      const uint8_t* __restrict__ pool, int64_t rows,
                                                      uint64_t* __restrict__ out_val,
                                                      uint64_t* __restrict__ out_vld) {
  expr_body<false>(prog, n_instr, cols, pool, rows, out_val, out_vld);
}

__global__ void __launch_bounds__(kBlock) expr_text_kernel(const XInstr* __restrict__ prog, int n_instr,
                                                           const DevCol* __restrict__ cols,
                                                           const uint8_t* __restrict__ pool, int64_t rows,
                                                           uint64_t* __restrict__ out_val,
                                                           uint64_t* __restrict__ out_vld) {
  expr_body<true>(prog, n_instr, cols, pool, rows, out_val, out_vld);
}

// ------------------------------------------------------------------------------------------------
// PatternMatch over a utf8 column (the program [XI_COL c, XI_REGEX]): its own kernel instead of the
// interpreter walk.  The automaton arrives fused (RegexTable, built on the host by
// build_regex_table): one u8 successor per (state, byte) -- the byte classes folded in, terminal
// states (sticky accept / dead) made self-loops -- then per state bit 0 = accepted after the
// end-of-text symbol, bit 1 = terminal.  The block stages it in LDS with 16-byte copies, so a byte
// costs one dependent LDS read.  A lane walks four rows (rows r, r + 64, r + 128 and r + 192 of a
// 256-row group of four bitmap words: four independent chains in flight), loading each string 16
// bytes at a time with one unaligned load -- byte-wise and bounds-checked within 16 bytes of the
// data buffer's end; a row stops at its end or in a terminal state, the wave when every row has.
// ------------------------------------------------------------------------------------------------
__device__ __forceinline__ uint4 ldg128_unaligned(const uint8_t* p) {
  typedef unsigned int v4u __attribute__((ext_vector_type(4), aligned(1)));
  const v4u v = *(const __attribute__((address_space(1))) v4u*)p;
  return make_uint4(v.x, v.y, v.z, v.w);
}

struct RxRow {
  int32_t pos, end;  // byte range left to walk in the data buffer (Arrow utf8: int32 offsets)
  uint32_t q;
  DQ_DEV bool active(const uint8_t* fin) const { return pos < end && !(fin[q] & 2u); }
  // the next (at most) 16 bytes of the row
  DQ_DEV void chunk(const uint8_t* data, int32_t data_len, uint32_t (&w)[4]) const {
    if ((int64_t)pos + 16 <= (int64_t)data_len) {
      const uint4 u = ldg128_unaligned(data + pos);
      w[0] = u.x;
      w[1] = u.y;
      w[2] = u.z;
      w[3] = u.w;
    } else {  // the buffer's last bytes: no read past its end
#pragma unroll
      for (int k = 0; k < 4; ++k) w[k] = 0;
      for (int j = 0; j < 16 && j < end - pos; ++j) w[j >> 2] |= (uint32_t)data[pos + j] << (8 * (j & 3));
    }
  }
};

// HR: rows per lane (independent chains of dependent LDS reads in flight)
template <int HR>
__global__ void __launch_bounds__(kBlock, HR == 4 ? 4 : 1)
regex_find_kernel(const uint8_t* __restrict__ valid, const int32_t* __restrict__ off,
                  const uint8_t* __restrict__ data, int64_t rows, const uint8_t* __restrict__ table,
                  int32_t ns, int32_t start, int32_t null_mode, uint64_t* __restrict__ out_val,
                  uint64_t* __restrict__ out_vld) {
  extern __shared__ uint4 rx_lds[];
  uint8_t* T = reinterpret_cast<uint8_t*>(rx_lds);
  const uint8_t* fin = T + (size_t)ns * 256;
  const int n16 = (ns * 257 + 15) / 16;
  for (int i = threadIdx.x; i < n16; i += kBlock) rx_lds[i] = reinterpret_cast<const uint4*>(table)[i];
  __syncthreads();
  const int lane = threadIdx.x & 63;
  const int64_t wave = ((int64_t)blockIdx.x * kBlock + threadIdx.x) >> 6;
  const int64_t n_waves = ((int64_t)gridDim.x * kBlock) >> 6;
  const int64_t n_words = (rows + 63) >> 6;
  const int32_t data_len = rows ? off[rows] : 0;
  for (int64_t w = HR * wave; w < n_words; w += HR * n_waves) {
    RxRow rr[HR];
    bool vld[HR];
#pragma unroll
    for (int h = 0; h < HR; ++h) {
      const int64_t r = (w + h) * 64 + lane;
      vld[h] = r < rows && bit1(valid, r);
      rr[h].q = (uint32_t)start;
      rr[h].pos = vld[h] ? off[r] : 0;
      rr[h].end = vld[h] ? off[r + 1] : 0;
    }
    auto any_active = [&]() {
      bool x = false;
#pragma unroll
      for (int h = 0; h < HR; ++h) x = x || rr[h].active(fin);
      return x;
    };
    while (__ballot(any_active())) {
      uint32_t c[HR][4];
#pragma unroll
      for (int h = 0; h < HR; ++h) {
        if (rr[h].active(fin)) rr[h].chunk(data, data_len, c[h]);
        else c[h][0] = c[h][1] = c[h][2] = c[h][3] = 0;
      }
#pragma unroll
      for (int j = 0; j < 16; ++j) {
#pragma unroll
        for (int h = 0; h < HR; ++h) {
          const uint32_t b = (c[h][j >> 2] >> (8 * (j & 3))) & 0xffu;
          const uint32_t nq = T[rr[h].q * 256u + b];
          rr[h].q = j < rr[h].end - rr[h].pos ? nq : rr[h].q;
        }
      }
#pragma unroll
      for (int h = 0; h < HR; ++h) rr[h].pos = rr[h].end - rr[h].pos > 16 ? rr[h].pos + 16 : rr[h].end;
    }
#pragma unroll
    for (int h = 0; h < HR; ++h) {
      // NULL: null_mode 1 (PatternMatch's otherwise(0)) -> FALSE, else NULL
      const bool res_valid = (w + h) * 64 + lane < rows && (vld[h] || null_mode);
      const bool truth = vld[h] && (fin[rr[h].q] & 1u);
      const uint64_t bv = __ballot(truth), bn = __ballot(res_valid);
      if (lane == 0 && w + h < n_words) {
        out_val[w + h] = bv;
        out_vld[w + h] = bn;
      }
    }
  }
}

// ------------------------------------------------------------------------------------------------
// Host-side launchers
// ------------------------------------------------------------------------------------------------
hipError_t launch_expr(const XInstr* prog, int n_instr, bool text, const DevCol* cols,
                       const uint8_t* pool, int64_t rows, uint64_t* out_val, uint64_t* out_vld,
                       hipStream_t stream) {
  if (rows <= 0) return hipSuccess;
  int64_t words = (rows + 63) / 64;
  int64_t blocks = (words + 3) / 4;
  if (blocks > 4096) blocks = 4096;
  hipLaunchKernelGGL(text ? expr_text_kernel : expr_kernel, dim3((unsigned)blocks), dim3(kBlock), 0,
                     stream, prog, n_instr, cols, pool, rows, out_val, out_vld);
  return hipGetLastError();
}

hipError_t launch_regex(const uint8_t* valid, const int32_t* offsets, const uint8_t* data,
                        int64_t rows, const uint8_t* table, int ns, int start, int null_mode,
                        uint64_t* out_val, uint64_t* out_vld, hipStream_t stream) {
  if (rows <= 0) return hipSuccess;
  if (ns < 1 || ns > kRegexMaxStates) return hipErrorInvalidValue;
  constexpr int hr = 4;  // rows per lane
  const int64_t groups = ((rows + 63) / 64 + hr - 1) / hr;
  int64_t blocks = (groups + 3) / 4;
  if (blocks > 8192) blocks = 8192;
  const size_t lds = ((size_t)ns * 257 + 15) / 16 * 16;
  hipLaunchKernelGGL(regex_find_kernel<hr>, dim3((unsigned)blocks), dim3(kBlock), lds, stream, valid,
                     offsets, data, rows, table, ns, start, null_mode, out_val, out_vld);
  return hipGetLastError();
}

}  // namespace dq
