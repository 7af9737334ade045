"""Case tables, probes and expected values for tests/test_format_cases.py (host) and
tests/test_gpu_format_rows.py (device): plain helper, no GPU, no fixtures.

`x RLIKE p` over a non-string x matches Spark's cast of x to string.  expr_kernel's XI_REGEX case
(csrc/expr.hip) prints that text per lane into a scratch buffer: jfmt::double_to_java /
float_to_java (csrc/jfmt.h), dec_format, date_format and ts_format (csrc/decimal.h).  A Family here
is one operand (a column, or casts over one) over one table whose rows are the values at which
those printers can go wrong; its expected text per row is the oracle's (oracle/deequ_oracle.py:
Python's repr / numpy's Dragon4 digits, Decimal and datetime, laid out as Java does).

The device never hands the text back: it answers regex predicates.  So the text is pinned by
PROBES, a set of predicates that determines every byte of it.  For an alphabet S (symbols numbered
from 1) and a longest text Lmax:

  * for each position p < Lmax and each bit k of a symbol's number, `^\\p{ASCII}{p}[the symbols
    whose number has bit k]`: TRUE when the row's byte p is such a symbol;
  * `^\\p{ASCII}{L}$` for L in 1..Lmax: the length;
  * `[^S]`: a byte outside the alphabet; FALSE on every row.

The skip is spelled \\p{ASCII} and not `.`: the compiler (deequ_amd/regex.py) decodes UTF-8 under
`.`, about ten states per position, so `^.{25}$` has 258 states and a decimal's 42 positions above
400; every probe stays at or below the 255 states the fused tables hold (test_format_cases.py).
Over ASCII text the two spellings say the same, and a byte above 0x7f before position p makes every
later probe FALSE, which no row expects.

Expected truth vectors come from the oracle's text by plain indexing (text[p] in cls), no regex
engine; a NULL row is NULL.  The observable is the fingerprint pair of tests/regex_cases.py:
Sum(w, where=p) and Sum(w, where=NOT (p)) over random weights.

Lmax is the longest oracle text of the family plus one (so that a byte too many shows), capped by
the printers' buffer sizes jfmt::kMaxChars and kFmtMax, read from the headers.

Row placement (place): the values in order, NULLs inserted at rows 0, 63, 64, 255, 256, the last
row and either side of the cut into two device batches, which is no multiple of 64.
"""
import datetime
import os
import random
import re
import struct
from collections import namedtuple
from decimal import Decimal
from functools import lru_cache

import numpy as np

import regex_cases as RC
from oracle import deequ_oracle as O

Family = namedtuple("Family", "name operand column kind values results prints texts raw alphabet lmax cut")
Probe = namedtuple("Probe", "what pos bit cls pattern")

FLOAT_ALPHABET = "0123456789.-ENaInfity"
DECIMAL_ALPHABET = "0123456789.-E"
DATE_ALPHABET = "0123456789-"
TIMESTAMP_ALPHABET = "0123456789-: ."

DECIMAL_TYPES = ((9, 2), (18, 6), (38, 0), (38, 2), (38, 10), (38, 37), (38, 38))
I64_MIN, I64_MAX = RC.I64_MIN, RC.I64_MAX
EPOCH_DAY = datetime.date(1970, 1, 1)
EPOCH = datetime.datetime(1970, 1, 1)
_C = O._DEC_CTX

# Plan.explain() (deequ_amd/runners/engine.py) reads dq_plan_explain into 8192 bytes and the text
# is cut there without notice.  dq_plan_create itself bounds neither expressions nor tasks (only 32
# HLL tasks and a stack of 16 per expression).  A probe costs two materialised expressions (<= 56
# bytes each in explain) and three tasks (two numeric, <= 60 bytes, one boolmap, <= 76 bytes): at
# most 308 bytes, so 24 probes and the closing line fit; test_format_cases.py checks that they do.
EXPLAIN_BYTES = 8192
PROBES_PER_SCAN = 24
assert PROBES_PER_SCAN * 308 + 64 <= EXPLAIN_BYTES


def _header_constant(header, name):
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "deequ_amd", "csrc", header)
    with open(path) as f:
        return int(re.search(r"constexpr int %s = (\d+);" % name, f.read()).group(1))


K_MAX_CHARS = _header_constant("jfmt.h", "kMaxChars")
K_FMT_MAX = _header_constant("decimal.h", "kFmtMax")


# ------------------------------------------------------------------------------------------------
# Probes
# ------------------------------------------------------------------------------------------------
def _in_class(chars):
    return "".join("\\" + c if c in ".-" else c for c in chars)


@lru_cache(maxsize=None)
def probes(alphabet, lmax):
    number = {c: i + 1 for i, c in enumerate(alphabet)}
    out = []
    for p in range(lmax):
        for k in range(len(alphabet).bit_length()):
            cls = "".join(c for c in alphabet if (number[c] >> k) & 1)
            out.append(Probe("byte", p, k, cls, "^\\p{ASCII}{%d}[%s]" % (p, _in_class(cls))))
    for n in range(1, lmax + 1):
        out.append(Probe("length", n, None, None, "^\\p{ASCII}{%d}$" % n))
    out.append(Probe("alien", None, None, alphabet, "[^%s]" % _in_class(alphabet)))
    return tuple(out)


def probe_id(pr):
    return f"{pr.what} {pr.pos} bit {pr.bit} /{pr.pattern}/"


def probe_value(pr, text):
    """The probe's verdict on one non-NULL text: plain indexing, no regex engine."""
    if pr.what == "byte":
        return len(text) > pr.pos and text[pr.pos] in pr.cls
    if pr.what == "length":
        return len(text) == pr.pos
    return any(c not in pr.cls for c in text)


def truth(pr, texts):
    """int8 per row: 1 TRUE, 0 FALSE, -1 NULL (regex_cases.truth_code's form)."""
    return np.array([-1 if t is None else int(probe_value(pr, t)) for t in texts], np.int8)


def decode(alphabet, lmax, verdict):
    """The text that the verdicts of probes(alphabet, lmax) spell (verdict: probe -> bool), or a
    description of why they spell none."""
    ps = probes(alphabet, lmax)
    lengths = [pr.pos for pr in ps if pr.what == "length" and verdict(pr)]
    if len(lengths) != 1:
        return f"<lengths {lengths}>"
    number = [0] * lmax
    for pr in ps:
        if pr.what == "byte" and verdict(pr):
            number[pr.pos] |= 1 << pr.bit
    if any(number[lengths[0]:]):
        return f"<bytes past the length {lengths[0]}: {number}>"
    if any(not 1 <= x <= len(alphabet) for x in number[:lengths[0]]):
        return f"<symbol numbers {number[:lengths[0]]}>"
    if any(verdict(pr) for pr in ps if pr.what == "alien"):
        return "<a byte outside the alphabet>"
    return "".join(alphabet[x - 1] for x in number[:lengths[0]])


def chunks(ps, n=PROBES_PER_SCAN):
    return [ps[k:k + n] for k in range(0, len(ps), n)]


# ------------------------------------------------------------------------------------------------
# Row placement
# ------------------------------------------------------------------------------------------------
def _cut(n):
    c = n // 2
    return c + 37 if c % 64 == 0 else c


def null_rows(n):
    c = _cut(n)
    return sorted({r for r in RC.NULL_ROWS + (n - 1, c - 1, c) if 0 <= r < n})


def place(values):
    """(rows, cut): every value, in order, with NULLs inserted at null_rows(len(rows))."""
    n = len(values) + len(RC.NULL_ROWS) + 3
    while len(values) + len(null_rows(n)) != n:
        n = len(values) + len(null_rows(n))
    nulls, it = set(null_rows(n)), iter(values)
    rows = [None if r in nulls else next(it) for r in range(n)]
    assert sum(r is not None for r in rows) == len(values) and _cut(n) % 64
    return rows, _cut(n)


def _uniq(values, key=lambda v: v):
    seen, out = set(), []
    for v in values:
        if key(v) not in seen:
            seen.add(key(v))
            out.append(v)
    return out


# ------------------------------------------------------------------------------------------------
# double
# ------------------------------------------------------------------------------------------------
def d_bits(d):
    return struct.unpack("<Q", struct.pack("<d", d))[0]


def d_from(bits):
    return struct.unpack("<d", struct.pack("<Q", bits))[0]


def f_from(bits):
    return float(np.array([bits], np.uint32).view(np.float32)[0])


def f_bits(f):
    return int(np.array([f], np.float32).view(np.uint32)[0])


def double_values():
    rng = random.Random(20)
    out = []
    # every binary exponent: mantissa 0 (the binade edge, mm_shift == 0) and a random mantissa;
    # together every row of kPow5 / kPow5Inv.  Every third pair is negative.
    for k in range(-1074, 1024):
        sign = (1 << 63) if k % 3 == 0 else 0
        if k < -1022:
            edge = 1 << (k + 1074)
            body = edge | rng.getrandbits(k + 1074) if k > -1074 else edge
        else:
            edge = (k + 1023) << 52
            body = edge | rng.getrandbits(52)
        out += [d_from(sign | edge), d_from(sign | body)]
    # vr_tz / vm_tz: small integers times 5^q (exact up to q = 22, rounded from there), powers of
    # ten, halves at 15 to 17 digits
    for q in range(0, 24):
        out += [float(m * 5 ** q) for m in (1, 2, 3, 7, 12)]
    out += [float(f"1e{q}") for q in range(-30, 31)]
    out += [123456789012345.5, 1234567890123.5, 4503599627370495.5, 2251799813685247.5,
            999999999999999.5, 99999999999999.5, 1000000000000000.5, -562949953421311.5]
    # layout edges
    out += [0.001, 9.999999999999999e-4, 9999999.999999998, 1.0e7, 1.0e-4, 123456.789, 9999999.0,
            0.00099, 12345678.9, 100.0, 1.1, 0.1, -2.5]
    # one digit and 17 digits; exponents of 1, 2 and 3 digits with both signs
    out += [float(f"{d}e{k}") for d in (1, 5, 9) for k in (-320, -300, -100, -10, -5, -4, -3, -1, 0, 5, 6, 7,
                                                         9, 10, 22, 23, 99, 100, 300)]
    out += [-1.2345678901234567e-308, 1.2345678901234567e308, 0.30000000000000004, 1.0000000000000002,
            9.999999999999998e22, 1.2345678901234567e-5, -1.2345678901234567e10, 1.2345678901234567e-100,
            1.2345678901234567e7, 0.0012345678901234567, 1234567.8901234567]
    # specials
    out += [0.0, -0.0, float("inf"), float("-inf")]
    out += [d_from(b) for b in (0x7ff8000000000000, 0x7ff0000000000001, 0x7fffffffffffffff,
                                0xfff8000000000000, 0xfff0000000000001, 0x7ff4000000000abc)]
    out += [5e-324, -5e-324, d_from(0x0010000000000000), d_from(0x000fffffffffffff),
            d_from(0x0010000000000001), -d_from(0x0010000000000000), 1.7976931348623157e308,
            -1.7976931348623157e308]
    # integers up to 2^53
    out += [float(v) for v in (1, 2, 10, 1234567, 10000000, 2 ** 24, 2 ** 24 + 1, 2 ** 31, 999999999999,
                               2 ** 53 - 1, 2 ** 53, -(2 ** 53), 2 ** 53 - 2, 2 ** 52 + 1)]
    out += [float(rng.getrandbits(rng.randint(1, 53))) for _ in range(60)]
    # random bits and short decimals
    out += [d_from(rng.getrandbits(64)) for _ in range(200)]
    out += [round(rng.uniform(-1e8, 1e8), rng.randint(0, 7)) for _ in range(100)]
    return _uniq(out, d_bits)


def float_values():
    """float32 values, as floats."""
    rng = random.Random(21)
    bits = []
    for e in range(0, 255):
        sign = (1 << 31) if e % 3 == 0 else 0
        bits += [sign | e << 23, sign | e << 23 | rng.getrandbits(23)]
    bits += list(range(1, 65))
    bits += [f_bits(v) for v in (1.0e7, 9999999.0, 0.001, 9.999999e-4, 16777216.0, 0.1, 1.1, 3.2, -2.5,
                                 100.0, 123456.79, 1.0e-4, 3.4028235e38, -3.4028235e38, 1e10, 1e-10)]
    bits += [1, 0x80000001, 0x7f7fffff, 0x00800000, 0x007fffff, 0, 0x80000000, 0x7f800000, 0xff800000,
             0x7fc00000, 0x7f800001, 0xffc00000, 0xffffffff]
    bits += [rng.getrandbits(32) for _ in range(300)]
    return [f_from(b) for b in _uniq(bits)]


def to_f32(d):
    """Java's (float) of a double: one rounding to nearest even, overflow to infinity."""
    with np.errstate(over="ignore", invalid="ignore"):
        return float(np.float32(d))


def long_to_f32(v):
    """Java's (float) of a long, in integer arithmetic: 24 bits, ties to even."""
    m, drop = abs(v), max(0, abs(v).bit_length() - 24)
    q, rem = m >> drop, m & ((1 << drop) - 1)
    if drop and (rem > 1 << (drop - 1) or (rem == 1 << (drop - 1) and q & 1)):
        q += 1
    r = float(q << drop)            # exact: at most 24 significant bits below 2^64
    assert r == to_f32(r)
    return -r if v < 0 else r


def long_values():
    rng = random.Random(22)
    out = [0, 1, -1, 7, -10, 1234567, 10000000, 9999999, I64_MIN, I64_MAX, I64_MIN + 1, I64_MAX - 1]
    for b in (24, 25, 53, 54, 62):
        for d in (-3, -2, -1, 0, 1, 2, 3):
            out += [2 ** b + d, -(2 ** b + d)]
    # halfway between two floats, and between two doubles, at several magnitudes
    out += [(2 ** 24 + 1) << k for k in range(0, 38, 3)] + [(2 ** 24 + 3) << k for k in range(0, 38, 5)]
    out += [(2 ** 53 + 1) << k for k in range(0, 9)] + [(2 ** 53 + 3) << k for k in range(0, 9)]
    out += [rng.getrandbits(rng.randint(1, 63)) * rng.choice((1, -1)) for _ in range(300)]
    return _uniq(out)


# ------------------------------------------------------------------------------------------------
# decimal, date, timestamp
# ------------------------------------------------------------------------------------------------
def decimal_unscaled(p, s):
    rng = random.Random(100 * p + s)
    top = 10 ** p - 1
    out = [0]
    for k in range(0, p + 1):
        out += [v for v in (10 ** k, -(10 ** k), 10 ** k - 1, -(10 ** k - 1)) if abs(v) <= top]
    # the chunk edges of u128_to_digits, the 64-bit word edge
    edges = (2 ** 64 - 1, 2 ** 64, 2 ** 64 + 1, 10 ** 19 - 1, 10 ** 19, 10 ** 19 + 1, 2 * 10 ** 19 - 1,
             10 ** 38 - 1, 10 ** 38 - 10 ** 19, 2 ** 126)
    out += [v * sg for v in edges for sg in (1, -1) if v <= top]
    # adjusted exponent (digits - 1 - scale) of -6 and -7: plain against E notation
    for nd in (s - 5, s - 6):
        if 1 <= nd <= p:
            out += [int("7" + "3" * (nd - 1)), -int("9" * nd)]
    for _ in range(120):
        out.append(rng.randint(0, 10 ** rng.randint(1, p) - 1) * rng.choice((1, -1)))
    return _uniq(out)


def dec_value(u, s):
    return Decimal(u).scaleb(-s, context=_C)


def date_values():
    rng = random.Random(23)
    D = datetime.date
    out = [EPOCH_DAY, D(1969, 12, 31), D(1970, 1, 2), D(2000, 2, 29), D(2024, 2, 29), D(1900, 2, 28),
           D(1900, 3, 1), D(2100, 2, 28), D(2100, 3, 1), D(1, 1, 1), D(9999, 12, 31), D(1, 12, 31),
           D(1600, 2, 29), D(1582, 10, 15), D(9999, 1, 1), D(1000, 1, 1), D(999, 12, 31)]
    for y in (2024, 2023):
        for m in range(1, 13):
            first_of_next = D(y + 1, 1, 1) if m == 12 else D(y, m + 1, 1)
            out += [first_of_next - datetime.timedelta(days=1), D(y, m, 1)]
    out += [D.fromordinal(rng.randint(1, D(9999, 12, 31).toordinal())) for _ in range(300)]
    return _uniq(out)


def timestamp_values():
    rng = random.Random(24)
    T, day = datetime.datetime, datetime.timedelta(days=1)
    us = lambda n: datetime.timedelta(microseconds=n)  # noqa: E731
    out = []
    for base in (EPOCH, EPOCH - day, EPOCH + day):
        out += [base + us(f) for f in (0, 1, 100000, 120000, 999999)]
    out += [EPOCH - us(1), EPOCH - us(999999), EPOCH - us(1000000), EPOCH - us(1000001),
            EPOCH - us(86400 * 10 ** 6 - 1), EPOCH - us(86400 * 10 ** 6 + 1)]
    # 23:59:59.999999 and 00:00:00 on both sides of a day, month and year rollover, a leap day
    for d in (T(1970, 1, 2), T(1969, 12, 31), T(2021, 2, 1), T(2000, 1, 1), T(2024, 2, 29), T(2024, 3, 1),
              T(1900, 3, 1), T(2100, 3, 1), T(1969, 1, 1)):
        out += [d - us(1), d, d - us(10 ** 6), d + us(1)]
    out += [T(1, 1, 1), T(1, 1, 1) + us(1), T(1, 12, 31, 23, 59, 59, 999999), T(9999, 1, 1),
            T(9999, 12, 31, 23, 59, 59, 999999), T(9999, 12, 31, 23, 59, 59)]
    lo = (T(1, 1, 1) - EPOCH) // us(1)
    hi = (T(9999, 12, 31, 23, 59, 59, 999999) - EPOCH) // us(1)
    for _ in range(300):
        unit = rng.choice((1, 1, 1000, 10 ** 5, 10 ** 6))       # fractions of 6, 3, 1 and 0 digits
        m = rng.randint(lo, hi) // unit * unit
        out.append(EPOCH + us(m if m >= lo else m + unit))
    return _uniq(out)


def micros_of(ts):
    return (ts - EPOCH) // datetime.timedelta(microseconds=1)


# ------------------------------------------------------------------------------------------------
# Families
# ------------------------------------------------------------------------------------------------
def oracle_text(prints, r):
    """The oracle's cast to string of a non-NULL value r of oracle type `prints`."""
    return O.java_to_string(r, prints)


def _family(name, operand, column, kind, values, result_of, prints, raw_of, alphabet, cap):
    """result_of: the oracle's value of the operand (in the type `prints`) for a column value."""
    rows, cut = place(values)
    results = tuple(None if v is None else result_of(v) for v in rows)
    texts = tuple(None if r is None else oracle_text(prints, r) for r in results)
    raw = tuple(None if v is None else raw_of(v) for v in rows)
    lmax = min(cap, max(len(t) for t in texts if t is not None) + 1)
    return Family(name, operand, column, kind, tuple(rows), results, prints, texts, raw, alphabet, lmax, cut)


def _hex_d(d):
    return "double 0x%016x" % d_bits(d)


def _hex_f(f):
    return "float 0x%08x" % f_bits(f)


def _same(v):
    return v


@lru_cache(maxsize=None)
def families():
    A, cap = FLOAT_ALPHABET, K_MAX_CHARS
    D, F, L = double_values(), float_values(), long_values()
    out = [
        _family("double", "d", "d", "double", D, _same, "double", _hex_d, A, cap),
        _family("float", "f", "f", "float", F, _same, "float", _hex_f, A, cap),
        _family("float as double", "CAST(f AS DOUBLE)", "f", "float", F, _same, "double", _hex_f, A, cap),
        _family("double as float", "CAST(d AS FLOAT)", "d", "double", D, to_f32, "float", _hex_d, A, cap),
        _family("double as float as double", "CAST(CAST(d AS FLOAT) AS DOUBLE)", "d", "double", D, to_f32,
                "double", _hex_d, A, cap),
        _family("long as float", "CAST(i AS FLOAT)", "i", "long", L, long_to_f32, "float", str, A, cap),
        _family("long as double", "CAST(i AS DOUBLE)", "i", "long", L, float, "double", str, A, cap),
        # s holds the oracle's own Java text of each double row: parse, then print, on the device
        _family("string as double", "CAST(s AS DOUBLE)", "s", "string",
                [O.java_double_to_string(v) for v in D], float, "double", repr, A, cap),
    ]
    for p, s in DECIMAL_TYPES:
        ty, U = f"decimal({p},{s})", decimal_unscaled(p, s)
        raw_of = lambda u, s=s: f"unscaled {u} scale {s}"  # noqa: E731
        out.append(_family(ty, "dec", "dec", ty, U, lambda u, s=s: dec_value(u, s), ty, raw_of,
                           DECIMAL_ALPHABET, K_FMT_MAX))
        # Decimal.toDouble: the double nearest to unscaled / 10^scale (Python's int / int)
        out.append(_family(ty + " as double", "CAST(dec AS DOUBLE)", "dec", ty, U,
                           lambda u, s=s: u / 10 ** s, "double", raw_of, A, cap))
    out.append(_family("date", "day", "day", "date", date_values(), _same, "date",
                       lambda v: f"day {(v - EPOCH_DAY).days}", DATE_ALPHABET, K_FMT_MAX))
    out.append(_family("timestamp", "ts", "ts", "timestamp", timestamp_values(), _same, "timestamp",
                       lambda v: f"micros {micros_of(v)}", TIMESTAMP_ALPHABET, K_FMT_MAX))
    assert len({f.name for f in out}) == len(out)
    return tuple(out)


def family(name):
    return next(f for f in families() if f.name == name)


def family_names():
    return [f.name for f in families()]


def arrow_column(fam, lo, hi):
    """Rows [lo, hi) of the family's column as a pyarrow array, bit for bit (NaN payloads kept)."""
    import pyarrow as pa
    rows = fam.values[lo:hi]
    mask = np.array([v is None for v in rows], bool)
    if fam.kind == "double":
        bits = np.array([0 if v is None else d_bits(v) for v in rows], np.uint64)
        return pa.array(bits.view(np.float64), mask=mask)
    if fam.kind == "float":
        bits = np.array([0 if v is None else f_bits(v) for v in rows], np.uint32)
        return pa.array(bits.view(np.float32), mask=mask)
    if fam.kind == "long":
        return pa.array(list(rows), pa.int64())
    if fam.kind == "string":
        return pa.array(list(rows), pa.string())
    if fam.kind == "date":
        return pa.array(list(rows), pa.date32())
    if fam.kind == "timestamp":
        return pa.array([None if v is None else micros_of(v) for v in rows], pa.timestamp("us"))
    p, s = O.decimal_ps(fam.kind)
    return pa.array([None if u is None else dec_value(u, s) for u in rows], pa.decimal128(p, s))


def arrow_batches(fam):
    """The two batches of the family's table: its column, id (the row), g = id % 8, w (weights)."""
    import pyarrow as pa
    n = len(fam.values)
    w = RC.weights(n)
    out = []
    for lo, hi in ((0, fam.cut), (fam.cut, n)):
        ids = np.arange(lo, hi)
        out.append(pa.table({fam.column: arrow_column(fam, lo, hi), "id": pa.array(ids.astype(np.int32)),
                             "g": pa.array((ids % 8).astype(np.int32)), "w": pa.array(w[lo:hi])}))
    return out


def predicate(fam, pr):
    """`operand RLIKE 'pattern'`: every probe is non-nullable, so RLIKE is find-non-empty."""
    assert not RC.is_nullable(pr.pattern)
    return f"{fam.operand} RLIKE {RC.sql_string(pr.pattern)}"


def scan_specs(fam, chunk, extra=None):
    """Three aggregations per probe p: Sum(w, where=p), Sum(w, where=NOT (p)), Size(where=p); with
    `extra` (a filter that is never NULL) each predicate is `(...) AND extra`."""
    from deequ_amd.analyzers import Size, Sum
    out = []
    for pr in chunk:
        p = predicate(fam, pr)
        yes, no = (p, f"NOT ({p})") if extra is None else (f"({p}) AND {extra}", f"(NOT ({p})) AND {extra}")
        for a in (Sum("w", where=yes), Sum("w", where=no), Size(where=yes)):
            out += a.aggregation_functions()
    assert len(out) == 3 * len(chunk)
    return out


def check_plan(explain, n_probes):
    """The plan's explain() is whole (not cut at EXPLAIN_BYTES) and holds, per probe, two
    materialised expressions and an expr-bitmap task that counts one of them."""
    lines = explain.splitlines()
    assert lines and lines[-1].startswith("launches per batch:") and explain.endswith("\n"), lines[-3:]
    assert sum(ln.startswith("expr[") for ln in lines) == 2 * n_probes, explain
    tasks = [ln for ln in lines if ln.startswith("task[")]
    assert sum(" boolmap " in t and "(expr bitmap)" in t for t in tasks) == n_probes, tasks
    assert sum(" numeric " in t and "where=-1" not in t for t in tasks) == 2 * n_probes, tasks


# ------------------------------------------------------------------------------------------------
# Edits a wrong printer would make (test_format_cases.py: each changes some probe's fingerprint)
# ------------------------------------------------------------------------------------------------
def _last_digit_at(t):
    body = t.split("E")[0]
    return max((i for i, c in enumerate(body) if c.isdigit()), default=None)


def edit_last_digit_up(t):
    i = _last_digit_at(t)
    return None if i is None else t[:i] + str((int(t[i]) + 1) % 10) + t[i + 1:]


def edit_last_digit_down(t):
    i = _last_digit_at(t)
    return None if i is None else t[:i] + str((int(t[i]) - 1) % 10) + t[i + 1:]


def edit_point_zero_dropped(t):
    return t.replace(".0", "", 1) if ".0" in t else None


def edit_exponent_sign_dropped(t):
    return t.replace("E-", "E") if "E-" in t else None


def edit_one_digit_fewer(t):
    i = _last_digit_at(t)
    return None if i is None or sum(c.isdigit() for c in t) < 2 else t[:i] + t[i + 1:]


def edit_sign_dropped(t):
    return t[1:] if t.startswith("-") else None


EDITS = (edit_last_digit_up, edit_last_digit_down, edit_point_zero_dropped, edit_exponent_sign_dropped,
         edit_one_digit_fewer, edit_sign_dropped)
