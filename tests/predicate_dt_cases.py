"""The date / timestamp / CAST AS STRING predicate matrix and its reference evaluator
(tests/test_gpu_predicates_dt.py, tests/test_predicates_dt_ref.py).

The style of predicate_ext_cases.py: every case carries its own reference, a closure over a row
built from the combinators below and predicate_ext_cases's.  They restate Spark 2.2 with tools that
are not the engine's: datetime.date.isoformat for a date's text, datetime + timedelta(microseconds)
for a timestamp's (the fraction without trailing zeros), integer floor division for timestamp ->
date, datetime.date's own fields for year / month / dayofmonth, and format_cases.oracle_text (the
oracle's Java number printers) for numbers.  A date value is a datetime.date, a timestamp a
datetime.datetime (naive: UTC), everything else as in predicate_ext_cases.

The table is predicate_cases.table() (same rows, same w / g columns) with the date columns `d`
(drawn from D_POOL: the boundary dates 1582-10-15, 1969-12-31, 1970-01-01, 2000-02-29, 2100-03-01,
9999-12-31 among them) and `d2` (d moved by -2 .. 2 days, so that d <op> d2 goes every way), the
timestamp columns `ts` (TS_POOL: negative microseconds, whole seconds, .1, .000001,
23:59:59.999999, midnight) and `ts2`, and the all-NULL date column `dn`.  Every date lies within
1582-10-15 .. 9999-12-31: below, Spark's text follows the hybrid calendar and the engine does not.
"""
import datetime
from decimal import Decimal
from functools import lru_cache

import numpy as np
import pyarrow as pa

import format_cases as FC
import predicate_cases as PC
import predicate_ext_cases as X
from predicate_cases import GROUPS, case  # noqa: F401  (re-exported for the tests)
from predicate_ext_cases import AND, C, G, IN, ISNULL, L, LEN, LIKE, NOT, OR, COALESCE, A  # noqa: F401

Date, DT = datetime.date, datetime.datetime
EPOCH_DAY, EPOCH = Date(1970, 1, 1), DT(1970, 1, 1)
US = datetime.timedelta(microseconds=1)
US_PER_DAY = 86_400_000_000

D_POOL = [Date(1582, 10, 15), Date(1969, 12, 31), Date(1970, 1, 1), Date(2000, 2, 29), Date(2100, 3, 1),
          Date(9999, 12, 31), Date(1970, 1, 2), Date(1999, 12, 31), Date(2000, 1, 1), Date(2000, 3, 1),
          Date(2020, 1, 1), Date(2020, 1, 2), Date(2019, 12, 31), Date(2023, 6, 15), Date(2024, 1, 1),
          Date(2024, 1, 8), Date(2024, 2, 29), Date(2024, 12, 31), Date(1900, 2, 28), Date(1600, 2, 29)]
# (a date column never moves out of 1582-10-15 .. 9999-12-31)
D_LO, D_HI = Date(1582, 10, 15), Date(9999, 12, 31)

TS_POOL = [EPOCH, EPOCH - US, EPOCH - 1_000_000 * US, EPOCH - 86_400_000_001 * US, EPOCH + US,
           DT(1970, 1, 1, 0, 0, 0, 100000), DT(1969, 12, 31, 23, 59, 59, 999999), DT(2020, 1, 1),
           DT(2020, 1, 1, 0, 0, 1), DT(2020, 1, 1, 0, 0, 0, 1), DT(2019, 12, 31, 23, 59, 59, 999999),
           DT(2020, 1, 1, 12, 30, 45, 100000), DT(2020, 1, 2), DT(2000, 2, 29, 23, 59, 59, 999999),
           DT(2000, 3, 1), DT(2023, 6, 15, 8, 0, 0), DT(2024, 1, 1), DT(2024, 2, 29, 1, 2, 3, 120000),
           DT(1582, 10, 15), DT(9999, 12, 31, 23, 59, 59, 999999), DT(1969, 1, 1, 0, 0, 0, 500000),
           DT(2100, 3, 1, 0, 0, 0, 1)]


# the decimal column: plain texts, and below 1E-6 BigDecimal.toString's scientific form
DEC_TYPE = "decimal(12,8)"
DEC_POOL = [Decimal(v) for v in ("0.00000000", "2.50000000", "-2.50000000", "0.00000001", "-0.00000012",
                                 "1234.50000000", "9999.99999999", "-9999.99999999", "1.00000000",
                                 "0.10000000", "0.00000100", "0.00000099")]


# ------------------------------------------------------------------------------------------------
# The reference evaluator: what predicate_ext_cases has not
# ------------------------------------------------------------------------------------------------
def date_text(d):
    return d.isoformat()                                      # yyyy-MM-dd (years of four digits)


def micros_of(t):
    return (t - EPOCH) // US


def ts_text(t):
    """yyyy-MM-dd HH:mm:ss, then '.' and the microseconds without trailing zeros unless zero."""
    t = EPOCH + micros_of(t) * US
    whole = t.replace(microsecond=0).isoformat(sep=" ")
    return whole if t.microsecond == 0 else whole + "." + ("%06d" % t.microsecond).rstrip("0")


def ts_to_date(t):
    return EPOCH_DAY + datetime.timedelta(days=micros_of(t) // US_PER_DAY)   # floor division


def S(a):
    """CAST(a AS STRING).  The text of a value by its Python type (numpy scalars carry the Spark
    type): the oracle's Java printers for numbers, isoformat for dates."""
    def f(r):
        x = a(r)
        if x is None or isinstance(x, str):
            return x
        if isinstance(x, (bool, np.bool_)):
            return "true" if x else "false"
        if isinstance(x, Decimal):
            return FC.oracle_text(DEC_TYPE, x)
        if isinstance(x, DT):
            return ts_text(x)
        if isinstance(x, Date):
            return date_text(x)
        if isinstance(x, np.float32):
            return FC.oracle_text("float", x)
        if isinstance(x, (float, np.float64)):
            return FC.oracle_text("double", x)
        return FC.oracle_text("long", int(x))
    return f


def DAY(a):
    """A date function's argument as a date: a timestamp is cast to date."""
    def f(r):
        x = a(r)
        return ts_to_date(x) if isinstance(x, DT) else x
    return f


def YEAR(a):
    return lambda r: None if a(r) is None else np.int32(DAY(a)(r).year)


def MONTH(a):
    return lambda r: None if a(r) is None else np.int32(DAY(a)(r).month)


def DAYOFMONTH(a):
    return lambda r: None if a(r) is None else np.int32(DAY(a)(r).day)


def TO_DATE(a):
    return DAY(a)


def DATEDIFF(end, start):
    def f(r):
        e, s = DAY(end)(r), DAY(start)(r)
        return None if e is None or s is None else np.int32((e - s).days)
    return f


class FarDate:
    """A date_add / date_sub result past 9999-12-31, where datetime.date ends: it still orders by
    its day count, as Spark's int days do; its text and fields (years above 9999) are not pinned,
    so no case may read them -- GUARD keeps them out of reach."""
    def __init__(self, ordinal):
        self.ordinal = ordinal

    def toordinal(self):
        return self.ordinal


def DATE_ADD(a, n, sign=1):
    def f(r):
        x, k = DAY(a)(r), n(r)
        if x is None or k is None:
            return None
        o = x.toordinal() + sign * int(k)
        return Date.fromordinal(o) if 1 <= o <= Date.max.toordinal() else FarDate(o)
    return f


def DATE_SUB(a, n):
    return DATE_ADD(a, n, -1)


def _cmp3(x, y):
    if isinstance(x, DT) or isinstance(y, DT):
        assert type(x) is type(y), "a timestamp compares natively with a timestamp only"
        return (x > y) - (x < y)
    if isinstance(x, (Date, FarDate)) or isinstance(y, (Date, FarDate)):
        assert isinstance(x, (Date, FarDate)) and isinstance(y, (Date, FarDate)) and not isinstance(y, DT)
        return (x.toordinal() > y.toordinal()) - (x.toordinal() < y.toordinal())
    return X._cmp3(x, y)


def GUARD(cond, a):
    """cond AND a, for a case whose `a` is not pinned on the rows where cond is FALSE (a year
    above 9999): FALSE there whatever `a` is, which is all Kleene's AND needs of it."""
    return lambda r: False if cond(r) is False else AND(cond, a)(r)


def GT(op, a, b):
    """A comparison that also takes two dates or two timestamps (days / microseconds)."""
    return lambda r: None if a(r) is None or b(r) is None else X._REL[op](_cmp3(a(r), b(r)))


def NSEQ(a, b):
    """a <=> b"""
    def f(r):
        x, y = a(r), b(r)
        return (x is None and y is None) if x is None or y is None else _cmp3(x, y) == 0
    return f


def IND(a, *items):
    def f(r):
        x, vals = a(r), [i(r) for i in items]
        if x is None:
            return None
        if any(v is not None and _cmp3(x, v) == 0 for v in vals):
            return True
        return None if any(v is None for v in vals) else False
    return f


def RLIKE(a, pattern):
    import re
    rx = re.compile(pattern)                                   # (the patterns here read alike in Java)
    return lambda r: None if a(r) is None else rx.search(a(r)) is not None


def F(a):
    """A string against a number: CAST AS DOUBLE."""
    return X.D(a)


# ------------------------------------------------------------------------------------------------
# The table
# ------------------------------------------------------------------------------------------------
_TABLE = []


def _date_columns(n, seed):
    rng = np.random.default_rng(seed)
    d = [D_POOL[k] for k in rng.integers(0, len(D_POOL), n)]
    shift = rng.integers(-2, 3, n)
    d2 = [Date.fromordinal(min(D_HI.toordinal(), max(D_LO.toordinal(), x.toordinal() + int(k))))
          for x, k in zip(d, shift)]
    ts = [TS_POOL[k] for k in rng.integers(0, len(TS_POOL), n)]
    # ts2: ts itself, ts a microsecond or a day away, or another pool value
    how = rng.integers(0, 4, n)
    other = [TS_POOL[k] for k in rng.integers(0, len(TS_POOL), n)]
    lo, hi = DT(1582, 10, 15), DT(9999, 12, 31, 23, 59, 59, 999999)
    step = (0, 1, -US_PER_DAY)
    clamp = lambda m: EPOCH + min(micros_of(hi), max(micros_of(lo), m)) * US  # noqa: E731
    ts2 = [o if h == 3 else clamp(micros_of(t) + step[h]) for t, o, h in zip(ts, other, how)]
    masks = [rng.random(n) < 0.1 for _ in range(5)]
    dec = [DEC_POOL[k] for k in rng.integers(0, len(DEC_POOL), n)]
    return {
        "dec": pa.array(dec, type=pa.decimal128(12, 8), mask=masks[4]),
        "d": pa.array(d, type=pa.date32(), mask=masks[0]),
        "d2": pa.array(d2, type=pa.date32(), mask=masks[1]),
        "ts": pa.array(ts, type=pa.timestamp("us"), mask=masks[2]),
        "ts2": pa.array(ts2, type=pa.timestamp("us"), mask=masks[3]),
        "dn": pa.nulls(n, pa.date32()),
    }


def table():
    """(arrow table, its rows as dicts) -- built once and never modified."""
    if not _TABLE:
        t = PC.table()[0]
        for name, col in _date_columns(t.num_rows, 29).items():
            t = t.append_column(name, col)
        _TABLE.append((t, t.to_pylist()))
    return _TABLE[0]


@lru_cache(maxsize=None)
def truth(c):
    return tuple(c.ref(r) for r in table()[1])


# ------------------------------------------------------------------------------------------------
# The matrix.  Case.empty names the row sets (T / F / N) a predicate leaves empty by its semantics.
# ------------------------------------------------------------------------------------------------
d, d2, ts, ts2, dn = C("d"), C("d2"), C("ts"), C("ts2"), C("dn")
i8, i32, i64, f32, f64, b, s = (C(k) for k in ("i8", "i32", "i64", "f32", "f64", "b", "s"))
dec = C("dec")


def _same_type_family():
    f = "same type"
    out = []
    for op in ("=", "<>", "<", "<=", ">", ">="):
        out.append(case(f, f"d {op} d2", "gen", ref=GT(op, d, d2)))
        out.append(case(f, f"ts2 {op} ts", "gen", ref=GT(op, ts2, ts)))
    out += [case(f, "d <=> d2", "gen", "N", ref=NSEQ(d, d2)),
            case(f, "ts <=> ts2", "gen", "N", ref=NSEQ(ts, ts2)),
            case(f, "d > DATE '2000-02-29'", "gen", ref=GT(">", d, L(Date(2000, 2, 29)))),
            case(f, "DATE '2000-2-29' >= d", "gen", ref=GT(">=", L(Date(2000, 2, 29)), d)),
            case(f, "ts < TIMESTAMP '1970-01-01 00:00:00'", "gen", ref=GT("<", ts, L(EPOCH))),
            case(f, "TIMESTAMP '2020-1-1 0:0:0.000001' = ts", "gen",
                 ref=GT("=", L(DT(2020, 1, 1, 0, 0, 0, 1)), ts)),
            case(f, "ts >= TIMESTAMP ' 1969-12-31 23:59:59.999999 '", "gen",
                 ref=GT(">=", ts, L(DT(1969, 12, 31, 23, 59, 59, 999999)))),
            case(f, "d2 = DATE '2024-02-30'", "gen", ref=GT("=", d2, L(Date(2024, 3, 1)))),   # lenient day
            case(f, "dn = d", "gen", "TF", ref=GT("=", dn, d)),
            case(f, "dn <=> d", "gen", "N", ref=NSEQ(dn, d))]
    return out


def _string_family():
    f = "date / timestamp x string"
    out = []
    for op in ("=", "<>", "<", "<=", ">", ">="):
        out.append(case(f, f"CAST(d AS STRING) {op} '2000-02-29'", "gen", ref=G(op, S(d), L("2000-02-29"))))
        out.append(case(f, f"'2020-01-01' {op} CAST(d2 AS STRING)", "gen", ref=G(op, L("2020-01-01"), S(d2))))
    for op in ("<", "<=", ">", ">="):
        out.append(case(f, f"ts {op} '2020-01-01'", "gen", ref=G(op, S(ts), L("2020-01-01"))))
        out.append(case(f, f"'2020-01-01 00:00:00.000001' {op} ts2", "gen",
                        ref=G(op, L("2020-01-01 00:00:00.000001"), S(ts2))))
    day, us1 = L(DT(2020, 1, 1)), L(DT(2020, 1, 1, 0, 0, 0, 1))
    out += [
        # a date against a string: Spark casts the date to string, and so must the predicate (the
        # implicit form stays refused); '2020-1-1' is no date's text
        case(f, "CAST(d AS STRING) = '2020-1-1'", "gen", "T", ref=G("=", S(d), L("2020-1-1"))),
        case(f, "CAST(d AS STRING) <=> '2020-01-01'", "gen", "N", ref=NSEQ(S(d), L("2020-01-01"))),
        case(f, "'2020-01-01' <=> CAST(d AS STRING)", "gen", "N", ref=NSEQ(L("2020-01-01"), S(d))),
        case(f, "CAST(d AS STRING) > s", "gen", ref=G(">", S(d), s)),
        case(f, "s <= CAST(d AS STRING)", "gen", ref=G("<=", s, S(d))),
        case(f, "CAST(d AS STRING) >= '2'", "gen", ref=G(">=", S(d), L("2"))),
        case(f, "CAST(d AS STRING) < ''", "gen", "T", ref=G("<", S(d), L(""))),
        case(f, "ts > s", "gen", ref=G(">", S(ts), s)),
        # equality of a timestamp and a string: the string is cast to timestamp
        case(f, "ts = '2020-01-01'", "gen", ref=GT("=", ts, day)),
        case(f, "'2020-01-01' <> ts", "gen", ref=GT("<>", day, ts)),
        case(f, "ts = '2020-01-01 00:00:00'", "gen", ref=GT("=", ts, day)),
        case(f, "ts2 = '2020-01-01 00:00:00.000001'", "gen", ref=GT("=", ts2, us1)),
        case(f, "ts <=> '2020-01-01 00:00:00.000001'", "gen", "N", ref=NSEQ(ts, us1)),
        case(f, "'2020-01-01' <=> ts", "gen", "N", ref=NSEQ(day, ts)),
        # a date against a timestamp: both as strings
        case(f, "d < ts", "gen", ref=G("<", S(d), S(ts))),
        case(f, "ts <= d", "gen", ref=G("<=", S(ts), S(d))),
        case(f, "d = ts", "gen", "T", ref=G("=", S(d), S(ts))),        # 10 bytes against 19 or more
        case(f, "ts <=> d", "gen", "N", ref=NSEQ(S(ts), S(d))),
        case(f, "to_date(ts) = d", "gen", ref=GT("=", TO_DATE(ts), d)),
        # NULL
        case(f, "d = NULL", "gen", "TF", ref=GT("=", d, L(None))),
        case(f, "NULL < ts", "gen", "TF", ref=GT("<", L(None), ts)),
        case(f, "d <=> NULL", "gen", "N", ref=NSEQ(d, L(None))),
        case(f, "NULL <=> ts", "gen", "N", ref=NSEQ(L(None), ts)),
    ]
    return out


def _in_between_family():
    f = "in / between"
    D = lambda y, m, dd: L(Date(y, m, dd))  # noqa: E731
    return [
        case(f, "d IN (DATE '2000-02-29', DATE '1970-01-01')", "gen", ref=IND(d, D(2000, 2, 29), D(1970, 1, 1))),
        case(f, "d IN (d2, DATE '1582-10-15', NULL)", "gen", "F", ref=IND(d, d2, D(1582, 10, 15), L(None))),
        case(f, "d NOT IN (d2)", "gen", ref=NOT(IND(d, d2))),
        case(f, "ts IN (ts2, TIMESTAMP '2020-01-01 00:00:00')", "gen", ref=IND(ts, ts2, L(DT(2020, 1, 1)))),
        case(f, "d IN ('2000-02-29', '9999-12-31', '2000-2-29')", "gen",
             ref=IN(S(d), L("2000-02-29"), L("9999-12-31"), L("2000-2-29"))),
        case(f, "d IN ('1970-01-01', NULL)", "gen", "F", ref=IN(S(d), L("1970-01-01"), L(None))),
        case(f, "ts IN ('2020-01-01 00:00:00', '1969-12-31 23:59:59.999999', '2020-01-01')", "gen",
             ref=IN(S(ts), L("2020-01-01 00:00:00"), L("1969-12-31 23:59:59.999999"), L("2020-01-01"))),
        case(f, "d IN (s, '2024-01-01')", "gen", ref=IN(S(d), s, L("2024-01-01"))),
        case(f, "CAST(d AS STRING) BETWEEN '1970-01-01' AND '2020-01-01'", "gen",
             ref=AND(G(">=", S(d), L("1970-01-01")), G("<=", S(d), L("2020-01-01")))),
        case(f, "d BETWEEN DATE '1970-01-01' AND d2", "gen", ref=AND(GT(">=", d, D(1970, 1, 1)), GT("<=", d, d2))),
        case(f, "ts NOT BETWEEN '2000' AND '2021'", "gen",
             ref=NOT(AND(G(">=", S(ts), L("2000")), G("<=", S(ts), L("2021"))))),
        case(f, "ts BETWEEN TIMESTAMP '1970-01-01 00:00:00' AND ts2", "gen",
             ref=AND(GT(">=", ts, L(EPOCH)), GT("<=", ts, ts2))),
        case(f, "d >= d2 AND CAST(d AS STRING) <= '2024-01-01'", "gen", ref=AND(GT(">=", d, d2), G("<=", S(d), L("2024-01-01")))),
    ]


def _function_family():
    f = "date functions"
    return [
        case(f, "year(d) = 2000", "gen", ref=G("=", YEAR(d), L(2000))),
        case(f, "year(ts) IN (2019, 2020)", "gen", ref=IN(YEAR(ts), L(2019), L(2020))),
        case(f, "year(d) > 9000 OR year(d) < 1600", "gen", ref=OR(G(">", YEAR(d), L(9000)), G("<", YEAR(d), L(1600)))),
        case(f, "month(d) = 2", "gen", ref=G("=", MONTH(d), L(2))),
        case(f, "month(ts) >= 12", "gen", ref=G(">=", MONTH(ts), L(12))),
        case(f, "dayofmonth(d) = 29", "gen", ref=G("=", DAYOFMONTH(d), L(29))),
        case(f, "dayofmonth(ts) = 31", "gen", ref=G("=", DAYOFMONTH(ts), L(31))),
        case(f, "year(d) * 100 + month(d) = 200002", "gen",
             ref=G("=", A("+", A("*", YEAR(d), L(100)), MONTH(d)), L(200002))),
        case(f, "to_date(ts) = DATE '1969-12-31'", "gen", ref=GT("=", TO_DATE(ts), L(Date(1969, 12, 31)))),
        case(f, "to_date(ts) < to_date(ts2)", "gen", ref=GT("<", TO_DATE(ts), TO_DATE(ts2))),
        case(f, "to_date(d) = d2", "gen", ref=GT("=", TO_DATE(d), d2)),
        case(f, "CAST(to_date(ts) AS STRING) >= '2020-01-01'", "gen", ref=G(">=", S(TO_DATE(ts)), L("2020-01-01"))),
        case(f, "datediff(d2, d) = 1", "gen", ref=G("=", DATEDIFF(d2, d), L(1))),
        case(f, "datediff(d, d2) > 0", "gen", ref=G(">", DATEDIFF(d, d2), L(0))),
        case(f, "datediff(ts, ts2) = 1", "gen", ref=G("=", DATEDIFF(ts, ts2), L(1))),
        case(f, "datediff(ts, d) < 0", "gen", ref=G("<", DATEDIFF(ts, d), L(0))),
        case(f, "datediff(d, DATE '2000-01-01') BETWEEN 0 AND 60", "gen",
             ref=AND(G(">=", DATEDIFF(d, L(Date(2000, 1, 1))), L(0)), G("<=", DATEDIFF(d, L(Date(2000, 1, 1))), L(60)))),
        case(f, "d < DATE '9999-12-01' AND CAST(date_add(d, 7) AS STRING) > '2024-01-01'", "gen",
             ref=GUARD(GT("<", d, L(Date(9999, 12, 1))), G(">", S(DATE_ADD(d, L(7))), L("2024-01-01")))),
        case(f, "date_add(d2, 1) = d", "gen", ref=GT("=", DATE_ADD(d2, L(1)), d)),
        case(f, "date_add(ts, 1) = DATE '1970-01-01'", "gen", ref=GT("=", DATE_ADD(ts, L(1)), L(EPOCH_DAY))),
        case(f, "date_sub(d, 1) = DATE '2000-02-29'", "gen", ref=GT("=", DATE_SUB(d, L(1)), L(Date(2000, 2, 29)))),
        case(f, "date_sub(d, i8) >= d2", "gen", ref=GT(">=", DATE_SUB(d, i8), d2)),
        case(f, "date_add(d, i8 % 3) = d2", "gen", ref=GT("=", DATE_ADD(d, A("%", i8, L(3))), d2)),
        case(f, "date_add(date_sub(d, 3), 3) = d", "gen", "F", ref=GT("=", DATE_ADD(DATE_SUB(d, L(3)), L(3)), d)),
        case(f, "d < DATE '9999-12-01' AND month(date_add(d, 1)) <> month(d)", "gen",
             ref=GUARD(GT("<", d, L(Date(9999, 12, 1))), G("<>", MONTH(DATE_ADD(d, L(1))), MONTH(d)))),
        case(f, "year(dn) = 2000", "gen", "TF", ref=G("=", YEAR(dn), L(2000))),
        case(f, "date_add(d, 1) IS NULL", "gen", "N", ref=ISNULL(DATE_ADD(d, L(1)))),
    ]


def _cast_family():
    f = "cast as string"
    cs = lambda name: S(C(name))  # noqa: E731
    return [
        case(f, "CAST(i32 AS STRING) = '3'", "gen", ref=G("=", cs("i32"), L("3"))),
        case(f, "CAST(i32 AS STRING) IN ('1', '2', '-2147483648', '03')", "gen",
             ref=IN(cs("i32"), L("1"), L("2"), L("-2147483648"), L("03"))),
        case(f, "CAST(i64 AS STRING) LIKE '-9%'", "gen", ref=LIKE(cs("i64"), "-9%")),
        case(f, "CAST(i8 AS STRING) RLIKE '^-?[0-9]$'", "gen", ref=RLIKE(cs("i8"), "^-?[0-9]$")),
        case(f, "length(CAST(i64 AS STRING)) > 10", "gen", ref=G(">", LEN(cs("i64")), L(10))),
        case(f, "coalesce(CAST(i32 AS STRING), s) = '5'", "gen", ref=G("=", COALESCE(None, cs("i32"), s), L("5"))),
        case(f, "CAST(i32 AS STRING) < '2'", "gen", ref=G("<", cs("i32"), L("2"))),        # byte order
        case(f, "CAST(i32 AS STRING) > 2", "gen", ref=G(">", F(cs("i32")), L(2.0))),        # as doubles
        case(f, "CAST(f64 AS STRING) = '2.5'", "gen", ref=G("=", cs("f64"), L("2.5"))),
        case(f, "CAST(f64 AS STRING) IN ('NaN', 'Infinity', '-0.0', '0.1')", "gen",
             ref=IN(cs("f64"), L("NaN"), L("Infinity"), L("-0.0"), L("0.1"))),
        case(f, "CAST(f64 AS STRING) LIKE '%E%'", "gen", ref=LIKE(cs("f64"), "%E%")),
        case(f, "CAST(f32 AS STRING) = '0.1'", "gen", ref=G("=", cs("f32"), L("0.1"))),     # Float.toString
        case(f, "CAST(f32 AS STRING) RLIKE 'E-?[0-9]+$'", "gen", ref=RLIKE(cs("f32"), "E-?[0-9]+$")),
        case(f, "length(CAST(f32 AS STRING)) = 3", "gen", ref=G("=", LEN(cs("f32")), L(3))),
        case(f, "CAST(CAST(f64 AS FLOAT) AS STRING) = CAST(f32 AS STRING)", "gen",
             ref=G("=", S(lambda r: None if r["f64"] is None else FC.to_f32(r["f64"])), cs("f32"))),
        case(f, "CAST(b AS STRING) = 'true'", "gen", ref=G("=", cs("b"), L("true"))),
        case(f, "CAST(b AS STRING) LIKE 'f%'", "gen", ref=LIKE(cs("b"), "f%")),
        case(f, "length(CAST(b AS STRING)) = 5", "gen", ref=G("=", LEN(cs("b")), L(5))),
        case(f, "CAST(s AS STRING) = 'abc'", "gen", ref=G("=", s, L("abc"))),
        case(f, "CAST(s AS STRING) LIKE 'abcdefgh%'", "gen", ref=LIKE(s, "abcdefgh%")),
        case(f, "CAST(d AS STRING) IN ('1582-10-15', '9999-12-31')", "gen",
             ref=IN(S(d), L("1582-10-15"), L("9999-12-31"))),
        case(f, "CAST(d AS STRING) LIKE '%-12-31'", "gen", ref=LIKE(S(d), "%-12-31")),
        case(f, "CAST(d AS STRING) LIKE '2___-0_-%'", "gen", ref=LIKE(S(d), "2___-0_-%")),
        case(f, "CAST(d AS STRING) RLIKE '^(19|20)[0-9]{2}-01'", "gen", ref=RLIKE(S(d), "^(19|20)[0-9]{2}-01")),
        case(f, "length(CAST(d AS STRING)) = 10", "gen", "F", ref=G("=", LEN(S(d)), L(10))),
        case(f, "coalesce(CAST(d AS STRING), CAST(d2 AS STRING)) >= '2000'", "gen",
             ref=G(">=", COALESCE(None, S(d), S(d2)), L("2000"))),
        case(f, "CAST(ts AS STRING) = '2020-01-01 00:00:00'", "gen", ref=G("=", S(ts), L("2020-01-01 00:00:00"))),
        case(f, "CAST(ts AS STRING) IN ('1970-01-01 00:00:00.1', '1969-12-31 23:59:59.999999')", "gen",
             ref=IN(S(ts), L("1970-01-01 00:00:00.1"), L("1969-12-31 23:59:59.999999"))),
        case(f, "CAST(ts AS STRING) LIKE '%.000001'", "gen", ref=LIKE(S(ts), "%.000001")),
        case(f, "CAST(ts AS STRING) LIKE '%:00'", "gen", ref=LIKE(S(ts), "%:00")),
        case(f, "CAST(ts AS STRING) RLIKE '\\\\.[0-9]+$'", "gen", ref=RLIKE(S(ts), "\\.[0-9]+$")),
        case(f, "length(CAST(ts AS STRING)) > 19", "gen", ref=G(">", LEN(S(ts)), L(19))),
        case(f, "length(CAST(ts AS STRING)) = 21", "gen", ref=G("=", LEN(S(ts)), L(21))),
        case(f, "coalesce(CAST(ts AS STRING), 'none') LIKE '1969%'", "gen", "N",
             ref=LIKE(COALESCE(None, S(ts), L("none")), "1969%")),
        case(f, "CAST(to_date(ts) AS STRING) = CAST(d AS STRING)", "gen", ref=G("=", S(TO_DATE(ts)), S(d))),
        case(f, "CAST(year(d) AS STRING) LIKE '2%'", "gen", ref=LIKE(S(YEAR(d)), "2%")),
        case(f, "CAST(dn AS STRING) = 'x'", "gen", "TF", ref=G("=", S(dn), L("x"))),
        case(f, "CAST(NULL AS STRING) = s", "gen", "TF", ref=G("=", S(L(None)), s)),
        # a decimal: BigDecimal.toString at the column's scale
        case(f, "CAST(dec AS STRING) = '2.50000000'", "gen", ref=G("=", S(dec), L("2.50000000"))),
        case(f, "CAST(dec AS STRING) IN ('1E-8', '-1.2E-7', '0E-8', '9.9E-7')", "gen",
             ref=IN(S(dec), L("1E-8"), L("-1.2E-7"), L("0E-8"), L("9.9E-7"))),
        case(f, "CAST(dec AS STRING) LIKE '%E-_'", "gen", ref=LIKE(S(dec), "%E-_")),
        case(f, "CAST(dec AS STRING) RLIKE '^-?[0-9]+\\.[0-9]{8}$'", "gen",
             ref=RLIKE(S(dec), "^-?[0-9]+\\.[0-9]{8}$")),
        case(f, "length(CAST(dec AS STRING)) = 10", "gen", ref=G("=", LEN(S(dec)), L(10))),
        case(f, "coalesce(CAST(dec AS STRING), s) LIKE '%9'", "gen", ref=LIKE(COALESCE(None, S(dec), s), "%9")),
        case(f, "CAST(dec AS STRING) > 1000", "gen", ref=G(">", F(S(dec)), L(1000.0))),
        # the operators the other column types lacked
        case(f, "CAST(b AS STRING) RLIKE '^t'", "gen", ref=RLIKE(S(b), "^t")),
        case(f, "CAST(b AS STRING) IN ('false', 'x')", "gen", ref=IN(S(b), L("false"), L("x"))),
        case(f, "coalesce(CAST(b AS STRING), 'true') = 'true'", "gen", "N",
             ref=G("=", COALESCE(None, S(b), L("true")), L("true"))),
        case(f, "CAST(f64 AS STRING) RLIKE '^-?[0-9]\\.[0-9]+E-?[0-9]+$'", "gen",
             ref=RLIKE(S(f64), "^-?[0-9]\\.[0-9]+E-?[0-9]+$")),
        case(f, "length(CAST(f64 AS STRING)) = 3", "gen", ref=G("=", LEN(S(f64)), L(3))),
        case(f, "coalesce(CAST(f64 AS STRING), CAST(f32 AS STRING)) = '0.25'", "gen",
             ref=G("=", COALESCE(None, S(f64), S(f32)), L("0.25"))),
        case(f, "CAST(f32 AS STRING) IN ('NaN', '-Infinity', '1.0E-45', '0.25')", "gen",
             ref=IN(S(f32), L("NaN"), L("-Infinity"), L("1.0E-45"), L("0.25"))),
        case(f, "CAST(f32 AS STRING) LIKE '-%.5'", "gen", ref=LIKE(S(f32), "-%.5")),
        case(f, "coalesce(CAST(f32 AS STRING), 'none') LIKE 'n%'", "gen", "N",
             ref=LIKE(COALESCE(None, S(f32), L("none")), "n%")),
        case(f, "CAST(i64 AS STRING) = '-9223372036854775808'", "gen", ref=G("=", S(i64), L("-9223372036854775808"))),
        case(f, "CAST(ts AS STRING) RLIKE '^1969'", "gen", ref=RLIKE(S(ts), "^1969")),
        case(f, "coalesce(CAST(i8 AS STRING), CAST(i64 AS STRING)) RLIKE '^-1'", "gen",
             ref=RLIKE(COALESCE(None, S(i8), S(i64)), "^-1")),
    ]


def _composition_family():
    f = "compositions"
    return [
        case(f, "CAST(d AS STRING) >= '2000-01-01' AND CAST(d AS STRING) < '2024-01-01'", "gen",
             ref=AND(G(">=", S(d), L("2000-01-01")), G("<", S(d), L("2024-01-01")))),
        case(f, "d < d2 OR ts > ts2", "gen", ref=OR(GT("<", d, d2), GT(">", ts, ts2))),
        case(f, "NOT (CAST(d AS STRING) = '2000-02-29')", "gen", ref=NOT(G("=", S(d), L("2000-02-29")))),
        case(f, "NOT (ts >= '2020-01-01') OR year(d) = 1970", "gen",
             ref=OR(NOT(G(">=", S(ts), L("2020-01-01"))), G("=", YEAR(d), L(1970)))),
        case(f, "d IS NULL OR CAST(d AS STRING) >= '1970-01-01'", "gen", "N", ref=OR(ISNULL(d), G(">=", S(d), L("1970-01-01")))),
        # a cast of a string hands its operand's text on: both slots of the coalesce stay alive
        # through it, whichever argument the row takes
        case(f, "CAST(coalesce(CAST(d AS STRING), CAST(d2 AS STRING)) AS STRING) < '2000'", "gen",
             ref=G("<", COALESCE(None, S(d), S(d2)), L("2000"))),
        case(f, "CAST(coalesce(CAST(d AS STRING), CAST(ts2 AS STRING)) AS STRING) LIKE '%-01' AND ts < '2020'", "gen",
             ref=AND(LIKE(COALESCE(None, S(d), S(ts2)), "%-01"), G("<", S(ts), L("2020")))),
        case(f, "CAST(CAST(d AS STRING) AS STRING) < CAST(CAST(ts AS STRING) AS STRING)", "gen",
             ref=G("<", S(d), S(ts))),
        # four casts, two alive at a time: the text slots are used again
        case(f, "CAST(d AS STRING) < CAST(ts AS STRING) AND CAST(i32 AS STRING) <> CAST(i64 AS STRING)", "gen",
             ref=AND(G("<", S(d), S(ts)), G("<>", S(i32), S(i64)))),
        case(f, "d < ts AND ts2 > d2 OR CAST(i8 AS STRING) = CAST(i32 AS STRING)", "gen",
             ref=OR(AND(G("<", S(d), S(ts)), G(">", S(ts2), S(d2))), G("=", S(i8), S(i32)))),
        case(f, "year(ts) = year(d) AND month(ts) = month(d) AND i32 > 0", "gen",
             ref=AND(AND(G("=", YEAR(ts), YEAR(d)), G("=", MONTH(ts), MONTH(d))), G(">", i32, L(0)))),
        case(f, "s LIKE 'a%' OR CAST(d AS STRING) LIKE '19%' AND NOT ts < '1970'", "gen",
             ref=OR(LIKE(s, "a%"), AND(LIKE(S(d), "19%"), NOT(G("<", S(ts), L("1970")))))),
    ]


CASES = (_same_type_family() + _string_family() + _in_between_family() + _function_family() +
         _cast_family() + _composition_family())
assert len({c.pred for c in CASES}) == len(CASES)


# ------------------------------------------------------------------------------------------------
# One string-cast comparison and one date function across batch and bitmap-word boundaries
# ------------------------------------------------------------------------------------------------
N_BATCHED = 40993      # 32768 + 8192 + 33: ten 4096-row batches and a 33-row tail


def batched_arrow(n=N_BATCHED, seed=31):
    rng = np.random.default_rng(seed)
    cols = _date_columns(n, seed)
    cols["g"] = pa.array((np.arange(n) % 8).astype(np.int32))
    cols["w"] = pa.array(rng.integers(0, 2 ** 32, n, dtype=np.int64))
    return pa.table(cols)


BATCHED = [case("batched", "ts >= '2020-01-01'", "gen", ref=G(">=", S(ts), L("2020-01-01"))),
           case("batched", "year(ts) = 2020 AND month(d) <= 2", "gen",
                ref=AND(G("=", YEAR(ts), L(2020)), G("<=", MONTH(d), L(2))))]
