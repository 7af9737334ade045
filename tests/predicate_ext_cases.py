"""The LIKE / arithmetic / scalar-function predicate matrix and its reference evaluator
(tests/test_gpu_predicates_ext.py, tests/test_predicates_ext_ref.py).

The oracle's parse_predicate has none of these forms, so every case carries its own reference: a
closure over a row built from the combinators below.  They restate Spark 2.2 with tools that are
not the engine's: numpy fixed-width integers for Java's wrap-around, np.float32 for Float results,
np.fmod for Java's %, and `re.fullmatch(..., re.S)` over `str` for LIKE.  A value is None (NULL), a
numpy scalar whose type is its Spark type (int8 Byte .. float64 Double), a str or a bool.

The table is predicate_cases.table() (same rows, same w / g columns) with two more string columns:
`t`, drawn from T_POOL (repeated prefixes for the matcher's backtracking, multi-byte text, % _ \\
and a newline as data, values above 64 bytes), and the all-NULL `sn`.
"""
import re
from functools import lru_cache

import numpy as np
import pyarrow as pa

import predicate_cases as PC
from predicate_cases import GROUPS, case, fingerprint  # noqa: F401  (re-exported for the tests)

NP = {"i8": np.int8, "i16": np.int16, "i32": np.int32, "i64": np.int64, "f32": np.float32,
      "f64": np.float64}
RANK = [np.int8, np.int16, np.int32, np.int64, np.float32, np.float64]   # numericPrecedence

X70 = "x" * 70
T_POOL = ["", "a", "ab", "abc", "a_c", "a%c", "a\nb", "aab", "aaab", "a" * 24 + "b", "a" * 24,
          "abcabcabd", "xaxbxc", "a.b.c", "añ😀", "😀", "ñ", "añb", "a😀b", X70 + "end",
          "pre" + X70, "CATEGORY-0-$ims_facets-0-", "BroadITKitem_type_keyword-0-",
          "Binding-0-value", "100%", "50% off", "back\\slash", "ba", "b", "c", "abxc", "a1b2c",
          "aaaaxb", "aabaab"]


# ------------------------------------------------------------------------------------------------
# The reference evaluator
# ------------------------------------------------------------------------------------------------
def wider(a, b):
    return RANK[max(RANK.index(a), RANK.index(b))]


def C(name):
    """A column: numeric ones in their Spark type, strings / booleans as they are."""
    return lambda r: r[name] if r[name] is None or name not in NP else NP[name](r[name])


def L(v):
    """A literal: an integer is Int if it fits, else Long; a float is a double."""
    if isinstance(v, int) and not isinstance(v, bool):
        v = np.int32(v) if -2 ** 31 <= v < 2 ** 31 else np.int64(v)
    return lambda r: np.float64(v) if isinstance(v, float) else v


def D(a):
    """A string operand of arithmetic: CAST AS DOUBLE (NULL when it is no number)."""
    def f(r):
        x = a(r)
        d = None if x is None else PC._python_double(x)
        return None if d is None else np.float64(d)
    return f


_OPS = {"+": np.add, "-": np.subtract, "*": np.multiply, "/": np.divide, "%": np.fmod}


def A(op, a, b):
    """a op b in the wider type (/ always in double); / and % by zero are NULL."""
    def f(r):
        x, y = a(r), b(r)
        if x is None or y is None:
            return None
        t = np.float64 if op == "/" else wider(type(x), type(y))
        x, y = t(x), t(y)
        if op in "/%" and y == 0:
            return None
        with np.errstate(all="ignore"):
            return t(_OPS[op](x, y))
    return f


def NEG(a):
    def f(r):
        x = a(r)
        with np.errstate(all="ignore"):
            return None if x is None else type(x)(-x)
    return f


def ABS(a):
    def f(r):
        x = a(r)
        with np.errstate(all="ignore"):
            return None if x is None else type(x)(np.abs(x))
    return f


def LEN(a):
    return lambda r: None if a(r) is None else np.int32(len(a(r)))     # code points of a str


def COALESCE(t, *args):
    """The first non-NULL argument in the common type t (None: strings)."""
    def f(r):
        for a in args:
            x = a(r)
            if x is not None:
                return x if t is None else t(x)
        return None
    return f


def ISNAN(a):
    return lambda r: a(r) is not None and bool(np.isnan(a(r)))


def ISNULL(a):
    return lambda r: a(r) is None


def like_regex(pattern):
    """escapeLikeRegex over the unescaped pattern: % -> .*, _ -> ., \\% \\_ \\\\ literals."""
    out, i = [], 0
    while i < len(pattern):
        c = pattern[i]
        if c == "\\":
            out.append(re.escape(pattern[i + 1]))
            i += 1
        else:
            out.append(".*" if c == "%" else "." if c == "_" else re.escape(c))
        i += 1
    return re.compile("".join(out), re.S)


def LIKE(a, pattern):
    rx = like_regex(pattern)
    return lambda r: None if a(r) is None else rx.fullmatch(a(r)) is not None


def _cmp3(x, y):
    if isinstance(x, str):
        x, y = x.encode(), y.encode()                      # UTF8String.compareTo: bytewise
        return (x > y) - (x < y)
    if isinstance(x, (np.floating, float)) or isinstance(y, (np.floating, float)):
        return PC._cmp_double(float(x), float(y))          # NaN = NaN, NaN above everything
    return (int(x) > int(y)) - (int(x) < int(y))


_REL = {"=": lambda c: c == 0, "<>": lambda c: c != 0, "<": lambda c: c < 0, "<=": lambda c: c <= 0,
        ">": lambda c: c > 0, ">=": lambda c: c >= 0}


def G(op, a, b):
    """A comparison; NULL when a side is NULL."""
    return lambda r: None if a(r) is None or b(r) is None else _REL[op](_cmp3(a(r), b(r)))


def IN(a, *items):
    def f(r):
        x, vals = a(r), [i(r) for i in items]
        if x is None:
            return None
        if any(v is not None and _cmp3(x, v) == 0 for v in vals):
            return True
        return None if any(v is None for v in vals) else False
    return f


def NOT(a):
    return lambda r: None if a(r) is None else not a(r)


def AND(a, b):
    def f(r):
        x, y = a(r), b(r)
        return False if x is False or y is False else (None if x is None or y is None else True)
    return f


def OR(a, b):
    def f(r):
        x, y = a(r), b(r)
        return True if x is True or y is True else (None if x is None or y is None else False)
    return f


# ------------------------------------------------------------------------------------------------
# The table
# ------------------------------------------------------------------------------------------------
_TABLE = []


def table():
    """(arrow table, its rows as dicts) -- built once and never modified."""
    if not _TABLE:
        t = PC.table()[0]
        rng = np.random.default_rng(19)
        n = t.num_rows
        idx = pa.array(rng.integers(0, len(T_POOL), n).astype(np.int32), mask=rng.random(n) < 0.1)
        t = t.append_column("t", pa.DictionaryArray.from_arrays(idx, pa.array(T_POOL, pa.string()))
                            .cast(pa.string()))
        t = t.append_column("sn", pa.nulls(n, pa.string()))
        _TABLE.append((t, t.to_pylist()))
    return _TABLE[0]


@lru_cache(maxsize=None)
def truth(c):
    return tuple(c.ref(r) for r in table()[1])


# ------------------------------------------------------------------------------------------------
# The matrix.  Case.empty names the row sets (T / F / N) a predicate leaves empty by its semantics.
# ------------------------------------------------------------------------------------------------
def _q(s):
    """A SQL string literal of the LIKE pattern s (backslashes doubled for unescapeSQLString,
    except before % and _, which keep theirs)."""
    return "'" + re.sub(r"\\(?![%_])", r"\\\\", s).replace("'", "''") + "'"


def _like(col, pattern, empty="", neg=False, family="like"):
    ref = LIKE(C(col), pattern)
    sql = f"{col} {'NOT ' if neg else ''}LIKE {_q(pattern)}"
    return case(family, sql, "gen", empty, ref=NOT(ref) if neg else ref)


PARTNER = {"i8": "i8", "i16": "i8", "i32": "i16", "i64": "i32", "f32": "i64", "f64": "f32"}


def _arith_family():
    out = []
    for col in PC.NUMERIC:
        for op in "+-*/%":
            # (x / 0 and x % 0 are NULL: a zero partner leaves NULL rows beyond the NULL operands)
            out.append(case("arith x literal", f"{col} {op} 3 > 1", "gen",
                            ref=G(">", A(op, C(col), L(3)), L(1))))
            p = PARTNER[col]
            # (i8 against itself stays Byte: x - x and x % x are 0, x / x is 1 -- never above 1)
            out.append(case("arith x column", f"{col} {op} {p} > 1", "gen",
                            "T" if col == p and op in "-/%" else "", ref=G(">", A(op, C(col), C(p)), L(1))))
    return out


def _wrap_family():
    f = "wrap"
    i8, i16, i32, i64 = C("i8"), C("i16"), C("i32"), C("i64")
    return [
        case(f, "i32 + 2147483647 < 0", "gen", ref=G("<", A("+", i32, L(2147483647)), L(0))),
        case(f, "i8 + i8 < -100", "gen", ref=G("<", A("+", i8, i8), L(-100))),
        case(f, "i8 + 1 > 127", "gen", ref=G(">", A("+", i8, L(1)), L(127))),        # Int: 128
        case(f, "i16 * i16 < 0", "gen", ref=G("<", A("*", i16, i16), L(0))),
        case(f, "i64 * 2 < i64", "gen", ref=G("<", A("*", i64, L(2)), i64)),
        case(f, "i64 - 9223372036854775807 > 0", "gen", ref=G(">", A("-", i64, L(2 ** 63 - 1)), L(0))),
        case(f, "-i8 = i8", "gen", ref=G("=", NEG(i8), i8)),                         # 0 and -128
        case(f, "-i64 < 0 AND i64 < 0", "gen", ref=AND(G("<", NEG(i64), L(0)), G("<", i64, L(0)))),
        case(f, "abs(i8) < 0", "gen", ref=G("<", ABS(i8), L(0))),                    # -128 only
        case(f, "abs(i32) < 0", "gen", ref=G("<", ABS(i32), L(0))),
        case(f, "abs(i64) < 0", "gen", ref=G("<", ABS(i64), L(0))),
        case(f, "(i32 * 1000003) % 7 = 3", "gen", ref=G("=", A("%", A("*", i32, L(1000003)), L(7)), L(3))),
        case(f, "(i64 * 31 + i32) % 11 = 5", "gen",
             ref=G("=", A("%", A("+", A("*", i64, L(31)), i32), L(11)), L(5))),
        case(f, "(i16 * i16) % 13 IN (1, 2, 3)", "gen",
             ref=IN(A("%", A("*", i16, i16), L(13)), L(1), L(2), L(3))),
        case(f, "i32 % 3 = -1", "gen", ref=G("=", A("%", i32, L(3)), L(-1))),
        case(f, "i32 % -3 = 1", "gen", ref=G("=", A("%", i32, L(-3)), L(1))),
        case(f, "i64 % -1 = 0", "gen", "F", ref=G("=", A("%", i64, L(-1)), L(0))),   # MIN % -1 is 0
    ]


def _zero_nan_family():
    f = "zero divisor / nan"
    i32, i8, f32, f64 = C("i32"), C("i8"), C("f32"), C("f64")
    return [
        case(f, "i32 / 0 > 1", "gen", "TF", ref=G(">", A("/", i32, L(0)), L(1))),
        case(f, "i32 % 0 = 0", "gen", "TF", ref=G("=", A("%", i32, L(0)), L(0))),
        case(f, "f64 / 0.0D > 1", "gen", "TF", ref=G(">", A("/", f64, L(0.0)), L(1))),
        case(f, "f64 / -0.0D > 1", "gen", "TF", ref=G(">", A("/", f64, L(-0.0)), L(1))),
        case(f, "f32 % 0.0D = 0", "gen", "TF", ref=G("=", A("%", f32, L(0.0)), L(0))),
        case(f, "i32 / i8 > 0.5", "gen", ref=G(">", A("/", i32, i8), L(0.5))),
        case(f, "f64 % f32 > 0.5", "gen", ref=G(">", A("%", f64, f32), L(0.5))),
        case(f, "f64 / f64 = 1", "gen", ref=G("=", A("/", f64, f64), L(1))),          # inf / inf: NaN
        case(f, "f64 + 1 > 0", "gen", ref=G(">", A("+", f64, L(1)), L(0))),           # NaN > 0
        case(f, "isnan(f64 * 0)", "gen", "N", ref=ISNAN(A("*", f64, L(0)))),          # inf * 0
        case(f, "f32 - f32 = 0", "gen", ref=G("=", A("-", f32, f32), L(0))),
        case(f, "isnan(f32)", "gen", "N", ref=ISNAN(f32)),
        case(f, "isnan(f64) OR f64 > 0", "gen", ref=OR(ISNAN(f64), G(">", f64, L(0)))),
    ]


def _float_family():
    f = "float"
    i64, f32, f64 = C("i64"), C("f32"), C("f64")
    return [
        case(f, "f32 * 2 > 1", "gen", ref=G(">", A("*", f32, L(2)), L(1))),
        case(f, "f32 + 0.5 > 1", "gen", ref=G(">", A("+", f32, L(0.5)), L(1))),        # Double
        case(f, "f32 * f32 > 1e38D", "gen", ref=G(">", A("*", f32, f32), L(1e38))),    # Float: inf
        case(f, "f32 + 16777216 = 16777216", "gen", ref=G("=", A("+", f32, L(16777216)), L(16777216))),
        case(f, "i64 + f32 > 0", "gen", ref=G(">", A("+", i64, f32), L(0))),           # Float
        case(f, "i64 + f32 >= f32", "gen", ref=G(">=", A("+", i64, f32), f32)),
        case(f, "f64 * 0.1 > 0.25", "gen", ref=G(">", A("*", f64, L(0.1)), L(0.25))),
        case(f, "f64 % 2 = -0.5", "gen", ref=G("=", A("%", f64, L(2)), L(-0.5))),
        case(f, "f32 / 3 > 0.1", "gen", ref=G(">", A("/", f32, L(3)), L(0.1))),        # Double
        case(f, "-f64 < 0", "gen", ref=G("<", NEG(f64), L(0))),
        case(f, "-f32 > 0.5", "gen", ref=G(">", NEG(f32), L(0.5))),
    ]


def _string_family():
    f = "string operand"
    s, t = C("s"), C("t")
    return [
        case(f, "s + 1 > 2", "gen", ref=G(">", A("+", D(s), L(1)), L(2))),
        case(f, "s * 2 = 10", "gen", ref=G("=", A("*", D(s), L(2)), L(10))),
        case(f, "-s < 0", "gen", ref=G("<", NEG(D(s)), L(0))),
        case(f, "s / i8 > 1", "gen", ref=G(">", A("/", D(s), C("i8")), L(1))),
        case(f, "abs(s) >= 5", "gen", ref=G(">=", ABS(D(s)), L(5))),
        case(f, "length(s) + 1 > 5", "gen", ref=G(">", A("+", LEN(s), L(1)), L(5))),
        case(f, "length(t) = 3", "gen", ref=G("=", LEN(t), L(3))),
        case(f, "length(s) > i8", "gen", ref=G(">", LEN(s), C("i8"))),
        case(f, "length(t) % 2 = 1", "gen", ref=G("=", A("%", LEN(t), L(2)), L(1))),
    ]


def _func_family():
    f = "functions"
    i8, i16, i32, i64, f32, f64, s, t = (C(k) for k in ("i8", "i16", "i32", "i64", "f32", "f64", "s", "t"))
    return [
        case(f, "abs(i32 - i64) IN (0, 1)", "gen", ref=IN(ABS(A("-", i32, i64)), L(0), L(1))),
        case(f, "abs(i8 - i16) IN (0, 1)", "gen", ref=IN(ABS(A("-", i8, i16)), L(0), L(1))),
        case(f, "abs(f64) > 2.5D", "gen", ref=G(">", ABS(f64), L(2.5))),
        case(f, "abs(f32) <= 0.5", "gen", ref=G("<=", ABS(f32), L(0.5))),
        case(f, "ABS(i16) = 3", "gen", ref=G("=", ABS(i16), L(3))),
        case(f, "coalesce(i32, 0) > 0", "gen", "N", ref=G(">", COALESCE(np.int32, i32, L(0)), L(0))),
        case(f, "coalesce(i8, i64, f32) > 0", "gen", ref=G(">", COALESCE(np.float32, i8, i64, f32), L(0))),
        case(f, "coalesce(i8, i16) + i8 > 100", "gen",
             ref=G(">", A("+", COALESCE(np.int16, i8, i16), i8), L(100))),
        case(f, "coalesce(NULL, i32, 3) = 3", "gen", "N", ref=G("=", COALESCE(np.int32, L(None), i32, L(3)), L(3))),
        case(f, "coalesce(s, t, 'z') LIKE 'a%'", "gen", "N", ref=LIKE(COALESCE(None, s, t, L("z")), "a%")),
        case(f, "coalesce(s, t) = 'a'", "gen", ref=G("=", COALESCE(None, s, t), L("a"))),
        case(f, "isnan(f64)", "gen", "N", ref=ISNAN(f64)),
        case(f, "NOT isnan(f32) AND f32 > 0", "gen", ref=AND(NOT(ISNAN(f32)), G(">", f32, L(0)))),
        case(f, "isnull(i32)", "gen", "N", ref=ISNULL(i32)),
        case(f, "isnotnull(s) AND s LIKE 'a%'", "gen", "N", ref=AND(NOT(ISNULL(s)), LIKE(s, "a%"))),
        case(f, "isnull(i8 + i16)", "gen", "N", ref=ISNULL(A("+", i8, i16))),
        case(f, "i64 BETWEEN i32 - 1 AND i32 + 1", "gen",
             ref=AND(G(">=", i64, A("-", i32, L(1))), G("<=", i64, A("+", i32, L(1))))),
        case(f, "i8 + i16 * 2 > i32", "gen", ref=G(">", A("+", i8, A("*", i16, L(2))), i32)),
        case(f, "-i8 + 1 > 0", "gen", ref=G(">", A("+", NEG(i8), L(1)), L(0))),
        case(f, "-(i8 + 1) > 0", "gen", ref=G(">", NEG(A("+", i8, L(1))), L(0))),
        case("depth 5", "((((i8 + 1) * 2 - i16) % 7) + abs(i32 % 5)) * 2 > 3", "gen",
             ref=G(">", A("*", A("+", A("%", A("-", A("*", A("+", i8, L(1)), L(2)), i16), L(7)),
                                 ABS(A("%", i32, L(5)))), L(2)), L(3))),
        case("depth 5", "abs(coalesce(i8, i16 - (i32 % (i8 + 3))) * 2) / (f32 + 1) > 1.5D", "gen",
             ref=G(">", A("/", ABS(A("*", COALESCE(np.int32, i8, A("-", i16, A("%", i32, A("+", i8, L(3))))),
                                     L(2))), A("+", f32, L(1))), L(1.5))),
    ]


def _like_family():
    long200 = "x" * 200
    out = [
        _like("t", "abc"), _like("t", "a"),                                   # lit
        _like("t", "CATEGORY%"), _like("t", "a%"), _like("s", "abcdefgh%"),   # lit%
        _like("t", "%c"), _like("t", "%-0-"), _like("t", "%aab"),             # %lit
        _like("t", "%facets%"), _like("t", "%keyword%"), _like("t", "%aab%"), _like("t", "%a%"),  # %lit%
        _like("t", "a%c"), _like("t", "aa%ab"), _like("t", "ab%ab", "T"),     # lit%lit (no overlap)
        _like("t", "%", "F"), _like("t", "", ), _like("t", "_"), _like("t", "__"), _like("t", "___"),
        _like("t", "a%b%c"), _like("t", "%a_b%"), _like("t", "%a_b"), _like("t", "a_b"),
        _like("t", "%aaa_b"), _like("t", "%a%ab"), _like("t", "a%a%a%b"), _like("t", "%_a_b%"),
        _like("t", "_%_"), _like("t", "%_"), _like("t", "a%_"),
        _like("t", long200 + "%", "T"), _like("t", "%" + long200 + "%", "T"),    # longer than any text
        _like("t", "_" + long200, "T"),
        _like("t", "%" + X70 + "end"), _like("t", "pre" + X70), _like("t", "_re" + X70),   # > 64 bytes
        _like("t", "%" + X70 + "%"), _like("t", "p%" + X70),
        _like("t", "a_😀"), _like("t", "%😀%"), _like("t", "a_"), _like("t", "_ñ_"), _like("t", "%ñ%"),
        _like("s", "_"), _like("s", "ß_漢"),
        _like("t", "100\\%"), _like("t", "%\\%%"), _like("t", "a\\_c"), _like("t", "a\\%c"),
        _like("t", "%\\\\%"), _like("t", "%\\_%"),
        _like("t", "a.b.c"), _like("t", "a.c", "T"),                           # . is a literal
        _like("t", "a%", neg=True), _like("t", "%a_b%", neg=True), _like("t", "%", "T", neg=True),
        _like("sn", "a%", "TF", family="like on an all-NULL column"),
        _like("sn", "%a_b%", "TF", family="like on an all-NULL column"),
        _like("sn", "%", "TF", neg=True, family="like on an all-NULL column"),
    ]
    t, s, i32 = C("t"), C("s"), C("i32")
    f = "like in a boolean expression"
    out += [
        case(f, "t LIKE 'a%' AND i32 > 0", "gen", ref=AND(LIKE(t, "a%"), G(">", i32, L(0)))),
        case(f, "t LIKE '%c' OR s IS NULL", "gen", ref=OR(LIKE(t, "%c"), ISNULL(s))),
        case(f, "t IS NULL OR t LIKE '%a%'", "gen", "N", ref=OR(ISNULL(t), LIKE(t, "%a%"))),
        case(f, "NOT (t LIKE '%b%') AND t LIKE 'a%'", "gen", ref=AND(NOT(LIKE(t, "%b%")), LIKE(t, "a%"))),
        case(f, "t LIKE 'a%' AND length(t) > 2 OR s LIKE '%g_'", "gen",
             ref=OR(AND(LIKE(t, "a%"), G(">", LEN(t), L(2))), LIKE(s, "%g_"))),
        case(f, "t like '%facets%' or t Like 'Binding%'", "gen", ref=OR(LIKE(t, "%facets%"), LIKE(t, "Binding%"))),
    ]
    return out


CASES = (_arith_family() + _wrap_family() + _zero_nan_family() + _float_family() + _string_family() +
         _func_family() + _like_family())
assert len({c.pred for c in CASES}) == len(CASES)


# ------------------------------------------------------------------------------------------------
# One LIKE predicate across batch and bitmap-word boundaries
# ------------------------------------------------------------------------------------------------
N_BATCHED = 40993      # 32768 + 8192 + 33: ten 4096-row batches and a 33-row tail


def batched_arrow(n=N_BATCHED, seed=23):
    rng = np.random.default_rng(seed)
    idx = pa.array(rng.integers(0, len(T_POOL), n).astype(np.int32), mask=rng.random(n) < 0.1)
    return pa.table({
        "t": pa.DictionaryArray.from_arrays(idx, pa.array(T_POOL, pa.string())).cast(pa.string()),
        "g": pa.array((np.arange(n) % 8).astype(np.int32)),
        "w": pa.array(rng.integers(0, 2 ** 32, n, dtype=np.int64))})
