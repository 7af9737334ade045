"""Tables, the predicate matrix and the row-set fingerprint for tests/test_gpu_predicates.py.

Everything here runs on the host: the table builders (numpy / pyarrow), the oracle's per-row truth
vector of a predicate, and what the device must report for it.  A case of the matrix names the
path Compliance(p) must take on the device ("num" = fused numeric, "str" = fused string list,
"gen" = generic interpreter bitmap) and which of its TRUE / FALSE / NULL row sets are empty BY THE
PREDICATE'S SEMANTICS (`c IS NULL OR ...` and `<=>` are never NULL, `s >= ''` is never FALSE, an
int column never equals 2.5): every other set must be non-empty on the matrix table, so that no
predicate passes vacuously.
"""
from collections import namedtuple
from functools import lru_cache

import numpy as np
import pyarrow as pa

TYPES = {"i8": "byte", "i16": "short", "i32": "int", "i64": "long", "f32": "float",
         "f64": "double", "b": "boolean", "s": "string", "g": "int", "w": "long"}
NUMERIC = ["i8", "i16", "i32", "i64", "f32", "f64"]
INTS = {"i8": np.int8, "i16": np.int16, "i32": np.int32, "i64": np.int64}
N_MATRIX = 3001           # 2 full 1024-row chunks + a 953-row tail; 47 bitmap words, the last partial
GROUPS = list(range(9))   # g = row % 8; group 8 holds no row (the oracle's None)

LONG65 = "x" * 65
LONG65B = "x" * 64 + "y"  # same length bucket (> 64 bytes) and 8-byte prefix as LONG65
LONG100 = "y" * 100
STR_POOL = [
    "", "a", "abcdefg", "abcdefgh", "abcdefghi", "x" * 63, "x" * 64, LONG65, LONG65B, LONG100,
    "é", "ß€漢", "z", "zé", "～", "\U0001f600",       # bytes EF.. < F0.. ; UTF-16 orders them D83D < FF5E
    "abcdefgh-1", "abcdefgh-2",                             # share their first 8 bytes
    "hig", "high", "low", "medium", "m",                    # "hig" is a prefix of the item 'high'
    " 12 ", "1e3", "-0", "NaN", "Infinity", "1.5d", "abc", "12", "5", "7.25", "-3",
]


def _nan(bits, dtype):
    return np.array([bits], np.uint64 if dtype == np.float64 else np.uint32).view(dtype)[0]


EDGES = {
    "i8": [-128, 127, 0, 1, -1],
    "i16": [-32768, 32767, 0, 1, -1],
    "i32": [-2 ** 31, 2 ** 31 - 1, 0, 1, -1],
    "i64": [-2 ** 63, 2 ** 63 - 1, 0, 1, -1, 2 ** 53, -2 ** 53, 2 ** 53 + 1, -(2 ** 53 + 1)],
    "f32": [0.0, -0.0, 1e-45, -1e-45, np.inf, -np.inf, _nan(0x7fc00000, np.float32),
            _nan(0x7f800123, np.float32), np.float32(0.1), np.float32(16777217.0)],
    "f64": [0.0, -0.0, 5e-324, -5e-324, 1.1e-308, np.inf, -np.inf, _nan(0x7ff8000000000000, np.float64),
            _nan(0x7ff0000000000123, np.float64), 0.1, 1.7e308],
}


def numeric_values(col, n, rng, edges=True):
    """Half the rows small (integers in [-8, 8]; floats multiples of 0.25 in [-8, 8], so equality
    with 3, 2.0D and 2.5 is hit), half across the type's range, and each edge value four times."""
    small = rng.random(n) < 0.5
    if col in INTS:
        info = np.iinfo(INTS[col])
        wide = rng.integers(info.min, info.max, n, dtype=np.int64, endpoint=True)
        v = np.where(small, rng.integers(-8, 9, n), wide).astype(INTS[col])
    else:
        dt = np.float32 if col == "f32" else np.float64
        wide = (rng.normal(0.0, 1.0, n) * 10.0 ** rng.integers(-3, 9, n)).astype(dt)
        v = np.where(small, rng.integers(-32, 33, n) * 0.25, wide).astype(dt)
    if edges:
        e = np.array(EDGES[col], dtype=v.dtype)
        pos = rng.choice(n, size=min(n, 4 * len(e)), replace=False)
        v[pos] = np.resize(e, len(pos))
    return v


def matrix_arrow(n=N_MATRIX, seed=7, all_null=(), edges=True, null_rate=0.1):
    rng = np.random.default_rng(seed)
    cols = {}
    for c in NUMERIC:
        v = numeric_values(c, n, rng, edges)
        mask = np.ones(n, bool) if c in all_null else rng.random(n) < null_rate
        cols[c] = pa.array(v, mask=mask)
    bmask = rng.random(n) < null_rate
    cols["b"] = pa.array(rng.random(n) < 0.5, mask=bmask)
    pool = pa.array(STR_POOL, type=pa.string())
    idx = rng.integers(0, len(STR_POOL), n).astype(np.int32)
    smask = np.ones(n, bool) if "s" in all_null else rng.random(n) < null_rate
    cols["s"] = pa.DictionaryArray.from_arrays(pa.array(idx, mask=smask), pool).cast(pa.string())
    cols["g"] = pa.array((np.arange(n) % 8).astype(np.int32))
    cols["w"] = pa.array(rng.integers(0, 2 ** 40 if n <= 8192 else 2 ** 32, n, dtype=np.int64))
    return pa.table(cols)


def oracle_table(t):
    from oracle.deequ_oracle import OTable
    return OTable({k: t.column(k).to_pylist() for k in t.column_names},
                  {k: TYPES[k] for k in t.column_names})


# ------------------------------------------------------------------------------------------------
# The matrix
# ------------------------------------------------------------------------------------------------
Case = namedtuple("Case", "family pred path empty where_ok ref")


def case(family, pred, path, empty="", where_ok=True, ref=None):
    return Case(family, pred, path, empty, where_ok, ref)


def _q(s):
    return "'" + s.replace("'", "''") + "'"


def _in(items):
    return "(" + ", ".join(_q(i) if isinstance(i, str) else str(i) for i in items) + ")"


SMALL8 = ["high", "low", "a", "", "abc", "12", "5", "abcdefg"]       # 8 items, none above 7 bytes
GENERAL8 = SMALL8[:7] + ["abcdefgh"]                                  # an 8-byte item: not list_small
NINE = SMALL8 + ["m"]                                                 # 9 items: not list_small
FORTY = (NINE + ["abcdefgh-1", "x" * 63, "x" * 64, LONG65, LONG100, "é", "～", "zé", "hig!",
                 "high", "low", ""] + [f"absent-{k}" for k in range(20)])[:40]
assert len(FORTY) == 40 and len(NINE) == 9 and len(SMALL8) == 8


def _cmp_family():
    out = []
    for col in NUMERIC:
        is_int = col in INTS
        for kind, lit in (("int literal", "3"), ("fractional literal", "2.5"), ("D literal", "2.0D")):
            for op in ("=", "<>", "<", "<=", ">", ">=", "<=>"):
                empty = ""
                if is_int and lit == "2.5" and op in ("=", "<=>"):
                    empty += "T"      # an integer is never 2.5
                if is_int and lit == "2.5" and op == "<>":
                    empty += "F"
                if op == "<=>":
                    empty += "N"      # null-safe equality is never NULL
                # (`<=>` is not one of leaf_cmp's comparisons, api.cpp:353: generic)
                out.append(case(f"cmp x {kind}", f"{col} {op} {lit}", "gen" if op == "<=>" else "num",
                                empty))
    return out


def _range_family():
    out = []
    for col, lo, hi in (("i8", -128, 127), ("i16", -32768, 32767), ("i32", -2 ** 31, 2 ** 31 - 1)):
        out += [case("type range", f"{col} < {hi}", "num"),
                case("type range", f"{col} <= {hi}", "num", "F"),
                case("type range", f"{col} < {hi + 1}", "num", "F"),
                case("type range", f"{col} >= {hi + 1}", "num", "T"),
                case("type range", f"{col} = {hi}", "num"),
                case("type range", f"{col} > {lo}", "num"),
                case("type range", f"{col} >= {lo}", "num", "F"),
                case("type range", f"{col} > {lo - 1}", "num", "F"),
                case("type range", f"{col} <= {lo - 1}", "num", "T")]
    out += [case("type range", "i64 < 9223372036854775807", "num"),
            case("type range", "i64 >= 9223372036854775807", "num"),
            case("type range", "i64 > -9223372036854775808", "num"),
            case("type range", "i64 = 9007199254740993", "num"),       # 2^53 + 1, integer domain
            case("type range", "i64 > 9007199254740992", "num"),
            case("type range", "f32 = 16777217", "num", "T"),          # the column holds 16777216.0f
            case("type range", "f32 = 16777216", "num")]
    return out


def _forms_family():
    out = [case("reversed operands", "5 < i32", "num"), case("reversed operands", "2.5 >= f64", "num"),
           case("reversed operands", "0 <> i8", "num"), case("reversed operands", "3 = i16", "num"),
           case("reversed operands", "2.0D > f32", "num"), case("reversed operands", "-1 <= i64", "num"),
           case("between", "i32 BETWEEN -3 AND 3", "num"),
           case("between", "f32 BETWEEN -0.5 AND 2.25", "num"),
           case("between", "i64 BETWEEN -2.5 AND 2.5", "num"),
           case("between", "i8 BETWEEN -100 AND 100", "num"),
           case("between", "i16 NOT BETWEEN -3 AND 3", "gen"),
           case("between", "f64 NOT BETWEEN -1.0 AND 1.0", "gen")]
    for col in NUMERIC:
        lo, hi = ("-2", "5") if col in INTS else ("-2.25", "5.0")
        out.append(case("null or range", f"{col} IS NULL OR ({col} >= {lo} AND {col} <= {hi})", "num", "N"))
    out += [case("null or range", "i32 IS NULL OR i32 > 0", "num", "N"),
            # fuse_numeric refuses an int and a double bound on an int column (api.cpp:398)
            case("mixed int / double bounds", "i32 >= 1 AND i32 <= 10.5", "gen"),
            case("mixed int / double bounds", "i32 IS NULL OR (i32 >= -2.5 AND i32 <= 4)", "gen", "N"),
            case("mixed int / double bounds", "i64 > -3 AND i64 < 2.0D", "gen"),
            case("mixed int / double bounds", "f64 >= 1 AND f64 <= 2.5", "num"),   # a float column: fused
            case("mixed int / double bounds", "f32 > -1.5 AND f32 < 4", "num")]
    return out


def _nan_family():
    return [case("nan", "f64 = f64", "gen", "F"), case("nan", "f32 = f32", "gen", "F"),
            case("nan", "f64 > 1e308", "num"), case("nan", "f64 >= 1.7e308", "num"),
            case("nan", "f64 <= 0.0", "num"), case("nan", "f64 = 0.0", "num"),
            case("nan", "f32 > 1e38", "num"), case("nan", "f32 <= 0", "num"),
            case("nan", "NOT (f64 > 1e308)", "gen"), case("nan", "f64 > 1e308 OR f64 < -1e308", "gen"),
            case("nan", "f32 < f64", "gen"), case("nan", "f64 <=> f32", "gen", "N")]
    # (f64 = f64: NaN = NaN is TRUE, so no non-NULL row is FALSE)


def _colcol_family():
    return [case("column x column", "i32 < i64", "gen"), case("column x column", "i64 > f64", "gen"),
            case("column x column", "f32 = f64", "gen"), case("column x column", "i8 <=> i16", "gen", "N"),
            case("column x column", "s = s", "gen", "F"), case("column x column", "i16 >= i8", "gen"),
            case("column x column", "i8 = i64", "gen"), case("column x column", "i32 <> f32", "gen")]


def _kleene_family():
    f = "kleene"
    return [case(f, "i8 > 0 AND i16 > 0", "gen"), case(f, "i8 > 0 OR i16 > 0", "gen"),
            case(f, "NOT (i8 > 0)", "gen"), case(f, "NOT (i8 > 0 AND i16 > 0)", "gen"),
            case(f, "NOT (i8 > 0 OR i16 > 0)", "gen"),
            case(f, "b", "gen"), case(f, "NOT b", "gen"), case(f, "b AND i8 > 0", "gen"),
            case(f, "b OR i8 > 0", "gen"), case(f, "b = TRUE", "gen"), case(f, "b <> FALSE", "gen"),
            case(f, "b OR NULL", "gen", "F"), case(f, "i8 > 0 AND NULL", "gen", "T"),
            case(f, "NULL OR i8 > 0", "gen", "F"), case(f, "NULL AND b", "gen", "T"),
            case(f, "(i8 > 0 AND TRUE) OR (i16 > 0 AND FALSE)", "gen"),
            case(f, "(b OR FALSE) AND NOT (i32 > 0 AND TRUE)", "gen"),
            case(f, "b IS NOT NULL AND b", "gen", "N"), case(f, "b IS NULL OR i8 > 0", "gen"),
            case(f, "i8 IS NULL AND i16 IS NOT NULL", "gen", "N"),
            case(f, "NOT (i8 > 0 AND (i16 < 0 OR NOT (i32 = 0 AND (f64 > 0.0 OR b))))", "gen"),
            case(f, "((i8 > 0 OR (i16 > 0 AND (i32 > 0 OR (i64 > 0 AND NOT b)))) AND f32 < 1.5) OR s = 'a'", "gen"),
            case("null-safe equality", "i32 <=> NULL", "gen", "N"),
            case("null-safe equality", "NULL <=> i32", "gen", "N"),
            case("null-safe equality", "(NULL <=> NULL) AND i32 > 0", "gen"),
            case("null-safe equality", "NOT (s <=> 'high')", "gen", "N"),
            case("null-safe equality", "b <=> NULL", "gen", "N")]


def _in_family():
    f, g = "numeric IN", "string IN"
    fifteen = list(range(-7, 8))          # 15 items + the value = kMaxStack (kernels.h:127)
    return [
        case(f, "i32 IN (3)", "gen"), case(f, "i32 IN (1, 2, 3, 4, 5, 6, 7, 8)", "gen"),
        case(f, "i8 IN (1, 2, 3, 4, 5, 6, 7, 8, -128)", "gen"), case(f, f"i16 IN {_in(fifteen)}", "gen"),
        case(f, "i32 NOT IN (1, 2, 3)", "gen"), case(f, "i32 IN (1, NULL)", "gen", "F"),
        case(f, "i32 NOT IN (1, NULL)", "gen", "T"), case(f, "i32 IN (1, 1, 2, 2)", "gen"),
        case(f, "f64 IN (0.5, 2.25, 2147483648.0)", "gen"), case(f, "i64 IN (2.5, 3)", "gen"),
        case(f, "f32 IN (0.25, -8)", "gen"), case(f, "i64 IN (9007199254740993, -9223372036854775808)", "gen"),
        case(g, "s IN ('high')", "str"), case(g, "s = 'high'", "str"), case(g, "s <> 'high'", "str"),
        case(g, "'high' = s", "str"), case(g, "s = ''", "str"), case(g, f"s = {_q(LONG65)}", "str"),
        case(g, f"s IN {_in(SMALL8)}", "str"), case(g, f"s IN {_in(GENERAL8)}", "str"),
        case(g, f"s IN {_in(NINE)}", "str"), case(g, f"s NOT IN {_in(NINE)}", "str"),
        # 41 stack slots: the interpreter refuses it (kMaxStack), so only the fused form runs
        case(g, f"s IN {_in(FORTY)}", "str", where_ok=False),
        case(g, f"s IS NULL OR s NOT IN {_in(FORTY)}", "str", "N", where_ok=False),
        case(g, "s IN ('abcdefgh-1')", "str"), case(g, "s IN ('abcdefgh-1', 'abcdefghi', 'abcdefg')", "str"),
        case(g, f"s IN {_in([LONG65, LONG100])}", "str"), case(g, f"s NOT IN {_in([LONG65B, 'x' * 64])}", "str"),
        case(g, "s IN ('low', 'low', 'high', 'low')", "str"), case(g, "s IN ('é', 'ß€漢', '\U0001f600')", "str"),
        case(g, "s IN ('high', NULL)", "gen", "F"), case(g, "s NOT IN ('high', NULL)", "gen", "T"),
        case(g, "s IS NULL OR s IN ('high', 'low')", "str", "N"),
        case(g, "s IS NULL OR s NOT IN ('high', 'low')", "str", "N"),
        case(g, "s NOT IN ('high', 'low')", "str"), case(g, "s IS NULL OR s = 'medium'", "str", "N"),
        case(g, "s IN (12, '5')", "str"),     # the int literal becomes the string '12'
    ]


def _string_family():
    f, p = "string ordering", "string x number"
    return [case(f, "s < 'm'", "gen"), case(f, "s >= ''", "gen", "F"), case(f, "s > 'z'", "gen"),
            case(f, "s < 'é'", "gen"), case(f, "s >= '～'", "gen"), case(f, "s > '～'", "gen"),
            case(f, "s <= 'abcdefgh'", "gen"), case(f, "'m' > s", "gen"), case(f, f"s < {_q(LONG65B)}", "gen"),
            case(p, "s > 5", "gen"), case(p, "s = 12", "gen"), case(p, "s <= 1.5", "gen"),
            case(p, "s < i32", "gen"), case(p, "s >= 1000.0D", "gen"), case(p, "s = 0", "gen"),
            case("cast", "CAST(s AS DOUBLE) >= 1.5", "gen", ref=_ref_cast_s),
            case("cast", "CAST(i64 AS DOUBLE) = f64", "gen", ref=_ref_cast_i64),
            case("cast", "CAST(f64 AS FLOAT) = f32", "gen", ref=_ref_cast_f32),
            case("cast", "CAST(i32 AS DOUBLE) > 2.5", "gen", ref=_ref_cast_i32)]


# The oracle's parser has no CAST: the expected rows of these four come from plain Python / numpy.
def _cmp_double(a, b):
    """Spark's double ordering: NaN = NaN and NaN above everything."""
    an, bn = a != a, b != b
    if an or bn:
        return 0 if an and bn else (1 if an else -1)
    return (a > b) - (a < b)


def _python_double(s):
    """float(str) with the two Java spellings float() lacks or adds (a d / f suffix; no 'nan' /
    'inf' words -- the pool holds only Java's 'NaN' / 'Infinity')."""
    s = s.strip(" ")
    if s[-1:] in ("d", "D", "f", "F") and s[:-1] and s[:-1][-1].isdigit():
        s = s[:-1]
    try:
        return float(s)
    except ValueError:
        return None


def _ref_cast_s(row):
    d = None if row["s"] is None else _python_double(row["s"])
    return None if d is None else _cmp_double(d, 1.5) >= 0


def _ref_cast_i64(row):
    if row["i64"] is None or row["f64"] is None:
        return None
    return _cmp_double(float(row["i64"]), row["f64"]) == 0


def _ref_cast_f32(row):
    if row["f64"] is None or row["f32"] is None:
        return None
    with np.errstate(over="ignore"):
        return _cmp_double(float(np.float32(row["f64"])), row["f32"]) == 0


def _ref_cast_i32(row):
    return None if row["i32"] is None else float(row["i32"]) > 2.5


CASES = (_cmp_family() + _range_family() + _forms_family() + _nan_family() + _colcol_family() +
         _kleene_family() + _in_family() + _string_family())
assert len({c.pred for c in CASES}) == len(CASES)

ALL_NULL_COLUMNS = ("i32", "s")
ALL_NULL_CASES = [case("all-null column", p, path) for p, path in [
    ("i32 > 0", "num"), ("i32 IS NULL OR i32 > 0", "num"), ("i32 IS NULL OR (i32 >= 0 AND i32 <= 5)", "num"),
    ("s IN ('a')", "str"), ("s IS NULL OR s IN ('a', 'high')", "str"), ("s <> 'a'", "str"),
    ("i32 < i64", "gen"), ("NOT (i32 > 0)", "gen"), ("i32 <=> NULL", "gen"), ("s > 5", "gen"),
    ("i32 IN (1, 2)", "gen"), ("i32 > 0 OR i8 > 0", "gen")]]

# Five predicates on one (column, where): three fuse (preds=3), two overflow to bitmaps (kMaxPreds,
# engine.h:31; the fallback is api.cpp:641-654)
OVERFLOW = ["i32 > 0", "i32 <= 3", "i32 IS NULL OR (i32 >= -2 AND i32 <= 5)", "i32 <> 0", "i32 >= 2.5"]


# ------------------------------------------------------------------------------------------------
# Truth vectors and what the device must report
# ------------------------------------------------------------------------------------------------
_TABLES = {}


def table(kind="matrix"):
    """(arrow table, oracle table) -- built once and never modified."""
    if kind not in _TABLES:
        t = matrix_arrow() if kind == "matrix" else matrix_arrow(1000, 11, ALL_NULL_COLUMNS)
        _TABLES[kind] = (t, oracle_table(t))
    return _TABLES[kind]


@lru_cache(maxsize=None)
def truth(kind, c):
    """The oracle's eval_predicate of every row: a tuple of True / False / None."""
    from oracle import deequ_oracle as O
    ot = table(kind)[1]
    if c.ref is not None:
        return tuple(c.ref(r) for r in ot.rows())
    node = O.parse_predicate(c.pred)
    return tuple(O.eval_predicate(node, r) for r in ot.rows())


def fingerprint(tv, w):
    """(sum of w over the TRUE rows, over the FALSE rows, over the NULL rows), exact integers.
    With w random in [0, 2^40) two different row sets have the same sum with probability ~2^-40,
    so equal sums identify the sets -- a count cannot tell a row gained from a row lost."""
    assert len(tv) == len(w)
    s = {True: 0, False: 0, None: 0}
    for v, x in zip(tv, w):
        s[v] += int(x)
    assert s[True] + s[False] + s[None] < 2 ** 53
    return s[True], s[False], s[None]


def count_true(tv):
    """sum(expr.cast(int)) over rows: None when no row is non-NULL (Compliance / conditionalCount)."""
    if all(v is None for v in tv):
        return None
    return sum(1 for v in tv if v is True)


def expected(tv, w, g):
    """Everything the tests compare for one predicate, derived from its truth vector."""
    st, sf, _ = fingerprint(tv, w)
    return {
        "sum_true": float(st) if any(v is True for v in tv) else None,
        "sum_false": float(sf) if any(v is False for v in tv) else None,
        "count": count_true(tv),
        "groups": [count_true([v for v, k in zip(tv, g) if k == grp]) for grp in GROUPS],
    }


# ------------------------------------------------------------------------------------------------
# Geometry: numpy references (value bits, known bits) of the reduced predicate set
# ------------------------------------------------------------------------------------------------
N_GEOMETRY = (1 << 20) + 8192 + 5
GEO_SMALL_IN = ("high", "low")
GEO_LONG_IN = ("medium", "abcdefgh-1", LONG65, "abcdefghi")


def geometry_columns(n=N_GEOMETRY, seed=3):
    """numpy columns (values, valid) of the geometry table; strings as indices into STR_POOL."""
    rng = np.random.default_rng(seed)
    cols = {}
    for c in NUMERIC:
        cols[c] = (numeric_values(c, n, rng), rng.random(n) >= 0.1)
    cols["s"] = (rng.integers(0, len(STR_POOL), n).astype(np.int32), rng.random(n) >= 0.1)
    cols["g"] = ((np.arange(n) % 8).astype(np.int32), np.ones(n, bool))
    cols["w"] = (rng.integers(0, 2 ** 32, n, dtype=np.int64), np.ones(n, bool))
    return cols


def geometry_arrow(cols, n, names=None):
    out = {}
    for k in names or list(cols):
        v, ok = cols[k]
        if k == "s":
            out[k] = pa.DictionaryArray.from_arrays(pa.array(v[:n], mask=~ok[:n]),
                                                    pa.array(STR_POOL, type=pa.string())).cast(pa.string())
        else:
            out[k] = pa.array(v[:n], mask=~ok[:n])
    return pa.table(out)


def _nan_cmp(x, lit):
    """(x > lit, x < lit) with Spark's NaN-largest order, on doubles."""
    with np.errstate(invalid="ignore"):      # (widening the signalling NaN payload)
        x = x.astype(np.float64)
    nan = np.isnan(x)
    return np.where(nan, True, x > lit), np.where(nan, False, x < lit)


def geometry_predicates(cols, n):
    """[(predicate, path, value bits, known bits)]: one fused numeric predicate per element type,
    both string-list paths, one generic."""
    c = {k: (v[:n], ok[:n]) for k, (v, ok) in cols.items()}
    pool_idx = {s: i for i, s in enumerate(STR_POOL)}
    out = []
    v, ok = c["i8"]
    out.append(("i8 >= 3", "num", v >= 3, ok))
    v, ok = c["i16"]
    out.append(("i16 IS NULL OR (i16 >= -100 AND i16 <= 1000)", "num", ~ok | ((v >= -100) & (v <= 1000)),
                np.ones(n, bool)))
    v, ok = c["i32"]
    out.append(("i32 < 12345", "num", v < 12345, ok))
    v, ok = c["i64"]
    out.append(("i64 > 0", "num", v > 0, ok))
    v, ok = c["f32"]
    gt, lt = _nan_cmp(v, 0.5)
    out.append(("f32 <= 0.5", "num", ~gt, ok))
    v, ok = c["f64"]
    gt, _ = _nan_cmp(v, 0.25)
    _, lt = _nan_cmp(v, 1e300)
    out.append(("f64 > 0.25 AND f64 < 1e300", "num", gt & lt, ok))
    v, ok = c["s"]
    small = np.isin(v, [pool_idx[s] for s in GEO_SMALL_IN])
    out.append((f"s IS NULL OR s IN {_in(GEO_SMALL_IN)}", "str", ~ok | small, np.ones(n, bool)))
    out.append((f"s NOT IN {_in(GEO_LONG_IN)}", "str", ~np.isin(v, [pool_idx[s] for s in GEO_LONG_IN]), ok))
    (a, oka), (b, okb) = c["i32"], c["i64"]
    out.append(("i32 < i64", "gen", a.astype(np.int64) < b, oka & okb))
    return out


def np_count(val, known, sel=None):
    if sel is not None:
        known = known & sel
    return None if not known.any() else int((val & known).sum())
