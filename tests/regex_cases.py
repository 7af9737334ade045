"""Deterministic case tables and the two references for tests/test_regex_cases.py (host) and
tests/test_gpu_regex_rows.py (device): plain helper, no GPU, no fixtures.

Two device code paths walk a compiled Java-regex automaton (csrc/expr.hip): regex_find_kernel (u8
successor table in LDS, four rows per lane, 16-byte chunks, byte-wise within 16 bytes of the data
buffer's end) and the XI_REGEX case of expr_kernel (u16 tables in global memory; every automaton
above 255 states, every regex inside a larger expression, every non-string operand).  A case here is
one pattern over one table whose rows are built so that a given walker feature decides each row.

References, both on the host:
  * oracle_truth: the oracle's regex_find_nonempty (Python `re`, independent of the compiler);
  * automaton_truth: compile_java_regex(p).matches(row) (the same automaton, walked on the host).
A truth vector holds True / False per non-NULL row and None for a NULL row.  What a device
observable makes of None depends on its spelling (see predicate / tv_nonempty).

Case.empty names the row sets ("T", "F", "N") that the case's CONSTRUCTION leaves empty (a one-row
table, an all-NULL column, `^(true|false)$` over booleans); every other case has TRUE and FALSE rows.
"""
from collections import namedtuple
from functools import lru_cache

import numpy as np

Case = namedtuple("Case", "family name pattern batches empty meta")

GEO_LENGTHS = tuple(range(0, 51)) + (63, 64, 65, 127, 128, 129)
ROW_COUNTS = (1, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 4099)
NULL_ROWS = (0, 63, 64, 255, 256)        # and the last row
LONG_ROW = 5000

# the two automaton-size edges (n_states asserted by the host test and again on the device)
PATTERN_NS_255 = "(a[ab]{6}|c[cd]{5}|e[ef]{4}|g[gh]{3}|i[ij]{3})$"
NS_255 = 255        # the fused table's dynamic LDS request is exactly 65 536 bytes
PATTERN_NS_263 = "a[ab]{7}$"
NS_263 = 263        # above kRegexMaxStates: the interpreter walks it


def sql_string(s):
    return "'" + s.replace("\\", "\\\\").replace("'", "''") + "'"


def rows_of(c):
    return [r for b in c.batches for r in b]


# ------------------------------------------------------------------------------------------------
# Geometry: the plant at every byte offset of rows of every length
# ------------------------------------------------------------------------------------------------
# name, pattern, filler (ASCII, cycled by byte position), plant, decoy (same byte length) or None
GEOMETRY_SPECS = [
    ("sticky accept", "q", "a", "q", None),
    ("dead on the first byte", "^q", "a", "q", None),
    ("must reach the end: $", "q$", "a", "q", None),
    ("must reach the end: .{3}$", "q.{3}$", "a", "q", None),
    ("must reach the end: \\z", "q\\z", "a", "q", None),
    ("two-byte plant, near-miss on byte 2", "é", "a", "é", "è"),                 # C3 A9 / C3 A8
    ("two-byte plant at the end", "é$", "a", "é", "è"),
    ("three-byte plant, near-miss on byte 2", "例", "a", "例", "佋"),             # E4 BE 8B / E4 BD 8B
    ("three-byte plant, near-miss on byte 3", "例", "a", "例", "侊"),             # E4 BE 8B / E4 BE 8A
    ("bounded repeat", "\\d{3}-\\d{2}", "a", "123-45", "123-4x"),
    ("case-insensitive", "(?i)qz", "a", "Qz", "Qx"),
    ("nullable", "\\d*", "a", "7", None),
    ("word boundary", "\\bq\\b", "a ", "q", None),
]


def _fill(filler, n):
    return (filler * (n // len(filler) + 1))[:n].encode("ascii")


def geometry_rows(filler, plant, decoy):
    """(rows, meta): per length L one row of filler, then for every offset j at which the plant
    fits (j in 0..L - len(plant)) the filler row with the plant's bytes at j, and the same with the
    decoy.  meta[i] = (L, j or None, "none" / "plant" / "decoy")."""
    pb = plant.encode("utf-8")
    db = decoy.encode("utf-8") if decoy is not None else None
    assert db is None or len(db) == len(pb)
    rows, meta = [], []
    for n in GEO_LENGTHS:
        base = _fill(filler, n)
        rows.append(base.decode("utf-8"))
        meta.append((n, None, "none"))
        for j in range(0, n - len(pb) + 1):
            rows.append((base[:j] + pb + base[j + len(pb):]).decode("utf-8"))
            meta.append((n, j, "plant"))
            if db is not None:
                rows.append((base[:j] + db + base[j + len(db):]).decode("utf-8"))
                meta.append((n, j, "decoy"))
    return rows, meta


def _geometry_cases():
    out = []
    for name, pattern, filler, plant, decoy in GEOMETRY_SPECS:
        rows, meta = geometry_rows(filler, plant, decoy)
        out.append(Case("geometry", name, pattern, (tuple(rows),), "N", tuple(meta)))
    return out


# ------------------------------------------------------------------------------------------------
# The data buffer's end: every batch is its own buffer, and its last row ends at off[rows]
# ------------------------------------------------------------------------------------------------
def buffer_end_batches():
    out = []
    for t in range(0, 18):
        hit = "a" * (t - 1) + "q" if t else ""
        # the rows before the last one also lie within 16 bytes of the end while t is small
        out.append(("aq", "a", "", hit))
        if t:
            out.append(("q", "aa", "a" * t))                        # the same length, no plant
        out.append(("a" * 20 + "q", "qa", hit))                     # a buffer above 16 bytes
        if t >= 4:
            out.append(("a", "a" * (t - 4) + "qaaa"))               # decided three bytes earlier
    out.append(("q", "a", "aq"))                                    # the whole buffer: 4 bytes
    out.append(("", "", "q"))                                       # ... 1 byte
    out.append(("aaaq", "a", None))                                 # the last row NULL
    out.append(("a" * 30 + "q", None, "aq", None))
    out.append((None, "q"))
    return tuple(out)


def _buffer_end_cases():
    b = buffer_end_batches()
    return [Case("buffer end", "must reach the end", "q$", b, "", None),
            Case("buffer end", "sticky accept", "q", b, "", None),
            Case("buffer end", "three from the end", "q.{3}$", b, "", None)]


# ------------------------------------------------------------------------------------------------
# Row counts at word (64), group (256) and block (1024) edges; validity
# ------------------------------------------------------------------------------------------------
def count_rows(n):
    """Rows of 0..22 bytes; a third hold a q inside, a third end in q.  From 63 rows on, NULLs at
    rows 0, 63, 64, 255, 256 and the last row, each with an empty string next to it."""
    rows = []
    for i in range(n):
        ln = (i * 7) % 23
        s = "a" * ln
        if i % 3 == 0:
            j = (i * 5) % ln if ln else 0
            s = s[:j] + "q" + s[j + 1:]
        elif i % 3 == 1:
            s += "q"
        rows.append(s)
    if n >= 63:
        nulls = [r for r in NULL_ROWS + (n - 1,) if r < n]
        for r in nulls:
            for k in (r - 1, r + 1):
                if 0 <= k < n:
                    rows[k] = ""
        for r in nulls:
            rows[r] = None
    return rows


def _split(rows, batch):
    if not batch:
        return (tuple(rows),)
    return tuple(tuple(rows[k:k + batch]) for k in range(0, len(rows), batch))


def _count_cases():
    out = []
    for n in ROW_COUNTS:
        for batch in (None, 1000):
            out.append(Case("row count", f"{n} rows, batch {batch}", "q$", _split(count_rows(n), batch),
                            "FN" if n == 1 else "", None))
    out.append(Case("validity", "all-NULL column", "q$", ((None,) * 70,), "TF", None))
    return out


WHERE_TABLE_ROWS = 257          # the where filters run over count_rows(257); g = row % 8
WHERES = (("g = 8", lambda r: False), ("g = 0", lambda r: r % 8 == 0))


# ------------------------------------------------------------------------------------------------
# Divergence: one 5000-byte row among short rows, in each of a lane's four row slots
# ------------------------------------------------------------------------------------------------
def divergence_batches():
    """Eight batches of 256 rows (one group of four bitmap words each).  Batch k holds one
    5000-byte row in word k % 4 (lane 17 + k) and 255 rows of 0..3 bytes; the long row's q is its
    last byte in batches 0-3 and its last but one in batches 4-7, so its verdict falls in its last
    chunk (5000 = 312 * 16 + 8)."""
    short = ("", "q", "aq", "aqa", "a", "qa", "aa", "aaq")
    out = []
    for k in range(8):
        rows = [short[(r * 3 + k) % len(short)] for r in range(256)]
        body = "a" * (LONG_ROW - 1) + "q" if k < 4 else "a" * (LONG_ROW - 2) + "qa"
        rows[(k % 4) * 64 + 17 + k] = body
        out.append(tuple(rows))
    return tuple(out)


def _divergence_cases():
    b = divergence_batches()
    return [Case("divergence", "must reach the end", "q$", b, "N", None),
            Case("divergence", "sticky accept on finished lanes", "q", b, "N", None),
            Case("divergence", "dead on finished lanes", "^a+q$", b, "N", None)]


# ------------------------------------------------------------------------------------------------
# Automaton size: 255 states (the largest fused table) and 263 (the interpreter by itself)
# ------------------------------------------------------------------------------------------------
def _bits(x, n, zero, one):
    return "".join(one if (x >> k) & 1 else zero for k in range(n))


def size_rows():
    """Rows over a..j that end in (or just miss) every alternative of PATTERN_NS_255, and rows of
    a / b of 0..14 bytes for PATTERN_NS_263; one NULL."""
    alts = (("a", 6, "a", "b"), ("c", 5, "c", "d"), ("e", 4, "e", "f"), ("g", 3, "g", "h"),
            ("i", 3, "i", "j"))
    rows = []
    for i in range(700):
        h = (i * 2654435761) & 0xffffffff
        s = _bits(h >> 8, i % 15, "a", "b")
        if i % 2:
            head, n, zero, one = alts[(i // 2) % len(alts)]
            s += head + _bits(h >> 3, n - (1 if i % 7 == 0 else 0), zero, one)
            if i % 11 == 0:
                s += "b"
        rows.append(s)
    rows[300] = None
    return rows


def _size_cases():
    rows = (tuple(size_rows()),)
    return [Case("automaton size", "255 states", PATTERN_NS_255, rows, "", None),
            Case("automaton size", "263 states", PATTERN_NS_263, rows, "", None)]


GEOMETRY_CASES = _geometry_cases()
STRING_CASES = (GEOMETRY_CASES + _buffer_end_cases() + _count_cases() + _divergence_cases() +
                _size_cases())
assert len({(c.family, c.name, c.pattern) for c in STRING_CASES}) == len(STRING_CASES)


def case_id(c):
    return f"{c.family}: {c.name} /{c.pattern}/"


def where_case():
    return next(c for c in STRING_CASES if c.name == f"{WHERE_TABLE_ROWS} rows, batch None")


# ------------------------------------------------------------------------------------------------
# Non-string operands (the interpreter prints them as Spark's cast to string, then walks)
# ------------------------------------------------------------------------------------------------
I64_MIN, I64_MAX = -2 ** 63, 2 ** 63 - 1
NONSTRING_COLUMNS = {
    "i64": ("int64", [I64_MIN, I64_MAX, 0, -1, 7, -7, 17, 1234567890123456789, I64_MIN + 1,
                      -1000000000000000007, None, 10, 9, -10, 999999999999999999, None, 1]),
    "i32": ("int32", [-2 ** 31, 2 ** 31 - 1, 0, -1, 7, -7, 17, 2147483637, -2 ** 31 + 1,
                      -1000000007, None, 10, 9, -10, 999999999, None, 1]),
    "i16": ("int16", [-2 ** 15, 2 ** 15 - 1, 0, -1, 7, -7, 17, 32757, -2 ** 15 + 1,
                      -10007, None, 10, 9, -10, 9999, None, 1]),
    "i8": ("int8", [-128, 127, 0, -1, 7, -7, 17, 107, -127, -107, None, 10, 9, -10, 99, None, 1]),
    "b": ("bool", [True, False, None, True, True, False, None, False, True, False, None, True,
                   False, False, True, None, True]),
}
N_NONSTRING = 17
assert all(len(v) == N_NONSTRING for _, v in NONSTRING_COLUMNS.values())

NsCase = namedtuple("NsCase", "col pattern empty")
NONSTRING_CASES = (
    [NsCase("i64", p, "") for p in ("^-9223372036854775808$", "^-", "7$", "^\\d{19}$", "^9223372036854775807$",
                                    "^-\\d{19}$", "^0$", "^-?1")] +
    [NsCase("i32", p, "") for p in ("^-2147483648$", "^-", "7$", "^\\d{10}$", "^2147483647$", "^-?1")] +
    [NsCase("i16", p, "") for p in ("^-32768$", "^-", "7$", "^\\d{5}$", "^32767$")] +
    [NsCase("i8", p, "") for p in ("^-128$", "^-", "7$", "^\\d{3}$", "^127$")] +
    [NsCase("b", "^(true|false)$", "F"), NsCase("b", "^true$", ""), NsCase("b", "^.{5}$", ""),
     NsCase("b", "^f", ""), NsCase("b", "ue$", "")])


def nonstring_text(col, v):
    """Spark's cast to string of an integral / boolean value, restated plainly."""
    if v is None:
        return None
    return ("true" if v else "false") if col == "b" else str(int(v))


def ns_case_id(c):
    return f"{c.col} /{c.pattern}/"


# ------------------------------------------------------------------------------------------------
# References, weights, fingerprints
# ------------------------------------------------------------------------------------------------
def _oracle_vector(texts, pattern):
    from oracle.deequ_oracle import regex_find_nonempty
    return tuple(None if t is None else bool(regex_find_nonempty(t, pattern)) for t in texts)


def _automaton_vector(texts, pattern):
    from deequ_amd.regex import compile_java_regex
    rx = compile_java_regex(pattern)
    return tuple(None if t is None else bool(rx.matches(t)) for t in texts)


@lru_cache(maxsize=None)
def oracle_truth(c):
    if isinstance(c, NsCase):
        return _oracle_vector([nonstring_text(c.col, v) for v in NONSTRING_COLUMNS[c.col][1]], c.pattern)
    return _oracle_vector(rows_of(c), c.pattern)


@lru_cache(maxsize=None)
def automaton_truth(c):
    if isinstance(c, NsCase):
        return _automaton_vector([nonstring_text(c.col, v) for v in NONSTRING_COLUMNS[c.col][1]], c.pattern)
    return _automaton_vector(rows_of(c), c.pattern)


@lru_cache(maxsize=None)
def n_states(pattern):
    from deequ_amd.regex import compile_java_regex
    return compile_java_regex(pattern).n_states


@lru_cache(maxsize=None)
def is_nullable(pattern):
    from deequ_amd.regex import nullable_pattern
    return nullable_pattern(pattern)


def predicate(col, pattern):
    """(SQL, NULL rows are FALSE?): `col RLIKE 'p'` (NULL on NULL).  RLIKE is find() INCLUDING an
    empty match, so over a nullable pattern it is TRUE for every row; the find-non-empty expression
    PatternMatch counts is spelled dq_find_nonempty(col, 'p') (FALSE on NULL) and used for those."""
    if is_nullable(pattern):
        return f"dq_find_nonempty({col}, {sql_string(pattern)})", True
    return f"{col} RLIKE {sql_string(pattern)}", False


def tv_nonempty(tv):
    """What PatternMatch / dq_find_nonempty report: a NULL row is FALSE."""
    return tuple(False if v is None else v for v in tv)


def kleene_and(tv, sel):
    """The truth vector of `(p) AND f` for a filter f that is never NULL (sel: its value per row)."""
    return tuple(False if not k else v for v, k in zip(tv, sel))


@lru_cache(maxsize=None)
def weights(n):
    """The predicate suite's weight column: random in [0, 2^40), fixed seed; none is 0."""
    w = np.random.default_rng(7).integers(1, 2 ** 40, n, dtype=np.int64)
    assert int(w.sum()) < 2 ** 53
    return w


def truth_code(tv):
    """A truth vector as int8: 1 TRUE, 0 FALSE, -1 NULL (an array already in this form passes)."""
    if isinstance(tv, np.ndarray):
        return tv
    return np.array([-1 if v is None else int(v) for v in tv], np.int8)


def fingerprint(tv, w, sel=None):
    """(sum of w over the TRUE rows, the FALSE rows, the NULL rows) among the selected rows: exact
    integers.  Two different row sets have equal sums with probability ~2^-40."""
    code = truth_code(tv)
    assert len(code) == len(w)
    keep = np.ones(len(code), bool) if sel is None else np.asarray(sel, bool)
    return tuple(int(w[(code == k) & keep].sum()) for k in (1, 0, -1))


def expected(tv, w, sel=None):
    """What the device must report for a predicate with truth vector tv (under an optional row
    selection): Sum(w, where=p), Sum(w, where=NOT p), the count of TRUE rows (None when no selected
    row is non-NULL: sum over nothing), the number of selected rows."""
    keep = [True] * len(tv) if sel is None else list(sel)
    st, sf, _ = fingerprint(tv, w, sel)
    live = [v for v, k in zip(tv, keep) if k]
    return {
        "sum_true": float(st) if any(v is True for v in live) else None,
        "sum_false": float(sf) if any(v is False for v in live) else None,
        "count": None if all(v is None for v in live) else sum(1 for v in live if v is True),
        "rows": len(live),
    }
