"""Row-exact conformance of the two device regex walkers (csrc/expr.hip) against the oracle.

The cases are tests/regex_cases.py (checked on the host by tests/test_regex_cases.py): the
deciding byte at every offset of rows of every length, multi-byte characters across the 16-byte
chunk boundaries, rows ending at the data buffer's end, row counts at the 64 / 256 / 1024-row
edges, NULLs at those edges, one 5000-byte row among short ones, automata of 255 and 263 states,
integers and booleans printed by the interpreter.  Every row is pinned, through three observables:

  * RowLevelSchemaValidator with a regex clause (rowschema.hip -> launch_regex, null_mode 0): the
    valid rows are the oracle's TRUE rows and the NULL rows (tests/schema_host.py: `s IS NULL OR
    matches`), the invalid rows its FALSE rows, row for row by an id column;
  * p = `s RLIKE '...'` as Compliance("c", p), Size(where=p), Sum(w, where=p) and
    Sum(w, where=NOT (p)) over random weights (the fingerprints of the TRUE and of the FALSE row
    set), and PatternMatch("s", pattern);
  * the same with p forced onto the interpreter: `p AND g >= 0`, g never negative.

Which walker ran: explain() does not name it ("boolmap ... (expr bitmap)" for both).  The path
follows from api.cpp's rule (dq_state_create, the caller of build_regex_table): a program of exactly
two instructions [XI_COL utf8, XI_REGEX] whose automaton has at most kRegexMaxStates = 255 states
runs regex_find_kernel; anything else runs expr_kernel's XI_REGEX walk.  So `s RLIKE '...'`,
dq_find_nonempty(s, '...') (PatternMatch's expression) and the schema clause are fused when n_states
<= 255; NOT (p), p AND g >= 0, the 263-state pattern and every non-string operand are interpreted.
The n_states assertions below (and in test_regex_cases.py) are the guard.

RLIKE is find() including an empty match, so over the one nullable pattern (\\d*) the predicate is
spelled dq_find_nonempty(s, '...') -- RLIKE itself must then be TRUE on every non-NULL row, which is
asserted too.  All comparisons are exact.
"""
import numpy as np
import pyarrow as pa
import pytest

import regex_cases as RC

pytestmark = pytest.mark.gpu


def _arrow(rows, first_id, extra=None):
    n = len(rows)
    ids = np.arange(first_id, first_id + n)
    cols = {"s": pa.array(list(rows), pa.string()), "id": pa.array(ids.astype(np.int32)),
            "g": pa.array((ids % 8).astype(np.int32))}
    cols.update(extra or {})
    return pa.table(cols)


def _device_table(batches, device):
    """One device batch per batch of the case: each has its own offsets and data buffer."""
    from deequ_amd.table import Table
    n = sum(len(b) for b in batches)
    w = RC.weights(n)
    tables, at = [], 0
    for b in batches:
        tables.append(Table.from_arrow(_arrow(b, at, {"w": pa.array(w[at:at + len(b)])}), device=device))
        at += len(b)
    return Table(tables[0].schema, [x for t in tables for x in t.batches], device)


def _specs(p, col, pattern, where=None):
    from deequ_amd.analyzers import Compliance, PatternMatch, Size, Sum
    both = p if where is None else f"({p}) AND {where}"
    neg = f"NOT ({p})" if where is None else f"(NOT ({p})) AND {where}"
    suite = [Sum("w", where=both), Sum("w", where=neg), Size(where=both), Compliance("c", p, where),
             PatternMatch(col, pattern, where)]
    return [s for a in suite for s in a.aggregation_functions()]


def _check_scan(df, col, pattern, tv, sel=None, where=None, forms=("plain", "interpreted")):
    """Sum / Size / Compliance / PatternMatch of the pattern over df[col] against the truth vector
    tv (None = a NULL row), as written and forced onto the interpreter."""
    from deequ_amd.runners.engine import get_plan, run_scan
    w = RC.weights(len(tv))
    p, null_is_false = RC.predicate(col, pattern)
    ptv = RC.tv_nonempty(tv) if null_is_false else tv
    e = RC.expected(ptv, w, sel)
    # Size(where=(p) AND f) counts over EVERY row: a row f rejects is FALSE there, not unselected
    size = e["count"] if sel is None else RC.expected(RC.kleene_and(ptv, sel), w)["count"]
    pm = RC.expected(RC.tv_nonempty(tv), w, sel)
    for form in forms:
        q = p if form == "plain" else f"{p} AND g >= 0"
        specs = _specs(q, col, pattern, where)
        tasks = [ln for ln in get_plan(df.schema, specs).explain().splitlines() if ln.startswith("task[")]
        assert sum(" boolmap " in t and "(expr bitmap)" in t for t in tasks) >= 2, tasks
        row = run_scan(df, specs)
        print(form, q, where, row, e, size, pm)
        assert row[0] == e["sum_true"], "rows called TRUE"
        assert row[1] == e["sum_false"], "rows called FALSE"
        assert row[2] == size
        assert (row[3], row[4]) == (e["count"], e["rows"])                    # Compliance
        assert row[5] == (pm["count"] if pm["rows"] else None) and row[6] == pm["rows"]     # PatternMatch


def _check_schema(df, pattern, tv):
    from deequ_amd import RowLevelSchema, RowLevelSchemaValidator
    from test_gpu_schema import table_to_lists
    res = RowLevelSchemaValidator.validate(df, RowLevelSchema().with_string_column("s", matches=pattern))
    valid, invalid = table_to_lists(res.valid_rows), table_to_lists(res.invalid_rows)
    want_valid = [i for i, v in enumerate(tv) if v is not False]       # s IS NULL OR matches
    want_invalid = [i for i, v in enumerate(tv) if v is False]
    print("schema", pattern, res.num_valid_rows, res.num_invalid_rows, len(want_valid), len(want_invalid))
    assert valid["id"] == want_valid and invalid["id"] == want_invalid
    assert (res.num_valid_rows, res.num_invalid_rows) == (len(want_valid), len(want_invalid))


@pytest.mark.parametrize("c", RC.STRING_CASES, ids=[RC.case_id(c) for c in RC.STRING_CASES])
def test_regex_rows_match_oracle(c, gpu_device):
    tv = RC.oracle_truth(c)
    ns = RC.n_states(c.pattern)
    df = _device_table(c.batches, gpu_device)
    assert df.num_rows == len(tv) and len(df.batches) == len(c.batches)
    if c.family == "automaton size":
        assert ns == {RC.PATTERN_NS_255: RC.NS_255, RC.PATTERN_NS_263: RC.NS_263}[c.pattern]
    else:
        assert ns <= 255
    _check_scan(df, "s", c.pattern, tv)
    if ns <= 255:
        _check_schema(df, c.pattern, tv)
    else:           # the validator takes fused tables only; the interpreter walked every form above
        from deequ_amd import RowLevelSchema, RowLevelSchemaValidator
        with pytest.raises(ValueError, match="at most 255"):
            RowLevelSchemaValidator.validate(df, RowLevelSchema().with_string_column("s", matches=c.pattern))


def test_the_two_walkers_agree_at_the_size_split(gpu_device):
    """The 255-state pattern through regex_find_kernel (65 536 bytes of LDS) and through the
    interpreter, and the 263-state pattern (the interpreter by itself), give the oracle's row sets
    over the same rows; the fused and the interpreted spelling of each report equal sums."""
    from deequ_amd.analyzers import Sum
    from deequ_amd.runners.engine import run_scan
    rows = (tuple(RC.size_rows()),)
    df = _device_table(rows, gpu_device)
    w = RC.weights(len(rows[0]))
    for pattern, ns in ((RC.PATTERN_NS_255, RC.NS_255), (RC.PATTERN_NS_263, RC.NS_263)):
        assert RC.n_states(pattern) == ns
        p = f"s RLIKE {RC.sql_string(pattern)}"
        suite = [Sum("w", where=p), Sum("w", where=f"{p} AND g >= 0"), Sum("w", where=f"NOT ({p})"),
                 Sum("w", where=f"NOT ({p} AND g >= 0)")]
        row = run_scan(df, [s for a in suite for s in a.aggregation_functions()])
        st, sf, _ = RC.fingerprint(RC._oracle_vector(rows[0], pattern), w)
        print(pattern, ns, row, st, sf)
        assert row == [float(st), float(st), float(sf), float(sf)]


@pytest.mark.parametrize("where,keep", RC.WHERES, ids=[x[0] for x in RC.WHERES])
def test_regex_under_a_where_filter(where, keep, gpu_device):
    """A where that selects no row (g = 8) and one that selects every eighth row (g = 0), over the
    257-row table with NULLs at rows 0, 63, 64, 255 and 256."""
    c = RC.where_case()
    tv = RC.oracle_truth(c)
    assert len(tv) == RC.WHERE_TABLE_ROWS
    df = _device_table(c.batches, gpu_device)
    sel = [keep(r) for r in range(len(tv))]
    assert sum(sel) == (0 if where == "g = 8" else 33)
    _check_scan(df, "s", c.pattern, tv, sel, where)


def test_rlike_of_a_nullable_pattern_is_true_on_every_row(gpu_device):
    c = next(c for c in RC.GEOMETRY_CASES if c.pattern == "\\d*")
    df = _device_table(c.batches, gpu_device)
    from deequ_amd.analyzers import Compliance
    from deequ_amd.runners.engine import run_scan
    n = df.num_rows
    for p in ("s RLIKE '\\\\d*'", "s RLIKE '\\\\d*' AND g >= 0"):
        assert run_scan(df, Compliance("c", p).aggregation_functions()) == [n, n]


# ------------------------------------------------------------------------------------------------
# Non-string operands: the interpreter prints the value, then walks
# ------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def nonstring_table(gpu_device):
    from deequ_amd.table import Table
    n = RC.N_NONSTRING
    cols = {k: pa.array(v, getattr(pa, "bool_" if t == "bool" else t)())
            for k, (t, v) in RC.NONSTRING_COLUMNS.items()}
    cols["g"] = pa.array((np.arange(n) % 8).astype(np.int32))
    cols["w"] = pa.array(RC.weights(n))
    return Table.from_arrow(pa.table(cols), device=gpu_device)


@pytest.mark.parametrize("c", RC.NONSTRING_CASES, ids=[RC.ns_case_id(c) for c in RC.NONSTRING_CASES])
def test_regex_over_integers_and_booleans(c, nonstring_table):
    """INT64_MIN (printed through 0 - (uint64)x), the other extremes of every integer width, 0,
    -1 and both booleans against patterns that tell the sign, the first and last digit and the
    length; NULL rows stay NULL under RLIKE and count as non-matching for PatternMatch."""
    _check_scan(nonstring_table, c.col, c.pattern, RC.oracle_truth(c))
