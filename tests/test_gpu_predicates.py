"""Row-exact predicate conformance of the three device paths against the ORACLE.

A predicate runs on the device in one of three implementations, chosen by its syntactic form:
the fused numeric scan body (fuse_numeric, api.cpp:377; pred_bits / num_vals, scan.hip:77/106), the
fused string list (fuse_str_in, api.cpp:450; TK_STR_IN, scan.hip:306-459) and the generic
interpreter (expr_kernel, expr.hip:153), which also runs EVERY where filter.  For each predicate p
of the matrix (tests/predicate_cases.py) the tests compare with oracle.deequ_oracle, exactly:

  * Sum("w", where=p) and Sum("w", where="NOT (p)") over random int64 weights: the fingerprint of
    the TRUE and of the FALSE row SET through the interpreter (a count cannot tell a row gained
    from a row lost), and Size(where=p);
  * Compliance(p) in total and under where "g = k" for the eight groups g = row % 8 plus the
    empty group 8 (the oracle's None), with explain() asserting the path Compliance took.

Families and the path explain() proved for Compliance(p) (the where form is always the interpreter:
"boolmap ... (expr bitmap)"):

  cmp x int / fractional / D literal, 6 column types x 6 operators ...... fused numeric
  the same with <=> ...................................................... interpreter
  literals at / beyond the column type's range, reversed operands ........ fused numeric
  BETWEEN, c IS NULL OR (range), c IS NULL OR cmp ........................ fused numeric
  NOT BETWEEN; an int and a double bound on an int column ................ interpreter
  NaN: f64 > 1e308, f64 <= 0.0, f64 = 0.0 ................................. fused numeric (double)
  NaN: f64 = f64, NOT (...), OR of two comparisons ....................... interpreter
  column x column across types, s = s .................................... interpreter
  Kleene AND / OR / NOT, NULL / TRUE / FALSE literals, depth 5, <=> ...... interpreter
  numeric IN / NOT IN (1, 8, 9, 15 items, NULL item, duplicates) ......... interpreter
  string IN / NOT IN / = / <> (1, 8, 9, 40 items), [c IS NULL OR] ........ fused string list
  string IN with a NULL item ............................................. interpreter
  string ordering, string x number (parse_f64), CAST ..................... interpreter

What ran, by construction:
  * all six BC_NUM_* element types (body_class, api.cpp:512-522): every cmp family case is a fused
    predicate on i8 / i16 / i32 / i64 / f32 / f64, and test_numeric_aggregates_* scans each type;
  * num_chunk_slow (scan.hip:194) via vec_ok = 0 (api.cpp:1450, 1508): the columns of
    test_unaligned_device_columns sit 104 / 52 / 26 / 13 bytes off 16-byte alignment, so num_item
    (scan.hip:222-224) sends every chunk there; their TK_VALIDITY task takes bits_item's word loop;
  * all three bits_item loops (scan.hip:255, 274, 287): 40 993 = 32768 + 8192 + 33 rows, and
    1 048 576 + 8192 + 5 rows (one whole boolmap item, api.cpp:1471/1509, then the next item's
    8192-row loop and word tail);
  * both TK_STR_IN paths: list_small (api.cpp:1484-1491; scan.hip:435) with SMALL8 / ('high','low'),
    the general length-bucketed path (str_in_match, scan.hip:306) with an 8-byte item, 9 and 40
    items and items above 64 bytes (kListLenSlots, scan.hip:308);
  * the kMaxPreds overflow (engine.h:31, api.cpp:641-654): five predicates on (i32, no where) in
    test_kmaxpreds_overflow give preds=3 plus two boolmap tasks;
  * item boundaries (api.cpp:1509-1513): 32768 / 65536 / 131072 / 262144 rows -1, +0, +1, and the
    guided tail split (api.cpp:1519) at 16 x 65536 + 777 int32 rows in one batch.

Findings this module pins ("Predicate conformance"): an int / float value IN a list
of strings is refused with an error (it evaluated to FALSE for every row); the oracle's string ->
double cast follows Double.parseDouble ("1.5d" is 1.5); a long beyond 2^53 against a fractional
literal compares as doubles on the device (unpinned corner).
"""
import ctypes
import math
import re
from fractions import Fraction as F

import numpy as np
import pyarrow as pa
import pytest

import predicate_cases as PC

gpu = pytest.mark.gpu


def _ids(cases):
    return [f"{c.family}: {c.pred[:70]}" for c in cases]


def _schema(t):
    from deequ_amd.table import StructField, StructType, arrow_field_type
    return StructType([StructField(f.name, arrow_field_type(f.type)[0]) for f in t.schema])


def _where_specs(p):
    from deequ_amd.analyzers import Size, Sum
    return [s for a in (Sum("w", where=p), Sum("w", where=f"NOT ({p})"), Size(where=p))
            for s in a.aggregation_functions()]


def _compliance_specs(p):
    from deequ_amd.analyzers import Compliance
    suite = [Compliance("p", p)] + [Compliance("p", p, where=f"g = {k}") for k in PC.GROUPS]
    return [s for a in suite for s in a.aggregation_functions()]


def _tasks(explain):
    return [ln for ln in explain.splitlines() if ln.startswith("task[")]


def _assert_compliance_path(explain, path):
    """Compliance(p) and its nine grouped copies took `path`; the only bitmaps beside them are the
    nine `g = k` filters, which gate the fused tasks (where >= 0)."""
    tasks = _tasks(explain)
    n = 1 + len(PC.GROUPS)
    fused_num = [t for t in tasks if re.search(r" numeric .* preds=[1-3] ", t)]
    fused_str = [t for t in tasks if " str_in " in t]
    bitmaps = [t for t in tasks if " boolmap " in t and "(expr bitmap)" in t]
    if path == "num":
        assert len(fused_num) == n and not fused_str and len(bitmaps) == len(PC.GROUPS), explain
        assert sum("where=-1" not in t for t in fused_num) == len(PC.GROUPS), explain
    elif path == "str":
        assert len(fused_str) == n and not fused_num and len(bitmaps) == len(PC.GROUPS), explain
    else:
        assert not fused_num and not fused_str and len(bitmaps) == n + len(PC.GROUPS), explain


def _assert_where_path(explain):
    tasks = _tasks(explain)
    assert any(" boolmap " in t and "(expr bitmap)" in t for t in tasks), explain
    assert not any(" str_in " in t or re.search(r" preds=[1-3] ", t) for t in tasks), explain


# ------------------------------------------------------------------------------------------------
# Host side (no GPU): the fingerprint, the matrix is not vacuous, the plans take the stated paths
# ------------------------------------------------------------------------------------------------
def test_fingerprint_detects_a_flipped_row_and_a_swapped_pair():
    t, _ = PC.table()
    w = t.column("w").to_pylist()
    tv = list(PC.truth("matrix", PC.CASES[0]))
    base = PC.fingerprint(tv, w)
    i = tv.index(True)
    j = tv.index(False)
    flipped = list(tv)
    flipped[i] = False
    assert PC.fingerprint(flipped, w) != base
    swapped = list(tv)
    swapped[i], swapped[j] = tv[j], tv[i]          # same counts, other rows
    assert PC.count_true(swapped) == PC.count_true(tv)
    assert PC.fingerprint(swapped, w) != base
    k = tv.index(None)
    nulled = list(tv)
    nulled[k], nulled[j] = False, None
    assert PC.fingerprint(nulled, w) != base
    assert sum(w) < 2 ** 53


@pytest.mark.parametrize("c", PC.CASES, ids=_ids(PC.CASES))
def test_oracle_row_sets_are_non_trivial(c):
    """TRUE, FALSE and NULL rows all occur, except the sets the predicate's semantics leave empty
    (Case.empty) -- those must be empty."""
    tv = PC.truth("matrix", c)
    for key, v in (("T", True), ("F", False), ("N", None)):
        n = sum(1 for x in tv if x is v)
        assert (n == 0) == (key in c.empty), (c.pred, key, n)


def test_derived_counts_are_the_oracles_aggregates():
    """expected() derives its counts from the truth vector; the oracle's own agg_compliance /
    agg_conditional_count give the same numbers (sampled: they re-evaluate every row)."""
    from oracle import deequ_oracle as O
    t, ot = PC.table()
    g = t.column("g").to_pylist()
    w = t.column("w").to_pylist()
    for c in [c for c in PC.CASES if c.ref is None][::23]:
        e = PC.expected(PC.truth("matrix", c), w, g)
        assert e["count"] == O.agg_compliance(ot, c.pred, None) == O.agg_conditional_count(ot, c.pred)
        for k in (2, 8):
            assert e["groups"][k] == O.agg_compliance(ot, c.pred, f"g = {k}")
        s = O.agg_sum(ot, "w", c.pred)
        assert s == e["sum_true"]


@pytest.mark.parametrize("c", PC.CASES + PC.ALL_NULL_CASES, ids=_ids(PC.CASES + PC.ALL_NULL_CASES))
def test_plan_takes_the_stated_path(c):
    from deequ_amd.runners.engine import get_plan
    schema = _schema(PC.table()[0])
    _assert_compliance_path(get_plan(schema, _compliance_specs(c.pred)).explain(), c.path)
    if c.where_ok:
        _assert_where_path(get_plan(schema, _where_specs(c.pred)).explain())
    else:
        with pytest.raises(Exception, match="nests deeper"):
            get_plan(schema, _where_specs(c.pred))


@pytest.mark.parametrize("pred", ["i32 IN ('1', '2')", "i64 NOT IN ('1')", "f64 IN ('1.0', 'NaN')",
                                  "i8 IN (1, '2')", "CAST(i32 AS DOUBLE) IN ('1.0')"])
def test_number_in_a_list_of_strings_is_refused(pred):
    """Spark 2.2 InConversion casts the value to STRING (1 IN ('1', '2') is TRUE, and so says the
    oracle); the engine compared the number with the strings as they were and called every row
    FALSE.  It has no cast to string outside a regex, so the form is refused."""
    from deequ_amd.exceptions import AnalysisException
    from deequ_amd.runners.engine import get_plan
    from deequ_amd.sqlexpr import SqlError, compile_expr
    from oracle import deequ_oracle as O
    schema = _schema(PC.table()[0])
    with pytest.raises(SqlError, match="IN a list of strings"):
        compile_expr(pred, schema, schema.index)
    with pytest.raises(AnalysisException):
        get_plan(schema, _compliance_specs(pred))
    node = O.parse_predicate("i32 IN ('1', '2', '03', '4.0')")
    assert [O.eval_predicate(node, {"i32": v}) for v in (1, 2, 3, 4, None)] == [True, True, False, False, None]


def test_lists_beyond_the_interpreter_stack():
    """A list of 16+ items fits no interpreter stack (kMaxStack, kernels.h:127).  The plan refused
    every such expression, also the isContainedIn form that fuses into a TK_STR_IN task and never
    reaches the interpreter (lists up to 256 items, api.cpp fuse_str_in); now only a form that
    has to be materialised is refused."""
    from deequ_amd.analyzers import Compliance
    from deequ_amd.runners.engine import get_plan
    schema = _schema(PC.table()[0])
    items = ", ".join(str(k) for k in range(40))
    for a in (Compliance("p", f"i32 IN ({items})"), Compliance("p", "i32 > 0", where=f"i32 IN ({items})"),
              Compliance("p", f"s IN {PC._in(PC.FORTY)} OR i32 > 0")):
        with pytest.raises(Exception, match="nests deeper"):
            get_plan(schema, a.aggregation_functions())
    fused = Compliance("p", f"s IS NULL OR s IN {PC._in(PC.FORTY)}", where="i32 > 0")
    assert " str_in " in get_plan(schema, fused.aggregation_functions()).explain()


def test_string_column_in_numbers_still_compiles():
    from deequ_amd.sqlexpr import compile_expr
    schema = _schema(PC.table()[0])
    assert compile_expr("s IN (12, '5')", schema, schema.index).words
    assert compile_expr("1 IN ('1', '2')", schema, schema.index).words


# ------------------------------------------------------------------------------------------------
# The matrix on the device
# ------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def tables(gpu_device):
    from deequ_amd import Table
    return {k: Table.from_arrow(PC.table(k)[0], device=gpu_device) for k in ("matrix", "all_null")}


def _check_case(kind, c, df):
    from deequ_amd.runners.engine import get_plan, run_scan
    t, _ = PC.table(kind)
    e = PC.expected(PC.truth(kind, c), t.column("w").to_pylist(), t.column("g").to_pylist())
    if c.where_ok:
        specs = _where_specs(c.pred)
        _assert_where_path(get_plan(df.schema, specs).explain())
        row = run_scan(df, specs)
        print(c.pred, "where form:", row, e)
        assert row[0] == e["sum_true"], "rows the interpreter calls TRUE"
        assert row[1] == e["sum_false"], "rows the interpreter calls FALSE"
        assert row[2] == e["count"]
    specs = _compliance_specs(c.pred)
    _assert_compliance_path(get_plan(df.schema, specs).explain(), c.path)
    row = run_scan(df, specs)
    print(c.pred, "compliance:", row[0], [row[2 + 2 * k] for k in PC.GROUPS], e)
    assert row[0] == e["count"]
    assert row[1] == t.num_rows
    assert [row[2 + 2 * k] for k in PC.GROUPS] == e["groups"]
    assert e["groups"][8] is None


@gpu
@pytest.mark.parametrize("c", PC.CASES, ids=_ids(PC.CASES))
def test_predicate_rows_match_oracle(c, tables):
    assert sum(PC.table()[0].column("w").to_pylist()) < 2 ** 53
    _check_case("matrix", c, tables["matrix"])


@gpu
@pytest.mark.parametrize("c", PC.ALL_NULL_CASES, ids=_ids(PC.ALL_NULL_CASES))
def test_predicates_over_an_all_null_column(c, tables):
    _check_case("all_null", c, tables["all_null"])


@gpu
def test_kmaxpreds_overflow(tables):
    """Five Compliance predicates on (i32, no where) in one Analysis: three fuse, two fall back to
    bitmaps, and all five match the oracle."""
    from deequ_amd import Analysis
    from deequ_amd.analyzers import Compliance
    from deequ_amd.runners.engine import get_plan
    from oracle import deequ_oracle as O
    df = tables["matrix"]
    ot = PC.table()[1]
    suite = [Compliance(f"p{k}", p) for k, p in enumerate(PC.OVERFLOW)]
    explain = get_plan(df.schema, [s for a in suite for s in a.aggregation_functions()]).explain()
    tasks = _tasks(explain)
    assert sum(" numeric " in t and " preds=3 " in t for t in tasks) == 1, explain
    assert sum(" boolmap " in t and "(expr bitmap)" in t for t in tasks) == 2, explain
    ctx = Analysis(suite).run(df)
    for a in suite:
        assert ctx.metric(a).value.get() == O.agg_compliance(ot, a.predicate, None) / df.num_rows, a.predicate


@gpu
def test_long_beyond_2p53_against_a_fractional_literal_compares_as_doubles(gpu_device):
    """Unpinned corner: i64 > 9007199254740992.5 on the row 2^53 + 1.  The device casts
    the long to double (both sides are 2^53: FALSE), the oracle compares the exact decimal (TRUE).
    The device's documented behaviour is asserted; an integer literal stays exact."""
    from deequ_amd import Table
    from deequ_amd.analyzers import Compliance
    from deequ_amd.runners.engine import run_scan
    from oracle import deequ_oracle as O
    vals = [2 ** 53, 2 ** 53 + 1, 2 ** 53 + 2, -(2 ** 53 + 1), 0, None]
    df = Table.from_pydict({"i64": vals}, {"i64": "int64"}, device=gpu_device)
    ot = O.OTable({"i64": vals}, {"i64": "long"})
    p = "i64 > 9007199254740992.5"
    as_double = sum(1 for v in vals if v is not None and float(v) > float("9007199254740992.5"))
    assert as_double == 1 and O.agg_compliance(ot, p, None) == 2
    assert run_scan(df, Compliance("p", p).aggregation_functions())[0] == as_double
    assert run_scan(df, Compliance("p", f"NOT ({p})").aggregation_functions())[0] == 5 - as_double
    q = "i64 > 9007199254740992"
    assert run_scan(df, Compliance("q", q).aggregation_functions())[0] == O.agg_compliance(ot, q, None) == 2


# ------------------------------------------------------------------------------------------------
# Geometry
# ------------------------------------------------------------------------------------------------
_GEO = {}


def _geo_cols():
    if "cols" not in _GEO:
        _GEO["cols"] = PC.geometry_columns()
    return _GEO["cols"]


GEOMETRY = ([(n, None) for n in (1, 31, 32, 33, 63, 64, 65, 1023, 1024, 1025, 8191, 8192, 8193, 40993)] +
            [(s + d, None) for s in (32768, 65536, 131072, 262144) for d in (-1, 0, 1)] +
            [(40993, 1000), (40993, 4096), (8193, 1000), ((1 << 20) + 8192 + 5, None)])


@gpu
@pytest.mark.parametrize("n,batch", GEOMETRY)
def test_geometry(n, batch, gpu_device):
    """One fused numeric predicate per element type, both string-list paths and one interpreter
    predicate (with its weight fingerprints) at row counts around every loop and item boundary;
    numpy references."""
    from deequ_amd import Table
    from deequ_amd.analyzers import Compliance, Sum
    from deequ_amd.runners.engine import get_plan, run_scan
    cols = _geo_cols()
    df = Table.from_arrow(PC.geometry_arrow(cols, n), device=gpu_device, max_batch_rows=batch)
    preds = PC.geometry_predicates(cols, n)
    w = cols["w"][0][:n]
    g3 = cols["g"][0][:n] == 3
    assert int(w.sum()) < 2 ** 53
    suite = []
    for p, _, _, _ in preds:
        suite += [Compliance("p", p), Compliance("p", p, where="g = 3")]
    gen = preds[-1][0]
    suite += [Sum("w", where=gen), Sum("w", where=f"NOT ({gen})")]
    specs = [s for a in suite for s in a.aggregation_functions()]
    tasks = _tasks(get_plan(df.schema, specs).explain())
    assert sum(bool(re.search(r" numeric .* preds=1 ", t)) for t in tasks) == 12
    assert sum(" str_in " in t for t in tasks) == 4
    row = run_scan(df, specs)
    for k, (p, _, val, known) in enumerate(preds):
        got = (row[4 * k], row[4 * k + 2])
        exp = (PC.np_count(val, known), PC.np_count(val, known, g3))
        print(n, batch, p, got, exp)
        assert got == exp, p
    _, _, val, known = preds[-1]
    st, sf = int(w[val & known].sum()), int(w[~val & known].sum())
    exp = (float(st) if (val & known).any() else None, float(sf) if (~val & known).any() else None)
    assert (row[-2], row[-1]) == exp


class _ArrowDeviceColumn:
    """A device column imported by dq_column_from_arrow at ArrowArray.offset (values start
    offset * width bytes into the buffer); what a Table batch needs: dtype, length, to_c()."""

    def __init__(self, arr, offset, device):
        import torch

        from deequ_amd import _native as N
        from deequ_amd.loader import ArrowArrayC, ArrowSchemaC
        fmt = {pa.int64(): b"l", pa.int32(): b"i", pa.int16(): b"s", pa.int8(): b"c", pa.float64(): b"g",
               pa.float32(): b"f"}[arr.type]
        self.dev = [torch.from_numpy(np.frombuffer(b, np.uint8).copy()).to(device) for b in arr.buffers()]
        self.ptrs = (ctypes.c_void_p * 2)(self.dev[0].data_ptr(), self.dev[1].data_ptr())
        n = len(arr) - offset
        self.array = ArrowArrayC(length=n, null_count=arr.slice(offset).null_count, offset=offset,
                                 n_buffers=2, n_children=0, buffers=self.ptrs)
        self.schema = ArrowSchemaC(format=fmt, name=b"x", flags=2)
        self.column = N.dq_column()
        N.check(N.lib.dq_column_from_arrow(ctypes.addressof(self.array), ctypes.addressof(self.schema),
                                           ctypes.byref(self.column)))
        self.dtype, self.length = int(self.column.type), n

    def to_c(self):
        return self.column

    def release(self):
        from deequ_amd import _native as N
        N.lib.dq_column_release(ctypes.byref(self.column))


def _moments_close(st, xs):
    """(n, avg, m2) of the device against exact rational arithmetic, on the scale
    test_moments_against_exact_arithmetic uses: avg within 1e-12 of sum|x|/n, m2 1e-12 relative."""
    from test_gpu_parity import _exact_moments
    e = _exact_moments(xs, xs)
    assert st[0] == e["n"]
    assert abs(F(st[1]) - e["mx"]) <= F(1, 10 ** 12) * e["sx"]
    assert abs(F(st[2]) - e["xm"]) <= F(1, 10 ** 12) * e["xm"]


def _wrap64(s):
    return (s + 2 ** 63) % 2 ** 64 - 2 ** 63


def _agg_specs(col, where):
    from deequ_amd.analyzers import Completeness, Maximum, Minimum, StandardDeviation, Sum
    suite = [Completeness(col, where), Sum(col, where), Minimum(col, where), Maximum(col, where),
             StandardDeviation(col, where)]
    return [s for a in suite for s in a.aggregation_functions()]


def _same(a, b):
    """Exact, NaN-aware; -0.0 == 0.0 holds (their order is documented as unpinned)."""
    if a is None or b is None:
        return a is None and b is None
    return (math.isnan(a) and math.isnan(b)) or a == b


def _check_aggregates(row, vals, valid, sel, is_int, exact_moments=True):
    """row = the result of _agg_specs: [notnull, count, sum, min, max, (n, avg, m2)]."""
    on = valid & sel
    xs = vals[on]
    assert row[0] == int(on.sum())
    if len(xs) == 0:
        assert row[2] is None and row[3] is None and row[4] is None
        return
    if is_int:
        assert row[2] == float(_wrap64(sum(int(x) for x in xs.astype(object)))) if len(xs) < 10_000 \
            else row[2] == float(xs.sum(dtype=np.int64))     # (no overflow: below 2^20 rows of int32)
    else:
        exact = sum(F(float(x)) for x in xs)
        assert abs(F(row[2]) - exact) <= F(1, 10 ** 12) * sum(abs(F(float(x))) for x in xs)
    assert _same(row[3], float(xs.min())) and _same(row[4], float(xs.max()))
    if exact_moments:
        _moments_close(row[5], [float(x) for x in xs])


@gpu
@pytest.mark.parametrize("dtype", ["int64", "int32", "int16", "int8"])
def test_unaligned_device_columns(dtype, gpu_device):
    """values 13 elements (104 / 52 / 26 / 13 bytes) into a device buffer: vec_ok = 0, so every
    chunk runs num_chunk_slow, and the column's TK_VALIDITY task bits_item's word loop.  Equal to
    the aligned copy and to the references."""
    from deequ_amd import Table
    from deequ_amd.analyzers import Completeness, Compliance
    from deequ_amd.runners.engine import run_scan
    from deequ_amd.table import StructField
    col = {"int64": "i64", "int32": "i32", "int16": "i16", "int8": "i8"}[dtype]
    n, off = 9001, 13
    rng = np.random.default_rng(off)
    vals = PC.numeric_values(col, n + off, rng)
    valid = rng.random(n + off) >= 0.1
    arr = pa.array(vals, mask=~valid)
    side = pa.table({"g": pa.array((np.arange(n) % 8).astype(np.int32)),
                     "w": pa.array(rng.integers(0, 2 ** 40, n, dtype=np.int64))})
    aligned = Table.from_arrow(side.append_column("x", pa.array(vals[off:], mask=~valid[off:])),
                               device=gpu_device)
    x = _ArrowDeviceColumn(arr, off, gpu_device)
    try:
        width = vals.dtype.itemsize
        assert x.column.values == x.dev[1].data_ptr() + off * width and x.column.values % 16 != 0
        batch = dict(aligned.batches[0])
        batch["x"] = x
        unaligned = Table(aligned.schema, [batch], gpu_device)
        assert [f.name for f in aligned.schema.fields] == ["g", "w", "x"]
        assert isinstance(aligned.schema.fields[2], StructField) and aligned.schema.fields[2].dtype == x.dtype
        v, ok = vals[off:], valid[off:]
        gsel = (np.arange(n) % 8) < 5
        for where, sel in ((None, np.ones(n, bool)), ("g < 5", gsel)):
            specs = _agg_specs("x", where)
            specs += Compliance("p", "x > 0", where).aggregation_functions()
            specs += Compliance("q", "x IS NULL OR (x >= -8 AND x <= 8)", where).aggregation_functions()
            got, ref = run_scan(unaligned, specs), run_scan(aligned, specs)
            print(dtype, where, got, ref)
            assert got[:5] == ref[:5] and got[6:] == ref[6:]
            _check_aggregates(got, v, ok, sel, True)
            _check_aggregates(ref, v, ok, sel, True)
            assert got[6] == int(((v > 0) & ok & sel).sum())
            assert got[8] == int(((~ok | ((v >= -8) & (v <= 8))) & sel).sum())
        only = Completeness("x").aggregation_functions()      # no numeric task: TK_VALIDITY
        assert run_scan(unaligned, only) == run_scan(aligned, only) == [int(ok.sum()), n]
    finally:
        x.release()


@gpu
@pytest.mark.parametrize("col", PC.NUMERIC)
def test_numeric_aggregates_match_exact_arithmetic(col, gpu_device):
    """Completeness / Sum / Minimum / Maximum exact, Mean / StandardDeviation within 1e-12 of exact
    rational arithmetic, for every element type (i8, i16 and f32 had no parity test), with and
    without a where, in one batch and in batches of 1000; on the matrix table (NaN, +-inf, type
    extremes) Sum / Minimum / Maximum against the oracle, NaN-aware."""
    from deequ_amd import Table
    from deequ_amd.runners.engine import run_scan
    from oracle import deequ_oracle as O
    n = 5003
    t = PC.matrix_arrow(n, 21, edges=False)
    valid = ~np.asarray(t.column(col).is_null())
    vals = t.column(col).combine_chunks().fill_null(0).to_numpy()      # (exact: no trip through double)
    assert vals.dtype == t.schema.field(col).type.to_pandas_dtype()
    for batch in (None, 1000):
        df = Table.from_arrow(t, device=gpu_device, max_batch_rows=batch)
        for where, sel in ((None, np.ones(n, bool)), ("g < 5", (np.arange(n) % 8) < 5),
                           ("g > 7", np.zeros(n, bool))):
            row = run_scan(df, _agg_specs(col, where))
            print(col, batch, where, row)
            _check_aggregates(row, vals, valid, sel, col in PC.INTS)
            if where is None:
                assert row[1] == n
    mt, ot = PC.table()
    df = Table.from_arrow(mt, device=gpu_device)
    for where in (None, "g < 5"):
        row = run_scan(df, _agg_specs(col, where))
        assert row[0] == O.agg_sum_notnull(ot, col, where)
        assert _same(row[2], O.agg_sum(ot, col, where)), (row[2], O.agg_sum(ot, col, where))
        assert _same(row[3], O.agg_min(ot, col, where)) and _same(row[4], O.agg_max(ot, col, where))


@gpu
@pytest.mark.parametrize("col,n", [("i8", 262144 + 1025), ("i32", 16 * 65536 + 777), ("f32", 65536 + 1),
                                   ("i16", 131072 + 33)])
def test_numeric_aggregates_across_item_boundaries(col, n, gpu_device):
    """One batch that crosses the element type's item size (api.cpp:1509), and for int32 one with
    n_items >= 16 so that the guided tail split cuts the last items (api.cpp:1519); numpy
    references (extended precision for the moments)."""
    from deequ_amd import Table
    from deequ_amd.runners.engine import run_scan
    cols = _geo_cols()
    df = Table.from_arrow(PC.geometry_arrow(cols, n, [col, "g"]), device=gpu_device)
    vals, valid = cols[col][0][:n], cols[col][1][:n]
    if col == "f32":                                   # finite values: the sums are then exact-able
        fin = np.isfinite(vals)
        assert (~fin & valid).any()
        vals = vals.copy()
        vals[~fin] = 0.5
        df = Table.from_arrow(pa.table({col: pa.array(vals, mask=~valid), "g": pa.array(cols["g"][0][:n])}),
                              device=gpu_device)
    for where, sel in ((None, np.ones(n, bool)), ("g < 5", cols["g"][0][:n] < 5)):
        row = run_scan(df, _agg_specs(col, where))
        print(col, n, where, row)
        xs = vals[valid & sel]
        if col in PC.INTS:
            _check_aggregates(row, vals, valid, sel, True, exact_moments=False)
        x = xs.astype(np.longdouble)
        mean = x.sum() / len(x)
        m2 = ((x - mean) ** 2).sum()
        assert row[0] == len(xs) and row[5][0] == len(xs)
        if col not in PC.INTS:
            exact = math.fsum(float(v) for v in xs)
            assert abs(row[2] - exact) <= 1e-12 * math.fsum(abs(float(v)) for v in xs)
            assert _same(row[3], float(xs.min())) and _same(row[4], float(xs.max()))
        assert abs(row[5][1] - float(mean)) <= 1e-12 * float(np.abs(x).sum() / len(x))
        assert abs(row[5][2] - float(m2)) <= 1e-12 * float(m2)
