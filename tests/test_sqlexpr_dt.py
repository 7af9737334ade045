"""Host-side typing of date / timestamp comparisons, the date functions, typed literals and
CAST AS STRING: the emitted words of each rule, the literal folding, the refusals and the plan's
text-slot assignment.  Before this feature every typing case here raised SqlError."""
import ctypes
import struct

import pytest

from deequ_amd import _native as N
from deequ_amd.sqlexpr import (SqlError, compile_expr, date_literal, timestamp_literal,
                               timestamp_of_string)
from deequ_amd.table import StructField, StructType

SCHEMA = StructType([StructField("s", N.UTF8), StructField("i8", N.INT8), StructField("i32", N.INT32),
                     StructField("i64", N.INT64), StructField("f32", N.FLOAT32), StructField("b", N.BOOL),
                     StructField("dec", N.decimal_type(10, 2)), StructField("d", N.DATE32),
                     StructField("d2", N.DATE32), StructField("ts", N.TIMESTAMP_US)])
COL = {f.name: k for k, f in enumerate(SCHEMA.fields)}
DAY = 86_400_000_000


def comp(sql):
    return compile_expr(sql, SCHEMA, SCHEMA.index).words


def lit(text):
    b = text.encode()
    p = b + b"\0" * (-len(b) % 8)
    return [N.X_STR, len(b)] + list(struct.unpack(f"<{len(p) // 8}q", p))


def c(name):
    return [N.X_COL, COL[name]]


def cs(name):
    return [N.X_CAST_STR] + c(name)


# ------------------------------------------------------------------------------------------------
# One word list per rule
# ------------------------------------------------------------------------------------------------
def test_same_type_pairs_compare_natively():
    assert comp("d2 >= d") == [N.X_GE] + c("d2") + c("d")
    assert comp("ts <=> ts") == [N.X_EQ_NULL_SAFE] + c("ts") + c("ts")
    assert comp("d = DATE '2000-02-29'") == [N.X_EQ] + c("d") + [N.X_DATE, 11016]
    assert comp("TIMESTAMP '1970-01-02 00:00:00.5' < ts") == [N.X_LT, N.X_TIMESTAMP, DAY + 500000] + c("ts")
    assert comp("to_date(ts) = d")[:5] == [N.X_EQ, N.X_FUNC, N.FN_TO_DATE, N.DATE32, 1]


def test_a_date_against_a_string_needs_its_cast_written_under_every_operator():
    """Spark casts the date to string; the implicit form stays refused (an earlier test pins
    `day >= '2020-01-01'` so) and the message names both explicit spellings."""
    for sym, op in (("=", N.X_EQ), ("<>", N.X_NE), ("<", N.X_LT), ("<=", N.X_LE), (">", N.X_GT),
                    (">=", N.X_GE), ("<=>", N.X_EQ_NULL_SAFE)):
        assert comp(f"CAST(d AS STRING) {sym} '2020-1-1'") == [op] + cs("d") + lit("2020-1-1")
        assert comp(f"s {sym} CAST(d AS STRING)") == [op] + c("s") + cs("d")
        assert comp(f"d {sym} DATE '1970-01-02'") == [op] + c("d") + [N.X_DATE, 1]
        for sql in (f"d {sym} '2020-01-01'", f"s {sym} d", f"to_date(ts) {sym} '2020-01-01'",
                    f"'x' {sym} date_add(d, 1)"):
            with pytest.raises(SqlError, match=r"of a date and a string.*CAST\(x AS STRING\).*DATE '...' literal"):
                comp(sql)
    with pytest.raises(SqlError, match="of a date and a string"):
        comp("d BETWEEN '2000-01-01' AND '2001-01-01'")


def test_a_timestamp_against_a_string():
    for sym, op in (("<", N.X_LT), ("<=", N.X_LE), (">", N.X_GT), (">=", N.X_GE)):
        assert comp(f"ts {sym} '2020-01-01'") == [op] + cs("ts") + lit("2020-01-01")
        assert comp(f"s {sym} ts") == [op] + c("s") + cs("ts")
    t0 = 18262 * DAY
    for sym, op in (("=", N.X_EQ), ("<>", N.X_NE), ("<=>", N.X_EQ_NULL_SAFE)):
        assert comp(f"ts {sym} '2020-01-01'") == [op] + c("ts") + [N.X_TIMESTAMP, t0]
        assert comp(f"'2020-01-01 00:00:01.25' {sym} ts") == [op, N.X_TIMESTAMP, t0 + 1_250_000] + c("ts")


def test_a_date_against_a_timestamp_casts_both():
    assert comp("d < ts") == [N.X_LT] + cs("d") + cs("ts")
    assert comp("ts = d") == [N.X_EQ] + cs("ts") + cs("d")


def test_null_operands_and_between():
    assert comp("d = NULL") == [N.X_EQ] + c("d") + [N.X_NULL]
    assert comp("NULL <=> ts") == [N.X_EQ_NULL_SAFE, N.X_NULL] + c("ts")
    assert comp("d BETWEEN DATE '1970-01-02' AND d2") == ([N.X_AND, N.X_GE] + c("d") + [N.X_DATE, 1] +
                                                         [N.X_LE] + c("d") + c("d2"))
    assert comp("ts BETWEEN '2000' AND '2021'")[:5] == [N.X_AND, N.X_GE] + cs("ts")


def test_in_lists():
    assert comp("d IN (d2, DATE '1970-01-02', NULL)") == ([N.X_IN, 3] + c("d") + c("d2") +
                                                         [N.X_DATE, 1, N.X_NULL])
    assert comp("d IN ('2000-02-29', NULL)") == [N.X_IN, 2] + cs("d") + lit("2000-02-29") + [N.X_NULL]
    assert comp("ts NOT IN ('x')") == [N.X_NOT, N.X_IN, 1] + cs("ts") + lit("x")
    assert comp("year(ts) IN (2023, 2024)") == ([N.X_IN, 2, N.X_FUNC, N.FN_YEAR, N.INT32, 1] + c("ts") +
                                                [N.X_I64, 2023, N.X_I64, 2024])


def test_date_functions():
    f = lambda which, rt, n: [N.X_FUNC, which, rt, n]  # noqa: E731
    assert comp("month(d) = 2") == [N.X_EQ] + f(N.FN_MONTH, N.INT32, 1) + c("d") + [N.X_I64, 2]
    assert comp("dayofmonth(ts) = 2")[1:5] == f(N.FN_DAYOFMONTH, N.INT32, 1)
    assert comp("datediff(ts, d) > 0") == [N.X_GT] + f(N.FN_DATEDIFF, N.INT32, 2) + c("ts") + c("d") + [N.X_I64, 0]
    assert comp("CAST(date_add(d, 7) AS STRING) > '2024-01-01'") == ([N.X_GT, N.X_CAST_STR] + f(N.FN_DATE_ADD, N.DATE32, 2) +
                                                     c("d") + [N.X_I64, 7] + lit("2024-01-01"))
    assert comp("date_sub(d, i8) = d2")[1:5] == f(N.FN_DATE_SUB, N.DATE32, 2)
    assert comp("year(d) + 1 > 2000")[:4] == [N.X_GT, N.X_ARITH, N.AR_ADD, N.INT32]
    assert comp("YEAR(to_date(ts)) = 1")[1:9] == f(N.FN_YEAR, N.INT32, 1) + f(N.FN_TO_DATE, N.DATE32, 1)


def test_cast_as_string_is_a_string_operand():
    assert comp("CAST(i32 AS STRING) IN ('1', '2')") == [N.X_IN, 2] + cs("i32") + lit("1") + lit("2")
    assert comp("CAST(f32 AS STRING) = '0.1'") == [N.X_EQ] + cs("f32") + lit("0.1")
    assert comp("CAST(dec AS STRING) <> s") == [N.X_NE] + cs("dec") + c("s")
    assert comp("CAST(b AS STRING) LIKE 't%'")[-3:] == cs("b")
    assert comp("CAST(d AS STRING) RLIKE '^2'")[-3:] == cs("d")
    assert comp("length(CAST(ts AS STRING)) = 19") == ([N.X_EQ, N.X_FUNC, N.FN_LENGTH, N.INT32, 1] + cs("ts") +
                                                       [N.X_I64, 19])
    assert comp("coalesce(CAST(i32 AS STRING), s) = 'a'")[:5] == [N.X_EQ, N.X_FUNC, N.FN_COALESCE, N.UTF8, 2]
    # against a number: the text goes through the string -> double path
    assert comp("CAST(i32 AS STRING) > 5")[:3] == [N.X_GT, N.X_CAST_F64, N.X_CAST_STR]
    assert comp("CAST(i32 AS STRING) + 1 > 5")[:6] == [N.X_GT, N.X_ARITH, N.AR_ADD, N.FLOAT64, N.X_CAST_F64,
                                                      N.X_CAST_STR]
    assert comp("cast(s as string) = 'a'") == [N.X_EQ] + cs("s") + lit("a")


def test_programs_without_the_new_forms_compile_as_before():
    """Word for word what the parent commit emitted (written out: no new op among them)."""
    assert comp("i32 >= -5") == [N.X_GE] + c("i32") + [N.X_I64, -5]
    assert comp("s LIKE 'a%'") == [N.X_LIKE, 5, int.from_bytes(bytes([1, 1, 0]) + b"a" + bytes([3]), "little")] + c("s")
    assert comp("s IS NULL OR s IN ('a', 'b')") == ([N.X_OR, N.X_IS_NULL] + c("s") + [N.X_IN, 2] + c("s") +
                                                   lit("a") + lit("b"))
    assert comp("d IS NOT NULL AND ts IS NULL") == [N.X_AND, N.X_IS_NOT_NULL] + c("d") + [N.X_IS_NULL] + c("ts")
    assert comp("abs(i8) + 1 > i64")[:4] == [N.X_GT, N.X_ARITH, N.AR_ADD, N.INT32]
    assert comp("s < 4")[:2] == [N.X_LT, N.X_CAST_F64]
    new = {N.X_CAST_STR, N.X_DATE, N.X_TIMESTAMP}
    for sql in ("i32 >= -5", "s LIKE 'a%'", "d IS NOT NULL AND ts IS NULL", "dec > 1.5", "s RLIKE 'a+'"):
        assert "text interpreter" not in _plan(sql).explain()
    assert not new & set(comp("i32 >= -5") + comp("s IS NULL OR s IN ('a', 'b')"))


# ------------------------------------------------------------------------------------------------
# Literal folding
# ------------------------------------------------------------------------------------------------
def test_date_literals_follow_date_valueof():
    assert date_literal("1970-01-01") == 0 and date_literal("1969-12-31") == -1
    assert date_literal("2000-2-29") == 11016 and date_literal("2000-02-29") == 11016
    assert date_literal("9999-12-31") == 2932896 and date_literal("1582-10-15") == -141427
    assert date_literal("2021-02-31") == date_literal("2021-03-03")      # lenient: day <= 31 rolls over
    for bad in ("2000-13-01", "2000-00-10", "2000-01-32", "2000-01-00", "200-01-01", "20000-01-01",
                "2000-001-01", "2000-01-01 ", "2000/01/01", "2000-01", "+200-01-01", "2000-+1-01", ""):
        with pytest.raises(SqlError, match="DATE"):
            date_literal(bad)


def test_timestamp_literals_follow_timestamp_valueof_in_utc():
    assert timestamp_literal("1970-01-01 00:00:00") == 0
    assert timestamp_literal("1969-12-31 23:59:59.999999") == -1
    assert timestamp_literal(" 1970-1-2 1:2:3.5 ") == DAY + (3600 + 120 + 3) * 10 ** 6 + 500000
    assert timestamp_literal("1970-01-01 00:00:00.000001") == 1
    assert timestamp_literal("1970-01-01 00:00:00.120") == 120000
    with pytest.raises(SqlError, match="more than 6 fractional digits"):
        timestamp_literal("1970-01-01 00:00:00.1234567")
    for bad in ("1970-01-01", "1970-01-01T00:00:00", "1970-01-01 24:00:00", "1970-01-01 00:60:00",
                "1970-01-01 00:00:60", "1970-13-01 00:00:00", "1970-01-01 00:00", "1970-01-01 00:00:00.",
                "70-01-01 00:00:00", "1970-01-01 00:00:00 UTC"):
        with pytest.raises(SqlError, match="TIMESTAMP"):
            timestamp_literal(bad)


def test_string_literals_against_a_timestamp_fold_only_in_the_exact_forms():
    assert timestamp_of_string("2020-01-01") == 18262 * DAY
    assert timestamp_of_string("2020-01-01 00:00:00") == 18262 * DAY
    assert timestamp_of_string("2020-01-01 23:59:59.999999") == 18263 * DAY - 1
    assert timestamp_of_string("2020-01-01 00:00:00.1") == 18262 * DAY + 100000
    assert timestamp_of_string("\u0662\u0660\u0662\u0660-01-01") is None    # ASCII digits only
    with pytest.raises(SqlError):
        date_literal("\u0662\u0660\u0662\u0660-01-01")
    for other in ("2020-1-1", "2020-01-01 ", "2020-01-01T00:00:00", "2020-01-01 00:00", "2020-02-30",
                  "2020-01-01 00:00:00.1234567", "2020-01-01 24:00:00", "2020", "abc", ""):
        assert timestamp_of_string(other) is None


# ------------------------------------------------------------------------------------------------
# Refusals
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sql,message", [
    ("ts = s", "Spark parses the string as a timestamp.*TIMESTAMP '...' literal"),
    ("s <> ts", "Spark parses the string as a timestamp"),
    ("ts <=> CAST(i32 AS STRING)", "Spark parses the string as a timestamp"),
    ("ts = '2020-1-1'", "Spark parses the string as a timestamp"),
    ("ts = '2020-01-01 00:00'", "Spark parses the string as a timestamp"),
    ("d = 5", "cannot compare a date value with a int one"),
    ("d < f32", "cannot compare a date value with a float one"),
    ("b = d", "cannot compare a date value with a bool one"),
    ("ts > 5", "cannot compare a ts value with a int one"),
    ("ts <=> b", "cannot compare a ts value with a bool one"),
    ("d IN (1, 2)", "IN a list that mixes other types"),
    ("d IN (ts)", "IN a list that mixes other types"),
    ("d IN ('2000-01-01', d2)", "IN a list that mixes other types"),
    ("ts IN (DATE '2000-01-01')", "IN a list that mixes other types"),
    ("i32 IN (d)", "IN over a date / timestamp / decimal value"),
    ("d + 1 > 2", "over a date operand"),
    ("to_date(ts) + 1 > 2", "over a date operand"),
    ("year(s) = 2000", r"year\(\) needs a date or timestamp argument, not a str one"),
    ("to_date('2000-01-01') = d", r"to_date\(\) needs a date or timestamp argument"),
    ("datediff(d, s) = 1", r"datediff\(\) needs a date or timestamp argument"),
    ("month(i32) = 1", r"month\(\) needs a date or timestamp argument, not a int one"),
    ("date_add(d, i64) = d", r"date_add\(\) needs an int number of days"),
    ("date_add(d, 1L) = d", r"date_add\(\) needs an int number of days"),
    ("date_sub(d, 1.5) = d", r"date_sub\(\) needs an int number of days"),
    ("date_sub(d, '1') = d", r"date_sub\(\) needs an int number of days"),
    ("date_add(d, NULL) = d", r"date_add\(\) needs an int number of days"),
    ("date_add(d) = d", r"date_add\(\) takes 2 arguments, not 1"),
    ("year(d)", "is not a predicate"),
    ("d = DATE '2000-13-01'", "no such date"),
    ("d = DATE '2000-1-1x'", "expected yyyy"),
    ("ts = TIMESTAMP '2000-01-01'", "expected yyyy"),
    ("ts = TIMESTAMP '2000-01-01 00:00:00.0000001'", "more than 6 fractional digits"),
    ("CAST(d AS INT) = 1", "CAST AS INT is not supported"),
    # the implicit casts stay refused, now with the hint
    ("i32 IN ('1', '2')", r"IN a list of strings.*CAST\(x AS STRING\)"),
    ("i32 LIKE '1%'", r"LIKE over a int operand.*CAST\(x AS STRING\)"),
    ("length(i32) > 1", r"needs a string operand.*CAST\(x AS STRING\)"),
    ("coalesce(s, 1) = 'a'", r"string and numeric arguments.*CAST\(x AS STRING\)"),
])
def test_refusals(sql, message):
    with pytest.raises(SqlError, match=message):
        comp(sql)


# ------------------------------------------------------------------------------------------------
# The plan: the text interpreter, its slots, what the C side refuses on its own
# ------------------------------------------------------------------------------------------------
def _plan(pred, where=None):
    from deequ_amd.analyzers import Compliance
    from deequ_amd.runners.engine import get_plan
    return get_plan(SCHEMA, Compliance("p", pred, where).aggregation_functions())


@pytest.mark.parametrize("pred,slots", [
    ("d2 >= d", 0), ("year(ts) = 2020", 0), ("ts = '2020-01-01'", 0), ("CAST(d AS STRING) >= '2000-01-01'", 1), ("ts >= '2020-01-01'", 1),
    ("CAST(i32 AS STRING) IN ('1', '2')", 1), ("d < ts", 2),
    ("CAST(CAST(i32 AS STRING) AS STRING) = 'x'", 1),
    # two alive at a time, four in all: the slots are used again
    ("CAST(d AS STRING) < CAST(ts AS STRING) AND CAST(i32 AS STRING) <> CAST(i64 AS STRING)", 2),
    ("coalesce(CAST(d AS STRING), CAST(d2 AS STRING)) = 'x'", 2),
    # a cast of a string returns its operand: the slots under it stay alive through it
    ("CAST(coalesce(CAST(d AS STRING), CAST(d2 AS STRING)) AS STRING) = 'x'", 2),
    ("CAST(CAST(d AS STRING) AS STRING) < CAST(CAST(ts AS STRING) AS STRING)", 2),
    ("CAST(coalesce(CAST(d AS STRING), s) AS STRING) < CAST(ts AS STRING)", 2),
    ("CAST(length(coalesce(CAST(d AS STRING), CAST(d2 AS STRING))) AS STRING) < CAST(ts AS STRING)", 2),
    ("length(CAST(d AS STRING)) > length(CAST(ts AS STRING)) + length(CAST(i32 AS STRING))", 1),
])
def test_text_slot_assignment(pred, slots):
    explain = _plan(pred).explain()
    assert f"text interpreter: {slots} text slots" in explain.splitlines()[0], explain
    tasks = [ln for ln in explain.splitlines() if ln.startswith("task[")]
    assert len(tasks) == 1 and " boolmap " in tasks[0] and "(expr bitmap)" in tasks[0], explain


def test_a_program_that_needs_more_slots_is_refused():
    with pytest.raises(Exception, match="3 values cast to string at once; the interpreter has 2 text slots"):
        _plan("coalesce(CAST(d AS STRING), CAST(d2 AS STRING)) = CAST(ts AS STRING)")
    with pytest.raises(Exception, match="text slots"):
        _plan("coalesce(CAST(d AS STRING), CAST(d2 AS STRING), CAST(ts AS STRING)) = 'x'")
    # the outer cast frees neither slot of the coalesce (its result may sit in the second one), so
    # the right-hand cast would need a third
    with pytest.raises(Exception, match="3 values cast to string at once"):
        _plan("CAST(coalesce(CAST(d AS STRING), CAST(d2 AS STRING)) AS STRING) < CAST(ts AS STRING)")


def _raw_plan(words):
    arr = (ctypes.c_int64 * len(words))(*words)
    types = (ctypes.c_int32 * 4)(N.UTF8, N.INT32, N.DATE32, N.TIMESTAMP_US)
    expr = N.dq_expr(ctypes.cast(arr, ctypes.POINTER(ctypes.c_int64)), len(words), 0)
    agg = N.dq_agg(N.AGG_COUNT_TRUE, -1, -1, 0, -1, 0)
    desc = N.dq_plan_desc()
    desc.n_columns, desc.column_types = 4, ctypes.cast(types, ctypes.POINTER(ctypes.c_int32))
    desc.n_exprs, desc.exprs = 1, ctypes.pointer(expr)
    desc.n_aggs, desc.aggs = 1, ctypes.pointer(agg)
    plan = ctypes.c_void_p()
    st = N.lib.dq_plan_create(ctypes.byref(desc), ctypes.byref(plan))
    if st == N.DQ_OK:
        N.lib.dq_plan_destroy(plan)
    return st


def test_plan_validates_the_new_words():
    s, i, d, ts = ([N.X_COL, k] for k in range(4))
    day, ok, inv, uns = [N.X_DATE, 3], N.DQ_OK, N.ERR_INVALID_ARGUMENT, N.ERR_UNSUPPORTED
    assert _raw_plan([N.X_EQ] + d + day) == ok
    assert _raw_plan([N.X_EQ] + ts + [N.X_TIMESTAMP, -1]) == ok
    assert _raw_plan([N.X_EQ, N.X_CAST_STR] + d + s) == ok
    assert _raw_plan([N.X_EQ] + d + [N.X_DATE, 2 ** 31]) == inv            # no int32 day count
    assert _raw_plan([N.X_EQ] + d + [N.X_DATE]) == inv                     # cut short
    assert _raw_plan([N.X_EQ, N.X_CAST_STR]) == inv
    assert _raw_plan([N.X_EQ, 30] + d + d) == inv                          # unknown op
    # a date / timestamp value against another type reaches no kernel
    assert _raw_plan([N.X_EQ] + d + ts) == uns
    assert _raw_plan([N.X_EQ] + d + s) == uns
    assert _raw_plan([N.X_LT] + i + day) == uns
    assert _raw_plan([N.X_IN, 2] + d + day + s) == uns
    assert _raw_plan([N.X_IN, 1] + i + day) == uns
    assert _raw_plan([N.X_GT, N.X_ARITH, N.AR_ADD, N.INT32] + d + i + [N.X_I64, 0]) == uns
    assert _raw_plan([N.X_IN, 2] + d + day + [N.X_NULL]) == ok
    gt0 = lambda x: [N.X_GT] + x + [N.X_I64, 0]  # noqa: E731
    assert _raw_plan(gt0([N.X_FUNC, N.FN_YEAR, N.INT32, 1] + ts)) == ok
    assert _raw_plan(gt0([N.X_FUNC, N.FN_YEAR, N.INT64, 1] + ts)) == inv
    assert _raw_plan(gt0([N.X_FUNC, N.FN_YEAR, N.INT32, 2] + ts + ts)) == inv
    assert _raw_plan(gt0([N.X_FUNC, N.FN_DATEDIFF, N.INT32, 1] + d)) == inv
    assert _raw_plan(gt0([N.X_FUNC, 23, N.INT32, 1] + d)) == inv           # past the last function
    assert _raw_plan(gt0([N.X_FUNC, 9, N.INT32, 1] + d)) == inv            # between the two groups
    assert _raw_plan(gt0([N.X_FUNC, N.FN_YEAR, N.INT32, 1] + s)) == uns    # no date argument
    assert _raw_plan(gt0([N.X_FUNC, N.FN_DATEDIFF, N.INT32, 2] + d + i)) == uns
    assert _raw_plan([N.X_EQ, N.X_FUNC, N.FN_DATE_ADD, N.DATE32, 2] + d + i + d) == ok
    assert _raw_plan([N.X_EQ, N.X_FUNC, N.FN_DATE_ADD, N.DATE32, 2] + d + s + d) == uns
    three = [N.X_EQ, N.X_FUNC, N.FN_COALESCE, N.UTF8, 2, N.X_CAST_STR] + d + [N.X_CAST_STR] + d + [N.X_CAST_STR] + ts
    assert _raw_plan(three) == uns and b"text slots" in N.lib.dq_last_error()
