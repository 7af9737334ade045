"""Host-side compiler of LIKE, arithmetic and the scalar functions: precedence, Spark 2.2 result
types, the emitted words, the refusals, and the plan's choice of the interpreter."""
import struct

import pytest

from deequ_amd import _native as N
from deequ_amd.sqlexpr import (LIKE_ANY1, LIKE_ANYSEQ, LIKE_LIT, SqlError, _Emitter, compile_expr,
                               like_program, parse)
from deequ_amd.table import StructField, StructType

SCHEMA = StructType([StructField("s", N.UTF8), StructField("i8", N.INT8), StructField("i16", N.INT16),
                     StructField("i32", N.INT32), StructField("i64", N.INT64),
                     StructField("f32", N.FLOAT32), StructField("f64", N.FLOAT64),
                     StructField("b", N.BOOL), StructField("dec", N.decimal_type(10, 2)),
                     StructField("d", N.DATE32)])
COL = {f.name: k for k, f in enumerate(SCHEMA.fields)}


def comp(sql):
    return compile_expr(sql, SCHEMA, lambda n: SCHEMA.index(n)).words


def rtype(sql):
    """The result type of the left operand of the comparison `sql`."""
    return _Emitter(SCHEMA, SCHEMA.index).result_type(parse(sql).kids[0])


def shape(n):
    if n.op in ("arith", "cmp"):
        return f"({shape(n.kids[0])} {n.name} {shape(n.kids[1])})"
    if n.op == "neg":
        return f"(-{shape(n.kids[0])})"
    if n.op == "func":
        return f"{n.name}({', '.join(shape(k) for k in n.kids)})"
    return str(n.name if n.op == "col" else n.value)


@pytest.mark.parametrize("sql,tree", [
    ("a + b * 2 > c", "((a + (b * 2)) > c)"),
    ("-a + 1 > 0", "(((-a) + 1) > 0)"),
    ("a - b - c = 0", "(((a - b) - c) = 0)"),
    ("a / b % c * d < 1", "((((a / b) % c) * d) < 1)"),
    ("a * (b + c) <> -1", "((a * (b + c)) <> -1)"),
    ("- - a = +b", "((-(-a)) = b)"),
    ("a - -1 > abs(b - c) * 2", "((a - -1) > (abs((b - c)) * 2))"),
])
def test_precedence(sql, tree):
    assert shape(parse(sql)) == tree


def test_arithmetic_binds_tighter_than_comparison_in_between_and_in():
    n = parse("x BETWEEN lo - 1 AND hi + 1")
    assert n.op == "and" and shape(n.kids[0]) == "(x >= (lo - 1))" and shape(n.kids[1]) == "(x <= (hi + 1))"
    n = parse("abs(a - b) IN (0, 1 + 1)")
    assert n.op == "in" and shape(n.kids[0]) == "abs((a - b))" and shape(n.kids[2]) == "(1 + 1)"
    n = parse("NOT a + 1 > 2 AND b LIKE 'x%' OR c")
    assert n.op == "or" and n.kids[0].op == "and" and n.kids[0].kids[0].op == "not"
    assert n.kids[0].kids[1].op == "like"


@pytest.mark.parametrize("sql,t", [
    ("i8 + 1 > 0", N.INT32), ("i8 + i8 > 0", N.INT8), ("i8 * i16 > 0", N.INT16), ("i16 - 1Y > 0", N.INT16),
    ("i32 + 2147483648 > 0", N.INT64), ("i32 + -2147483648 > 0", N.INT32), ("i8 + 1L > 0", N.INT64),
    ("i64 + f32 > 0", N.FLOAT32), ("f32 * 2 > 0", N.FLOAT32), ("f32 + f64 > 0", N.FLOAT64),
    ("f32 + 0.5 > 0", N.FLOAT64), ("f32 + 0.5D > 0", N.FLOAT64), ("i8 / i8 > 0", N.FLOAT64),
    ("f32 / f32 > 0", N.FLOAT64), ("i64 / 2 > 0", N.FLOAT64), ("i64 % 2 > 0", N.INT64),
    ("s + 1 > 0", N.FLOAT64), ("-i8 > 0", N.INT8), ("-s > 0", N.FLOAT64), ("abs(i16) > 0", N.INT16),
    ("abs(i8 - i32) > 0", N.INT32), ("length(s) > 0", N.INT32), ("coalesce(i8, i64, f32) > 0", N.FLOAT32),
    ("coalesce(i8, 1) > 0", N.INT32), ("coalesce(s, 'x') > 'a'", N.UTF8), ("i8 + NULL > 0", N.INT8),
    ("CAST(i8 AS FLOAT) + 1 > 0", N.FLOAT32), ("abs(i8 + 1) * i64 > 0", N.INT64),
])
def test_result_types(sql, t):
    assert rtype(sql) == t


def _bits(x):
    return struct.unpack("<q", struct.pack("<d", x))[0]


def _packed(b):
    b = b + b"\0" * (-len(b) % 8)
    return list(struct.unpack(f"<{len(b) // 8}q", b))


def test_emitted_words_of_each_new_operator():
    assert comp("i8 + 1 > 2") == [N.X_GT, N.X_ARITH, N.AR_ADD, N.INT32, N.X_COL, COL["i8"], N.X_I64, 1,
                                  N.X_I64, 2]
    assert comp("-i64 < 0") == [N.X_LT, N.X_ARITH, N.AR_NEG, N.INT64, N.X_COL, COL["i64"], N.X_I64, 0]
    assert comp("i64 / 2 > 1")[:4] == [N.X_GT, N.X_ARITH, N.AR_DIV, N.FLOAT64]
    assert comp("i32 % 3 = 1")[:4] == [N.X_EQ, N.X_ARITH, N.AR_MOD, N.INT32]
    # a string operand goes through the existing CAST AS DOUBLE; a decimal literal beside a float
    # operand is its double
    assert comp("s + 1 > 2") == [N.X_GT, N.X_ARITH, N.AR_ADD, N.FLOAT64, N.X_CAST_F64, N.X_COL, COL["s"],
                                 N.X_I64, 1, N.X_F64, _bits(2.0)]
    assert comp("f32 * 1.5 > 2") == [N.X_GT, N.X_ARITH, N.AR_MUL, N.FLOAT64, N.X_COL, COL["f32"],
                                     N.X_F64, _bits(1.5), N.X_F64, _bits(2.0)]
    assert comp("abs(i8) = 3") == [N.X_EQ, N.X_FUNC, N.FN_ABS, N.INT8, 1, N.X_COL, COL["i8"], N.X_I64, 3]
    assert comp("length(s) > 2") == [N.X_GT, N.X_FUNC, N.FN_LENGTH, N.INT32, 1, N.X_COL, COL["s"],
                                     N.X_I64, 2]
    assert comp("coalesce(i8, 3) = 3") == [N.X_EQ, N.X_FUNC, N.FN_COALESCE, N.INT32, 2, N.X_COL, COL["i8"],
                                           N.X_I64, 3, N.X_I64, 3]
    assert comp("isnan(f32)") == [N.X_FUNC, N.FN_ISNAN, N.BOOL, 1, N.X_COL, COL["f32"]]
    assert comp("isnull(s)") == [N.X_IS_NULL, N.X_COL, COL["s"]]
    assert comp("ISNOTNULL(i8 + 1)")[:2] == [N.X_IS_NOT_NULL, N.X_ARITH]
    prog = bytes([LIKE_LIT, 1, 0]) + b"a" + bytes([LIKE_ANYSEQ])
    assert comp("s LIKE 'a%'") == [N.X_LIKE, len(prog)] + _packed(prog) + [N.X_COL, COL["s"]]
    assert comp("s NOT LIKE 'a%'") == [N.X_NOT] + comp("s LIKE 'a%'")
    assert comp("s like ''") == [N.X_LIKE, 0, N.X_COL, COL["s"]]


def test_like_pattern_programs():
    lit = lambda b: bytes([LIKE_LIT, len(b) & 255, len(b) >> 8]) + b  # noqa: E731
    any1, anyseq = bytes([LIKE_ANY1]), bytes([LIKE_ANYSEQ])
    assert like_program("%%a%%%_b%") == anyseq + lit(b"a") + anyseq + any1 + lit(b"b") + anyseq
    assert like_program("a\\%b\\_c\\\\") == lit(b"a%b_c\\")
    assert like_program("ñ_") == lit("ñ".encode()) + any1
    assert like_program("x" * 300) == lit(b"x" * 300)
    # unescapeSQLString leaves \% and \_ for the LIKE reader and resolves every other escape
    assert parse(r"s LIKE 'a\%b\_c\\\\d\n'").value == lit(b"a%b_c\\d\n")
    assert parse(r"s = 'a\%b'").kids[1].value == "a%b"          # outside LIKE: as before


@pytest.mark.parametrize("sql,message", [
    ("i32 LIKE '1%'", "LIKE over a int operand"),
    ("b LIKE 't%'", "LIKE over a bool operand"),
    ("s LIKE s", "LIKE needs a string literal pattern"),
    (r"s LIKE 'a\\x'", "the escape character is not allowed to precede 'x'"),
    (r"s LIKE 'abc\\'", "not allowed to end with the escape character"),
    ("i32 * 1.5 > 2", "Spark does decimal arithmetic"),
    ("i64 + 0.5 > 2", "Spark does decimal arithmetic"),
    ("dec + 1 > 2", "Spark does decimal arithmetic"),
    ("1.5 / 0.5 > 2", "Spark does decimal arithmetic"),
    ("d + 1 > 2", "over a date operand"),
    ("b + 1 > 2", "over a bool operand"),
    ("upper(s) = 'A'", r"function upper\(\) is not supported"),
    ("substring(s, 1, 2) = 'A'", r"function substring\(\) is not supported"),
    ("coalesce(s, 1) = 'a'", "string and numeric arguments"),
    ("coalesce(i8) = 1", r"coalesce\(\) takes 2 arguments to 8, not 1"),
    ("coalesce(1, 2, 3, 4, 5, 6, 7, 8, 9) = 1", "not 9"),
    ("length(i32) > 1", "needs a string operand"),
    ("isnan(i32)", "needs a float or double operand"),
    ("abs(i8, 1) > 1", r"abs\(\) takes 1 argument, not 2"),
    ("i8 + 1", "is not a predicate"),
    ("NOT (i8 + 1)", "NOT needs a boolean operand"),
    ("CAST(s AS FLOAT) + 1 > 0", r"CAST\(string AS FLOAT\)"),
])
def test_refusals(sql, message):
    with pytest.raises(SqlError, match=message):
        comp(sql)


def test_word_lists_of_the_check_forms_are_unchanged():
    """What tests/test_sqlexpr.py asserts, restated on this schema: the new precedence levels and
    the constant folding of a signed literal leave every earlier form's words as they were."""
    assert comp("i32 >= 0") == [N.X_GE, N.X_COL, COL["i32"], N.X_I64, 0]
    assert comp("i32 >= -5") == [N.X_GE, N.X_COL, COL["i32"], N.X_I64, -5]
    assert comp("f64 > -(2.5)") == [N.X_GT, N.X_COL, COL["f64"], N.X_F64, _bits(-2.5)]
    w = comp("s IS NULL OR s IN ('a''b','c')")
    assert w[0] == N.X_OR and w[1] == N.X_IS_NULL and w[4] == N.X_IN and w[5] == 2
    assert N.X_F64 in comp("f64 IS NULL OR (f64 >= 1.0 AND f64 <= 3.5E2)")
    w = comp("s < 4")
    assert w[:2] == [N.X_LT, N.X_CAST_F64] and w[-2] == N.X_F64
    assert comp("I32 > 3") == comp("i32 > 3")
    assert comp("i32 BETWEEN 1 AND 3")[0] == N.X_AND and comp("s NOT IN ('x')")[0] == N.X_NOT
    assert comp("CAST(f64 AS FLOAT) > 1.5")[:2] == [N.X_GT, N.X_CAST_F32]
    assert comp("CAST(i32 AS DOUBLE) > 1.5")[:2] == [N.X_GT, N.X_CAST_F64]
    n = parse("a > 1 AND NOT b IS NULL OR c = 'x'")
    assert n.op == "or" and n.kids[0].op == "and"


# ------------------------------------------------------------------------------------------------
# The plan: always the interpreter, the stack depth counted, malformed words refused
# ------------------------------------------------------------------------------------------------
def _plan(pred, where=None):
    from deequ_amd.analyzers import Compliance
    from deequ_amd.runners.engine import get_plan
    return get_plan(SCHEMA, Compliance("p", pred, where).aggregation_functions())


@pytest.mark.parametrize("pred", ["i32 + 0 > 3", "i32 IS NULL OR (i32 + 0 >= 1 AND i32 <= 5)", "s LIKE 'a'",
                                  "s IS NULL OR NOT s LIKE 'a'", "abs(i32) > 1", "coalesce(s, 'a') IN ('a', 'b')",
                                  "s IS NULL OR coalesce(s, 'a') = 'a'"])
def test_new_operators_are_never_fused(pred):
    explain = _plan(pred).explain()
    tasks = [ln for ln in explain.splitlines() if ln.startswith("task[")]
    assert len(tasks) == 1 and " boolmap " in tasks[0] and "(expr bitmap)" in tasks[0], explain


def test_stack_depth_counts_the_new_operators_operands():
    deep = "i8" + "".join(f" + (i8 * {k}" for k in range(16)) + ")" * 16 + " > 0"
    with pytest.raises(Exception, match="nests deeper"):
        _plan(deep)
    with pytest.raises(Exception, match="nests deeper"):
        # the value, eight items, then the eight arguments on top of them: 17 slots
        _plan("i8 IN (1, 2, 3, 4, 5, 6, 7, 8, coalesce(i8, i8, i8, i8, i8, i8, i8, i8))")
    assert _plan("i8 IN (1, 2, 3, 4, 5, 6, 7, coalesce(i8, i8, i8, i8, i8, i8, i8, i8))").explain()


def _raw_plan(words):
    import ctypes
    arr = (ctypes.c_int64 * len(words))(*words)
    types = (ctypes.c_int32 * 2)(N.UTF8, N.INT32)
    expr = N.dq_expr(ctypes.cast(arr, ctypes.POINTER(ctypes.c_int64)), len(words), 0)
    agg = N.dq_agg(N.AGG_COUNT_TRUE, -1, -1, 0, -1, 0)
    desc = N.dq_plan_desc()
    desc.n_columns, desc.column_types = 2, ctypes.cast(types, ctypes.POINTER(ctypes.c_int32))
    desc.n_exprs, desc.exprs = 1, ctypes.pointer(expr)
    desc.n_aggs, desc.aggs = 1, ctypes.pointer(agg)
    plan = ctypes.c_void_p()
    st = N.lib.dq_plan_create(ctypes.byref(desc), ctypes.byref(plan))
    if st == N.DQ_OK:
        N.lib.dq_plan_destroy(plan)
    return st


def _like_words(prog):
    return [N.X_LIKE, len(prog)] + _packed(prog) + [N.X_COL, 0]


def test_plan_validates_the_new_operators_words():
    ok = bytes([LIKE_ANYSEQ, LIKE_LIT, 2, 0]) + b"ab" + bytes([LIKE_ANY1])
    assert _raw_plan(_like_words(ok)) == N.DQ_OK
    for bad in (bytes([7]),                                    # unknown token kind
                bytes([LIKE_LIT, 3, 0]) + b"ab",               # literal runs past the program
                bytes([LIKE_LIT, 0, 0]),                       # empty literal
                bytes([LIKE_LIT, 1]),                          # truncated length
                bytes([LIKE_ANYSEQ, LIKE_ANYSEQ]),             # not collapsed
                bytes([LIKE_ANY1]) * 4097):                    # above the size cap
        assert _raw_plan(_like_words(bad)) == N.ERR_INVALID_ARGUMENT, bad[:8]
    assert _raw_plan([N.X_LIKE, 64, 0, N.X_COL, 0]) == N.ERR_INVALID_ARGUMENT   # payload cut short
    gt0 = lambda x: [N.X_GT] + x + [N.X_I64, 0]  # noqa: E731
    col = [N.X_COL, 1]
    assert _raw_plan(gt0([N.X_ARITH, N.AR_ADD, N.INT32] + col + col)) == N.DQ_OK
    assert _raw_plan(gt0([N.X_ARITH, 7, N.INT32] + col + col)) == N.ERR_INVALID_ARGUMENT
    assert _raw_plan(gt0([N.X_ARITH, N.AR_ADD, N.UTF8] + col + col)) == N.ERR_INVALID_ARGUMENT
    assert _raw_plan(gt0([N.X_ARITH, N.AR_DIV, N.INT32] + col + col)) == N.ERR_INVALID_ARGUMENT
    assert _raw_plan(gt0([N.X_ARITH, N.AR_NEG, N.INT32] + col)) == N.DQ_OK
    assert _raw_plan(gt0([N.X_FUNC, N.FN_ABS, N.INT32, 1] + col)) == N.DQ_OK
    assert _raw_plan(gt0([N.X_FUNC, 9, N.INT32, 1] + col)) == N.ERR_INVALID_ARGUMENT
    assert _raw_plan(gt0([N.X_FUNC, N.FN_ABS, N.BOOL, 1] + col)) == N.ERR_INVALID_ARGUMENT
    assert _raw_plan(gt0([N.X_FUNC, N.FN_COALESCE, N.INT32, 9] + col * 9)) == N.ERR_INVALID_ARGUMENT
    assert _raw_plan(gt0([N.X_FUNC, N.FN_COALESCE, N.INT32, 1] + col)) == N.ERR_INVALID_ARGUMENT
