"""Guards the reference evaluator of tests/predicate_ext_cases.py with hand-derived known answers
(Java / Spark 2.2 semantics worked out on paper, on rows of at most eight values), and the matrix
against vacuous cases."""
import numpy as np
import pytest

import predicate_ext_cases as X
from predicate_ext_cases import A, ABS, AND, C, COALESCE, D, G, IN, ISNAN, L, LEN, LIKE, NEG, NOT, OR


def col(name, values, f):
    return [f({name: v}) for v in values]


def test_int_addition_wraps_at_the_result_width():
    assert col("i32", [2147483647, -1, None], A("+", C("i32"), L(1))) == [-2147483648, 0, None]
    r = {"i8": 127}
    byte = A("+", C("i8"), lambda r: np.int8(1))(r)
    assert byte == -128 and type(byte) is np.int8                      # Byte + Byte
    widened = A("+", C("i8"), L(1))(r)
    assert widened == 128 and type(widened) is np.int32                # Byte + Int literal
    assert A("*", C("i64"), L(2))({"i64": 2 ** 62}) == -2 ** 63
    assert type(A("+", C("i64"), C("f32"))({"i64": 1, "f32": 0.5})) is np.float32
    assert A("+", C("i64"), C("f32"))({"i64": 16777217, "f32": 0.0}) == 16777216.0   # computed in float


def test_remainder_takes_the_sign_of_the_dividend():
    assert A("%", L(7), L(-3))({}) == 1 and A("%", L(-7), L(3))({}) == -1
    assert A("%", C("i64"), L(-1))({"i64": -2 ** 63}) == 0
    assert A("%", C("f64"), L(2))({"f64": -2.5}) == -0.5
    assert A("%", C("f32"), L(3))({"f32": 7.5}) == 1.5


def test_zero_divisors_give_null():
    x = C("i32")
    assert col("i32", [5, 0, None], A("/", x, L(0))) == [None, None, None]
    assert col("i32", [5, 0, None], A("%", x, L(0))) == [None, None, None]
    assert A("/", L(1.5), L(-0.0))({}) is None and A("/", L(1.5), L(0.0))({}) is None
    assert A("%", L(1.5), L(-0.0))({}) is None
    assert A("/", L(7), L(2))({}) == 3.5                               # always a double division
    assert G(">", A("/", x, L(0)), L(1))({"i32": 5}) is None


def test_abs_and_negation_wrap_at_the_minimum():
    assert col("i8", [-128, -127, 5, None], ABS(C("i8"))) == [-128, 127, 5, None]
    assert col("i8", [-128, 1], NEG(C("i8"))) == [-128, -1]
    assert ABS(C("i64"))({"i64": -2 ** 63}) == -2 ** 63
    assert ABS(C("f64"))({"f64": -0.5}) == 0.5


def test_length_counts_code_points():
    assert col("s", ["añ😀", "", "abc", None], LEN(C("s"))) == [3, 0, 3, None]


def test_like():
    s = C("s")
    assert col("s", ["a_c", "abc"], LIKE(s, "a\\_c")) == [True, False]
    assert col("s", ["a\nb", "ab", "a😀b", None], LIKE(s, "a_b")) == [True, False, True, None]
    assert col("s", ["", "x", "\n\n"], LIKE(s, "%")) == [True, True, True]
    assert col("s", ["", "x", "xy"], LIKE(s, "_")) == [False, True, False]
    assert col("s", ["😀", "ñ"], LIKE(s, "_")) == [True, True]
    assert col("s", ["", "a"], LIKE(s, "")) == [True, False]
    assert col("s", ["abc", "xabcx", "ab"], LIKE(s, "%abc%")) == [True, True, False]
    assert col("s", ["a.c", "abc"], LIKE(s, "a.c")) == [True, False]
    assert col("s", ["100%", "100x"], LIKE(s, "100\\%")) == [True, False]
    assert col("s", ["a\\b", "ab"], LIKE(s, "a\\\\b")) == [True, False]
    assert col("s", ["aaab", "aab", "ab"], LIKE(s, "%aab")) == [True, True, False]


def test_null_handling_of_the_functions():
    assert ISNAN(C("f64"))({"f64": None}) is False
    assert ISNAN(C("f64"))({"f64": float("nan")}) is True and ISNAN(C("f64"))({"f64": 1.0}) is False
    assert COALESCE(np.int32, L(None), L(3))({}) == 3
    assert COALESCE(np.int32, C("i8"), L(3))({"i8": -4}) == -4
    assert COALESCE(None, C("s"), L("z"))({"s": None}) == "z"
    assert A("+", C("i8"), L(1))({"i8": None}) is None and NEG(C("i8"))({"i8": None}) is None


def test_string_operands_are_cast_to_double():
    assert col("s", ["5", " 12 ", "abc", "1.5d", None], A("+", D(C("s")), L(1))) == [6.0, 13.0, None, 2.5, None]


def test_comparisons_and_kleene_logic():
    nan = float("nan")
    assert G(">", C("f64"), L(0))({"f64": nan}) is True and G("=", C("f64"), C("f64"))({"f64": nan}) is True
    assert IN(C("i32"), L(1), L(None))({"i32": 2}) is None and IN(C("i32"), L(1), L(None))({"i32": 1}) is True
    t, f, n = (lambda r: True), (lambda r: False), (lambda r: None)
    assert AND(f, n)({}) is False and AND(t, n)({}) is None and OR(t, n)({}) is True and OR(f, n)({}) is None
    assert NOT(n)({}) is None and NOT(t)({}) is False


@pytest.mark.parametrize("c", X.CASES, ids=[c.pred[:60] for c in X.CASES])
def test_matrix_row_sets_are_non_trivial(c):
    """TRUE, FALSE and NULL rows all occur on the matrix table, except the sets the predicate's
    semantics leave empty (Case.empty) -- those must be empty."""
    tv = X.truth(c)
    for key, v in (("T", True), ("F", False), ("N", None)):
        n = sum(1 for x in tv if x is v)
        assert (n == 0) == (key in c.empty), (c.pred, key, n)


def test_matrix_covers_what_it_must():
    preds = [c.pred for c in X.CASES]
    for col_ in X.PC.NUMERIC:
        for op in "+-*/%":
            assert f"{col_} {op} 3 > 1" in preds and f"{col_} {op} {X.PARTNER[col_]} > 1" in preds
    assert len(X.table()[1]) == X.PC.N_MATRIX
    assert any(len(v.encode()) > 64 for v in X.T_POOL) and "a" * 24 + "b" in X.T_POOL
