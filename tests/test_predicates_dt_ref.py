"""Guards the reference evaluator of tests/predicate_dt_cases.py with hand-derived known answers
(Spark 2.2's PromoteStrings rules and DateTimeUtils worked out on paper), and the matrix against
vacuous cases."""
import datetime

import numpy as np
import pytest

import predicate_dt_cases as T
from predicate_dt_cases import (DATE_ADD, DATE_SUB, DATEDIFF, DAYOFMONTH, DT, EPOCH, GT, IND, MONTH, NSEQ,
                                S, TO_DATE, US, YEAR, C, Date, G, L)


def col(name, values, f):
    return [f({name: v}) for v in values]


def test_a_date_against_a_string_compares_as_text():
    d = C("d")
    # Spark casts the DATE to string: '2020-1-1' is not the text of 2020-01-01
    assert col("d", [Date(2020, 1, 1), None], G("=", S(d), L("2020-1-1"))) == [False, None]
    assert col("d", [Date(2020, 1, 1), Date(2020, 1, 2)], G("=", S(d), L("2020-01-01"))) == [True, False]
    # byte order: '9999-12-31' > '2' > '1582-10-15'
    assert col("d", [Date(9999, 12, 31), Date(1582, 10, 15)], G(">", S(d), L("2"))) == [True, False]


def test_a_timestamp_against_a_string():
    ts = C("ts")
    midnight = DT(2020, 1, 1)
    # relational: the timestamp as text; the longer string sorts higher
    assert G(">=", S(ts), L("2020-01-01"))({"ts": midnight}) is True
    assert G("<=", S(ts), L("2020-01-01"))({"ts": midnight}) is False
    assert G(">=", S(ts), L("2020-01-01"))({"ts": midnight - US}) is False
    # equality: the string as a timestamp
    assert GT("=", ts, L(midnight))({"ts": midnight}) is True
    assert NSEQ(ts, L(midnight))({"ts": None}) is False


def test_timestamp_text():
    text = lambda t: S(C("ts"))({"ts": t})  # noqa: E731
    assert text(EPOCH) == "1970-01-01 00:00:00"
    assert text(EPOCH - US) == "1969-12-31 23:59:59.999999"
    assert text(DT(1970, 1, 1, 0, 0, 0, 100000)) == "1970-01-01 00:00:00.1"
    assert text(EPOCH + US) == "1970-01-01 00:00:00.000001"
    assert text(DT(2024, 2, 29, 1, 2, 3, 120000)) == "2024-02-29 01:02:03.12"
    assert S(C("d"))({"d": Date(1582, 10, 15)}) == "1582-10-15"


def test_number_and_boolean_text():
    assert S(C("i32"))({"i32": -5}) == "-5" and S(C("b"))({"b": True}) == "true"
    assert S(C("f64"))({"f64": 1e21}) == "1.0E21" and S(C("f64"))({"f64": 2.5}) == "2.5"
    assert S(C("f32"))({"f32": 0.1}) == "0.1"                      # Float.toString of 0.1f
    assert S(C("f64"))({"f64": float(np.float32(0.1))}) == "0.10000000149011612"
    assert S(C("s"))({"s": "x"}) == "x" and S(C("s"))({"s": None}) is None


def test_date_fields_of_the_boundary_dates():
    fields = lambda v: (YEAR(C("d"))({"d": v}), MONTH(C("d"))({"d": v}), DAYOFMONTH(C("d"))({"d": v}))  # noqa: E731
    assert fields(Date(1582, 10, 15)) == (1582, 10, 15)
    assert fields(Date(1969, 12, 31)) == (1969, 12, 31)
    assert fields(Date(1970, 1, 1)) == (1970, 1, 1)
    assert fields(Date(2000, 2, 29)) == (2000, 2, 29)
    assert fields(Date(2100, 3, 1)) == (2100, 3, 1)
    assert fields(Date(9999, 12, 31)) == (9999, 12, 31)
    assert fields(None) == (None, None, None)
    assert type(YEAR(C("d"))({"d": Date(2000, 1, 1)})) is np.int32


def test_a_timestamp_is_cast_to_date_by_floor_division():
    ts = C("ts")
    assert TO_DATE(ts)({"ts": EPOCH - US}) == Date(1969, 12, 31)          # -1 microsecond
    assert TO_DATE(ts)({"ts": EPOCH}) == Date(1970, 1, 1)
    assert TO_DATE(ts)({"ts": EPOCH - 86_400_000_001 * US}) == Date(1969, 12, 30)
    assert TO_DATE(ts)({"ts": DT(2020, 1, 1, 23, 59, 59, 999999)}) == Date(2020, 1, 1)
    assert YEAR(ts)({"ts": EPOCH - US}) == 1969 and DAYOFMONTH(ts)({"ts": EPOCH - US}) == 31


def test_date_arithmetic():
    r = {"d": Date(2000, 2, 28), "d2": Date(2000, 3, 1), "ts": DT(2000, 3, 1, 12, 0, 0), "i8": -2}
    assert DATEDIFF(C("d2"), C("d"))(r) == 2 and DATEDIFF(C("d"), C("d2"))(r) == -2
    assert DATEDIFF(C("ts"), C("d"))(r) == 2
    assert DATE_ADD(C("d"), L(1))(r) == Date(2000, 2, 29) and DATE_SUB(C("d2"), L(1))(r) == Date(2000, 2, 29)
    assert DATE_SUB(C("d"), C("i8"))(r) == Date(2000, 3, 1)
    assert DATE_ADD(C("d"), L(None))(r) is None and DATEDIFF(C("d"), L(None))(r) is None
    far = DATE_ADD(C("d"), L(1))({"d": Date(9999, 12, 31)})
    assert isinstance(far, T.FarDate) and GT(">", lambda r: far, C("d"))({"d": Date(9999, 12, 31)}) is True


def test_in_and_null_safe_equality():
    d = C("d")
    assert IND(d, L(Date(2000, 1, 1)), L(None))({"d": Date(2000, 1, 2)}) is None
    assert IND(d, L(Date(2000, 1, 1)), L(None))({"d": Date(2000, 1, 1)}) is True
    assert NSEQ(d, L(None))({"d": None}) is True and NSEQ(d, L(None))({"d": Date(2000, 1, 1)}) is False
    with pytest.raises(AssertionError):
        GT("=", d, C("ts"))({"d": Date(2000, 1, 1), "ts": DT(2000, 1, 1)})   # never natively


# <=> is never NULL, `x IS NULL OR ...` neither; the others below are FALSE- or TRUE-free by what
# their operands can be (a date's text has 10 bytes, a timestamp's at least 19; an all-NULL column)
def test_the_cases_with_an_empty_row_set_are_the_stated_few():
    partial = [c.pred for c in T.CASES if c.empty]
    assert len(partial) <= 32 and len(T.CASES) >= 170
    for c in T.CASES:
        if c.empty:
            assert ("<=>" in c.pred or "IS NULL" in c.pred or "dn" in c.pred or "NULL" in c.pred
                    or c.pred in ("CAST(d AS STRING) = '2020-1-1'", "CAST(d AS STRING) < ''", "d = ts",
                                  "length(CAST(d AS STRING)) = 10",
                                  "date_add(date_sub(d, 3), 3) = d", "d IN (d2, DATE '1582-10-15', NULL)",
                                  "coalesce(CAST(ts AS STRING), 'none') LIKE '1969%'",
                                  # (a coalesce that ends in a literal is never NULL)
                                  "coalesce(CAST(b AS STRING), 'true') = 'true'",
                                  "coalesce(CAST(f32 AS STRING), 'none') LIKE 'n%'")), c.pred


@pytest.mark.parametrize("c", T.CASES, ids=[c.pred[:60] for c in T.CASES])
def test_matrix_row_sets_are_non_trivial(c):
    """TRUE, FALSE and NULL rows all occur on the matrix table, except the sets the predicate's
    semantics leave empty (Case.empty) -- those must be empty."""
    tv = T.truth(c)
    for key, v in (("T", True), ("F", False), ("N", None)):
        n = sum(1 for x in tv if x is v)
        assert (n == 0) == (key in c.empty), (c.pred, key, n)


def test_table_holds_what_it_must():
    arrow, rows = T.table()
    assert len(rows) == T.PC.N_MATRIX
    dates = {r["d"] for r in rows}
    for v in (Date(1582, 10, 15), Date(1969, 12, 31), Date(1970, 1, 1), Date(2000, 2, 29), Date(2100, 3, 1),
              Date(9999, 12, 31), None):
        assert v in dates
    stamps = {r["ts"] for r in rows}
    for v in (EPOCH - US, EPOCH, DT(2020, 1, 1, 0, 0, 1), DT(1970, 1, 1, 0, 0, 0, 100000), EPOCH + US,
              DT(1969, 12, 31, 23, 59, 59, 999999), DT(2020, 1, 1), None):
        assert v in stamps
    assert all(r["dn"] is None for r in rows)
    for name in ("d", "d2"):
        assert all(r[name] is None or T.D_LO <= r[name] <= T.D_HI for r in rows)
    for name in ("ts", "ts2"):
        assert all(r[name] is None or r[name] >= DT(1582, 10, 15) for r in rows)
    both = [(r["d"], r["d2"]) for r in rows if r["d"] and r["d2"]]
    assert any(a < b for a, b in both) and any(a > b for a, b in both) and any(a == b for a, b in both)
    assert isinstance(rows[0]["ts"] or EPOCH, datetime.datetime)
