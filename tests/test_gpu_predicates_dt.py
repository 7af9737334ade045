"""Row-exact conformance of date / timestamp comparisons, the date functions and CAST AS STRING on
the device.

The method of tests/test_gpu_predicates_ext.py (its _check, by import): for every predicate p of
the matrix (tests/predicate_dt_cases.py) Sum("w", where=p), Sum("w", where="NOT (p)") and
Size(where=p) must give the weight fingerprints of the reference evaluator's TRUE and FALSE row sets
and its count; Compliance(p) in total and under `g = k` its counts; explain() must show the
interpreter's expression bitmaps.  The evaluator lives with the cases (datetime, integer floor
division, the oracle's Java number printers) and is pinned by tests/test_predicates_dt_ref.py.

Before this feature every case of the matrix failed at planning (SqlError / AnalysisException).
A date against a string is written with its cast, CAST(d AS STRING) >= '2000-01-01': the implicit
form stays refused (tests/test_decimal_types.py pins that), with a message that says so.
"""
import numpy as np
import pyarrow as pa
import pytest

import predicate_cases as PC
import predicate_dt_cases as T
import test_gpu_predicates as TP
from test_gpu_predicates_ext import _check

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dt_table(gpu_device):
    from deequ_amd import Table
    return Table.from_arrow(T.table()[0], device=gpu_device)


@pytest.mark.parametrize("c", T.CASES, ids=TP._ids(T.CASES))
def test_date_predicate_rows_match_reference(c, dt_table):
    assert c.path == "gen"
    _check(c, dt_table, T.table()[0], T.truth(c))


def _truth_over(c, arrow):
    tv = tuple(c.ref(r) for r in arrow.to_pylist())
    assert {True, False, None} == set(tv)
    return tv


def test_across_batches_and_bitmap_words(gpu_device):
    """40 993 rows in batches of 4096: ten batches and a 33-row tail, every batch ending inside a
    bitmap word of the next one's numbering; a string-cast comparison and a date function."""
    from deequ_amd import Table
    arrow = T.batched_arrow()
    df = Table.from_arrow(arrow, device=gpu_device, max_batch_rows=4096)
    for c in T.BATCHED:
        _check(c, df, arrow, _truth_over(c, arrow))


def test_sliced_arrow_table(gpu_device):
    """A slice that starts inside a validity byte and a bitmap word: offsets 37 .. 37 + 1500."""
    from deequ_amd import Table
    arrow = T.batched_arrow(4000, seed=37).slice(37, 1500)
    df = Table.from_arrow(arrow, device=gpu_device)
    for c in T.BATCHED + [T.case("sliced", "d <= d2", "gen", ref=T.GT("<=", T.d, T.d2))]:
        _check(c, df, arrow, _truth_over(c, arrow))


def test_dictionary_encoded_date_column(gpu_device):
    from deequ_amd import Table
    plain = T.batched_arrow(3000, seed=41)
    arrow = plain.set_column(plain.schema.get_field_index("d"), "d", plain.column("d").dictionary_encode())
    assert pa.types.is_dictionary(arrow.schema.field("d").type)
    df = Table.from_arrow(arrow, device=gpu_device)
    for c in (T.case("dictionary", "CAST(d AS STRING) >= '2000-01-01'", "gen", ref=T.G(">=", T.S(T.d), T.L("2000-01-01"))),
              T.case("dictionary", "year(d) = 2024", "gen", ref=T.G("=", T.YEAR(T.d), T.L(2024)))):
        _check(c, df, plain, _truth_over(c, plain))


# ------------------------------------------------------------------------------------------------
# Through the public API
# ------------------------------------------------------------------------------------------------
def _count(c, rows):
    return sum(1 for r in rows if c.ref(r) is True)


def test_verification_suite_over_a_date_partition(gpu_device):
    from deequ_amd import Table
    from deequ_amd.analyzers import Compliance, Size
    from deequ_amd.checks import Check, CheckLevel, CheckStatus
    from deequ_amd.verification import VerificationSuite
    arrow, rows = T.table()
    df = Table.from_arrow(arrow, device=gpu_device)
    since = T.case("api", "CAST(d AS STRING) >= '2000-01-01'", "gen", ref=T.G(">=", T.S(T.d), T.L("2000-01-01")))
    later = T.case("api", "d2 >= d", "gen", ref=T.GT(">=", T.d2, T.d))
    small = T.case("api", "CAST(i32 AS STRING) IN ('1', '2', '3')", "gen",
                   ref=T.IN(T.S(T.i32), T.L("1"), T.L("2"), T.L("3")))
    n = len(rows)
    n_since = _count(since, rows)
    f_later, f_small = _count(later, rows) / n, _count(small, rows) / n
    assert 0 < n_since < n and 0 < f_later < 1 and 0 < f_small < 1
    check = (Check(CheckLevel.Error, "date partition")
             .has_size(lambda v: v == n_since).where(since.pred)
             .satisfies(later.pred, "d2 not before d", lambda v: v == f_later)
             .satisfies(small.pred, "i32 in 1..3 as text", lambda v: v == f_small)
             .satisfies(later.pred, "every d2 not before d (fails)", lambda v: v == 1.0))
    result = VerificationSuite().on_data(df).add_check(check).run()
    statuses = [cr.status.name for cr in result.check_results[check].constraint_results]
    print(statuses, result.metrics)
    assert statuses == ["Success", "Success", "Success", "Failure"]
    assert result.status == CheckStatus.Error
    assert result.metrics[Size(where=since.pred)].value.get() == float(n_since)
    assert result.metrics[Compliance("d2 not before d", later.pred)].value.get() == f_later
    assert result.metrics[Compliance("i32 in 1..3 as text", small.pred)].value.get() == f_small


def test_incremental_run_equals_the_whole_table(gpu_device):
    """States saved on one half, the other half aggregated with them: the whole table's metrics."""
    from deequ_amd import Table
    from deequ_amd.analyzers import Compliance, InMemoryStateProvider, Size
    from deequ_amd.runners import Analysis, AnalysisRunner
    arrow, rows = T.table()
    half = arrow.num_rows // 2 + 13
    analyzers = [Compliance("since", "CAST(d AS STRING) >= '2000-01-01'"), Compliance("later", "d2 >= d"),
                 Compliance("y", "year(ts) IN (2019, 2020)"), Size(where="ts >= '2020-01-01'")]
    analysis = Analysis(analyzers)
    states = InMemoryStateProvider()
    AnalysisRunner.run(Table.from_arrow(arrow.slice(0, half), device=gpu_device), analysis,
                       save_states_with=states)
    results = AnalysisRunner.run(Table.from_arrow(arrow.slice(half), device=gpu_device), analysis,
                                 aggregate_with=states)
    whole = Table.from_arrow(arrow, device=gpu_device)
    refs = [T.G(">=", T.S(T.d), T.L("2000-01-01")), T.GT(">=", T.d2, T.d),
            T.IN(T.YEAR(T.ts), T.L(2019), T.L(2020)), T.G(">=", T.S(T.ts), T.L("2020-01-01"))]
    for a, ref in zip(analyzers, refs):
        direct = a.calculate(whole).value.get()
        n_true = sum(1 for r in rows if ref(r) is True)
        expect = float(n_true) if isinstance(a, Size) else n_true / len(rows)
        print(a, results.metric(a).value.get(), direct, expect)
        assert results.metric(a).value.get() == direct == expect
