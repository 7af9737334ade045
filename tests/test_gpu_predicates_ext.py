"""Row-exact conformance of LIKE, arithmetic and the scalar functions on the device.

The method of tests/test_gpu_predicates.py: for every predicate p of the matrix
(tests/predicate_ext_cases.py) Sum("w", where=p), Sum("w", where="NOT (p)") and Size(where=p) must
give the weight fingerprints of the reference evaluator's TRUE and FALSE row sets and its count;
Compliance(p) in total and under `g = k` (eight groups and the empty ninth) its counts; explain()
must show the interpreter's expression bitmaps for both forms.  The oracle cannot parse these
forms, so the reference is the evaluator that lives with the cases (numpy fixed-width integers,
np.float32, re.fullmatch), itself pinned by tests/test_predicates_ext_ref.py.

Reference-backed: the analyzers of IncrementalAnalysisTest.scala:52-57 over its own rows
(tests/golden/incremental_analysis_rows.json) through saved states, and
Compliance("attribute", "attribute like '%facets%'") of StateAggregationTests.scala:23 through
merged partition states.
"""
import json
import os

import pyarrow as pa
import pytest

import predicate_cases as PC
import predicate_ext_cases as X
import test_gpu_predicates as TP

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ext_table(gpu_device):
    from deequ_amd import Table
    return Table.from_arrow(X.table()[0], device=gpu_device)


def _check(c, df, arrow, tv):
    from deequ_amd.runners.engine import get_plan, run_scan
    e = PC.expected(tv, arrow.column("w").to_pylist(), arrow.column("g").to_pylist())
    specs = TP._where_specs(c.pred)
    TP._assert_where_path(get_plan(df.schema, specs).explain())
    row = run_scan(df, specs)
    print(c.pred, "where form:", row, e)
    assert row[0] == e["sum_true"], "rows the interpreter calls TRUE"
    assert row[1] == e["sum_false"], "rows the interpreter calls FALSE"
    assert row[2] == e["count"]
    specs = TP._compliance_specs(c.pred)
    TP._assert_compliance_path(get_plan(df.schema, specs).explain(), "gen")
    row = run_scan(df, specs)
    print(c.pred, "compliance:", row[0], [row[2 + 2 * k] for k in X.GROUPS], e)
    assert row[0] == e["count"]
    assert row[1] == arrow.num_rows
    assert [row[2 + 2 * k] for k in X.GROUPS] == e["groups"]
    assert e["groups"][8] is None


@pytest.mark.parametrize("c", X.CASES, ids=TP._ids(X.CASES))
def test_extended_predicate_rows_match_reference(c, ext_table):
    assert c.path == "gen"
    _check(c, ext_table, X.table()[0], X.truth(c))


def test_like_across_batches_and_bitmap_words(gpu_device):
    """40 993 rows in batches of 4096: ten batches and a 33-row tail, every batch ending inside a
    bitmap word of the next one's numbering; a general-matcher pattern and a fast shape."""
    from deequ_amd import Table
    arrow = X.batched_arrow()
    df = Table.from_arrow(arrow, device=gpu_device, max_batch_rows=4096)
    rows = arrow.to_pylist()
    for pattern in ("%a_b%", "%keyword%"):
        c = X.case("batched", f"t LIKE '{pattern}'", "gen", ref=X.LIKE(X.C("t"), pattern))
        tv = tuple(c.ref(r) for r in rows)
        assert {True, False, None} == set(tv)
        _check(c, df, arrow, tv)


# ------------------------------------------------------------------------------------------------
# The reference's own LIKE predicates, through the public API
# ------------------------------------------------------------------------------------------------
def _reference_rows():
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "incremental_analysis_rows.json")
    with open(path) as f:
        doc = json.load(f)

    def arrow(rows):
        cols = list(zip(*rows))
        return pa.table({name: pa.array(list(cols[k]), type=getattr(pa, doc["types"][name])())
                         for k, name in enumerate(doc["columns"])})
    return arrow(doc["initial"]), arrow(doc["delta"])


def test_incremental_analysis_with_like_predicates(gpu_device):
    """IncrementalAnalysisTest.scala:43-68: states of `initial` saved, `delta` aggregated with them;
    every metric equals analyzer.calculate(everything)."""
    from deequ_amd import Table
    from deequ_amd.analyzers import Completeness, Compliance, InMemoryStateProvider
    from deequ_amd.runners import Analysis, AnalysisRunner
    initial, delta = _reference_rows()
    everything = Table.from_arrow(pa.concat_tables([initial, delta]), device=gpu_device)
    analyzers = [Compliance("attributeNonNull", "attribute IS NOT NULL"),
                 Compliance("categoryAttribute", "attribute LIKE 'CATEGORY%'"),
                 Compliance("attributeKeyword", "attribute LIKE '%keyword%'"),
                 Completeness("marketplace_id"), Completeness("item")]
    analysis = Analysis(analyzers)
    states = InMemoryStateProvider()
    AnalysisRunner.run(Table.from_arrow(initial, device=gpu_device), analysis, save_states_with=states)
    results = AnalysisRunner.run(Table.from_arrow(delta, device=gpu_device), analysis, aggregate_with=states)
    for a in analyzers:
        direct = a.calculate(everything)
        assert direct.value.is_success, str(a)
        assert results.metric(a).value.get() == direct.value.get(), str(a)
    # the rows hold 12 CATEGORY... attributes and 20 ...keyword... ones out of 40
    assert results.metric(analyzers[1]).value.get() == 12 / 40
    assert results.metric(analyzers[2]).value.get() == 20 / 40
    assert results.metric(analyzers[0]).value.get() == 1.0


def test_state_aggregation_of_a_like_compliance(gpu_device):
    """StateAggregationTests.scala:23 (correctlyAggregatesStates): the states of two partitions,
    merged, give the metric of the whole table."""
    from deequ_amd import Table
    from deequ_amd.analyzers import Compliance
    from deequ_amd.analyzers.base import merge_states
    initial, delta = _reference_rows()
    a = Compliance("attribute", "attribute like '%facets%'")
    parts = [a.compute_state_from(Table.from_arrow(t, device=gpu_device)) for t in (initial, delta)]
    merged = a.compute_metric_from(merge_states(*parts))
    direct = a.calculate(Table.from_arrow(pa.concat_tables([initial, delta]), device=gpu_device))
    assert merged.value.get() == direct.value.get() == 16 / 40
