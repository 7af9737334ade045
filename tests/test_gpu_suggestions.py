"""ConstraintSuggestionRunner on the device: the reference's JSON documents
(ConstraintSuggestionResultTest.scala), the repository cases of ConstraintSuggestionRunnerTest.scala
restated on the metric maps, the integration scenario of ConstraintSuggestionsIntegrationTest.scala
and the hold-out evaluation on Table.random_split."""
import json

import numpy as np
import pytest

import split_host as S
from fixtures import arrow_table
from test_suggestions_host import assertion_of, load_golden

pytestmark = pytest.mark.gpu


def fixture_table(name, device):
    from deequ_amd.table import Table
    return Table.from_arrow(arrow_table(name), device=device)


def runner(data):
    from deequ_amd import ConstraintSuggestionRunner, Rules
    return ConstraintSuggestionRunner().on_data(data).add_constraint_rules(Rules.DEFAULT)


def expand_profiles(doc):
    cols = []
    for c in doc["columns"]:
        c = dict(c)
        runs = c.pop("approxPercentiles_runs", None)
        if runs is not None:
            c["approxPercentiles"] = [v for v, k in runs for _ in range(k)]
        cols.append(c)
    return {"columns": cols}


def by_column(rows):
    out = {}
    for r in rows:
        out.setdefault(r["column_name"], []).append(r)
    return out


def test_reference_documents_of_df_full(gpu_device):
    """ConstraintSuggestionResultTest.scala:21-260 (getDfFull; Spark's 0.1 split with seed 0 happened
    to keep all four rows for training, so the documents are those of the whole table).  The
    reference's suggestion order across columns is its HashMap's; within a column it is rule order,
    which is what is compared."""
    from deequ_amd import ConstraintSuggestionResult as R
    docs = load_golden()["documents"]
    res = runner(fixture_table(docs["table"], gpu_device)).run()
    assert res.verification_result is None
    got = json.loads(R.get_column_profiles_as_json(res))
    want = expand_profiles(docs["column_profiles"])
    assert got["columns"][0] == want["columns"][0]
    for g, w in zip(got["columns"][1:], want["columns"][1:]):  # histogram entries: the map's order
        assert sorted(g.pop("histogram"), key=lambda e: e["value"]) == \
            sorted(w.pop("histogram"), key=lambda e: e["value"])
        assert g == w
    got = json.loads(R.get_constraint_suggestions_as_json(res))["constraint_suggestions"]
    want = docs["constraint_suggestions"]["constraint_suggestions"]
    assert by_column(got) == by_column(want)
    assert [r["column_name"] for r in got] == ["item"] * 4 + ["att1", "att2"]  # column order here
    # without a split the evaluation getter returns the profiles (ConstraintSuggestionResult.scala)
    assert R.get_evaluation_results_as_json(res) == R.get_column_profiles_as_json(res)


def test_numeric_values_documents_and_files(gpu_device, tmp_path):
    """getDfWithNumericValues through the runner (ConstraintSuggestionRunnerTest.scala:147-174 writes
    the three files).  Expected by hand from the rules: item ("1".."6": complete, 6 of 6 distinct,
    inferred Integral, minimum 1.0) gets NOT NULL, UNIQUE, the type and the positive rule; att1 (an
    int column 1..6: its type is known, not inferred) NOT NULL, UNIQUE, positive; att2 (0 0 0 5 6 7:
    4 of 6 distinct = 0.667, minimum 0.0) NOT NULL and non-negative."""
    from deequ_amd import ConstraintSuggestionResult as R
    data = fixture_table("dfWithNumericValues", gpu_device)
    res = runner(data).run()
    rows = json.loads(R.get_constraint_suggestions_as_json(res))["constraint_suggestions"]
    assert [(r["column_name"], r["suggesting_rule"]) for r in rows] == [
        ("item", "CompleteIfCompleteRule"), ("item", "UniqueIfApproximatelyUniqueRule"),
        ("item", "RetainTypeRule"), ("item", "PositiveNumbersRule"),
        ("att1", "CompleteIfCompleteRule"), ("att1", "UniqueIfApproximatelyUniqueRule"),
        ("att1", "PositiveNumbersRule"),
        ("att2", "CompleteIfCompleteRule"), ("att2", "NonNegativeNumbersRule")]
    assert rows[8] == {
        "constraint_name": "ComplianceConstraint(Compliance('att2' has no negative values,"
                           "att2 >= 0,None))",
        "column_name": "att2", "current_value": "Minimum: 0.0",
        "description": "'att2' has no negative values", "suggesting_rule": "NonNegativeNumbersRule",
        "rule_description": "If we see only non-negative numbers in a column, we suggest a "
                            "corresponding constraint",
        "code_for_constraint": '.isNonNegative("att2")'}
    assert rows[1]["current_value"] == "ApproxDistinctness: 1.0"
    profiles = json.loads(R.get_column_profiles_as_json(res))["columns"]
    assert [(p["column"], p["dataType"], p["isDataTypeInferred"], p["minimum"], p["sum"])
            for p in profiles] == [("item", "Integral", "true", 1.0, 21.0),
                                   ("att1", "Integral", "false", 1.0, 21.0),
                                   ("att2", "Integral", "false", 0.0, 18.0)]
    # with a train/test split: the three files hold what the result's getters give
    paths = [str(tmp_path / n) for n in ("profiles.json", "suggestions.json", "evaluation.json")]
    res = (runner(data).save_column_profiles_json_to_path(paths[0])
           .save_constraint_suggestions_json_to_path(paths[1])
           .use_train_test_split_with_testset_ratio(0.1, 0)
           .save_evaluation_results_json_to_path(paths[2]).run())
    getters = (R.get_column_profiles_as_json, R.get_constraint_suggestions_as_json,
               R.get_evaluation_results_as_json)
    for path, getter in zip(paths, getters):
        assert open(path, encoding="utf-8").read() == getter(res) + "\n"
    ev = json.loads(open(paths[2], encoding="utf-8").read())["constraint_suggestions"]
    sg = json.loads(open(paths[1], encoding="utf-8").read())["constraint_suggestions"]
    assert len(ev) == len(sg) > 0
    for e, s in zip(ev, sg):  # the shape: the shared properties, then the result
        assert list(e) == list(s) + ["constraint_result"]
        assert {k: e[k] for k in s} == s and e["constraint_result"] in ("Success", "Failure")
    train = int((S.assign(0, 0, 6, [1.0 - 0.1, 0.1]) == 0).sum())
    assert res.column_profiles["item"].completeness == 1.0
    assert len(res.verification_result.check_results) == 1 and train <= 6
    with pytest.raises(FileExistsError):
        runner(data).save_column_profiles_json_to_path(paths[0]).run()
    runner(data).save_column_profiles_json_to_path(paths[0]).overwrite_previous_files(True).run()


def test_repository_reuse_save_and_fail_if_missing(gpu_device):
    """ConstraintSuggestionRunnerTest.scala:37-146, 176-189 on the metric maps."""
    from deequ_amd import AnalysisRunner, ConstraintSuggestionResult as R
    from deequ_amd.analyzers import Completeness, Size
    from deequ_amd.exceptions import ReusingNotPossibleResultsMissingException
    from deequ_amd.metrics import DoubleMetric, Entity, Success
    from deequ_amd.repository import InMemoryMetricsRepository, ResultKey
    from deequ_amd.runners import AnalyzerContext
    data = fixture_table("dfWithNumericValues", gpu_device)
    repo, key = InMemoryMetricsRepository(), ResultKey(0, {})
    runner(data).use_repository(repo).save_or_append_result(key).run()
    separate = runner(data).run()
    # fail_if_results_missing=True: a reusing run that had to compute anything would raise
    reusing = runner(data).use_repository(repo).reuse_existing_results_for_key(key, True).run()
    assert separate.column_profiles == reusing.column_profiles
    assert R.get_constraint_suggestions_as_json(separate) == \
        R.get_constraint_suggestions_as_json(reusing)
    # :70-88 the saved results hold what an analysis run computes
    ctx = AnalysisRunner.on_data(data).add_analyzers([Size(), Completeness("item")]).run()
    saved = repo.load_by_key(key).metric_map
    assert len(ctx.metric_map) == 2
    assert all(saved[a] == m for a, m in ctx.metric_map.items())
    # :118-145 new results win over a conflicting stored one
    repo2 = InMemoryMetricsRepository()
    repo2.save(key, AnalyzerContext({Size(): DoubleMetric(Entity.Dataset, "", "", Success(100.0))}))
    runner(data).use_repository(repo2).save_or_append_result(key).run()
    saved = repo2.load_by_key(key).metric_map
    assert all(saved[a] == m for a, m in ctx.metric_map.items())
    # :176-189
    with pytest.raises(ReusingNotPossibleResultsMissingException):
        runner(data).use_repository(InMemoryMetricsRepository()) \
            .reuse_existing_results_for_key(ResultKey(0, {}), True).run()


# ------------------------------------------------------------------------------------------------
# the integration scenario
# ------------------------------------------------------------------------------------------------
N_RECORDS = 10_000


@pytest.fixture(scope="module")
def records(gpu_device):
    """ConstraintSuggestionsIntegrationTest.scala:44-72 from a NumPy generator."""
    import pyarrow as pa
    from deequ_amd.table import Table
    rng = np.random.default_rng(0)
    n = N_RECORDS
    raw = rng.integers(0, 256, (n, 16), dtype=np.uint8)
    ids = [bytes(r).hex() for r in raw]
    ids = [f"{h[:8]}-{h[8:12]}-{h[12:16]}-{h[16:20]}-{h[20:]}" for h in ids]
    assert len(set(ids)) == n  # (the oracle's HLL++ estimate of these ids is 10389: within 8%)
    categories = ["DE", "NA", "IN", "EU"]
    m3 = rng.random(n)
    table = pa.table({
        "id": pa.array(ids, pa.string()),
        "marketplace": pa.array([categories[i] for i in rng.integers(0, 4, n)], pa.string()),
        "measurement": pa.array(rng.random(n) + 1e-9, pa.float64()),
        "propertyA": pa.array([str(bool(b)).lower() for b in rng.integers(0, 2, n)], pa.string()),
        "measurement2": pa.array([str(float(v) - 0.5) for v in rng.integers(0, 100, n)], pa.string()),
        # (12 decimals: the profiler's device cast of a string to double converts digit strings
        # up to 2^53 exactly and refuses longer ones loudly, so a full 17-digit Double.toString
        # is not a column this engine profiles; the scenario asserts only the column's completeness)
        "measurement3": pa.array([repr(round(float(d), 12)) if d >= 0.5 else None for d in m3],
                                 pa.string()),
        "allNullColumn": pa.array([None] * n, pa.string()),
        "allNullColumn2": pa.array([None] * n, pa.float64()),
    })
    return Table.from_arrow(table, device=gpu_device)


def constraints_of(result):
    out = []
    for group in result.constraint_suggestions.values():
        for s in group:
            inner = s.constraint.inner if hasattr(s.constraint, "inner") else s.constraint
            out.append((inner.analyzer, assertion_of(s.constraint)))
    return out


def test_integration_scenario(gpu_device, records):
    from deequ_amd.analyzers import Completeness, Compliance, DataType, Uniqueness
    res = runner(records).run()
    cs = constraints_of(res)

    def exists(pred):
        return any(pred(a, f) for a, f in cs)

    for col in ("id", "marketplace", "measurement", "propertyA", "measurement2"):
        assert exists(lambda a, f: a == Completeness(col) and f(1.0)), col
    assert exists(lambda a, f: a == Uniqueness(["id"]) and f(1.0))
    assert not exists(lambda a, f: a == DataType("id"))
    assert exists(lambda a, f: f(1.0) and isinstance(a, Compliance)
                  and a.instance.startswith("'marketplace' has value range"))
    assert exists(lambda a, f: f(1.0) and isinstance(a, Compliance)
                  and a.instance == "'measurement' has only positive values")
    assert not exists(lambda a, f: a == DataType("measurement") and f(1.0))
    assert exists(lambda a, f: a == DataType("propertyA") and f(1.0))
    for text in ("has only positive values", "has no negative values"):
        assert not exists(lambda a, f: f(1.0) and isinstance(a, Compliance)
                          and a.instance == f"'measurement2' {text}")
    assert exists(lambda a, f: a == DataType("measurement2") and f(1.0))
    assert exists(lambda a, f: a == Completeness("measurement3") and f(0.8))
    assert not exists(lambda a, f: a == Completeness("measurement3") and f(0.2))
    from deequ_amd.analyzers.datatype import DataTypeInstances
    assert res.column_profiles["propertyA"].data_type == DataTypeInstances.Boolean
    assert res.column_profiles["measurement2"].data_type == DataTypeInstances.Fractional


def test_hold_out_evaluation(gpu_device, records):
    from deequ_amd import Check, CheckLevel, VerificationSuite
    res = runner(records).use_train_test_split_with_testset_ratio(0.1, 0).run()
    suggestions = [s for group in res.constraint_suggestions.values() for s in group]
    assert suggestions
    (check, check_result), = res.verification_result.check_results.items()
    assert (check.level, check.description) == (CheckLevel.Warning, "generated constraints")
    assert [r.constraint for r in check_result.constraint_results] == \
        [s.constraint for s in suggestions]
    # the same check on the hold-out taken apart by hand
    test = records.random_split([1.0 - 0.1, 0.1], 0)[1]
    again = VerificationSuite().on_data(test).add_check(
        Check(CheckLevel.Warning, "generated constraints", [s.constraint for s in suggestions])).run()
    (_, again_result), = again.check_results.items()
    assert [r.status for r in again_result.constraint_results] == \
        [r.status for r in check_result.constraint_results]
    a = S.assign(0, 0, N_RECORDS, [1.0 - 0.1, 0.1])
    assert test.num_rows == int((a == 1).sum())
    # the profile was taken over the training rows alone: its histogram counts every one of them
    hist = res.column_profiles["marketplace"].histogram
    assert sum(v.absolute for v in hist.values.values()) == int((a == 0).sum())


def test_profile_counts_the_training_rows(gpu_device, records):
    from deequ_amd import ConstraintSuggestionRunner
    train = int((S.assign(3, 0, N_RECORDS, [1.0 - 0.25, 0.25]) == 0).sum())
    profiles, _ = ConstraintSuggestionRunner.profile_and_suggest(
        records.random_split([1.0 - 0.25, 0.25], 3)[0], [], ["marketplace"], 120, False)
    assert profiles.num_records == train


@pytest.mark.parametrize("ratio", [0, 1, 1.5])
def test_ratio_outside_the_open_interval(gpu_device, records, ratio):
    with pytest.raises(ValueError, match=r"requirement failed: Testset ratio must be in \]0, 1\["):
        runner(records).use_train_test_split_with_testset_ratio(ratio, 0).run()
