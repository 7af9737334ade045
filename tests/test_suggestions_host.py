"""Constraint suggestion on the host: the reference's rule cases over hand-built profiles
(tests/golden/suggestion_known_answers.json), the text of the candidates, the two JSON documents
with stub constraint results, and the restatement of the split's draw (tests/split_host.py)."""
import json
import math
import os

import numpy as np
import pytest

import split_host as S

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden",
                      "suggestion_known_answers.json")


def load_golden():
    with open(GOLDEN, encoding="utf-8") as fh:
        return json.load(fh)


def make_profile(p):
    from deequ_amd import Distribution, DistributionValue
    from deequ_amd.analyzers.datatype import DataTypeInstances
    from deequ_amd.profiles import NumericColumnProfile, StandardColumnProfile
    hist = None
    if p["histogram"] is not None:
        hist = Distribution({k: DistributionValue(a, r) for k, a, r in p["histogram"]["values"]},
                            p["histogram"]["bins"])
    base = dict(column=p["column"], completeness=p["completeness"],
                approximate_num_distinct_values=p["approx_distinct"],
                data_type=DataTypeInstances[p["data_type"]], is_data_type_inferred=p["inferred"],
                type_counts={}, histogram=hist)
    if p["kind"] == "numeric":
        return NumericColumnProfile(**base, mean=p["mean"], maximum=p["maximum"],
                                    minimum=p["minimum"], sum=p["sum"], std_dev=p["std_dev"])
    return StandardColumnProfile(**base)


def std_profile(column="c", completeness=1.0, approx=100, dtype="String", inferred=False, hist=None):
    return make_profile({"kind": "standard", "column": column, "completeness": completeness,
                         "approx_distinct": approx, "data_type": dtype, "inferred": inferred,
                         "histogram": hist})


def rule_named(name):
    import deequ_amd
    return getattr(deequ_amd, name)()


def assertion_of(constraint):
    return constraint.inner.assertion if hasattr(constraint, "inner") else constraint.assertion


@pytest.mark.parametrize("case", load_golden()["rule_applies"],
                         ids=lambda c: f"{c['rule']}-{c['name']}")
def test_rule_applies_as_in_the_reference(case):
    rule = rule_named(case["rule"])
    assert rule.should_be_applied(make_profile(case["profile"]), case["num_records"]) \
        is case["applies"], case["cite"]


@pytest.mark.parametrize("case", load_golden()["rule_candidates"], ids=lambda c: c["rule"])
def test_candidate_code_and_assertion(case):
    rule = rule_named(case["rule"])
    s = rule.candidate(make_profile(case["profile"]), case["num_records"])
    assert s.code_for_constraint == case["code"], case["cite"]
    assert s.column_name == case["profile"]["column"] and s.suggesting_rule is rule
    for value, holds in case["probes"]:
        assert bool(assertion_of(s.constraint)(value)) is holds


def test_rules_default_is_the_reference_order():
    from deequ_amd import Rules
    assert [type(r).__name__ for r in Rules.DEFAULT] == [
        "CompleteIfCompleteRule", "RetainCompletenessRule", "UniqueIfApproximatelyUniqueRule",
        "RetainTypeRule", "CategoricalRangeRule", "FractionalCategoricalRangeRule",
        "NonNegativeNumbersRule", "PositiveNumbersRule"]
    assert Rules.DEFAULT[5].target_data_coverage_fraction == 0.9


def test_retain_completeness_text():
    """p = 0.5, n = 100: 0.5 - 1.96 * sqrt(0.25 / 100) = 0.5 - 0.098 = 0.402 -> DOWN to 0.40, printed
    0.4; (1 - 0.4) * 100 = 60.0 -> 60.
    p = 0.25, n = 1000: 0.25 - 1.96 * sqrt(0.1875 / 1000) = 0.25 - 0.026838... = 0.22316... -> 0.22;
    (1 - 0.22) * 100 = 78.0 -> 78.
    p = 0.9, n = 10: 0.9 - 1.96 * sqrt(0.09 / 10) = 0.9 - 0.185942... = 0.714057... -> 0.71;
    (1 - 0.71) * 100 = 29.000000000000004 in fp64 -> 29.
    p = 0.3, n = 4: 0.3 - 1.96 * sqrt(0.21 / 4) = 0.3 - 0.449092... = -0.149092... -> DOWN is toward
    zero: -0.14; (1 + 0.14) * 100 = 114.00000000000001 -> 114."""
    from deequ_amd import RetainCompletenessRule
    rule = RetainCompletenessRule()
    for p, n, target, percent in [(0.5, 100, "0.4", 60), (0.25, 1000, "0.22", 78),
                                  (0.9, 10, "0.71", 29), (0.3, 4, "-0.14", 114)]:
        s = rule.candidate(std_profile("att1", p), n)
        assert s.description == f"'att1' has less than {percent}% missing values"
        assert s.current_value == f"Completeness: {p}"
        assert s.code_for_constraint == (f'.hasCompleteness("att1", _ >= {target}, '
                                         f'Some("It should be above {target}!"))')
        assert str(s.constraint) == "CompletenessConstraint(Completeness(att1,None))"
        f = assertion_of(s.constraint)
        assert f(float(target)) and not f(float(target) - 0.001)
        assert s.constraint.inner.hint is None  # (the hint is in the code string only)


def test_constraint_names_of_every_kind():
    """ConstraintSuggestionResultTest.scala:196-257: the toString of each constraint kind."""
    from deequ_amd import (CategoricalRangeRule, CompleteIfCompleteRule, NonNegativeNumbersRule,
                           PositiveNumbersRule, RetainTypeRule, UniqueIfApproximatelyUniqueRule)
    p = std_profile("item", dtype="Integral", inferred=True)
    assert str(CompleteIfCompleteRule().candidate(p, 4).constraint) == \
        "CompletenessConstraint(Completeness(item,None))"
    assert str(UniqueIfApproximatelyUniqueRule().candidate(p, 100).constraint) == \
        "UniquenessConstraint(Uniqueness(List(item)))"
    assert str(RetainTypeRule().candidate(p, 4).constraint) == \
        "AnalysisBasedConstraint(DataType(item,None),<function1>,Some(<function1>),None)"
    assert str(PositiveNumbersRule().candidate(p, 4).constraint) == \
        "ComplianceConstraint(Compliance('item' has only positive values,item > 0,None))"
    assert str(NonNegativeNumbersRule().candidate(p, 4).constraint) == \
        "ComplianceConstraint(Compliance('item' has no negative values,item >= 0,None))"
    hist = {"values": [["a", 2, 0.5], ["b", 2, 0.5]], "bins": 2}
    assert str(CategoricalRangeRule().candidate(std_profile("c", hist=hist), 4).constraint) == \
        "ComplianceConstraint(Compliance('c' has value range 'b', 'a',c IN ('b', 'a'),None))"


NASTY = "a'b\"c\\d\teé\U0001F600"  # ' " \ tab e-acute and a non-BMP character


def test_category_escaping():
    """The SQL list doubles the single quote and nothing else; the code list is escapeJava: \" and \\
    take a backslash, the tab goes by name, U+00E9 -> \\u00E9, U+1F600 -> its two UTF-16 units
    \\uD83D\\uDE00 (0x1F600 - 0x10000 = 0xF600: high 0xD800 + (0xF600 >> 10) = 0xD83D, low
    0xDC00 + (0xF600 & 0x3FF) = 0xDE00)."""
    from deequ_amd import CategoricalRangeRule
    hist = {"values": [[NASTY, 3, 0.6], ["plain", 2, 0.4]], "bins": 2}
    s = CategoricalRangeRule().candidate(std_profile("c", hist=hist), 5)
    sql = "'a''b\"c\\d\teé\U0001F600', 'plain'"
    assert s.description == f"'c' has value range {sql}"
    assert str(s.constraint) == f"ComplianceConstraint(Compliance({s.description},c IN ({sql}),None))"
    assert s.code_for_constraint == \
        '.isContainedIn("c", Array("a\'b\\"c\\\\d\\te\\u00E9\\uD83D\\uDE00", "plain"))'
    assert s.current_value == "Compliance: 1"


def test_categories_drop_the_null_replacement_and_sort_like_scala():
    """sortBy(absolute).reverse is a stable ascending sort reversed: ties come out in reverse map
    order.  "NullValue" is dropped, a real value of that text included."""
    from deequ_amd import CategoricalRangeRule
    hist = {"values": [["x", 2, 0.2], ["NullValue", 4, 0.4], ["y", 2, 0.2], ["z", 2, 0.2]], "bins": 4}
    s = CategoricalRangeRule().candidate(std_profile("c", hist=hist), 10)
    assert s.code_for_constraint == '.isContainedIn("c", Array("z", "y", "x"))'


def test_fractional_rule_text():
    """Ratios 0.65 and 0.3 reach the 0.9 coverage (0.65 < 0.9 takes the next, 0.95 stops): p = 0.65 +
    0.3 = 0.95 in fp64 (printed 0.95), n = 100: 0.95 - 1.96 * sqrt(0.0475 / 100) = 0.95 - 0.042717...
    = 0.907282... -> 0.90, printed 0.9; 0.9 * 100 = 90.0 in fp64.
    Ratios 0.5, 0.41 (0.91 stops, 0.09 left out), n = 50: p = 0.5 + 0.41 = 0.9099999999999999 in fp64,
    printed so by Double.toString; 0.91 - 1.96 * sqrt(0.0819 / 50) =
    0.91 - 0.079325... = 0.830674... -> 0.83; 0.83 * 100 = 83.0 in fp64 (asserted below)."""
    from deequ_amd import FractionalCategoricalRangeRule
    rule = FractionalCategoricalRangeRule()
    hist = {"values": [["'_[a_[]}!@'", 6, 0.3], ["_b%%__", 13, 0.65], ["_b%__", 1, 0.05]], "bins": 20}
    s = rule.candidate(std_profile("cat", hist=hist), 100)
    sql = "'_b%%__', '''_[a_[]}!@'''"
    assert s.description == f"'cat' has value range {sql} for at least 90.0% of values"
    assert s.current_value == "Compliance: 0.95"
    assert s.constraint.inner.hint == "It should be above 0.9!"
    assert str(s.constraint) == f"ComplianceConstraint(Compliance({s.description},cat IN ({sql}),None))"
    f = assertion_of(s.constraint)
    assert f(0.9) and not f(0.89)
    hist = {"values": [["a", 50, 0.5], ["b", 41, 0.41], ["c", 9, 0.09]], "bins": 3}
    s = rule.candidate(std_profile("cat", hist=hist), 50)
    assert 0.83 * 100 == 83.0 and repr(0.5 + 0.41) == "0.9099999999999999"
    assert s.description == "'cat' has value range 'a', 'b' for at least 83.0% of values"
    assert s.current_value == "Compliance: 0.9099999999999999"
    assert s.code_for_constraint == ('.isContainedIn("cat", Array("a", "b"), _ >= 0.83, '
                                     'Some("It should be above 0.83!"))')
    assert FractionalCategoricalRangeRule(0.4).candidate(std_profile("cat", hist=hist), 50) \
        .code_for_constraint.startswith('.isContainedIn("cat", Array("a"), _ >= 0.36,')
    # 0.5 - 1.96 * sqrt(0.25 / 50) = 0.5 - 0.138592... = 0.361407... -> 0.36


def test_unique_rule_without_an_approximate_count():
    """The HLL++ bias range gives no number: the rule does not apply (documented deviation)."""
    from deequ_amd import UniqueIfApproximatelyUniqueRule
    rule = UniqueIfApproximatelyUniqueRule()
    p = std_profile("c", approx=None)
    assert rule.should_be_applied(p, 100) is False
    with pytest.raises(ValueError, match="column c"):
        rule.candidate(p, 100)
    s = rule.candidate(std_profile("c", approx=95), 100)
    assert s.current_value == "ApproxDistinctness: 0.95"


def test_sign_rules_text():
    from deequ_amd import NonNegativeNumbersRule, PositiveNumbersRule
    num = make_profile({"kind": "numeric", "column": "m", "completeness": 1.0, "approx_distinct": 9,
                        "data_type": "Fractional", "inferred": False, "histogram": None,
                        "mean": 1.0, "maximum": 2.0, "minimum": 1.0e-5, "sum": 3.0, "std_dev": 1.0})
    assert PositiveNumbersRule().candidate(num, 9).current_value == "Minimum: 1.0E-5"
    assert NonNegativeNumbersRule().candidate(std_profile("m"), 9).current_value == \
        "Minimum: Error while calculating minimum!"


class _StubResult:
    def __init__(self, status):
        from deequ_amd import ConstraintStatus
        self.status = ConstraintStatus[status]


def golden_suggestions():
    """The suggestions of the golden documents rebuilt from the rules, in the documents' order."""
    from deequ_amd import (CompleteIfCompleteRule, PositiveNumbersRule, RetainTypeRule,
                           UniqueIfApproximatelyUniqueRule)
    item = make_profile({"kind": "numeric", "column": "item", "completeness": 1.0,
                         "approx_distinct": 4, "data_type": "Integral", "inferred": True,
                         "histogram": None, "mean": 2.5, "maximum": 4.0, "minimum": 1.0, "sum": 10.0,
                         "std_dev": 1.118033988749895})
    return [CompleteIfCompleteRule().candidate(std_profile("att2", approx=2, inferred=True), 4),
            CompleteIfCompleteRule().candidate(std_profile("att1", approx=2, inferred=True), 4),
            CompleteIfCompleteRule().candidate(item, 4),
            UniqueIfApproximatelyUniqueRule().candidate(item, 4),
            RetainTypeRule().candidate(item, 4), PositiveNumbersRule().candidate(item, 4)]


def test_json_documents_against_the_reference():
    from deequ_amd import (Check, CheckLevel, CheckResult, CheckStatus, ConstraintSuggestions,
                           VerificationResult)
    docs = load_golden()["documents"]
    suggestions = golden_suggestions()
    text = ConstraintSuggestions.to_json(suggestions)
    assert json.loads(text) == docs["constraint_suggestions"]
    check = Check(CheckLevel.Warning, "generated constraints", [s.constraint for s in suggestions])
    result = VerificationResult(CheckStatus.Warning, {check: CheckResult(
        check, CheckStatus.Warning, [_StubResult("Failure") for _ in suggestions])}, {})
    ev = ConstraintSuggestions.evaluation_results_to_json(suggestions, result)
    assert json.loads(ev) == docs["evaluation_results"]
    assert list(json.loads(ev)["constraint_suggestions"][0])[-1] == "constraint_result"
    # Gson's pretty printer: two-space indentation and its HTML-safe escapes.  Both documents come
    # from one GsonBuilder, so both write ' as \\u0027 and < > as \\u003c \\u003e (the reference's
    # expected strings are compared as parsed trees, which is why :199 can show a bare quote)
    for doc in (text, ev):
        assert doc.startswith('{\n  "constraint_suggestions": [\n    {\n      "constraint_name": ')
        assert '"description": "\\u0027att2\\u0027 is not null"' in doc
        assert "\\u003cfunction1\\u003e,Some(\\u003cfunction1\\u003e),None)" in doc
        assert 'item \\u003e 0,None))"' in doc and '".isComplete(\\"att2\\")"' in doc
        assert "'" not in doc and "<" not in doc and ">" not in doc
    assert json.loads(ConstraintSuggestions.to_json([])) == {"constraint_suggestions": []}


def test_json_keeps_non_ascii_text_and_escapes_controls():
    from deequ_amd import CategoricalRangeRule, ConstraintSuggestions
    hist = {"values": [[NASTY, 3, 0.6], ["k=v&w", 2, 0.4]], "bins": 2}
    s = CategoricalRangeRule().candidate(std_profile("c", hist=hist), 5)
    text = ConstraintSuggestions.to_json([s])
    row = json.loads(text)["constraint_suggestions"][0]
    assert row["description"] == s.description and row["code_for_constraint"] == s.code_for_constraint
    assert "é\U0001F600" in text and "\\t" in text and "k\\u003dv\\u0026w" in text


def test_result_getters_without_a_split():
    from deequ_amd import ConstraintSuggestionResult
    from deequ_amd.profiles import ColumnProfiles
    suggestions = golden_suggestions()
    profiles = {"att2": std_profile("att2", approx=2, inferred=True)}
    res = ConstraintSuggestionResult(profiles, {"att2": suggestions[:1], "item": suggestions[2:]})
    got = json.loads(ConstraintSuggestionResult.get_constraint_suggestions_as_json(res))
    assert [r["column_name"] for r in got["constraint_suggestions"]] == ["att2"] + ["item"] * 4
    # without a verification result the evaluation getter returns the profiles (as the reference)
    assert ConstraintSuggestionResult.get_evaluation_results_as_json(res) == \
        ColumnProfiles.to_json(list(profiles.values()))


@pytest.mark.parametrize("ratio", [0, 1, 1.5])
def test_testset_ratio_outside_the_open_interval(ratio):
    from deequ_amd import ConstraintSuggestionRunner, Rules
    builder = ConstraintSuggestionRunner().on_data(None).add_constraint_rules(Rules.DEFAULT) \
        .use_train_test_split_with_testset_ratio(ratio, 0)
    with pytest.raises(ValueError, match=r"Testset ratio must be in \]0, 1\["):
        builder.run()


# ------------------------------------------------------------------------------------------------
# the draw
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed,row_base", [(0, 0), (1, 2**33 + 5), (2**63, 7), (2**64 - 1, 0)])
def test_vectorised_draw_equals_the_integer_one(seed, row_base):
    n = 10_000
    u = S.draw(seed, row_base, n)
    assert u.tolist() == [S.draw_int(seed, row_base + i) for i in range(n)]
    assert 0.0 <= u.min() and u.max() < 1.0
    for weights in ([0.9, 0.1], [1, 1, 1], [1e-9, 1], [1] * 8):
        bnd = S.bounds(weights)
        assert bnd[-1] == 1.0 and bnd == sorted(bnd)
        a = S.assign(seed, row_base, n, weights)
        assert a.tolist() == [S.split_int(seed, row_base + i, bnd) for i in range(n)]
        words, counts = S.bitmaps(seed, row_base, n, weights)
        assert sum(counts) == n and all(len(w) == (n + 63) // 64 for w in words)


def test_split_sizes_are_binomial():
    """Seed 0, weights [0.9, 0.1], 100,003 rows: the second split is Binomial(n, 0.1), mean 10,000.3,
    sigma = sqrt(n * 0.1 * 0.9) = 94.9; 6 sigma = 570."""
    n = 100_003
    a = S.assign(0, 0, n, [0.9, 0.1])
    size = int((a == 1).sum())
    print("second split:", size)
    assert abs(size - 0.1 * n) <= 6 * math.sqrt(n * 0.1 * 0.9)
    assert int((a == 0).sum()) + size == n
    assert np.array_equal(a[:1000], S.assign(0, 0, 1000, [0.9, 0.1]))
