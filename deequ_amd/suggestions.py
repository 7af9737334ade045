"""Constraint suggestion (reference: suggestions/ConstraintSuggestionRunner.scala,
ConstraintSuggestionRunBuilder.scala, ConstraintSuggestion.scala, ConstraintSuggestionResult.scala,
suggestions/rules/*.scala): profile a table, turn the profiles into candidate constraints by rule,
and optionally evaluate the suggested check on a random hold-out of the rows.

The profile is ColumnProfiler's three device passes, the hold-out is Table.random_split (a device
draw, dq_split_rows, over the engine's select and gather), the evaluation a VerificationSuite run;
the rules themselves are host code over a handful of numbers per column.

Two places where a profile of this engine differs from Spark's:
  * approximate_num_distinct_values is None in the HLL++ bias range (the bias tables are not part
    of this build); UniqueIfApproximatelyUniqueRule does not apply to such a profile.
  * the categorical rules drop the histogram key "NullValue" (Histogram.NullFieldReplacement) as
    the reference does, so a column whose real value is that string loses it too.
"""
from __future__ import annotations

import json
import math
import os
from dataclasses import dataclass
from decimal import ROUND_DOWN, Decimal
from typing import Dict, List, Optional, Sequence

from .analyzers.datatype import DataTypeInstances
from .analyzers.grouping import NULL_FIELD_REPLACEMENT
from .checks import (IS_ONE, Check, CheckLevel, ConstrainableDataTypes, Constraint, _scala_str)
from .profiles import (DEFAULT_CARDINALITY_THRESHOLD, ColumnProfiler, ColumnProfiles,
                       NumericColumnProfile, StandardColumnProfile)
from .verification import VerificationResult, VerificationSuite


def escape_java(s: str) -> str:
    """StringEscapeUtils.escapeJava (commons-lang3): \" and \\ take a backslash, \\b \\t \\n \\f \\r go by
    name, every other char below 0x20 or above 0x7f becomes \\uXXXX (upper-case hex), one escape per
    UTF-16 unit."""
    named = {'"': '\\"', "\\": "\\\\", "\b": "\\b", "\t": "\\t", "\n": "\\n", "\f": "\\f",
             "\r": "\\r"}
    out = []
    for ch in s:
        if ch in named:
            out.append(named[ch])
            continue
        cp = ord(ch)
        if 0x20 <= cp <= 0x7f:
            out.append(ch)
        elif cp < 0x10000:
            out.append(f"\\u{cp:04X}")
        else:
            cp -= 0x10000
            out.append(f"\\u{0xD800 + (cp >> 10):04X}\\u{0xDC00 + (cp & 0x3FF):04X}")
    return "".join(out)


def gson_pretty(obj) -> str:
    """new GsonBuilder().setPrettyPrinting().create().toJson(obj): two-space indentation, and Gson's
    default HTML-safe escapes of < > & = ' (and U+2028 / U+2029) inside strings; other non-ASCII
    text is written as it is.  None of those characters occurs in JSON outside a string."""
    text = json.dumps(obj, indent=2, ensure_ascii=False)
    for ch in "<>&='\u2028\u2029":
        text = text.replace(ch, f"\\u{ord(ch):04x}")
    return text


def _lower_bound(p: float, n: int) -> float:
    """BigDecimal(p - z * sqrt(p (1 - p) / n)).setScale(2, RoundingMode.DOWN).toDouble, z = 1.96.
    Scala's BigDecimal(Double) reads the double's shortest decimal string."""
    z = 1.96
    x = p - z * math.sqrt(p * (1 - p) / n)
    return float(Decimal(repr(x)).quantize(Decimal("0.01"), rounding=ROUND_DOWN))


def _constraint(check_method: str, *args, **kwargs) -> Constraint:
    """The constraint the Check DSL builds for these arguments (so its toString is the DSL's)."""
    check = getattr(Check(CheckLevel.Warning, "suggestion"), check_method)(*args, **kwargs)
    return check.constraints[-1]


@dataclass(frozen=True)
class ConstraintSuggestion:
    """ConstraintSuggestion.scala:25-32."""
    constraint: Constraint
    column_name: str
    current_value: str
    description: str
    suggesting_rule: "ConstraintRule"
    code_for_constraint: str


class ConstraintRule:
    """rules/ConstraintRule.scala: decides per column profile whether it applies, and builds the
    candidate."""
    rule_description: str = ""

    def should_be_applied(self, profile: StandardColumnProfile, num_records: int) -> bool:
        raise NotImplementedError

    def candidate(self, profile: StandardColumnProfile, num_records: int) -> ConstraintSuggestion:
        raise NotImplementedError


@dataclass(frozen=True)
class CompleteIfCompleteRule(ConstraintRule):
    """If a column is complete in the sample, we suggest a NOT NULL constraint."""
    rule_description = ("If a column is complete in the sample, we suggest a NOT NULL constraint")

    def should_be_applied(self, profile, num_records):
        return profile.completeness == 1.0

    def candidate(self, profile, num_records):
        return ConstraintSuggestion(
            _constraint("has_completeness", profile.column, IS_ONE), profile.column,
            "Completeness: " + _scala_str(float(profile.completeness)),
            f"'{profile.column}' is not null", self, f'.isComplete("{profile.column}")')


@dataclass(frozen=True)
class RetainCompletenessRule(ConstraintRule):
    """An incomplete column's completeness as a binomial variable: the lower end of its confidence
    interval becomes the bound."""
    rule_description = ("If a column is incomplete in the sample, we model its completeness as a "
                        "binomial variable, estimate a confidence interval and use this to define "
                        "a lower bound for the completeness")

    def should_be_applied(self, profile, num_records):
        return 0.2 < profile.completeness < 1.0

    def candidate(self, profile, num_records):
        target = _lower_bound(profile.completeness, num_records)
        bound_in_percent = int((1.0 - target) * 100)  # .toInt truncates
        t = _scala_str(target)
        return ConstraintSuggestion(
            _constraint("has_completeness", profile.column, lambda v: v >= target), profile.column,
            "Completeness: " + _scala_str(float(profile.completeness)),
            f"'{profile.column}' has less than {bound_in_percent}% missing values", self,
            f'.hasCompleteness("{profile.column}", _ >= {t}, Some("It should be above {t}!"))')


@dataclass(frozen=True)
class UniqueIfApproximatelyUniqueRule(ConstraintRule):
    """A complete column whose approximate distinct count is within the HLL sketch's error of the
    number of records gets a UNIQUE constraint."""
    rule_description = ("If the ratio of approximate num distinct values in a column is close to "
                        "the number of records (within the error of the HLL sketch), we suggest a "
                        "UNIQUE constraint")

    def should_be_applied(self, profile, num_records):
        if profile.approximate_num_distinct_values is None:  # HLL++ bias range: no number
            return False
        distinctness = float(profile.approximate_num_distinct_values) / num_records
        return profile.completeness == 1.0 and abs(1.0 - distinctness) <= 0.08

    def candidate(self, profile, num_records):
        if profile.approximate_num_distinct_values is None:
            raise ValueError(f"column {profile.column}: no approximate distinct count")
        distinctness = float(profile.approximate_num_distinct_values) / num_records
        return ConstraintSuggestion(
            _constraint("has_uniqueness", [profile.column], IS_ONE), profile.column,
            "ApproxDistinctness: " + _scala_str(distinctness), f"'{profile.column}' is unique",
            self, f'.isUnique("{profile.column}")')


@dataclass(frozen=True)
class RetainTypeRule(ConstraintRule):
    """If we detect a non-string type, we suggest a type constraint."""
    rule_description = "If we detect a non-string type, we suggest a type constraint"

    _TESTABLE = (DataTypeInstances.Integral, DataTypeInstances.Fractional, DataTypeInstances.Boolean)

    def should_be_applied(self, profile, num_records):
        return bool(profile.is_data_type_inferred) and profile.data_type in self._TESTABLE

    def candidate(self, profile, num_records):
        if profile.data_type not in self._TESTABLE:
            raise ValueError(f"column {profile.column}: no type constraint for {profile.data_type.name}")
        name = profile.data_type.name
        return ConstraintSuggestion(
            _constraint("has_data_type", profile.column, ConstrainableDataTypes[name], IS_ONE),
            profile.column, "DataType: " + name, f"'{profile.column}' has type {name}", self,
            f'.hasDataType("{profile.column}", ConstrainableDataTypes.{name})')


def _unique_value_ratio(profile) -> Optional[float]:
    """Unique entries / entries of a String column's histogram; None without one."""
    if profile.histogram is None or profile.data_type != DataTypeInstances.String:
        return None
    entries = profile.histogram.values
    unique = sum(1 for v in entries.values() if v.absolute == 1)
    return unique / len(entries) if entries else float("nan")  # (0.0 / 0: every comparison false)


def _category_lists(items) -> tuple:
    """(SQL list, code list) of the categories by falling popularity: sortBy(absolute).reverse, the
    NULL replacement dropped; ' doubled in SQL, escapeJava in code."""
    by_popularity = sorted(((k, v) for k, v in items if k != NULL_FIELD_REPLACEMENT),
                           key=lambda kv: kv[1].absolute)[::-1]
    sql = "'" + "', '".join(k.replace("'", "''") for k, _ in by_popularity) + "'"
    code = '"' + '", "'.join(escape_java(k) for k, _ in by_popularity) + '"'
    return sql, code


@dataclass(frozen=True)
class CategoricalRangeRule(ConstraintRule):
    """If we see a categorical range for a column, we suggest an IS IN (...) constraint."""
    rule_description = ("If we see a categorical range for a column, we suggest an IS IN (...) "
                        "constraint")

    def should_be_applied(self, profile, num_records):
        ratio = _unique_value_ratio(profile)
        return ratio is not None and ratio <= 0.1

    def candidate(self, profile, num_records):
        sql, code = _category_lists(profile.histogram.values.items())
        description = f"'{profile.column}' has value range {sql}"
        return ConstraintSuggestion(
            _constraint("satisfies", f"{profile.column} IN ({sql})", description, IS_ONE),
            profile.column, "Compliance: 1", description, self,
            f'.isContainedIn("{profile.column}", Array({code}))')


@dataclass(frozen=True)
class FractionalCategoricalRangeRule(ConstraintRule):
    """If we see a categorical range for most values in a column, we suggest an IS IN (...)
    constraint that should hold for most values."""
    target_data_coverage_fraction: float = 0.9
    rule_description = ("If we see a categorical range for most values in a column, we suggest an "
                        "IS IN (...) constraint that should hold for most values")

    def _top_categories(self, profile) -> list:
        by_ratio = sorted(profile.histogram.values.items(), key=lambda kv: kv[1].ratio)[::-1]
        coverage, out = 0.0, []
        for k, v in by_ratio:
            if coverage < self.target_data_coverage_fraction:
                coverage += v.ratio
                out.append((k, v))
        return out

    def should_be_applied(self, profile, num_records):
        ratio = _unique_value_ratio(profile)
        if ratio is None:
            return False
        ratio_sums = sum(v.ratio for _, v in self._top_categories(profile))
        return ratio <= 0.4 and ratio_sums < 1

    def candidate(self, profile, num_records):
        top = self._top_categories(profile)
        ratio_sums = sum(v.ratio for _, v in top)
        sql, code = _category_lists(top)
        target = _lower_bound(ratio_sums, num_records)
        t = _scala_str(target)
        description = (f"'{profile.column}' has value range {sql} for at least "
                       f"{_scala_str(target * 100)}% of values")
        hint = f"It should be above {t}!"
        return ConstraintSuggestion(
            _constraint("satisfies", f"{profile.column} IN ({sql})", description,
                        lambda v: v >= target, hint),
            profile.column, "Compliance: " + _scala_str(float(ratio_sums)), description, self,
            f'.isContainedIn("{profile.column}", Array({code}), _ >= {t}, Some("{hint}"))')


def _minimum_text(profile) -> str:
    if isinstance(profile, NumericColumnProfile) and profile.minimum is not None:
        return _scala_str(float(profile.minimum))
    return "Error while calculating minimum!"


@dataclass(frozen=True)
class NonNegativeNumbersRule(ConstraintRule):
    """If we see only non-negative numbers in a column, we suggest a corresponding constraint."""
    rule_description = ("If we see only non-negative numbers in a column, we suggest a "
                        "corresponding constraint")

    def should_be_applied(self, profile, num_records):
        return (isinstance(profile, NumericColumnProfile) and profile.minimum is not None
                and profile.minimum == 0.0)

    def candidate(self, profile, num_records):
        description = f"'{profile.column}' has no negative values"
        return ConstraintSuggestion(
            _constraint("satisfies", f"{profile.column} >= 0", description, IS_ONE), profile.column,
            "Minimum: " + _minimum_text(profile), description, self,
            f'.isNonNegative("{profile.column}")')


@dataclass(frozen=True)
class PositiveNumbersRule(ConstraintRule):
    """If we see only positive numbers in a column, we suggest a corresponding constraint."""
    rule_description = ("If we see only positive numbers in a column, we suggest a corresponding "
                        "constraint")

    def should_be_applied(self, profile, num_records):
        return (isinstance(profile, NumericColumnProfile) and profile.minimum is not None
                and profile.minimum > 0.0)

    def candidate(self, profile, num_records):
        description = f"'{profile.column}' has only positive values"
        return ConstraintSuggestion(
            _constraint("satisfies", f"{profile.column} > 0", description, IS_ONE), profile.column,
            "Minimum: " + _minimum_text(profile), description, self,
            f'.isPositive("{profile.column}")')


class Rules:
    """ConstraintSuggestionRunner.scala:32-38."""
    DEFAULT: Sequence[ConstraintRule] = (
        CompleteIfCompleteRule(), RetainCompletenessRule(), UniqueIfApproximatelyUniqueRule(),
        RetainTypeRule(), CategoricalRangeRule(), FractionalCategoricalRangeRule(),
        NonNegativeNumbersRule(), PositiveNumbersRule())


class ConstraintSuggestions:
    """ConstraintSuggestion.scala:34-109: the two JSON documents."""
    FIELD = "constraint_suggestions"

    @staticmethod
    def _shared(s: ConstraintSuggestion) -> dict:
        return {"constraint_name": str(s.constraint), "column_name": s.column_name,
                "current_value": s.current_value, "description": s.description,
                "suggesting_rule": type(s.suggesting_rule).__name__,
                "rule_description": s.suggesting_rule.rule_description,
                "code_for_constraint": s.code_for_constraint}

    @staticmethod
    def to_json(suggestions: Sequence[ConstraintSuggestion]) -> str:
        return gson_pretty({ConstraintSuggestions.FIELD:
                            [ConstraintSuggestions._shared(s) for s in suggestions]})

    @staticmethod
    def evaluation_results_to_json(suggestions: Sequence[ConstraintSuggestion],
                                   result: VerificationResult) -> str:
        constraint_results = next(iter(result.check_results.values())).constraint_results
        rows = []
        for s, r in zip(suggestions, constraint_results):
            row = ConstraintSuggestions._shared(s)
            row["constraint_result"] = r.status.value
            rows.append(row)
        return gson_pretty({ConstraintSuggestions.FIELD: rows})


@dataclass
class ConstraintSuggestionResult:
    """ConstraintSuggestionResult.scala: the profiles, the suggestions per column, and the
    verification result when a train/test split was used."""
    column_profiles: Dict[str, StandardColumnProfile]
    constraint_suggestions: Dict[str, List[ConstraintSuggestion]]
    verification_result: Optional[VerificationResult] = None

    def _all_suggestions(self) -> List[ConstraintSuggestion]:
        return [s for group in self.constraint_suggestions.values() for s in group]

    @staticmethod
    def get_column_profiles_as_json(result: "ConstraintSuggestionResult") -> str:
        return ColumnProfiles.to_json(list(result.column_profiles.values()))

    @staticmethod
    def get_constraint_suggestions_as_json(result: "ConstraintSuggestionResult") -> str:
        return ConstraintSuggestions.to_json(result._all_suggestions())

    @staticmethod
    def get_evaluation_results_as_json(result: "ConstraintSuggestionResult") -> str:
        if result.verification_result is not None:
            return ConstraintSuggestions.evaluation_results_to_json(result._all_suggestions(),
                                                                    result.verification_result)
        return ConstraintSuggestionResult.get_column_profiles_as_json(result)  # (as the reference)


def _write(path: str, text: str, overwrite: bool) -> None:
    if os.path.exists(path) and not overwrite:
        raise FileExistsError(f"{path} already exists")
    with open(path, "w", encoding="utf-8") as fh:
        fh.write(text + "\n")


class ConstraintSuggestionRunBuilder:
    """ConstraintSuggestionRunBuilder.scala (no Spark session: the save paths are local paths, as
    in ColumnProfilerRunBuilder)."""

    def __init__(self, data):
        self.data = data
        self._rules: List[ConstraintRule] = []
        self._print = False
        self._testset_ratio: Optional[float] = None
        self._testset_seed: Optional[int] = None
        self._threshold = DEFAULT_CARDINALITY_THRESHOLD
        self._columns: Optional[List[str]] = None
        self._repository = None
        self._reuse_key = None
        self._fail_if_missing = False
        self._save_key = None
        self._overwrite = False
        self._profiles_path: Optional[str] = None
        self._suggestions_path: Optional[str] = None
        self._evaluation_path: Optional[str] = None

    def add_constraint_rule(self, rule: ConstraintRule):
        self._rules.append(rule)
        return self

    def add_constraint_rules(self, rules: Sequence[ConstraintRule]):
        self._rules.extend(rules)
        return self

    def print_status_updates(self, flag: bool):
        self._print = flag
        return self

    def cache_inputs(self, _flag: bool):  # the table is already resident in HBM
        return self

    def use_train_test_split_with_testset_ratio(self, testset_ratio: float,
                                                testset_split_random_seed: Optional[int] = None):
        self._testset_ratio = testset_ratio
        self._testset_seed = testset_split_random_seed
        return self

    def with_low_cardinality_histogram_threshold(self, threshold: int):
        self._threshold = threshold
        return self

    def only_consider_column_subset(self, columns: Sequence[str]):
        self._columns = list(columns)
        return self

    def use_repository(self, repository):
        self._repository = repository
        return self

    def reuse_existing_results_for_key(self, key, fail_if_results_missing: bool = False):
        self._reuse_key = key
        self._fail_if_missing = fail_if_results_missing
        return self

    def save_or_append_result(self, key):
        self._save_key = key
        return self

    def save_column_profiles_json_to_path(self, path: str):
        self._profiles_path = path
        return self

    def save_constraint_suggestions_json_to_path(self, path: str):
        self._suggestions_path = path
        return self

    def save_evaluation_results_json_to_path(self, path: str):
        self._evaluation_path = path
        return self

    def overwrite_previous_files(self, flag: bool):
        self._overwrite = flag
        return self

    def run(self) -> ConstraintSuggestionResult:
        """ConstraintSuggestionRunner.run (ConstraintSuggestionRunner.scala:61-139)."""
        ratio = self._testset_ratio
        if ratio is not None and not (ratio > 0 and ratio < 1.0):
            raise ValueError("requirement failed: Testset ratio must be in ]0, 1[")
        training, test = self.data, None
        if ratio is not None:
            training, test = self.data.random_split([1.0 - ratio, ratio], self._testset_seed)
        profiles, suggestions = ConstraintSuggestionRunner.profile_and_suggest(
            training, self._rules, self._columns, self._threshold, self._print, self._repository,
            self._reuse_key, self._fail_if_missing, self._save_key)
        if self._profiles_path is not None:
            if self._print:
                print(f"### WRITING COLUMN PROFILES TO {self._profiles_path}")
            _write(self._profiles_path, ColumnProfiles.to_json(list(profiles.profiles.values())),
                   self._overwrite)
        if self._suggestions_path is not None:
            if self._print:
                print(f"### WRITING CONSTRAINTS TO {self._suggestions_path}")
            _write(self._suggestions_path, ConstraintSuggestions.to_json(suggestions), self._overwrite)
        verification = None
        if test is not None:
            if self._print:
                print("### RUNNING EVALUATION")
            check = Check(CheckLevel.Warning, "generated constraints",
                          [s.constraint for s in suggestions])
            verification = VerificationSuite().on_data(test).add_check(check).run()
            if self._evaluation_path is not None:
                if self._print:
                    print(f"### WRITING EVALUATION RESULTS TO {self._evaluation_path}")
                _write(self._evaluation_path,
                       ConstraintSuggestions.evaluation_results_to_json(suggestions, verification),
                       self._overwrite)
        by_column: Dict[str, List[ConstraintSuggestion]] = {}
        for s in suggestions:
            by_column.setdefault(s.column_name, []).append(s)
        return ConstraintSuggestionResult(profiles.profiles, by_column, verification)


class ConstraintSuggestionRunner:
    def on_data(self, data) -> ConstraintSuggestionRunBuilder:
        return ConstraintSuggestionRunBuilder(data)

    @staticmethod
    def profile_and_suggest(training, rules, from_columns, threshold, print_status_updates,
                            repository=None, reuse_key=None, fail_if_missing=False, save_key=None):
        """profileAndSuggest / applyRules (ConstraintSuggestionRunner.scala:141-182): the rules in
        column order, then rule order."""
        columns = list(from_columns) if from_columns is not None else training.schema.field_names
        profiles = ColumnProfiler.profile(
            training, columns, print_status_updates, threshold, metrics_repository=repository,
            reuse_existing_results_using_key=reuse_key,
            fail_if_results_for_reusing_missing=fail_if_missing,
            save_in_metrics_repository_using_key=save_key)
        suggestions = []
        for column in columns:
            profile = profiles.profiles.get(column)
            if profile is None:
                continue
            suggestions += [r.candidate(profile, profiles.num_records) for r in rules
                            if r.should_be_applied(profile, profiles.num_records)]
        return profiles, suggestions


__all__ = ["ConstraintRule", "CompleteIfCompleteRule", "RetainCompletenessRule", "RetainTypeRule",
           "CategoricalRangeRule", "FractionalCategoricalRangeRule", "NonNegativeNumbersRule",
           "PositiveNumbersRule", "UniqueIfApproximatelyUniqueRule", "Rules", "ConstraintSuggestion",
           "ConstraintSuggestions", "ConstraintSuggestionResult", "ConstraintSuggestionRunner",
           "ConstraintSuggestionRunBuilder", "escape_java", "gson_pretty"]
