"""Host-side checks of tests/regex_cases.py (no GPU): every pattern compiles, the two references
agree on every row, no case passes vacuously, the geometry tables hold the (length, offset) pairs
they claim, the size-edge patterns sit on their sides of the 255-state split, and one flipped row
changes the fingerprint tests/test_gpu_regex_rows.py compares."""
import numpy as np
import pytest

import regex_cases as RC

ALL_CASES = RC.STRING_CASES + RC.NONSTRING_CASES
ALL_IDS = [RC.case_id(c) for c in RC.STRING_CASES] + [RC.ns_case_id(c) for c in RC.NONSTRING_CASES]


def test_every_pattern_compiles():
    """PatternNotSupported (a ValueError) fails the test: no case may be skipped for it."""
    from deequ_amd.regex import compile_java_regex
    for p in sorted({c.pattern for c in ALL_CASES}):
        rx = compile_java_regex(p)
        assert rx.n_states >= 1 and len(rx.blob()) > 16 + 256, p


@pytest.mark.parametrize("c", ALL_CASES, ids=ALL_IDS)
def test_the_two_references_agree_on_every_row(c):
    o, a = RC.oracle_truth(c), RC.automaton_truth(c)
    bad = [i for i, (x, y) in enumerate(zip(o, a)) if x is not y]
    assert not bad, (c.pattern, bad[:10])


@pytest.mark.parametrize("c", ALL_CASES, ids=ALL_IDS)
def test_no_case_is_vacuous(c):
    """TRUE and FALSE rows both occur (and NULL rows where the table has them), except the sets a
    case's construction leaves empty (Case.empty) -- those must be empty."""
    tv = RC.oracle_truth(c)
    for key, v in (("T", True), ("F", False)) + ((("N", None),) if isinstance(c, RC.Case) else ()):
        n = sum(1 for x in tv if x is v)
        assert (n == 0) == (key in c.empty), (c.pattern, key, n)


def test_predicate_spelling_of_a_nullable_pattern():
    assert RC.predicate("s", "\\d*") == ("dq_find_nonempty(s, '\\\\d*')", True)
    assert RC.predicate("s", "q$") == ("s RLIKE 'q$'", False)
    nullable = [c.pattern for c in RC.STRING_CASES if RC.is_nullable(c.pattern)]
    assert nullable == ["\\d*"]


@pytest.mark.parametrize("spec,c", list(zip(RC.GEOMETRY_SPECS, RC.GEOMETRY_CASES)),
                         ids=[s[0] for s in RC.GEOMETRY_SPECS])
def test_geometry_tables_hold_every_length_and_offset(spec, c):
    _, _, filler, plant, decoy = spec
    rows = RC.rows_of(c)
    pb = plant.encode("utf-8")
    seen = set()
    for row, (n, j, kind) in zip(rows, c.meta):
        b = row.encode("utf-8")
        base = RC._fill(filler, n)
        assert len(b) == n
        if kind == "none":
            assert b == base
        else:
            mark = pb if kind == "plant" else decoy.encode("utf-8")
            assert b[j:j + len(mark)] == mark and b[:j] == base[:j] and b[j + len(mark):] == base[j + len(mark):]
        seen.add((n, j, kind))
    assert len(seen) == len(rows) == len(c.meta)
    for n in tuple(range(0, 51)) + (63, 64, 65, 127, 128, 129):
        assert (n, None, "none") in seen
        for j in range(0, n - len(pb) + 1):
            assert (n, j, "plant") in seen
            assert decoy is None or (n, j, "decoy") in seen
    if len(pb) == 1:                                   # every offset 0..L-1
        assert all((n, j, "plant") in seen for n in RC.GEO_LENGTHS for j in range(n))
    if len(pb) > 1:                                    # the plant's bytes straddle 15|16 and 31|32
        for edge in (16, 32):
            for k in range(1, len(pb)):
                assert (50, edge - k, "plant") in seen and (129, edge - k, "plant") in seen


def test_multi_byte_decoys_share_the_stated_prefix():
    assert "é".encode() == b"\xc3\xa9" and "è".encode() == b"\xc3\xa8"
    assert "例".encode() == b"\xe4\xbe\x8b" and "佋".encode() == b"\xe4\xbd\x8b" and "侊".encode() == b"\xe4\xbe\x8a"


def test_buffer_end_batches_end_in_every_length():
    batches = RC.buffer_end_batches()
    last = {len(b[-1].encode()) for b in batches if b[-1] is not None}
    assert last >= set(range(0, 18))
    assert any(b[-1] is None for b in batches)
    assert any(sum(len(r.encode()) for r in b if r is not None) < 16 for b in batches)
    assert any(sum(len(r.encode()) for r in b if r is not None) == 1 for b in batches)


def test_row_count_tables():
    for n in RC.ROW_COUNTS:
        rows = RC.count_rows(n)
        assert len(rows) == n
        if n >= 63:
            for r in [r for r in RC.NULL_ROWS + (n - 1,) if r < n]:
                assert rows[r] is None
                # (rows 63 | 64 and 255 | 256 are NULL side by side: the empty string is beyond)
                assert all(rows[k] in ("", None) for k in (r - 1, r + 1) if 0 <= k < n)
            assert rows[1] == ""
    sizes = {(sum(len(b) for b in c.batches), len(c.batches)) for c in RC.STRING_CASES if c.family == "row count"}
    assert (4099, 1) in sizes and (4099, 5) in sizes and (1025, 2) in sizes and (1, 1) in sizes


def test_divergence_tables():
    batches = RC.divergence_batches()
    assert len(batches) == 8
    for k, b in enumerate(batches):
        assert len(b) == 256
        long_at = [r for r, s in enumerate(b) if len(s) > 3]
        assert long_at == [(k % 4) * 64 + 17 + k] and len(b[long_at[0]]) == RC.LONG_ROW
        assert RC.LONG_ROW - b[long_at[0]].index("q") <= RC.LONG_ROW % 16     # in the last chunk


def test_automaton_sizes_sit_on_their_side_of_the_split():
    """api.cpp fuses a two-instruction program whose automaton has at most kRegexMaxStates = 255
    states; these two must not drift to the other side when the compiler changes."""
    assert RC.n_states(RC.PATTERN_NS_255) == RC.NS_255 == 255
    assert 250 <= RC.NS_255 <= 255 and (RC.NS_255 * 257 + 15) // 16 * 16 == 65536
    assert RC.n_states(RC.PATTERN_NS_263) == RC.NS_263 and 256 <= RC.NS_263 <= 1000
    for c in RC.STRING_CASES:
        if c.family != "automaton size":
            assert RC.n_states(c.pattern) <= 255, c.pattern


def test_nonstring_text_is_the_oracles_cast_to_string():
    from oracle.deequ_oracle import java_to_string
    types = {"i64": "long", "i32": "int", "i16": "short", "i8": "byte", "b": "boolean"}
    for col, (_, vals) in RC.NONSTRING_COLUMNS.items():
        for v in vals:
            if v is not None:
                assert RC.nonstring_text(col, v) == java_to_string(v, types[col]), (col, v)
    assert RC.nonstring_text("i64", RC.I64_MIN) == "-9223372036854775808"


@pytest.mark.parametrize("c", ALL_CASES, ids=ALL_IDS)
def test_one_flipped_row_changes_the_fingerprint(c):
    tv = list(RC.oracle_truth(c))
    w = RC.weights(len(tv))
    assert (w > 0).all() and int(w.sum()) < 2 ** 53
    base = RC.fingerprint(tv, w)
    assert sum(base) == int(w.sum())
    code = RC.truth_code(tv).copy()
    assert RC.fingerprint(code, w) == base
    for i in range(len(code)):
        v = code[i]
        for other in {1, 0, -1} - {int(v)}:
            code[i] = other
            assert RC.fingerprint(code, w) != base, (c.pattern, i)
        code[i] = v
    # and the pair of sums the device reports moves too (sum over TRUE rows, over FALSE rows)
    e = RC.expected(tv, w)
    for i in range(0, len(tv), max(1, len(tv) // 97)):
        if tv[i] is not None:
            flipped = tv[:i] + [not tv[i]] + tv[i + 1:]
            f = RC.expected(flipped, w)
            assert (f["sum_true"], f["sum_false"]) != (e["sum_true"], e["sum_false"])


def test_fingerprint_tells_a_swapped_pair_from_the_original():
    c = RC.GEOMETRY_CASES[2]
    tv = list(RC.oracle_truth(c))
    w = RC.weights(len(tv))
    i, j = tv.index(True), tv.index(False)
    swapped = list(tv)
    swapped[i], swapped[j] = tv[j], tv[i]
    assert sum(1 for v in swapped if v) == sum(1 for v in tv if v)
    assert RC.fingerprint(swapped, w) != RC.fingerprint(tv, w)
    sel = np.arange(len(tv)) % 8 == 0
    assert RC.fingerprint(tv, w, sel)[0] <= RC.fingerprint(tv, w)[0]
