"""Host checks of tests/format_cases.py, the cases of tests/test_gpu_format_rows.py.  No GPU.

  * the probes pin the text: the oracle's truth vectors of all probes of a family, decoded, give
    the oracle's text of every row back;
  * the host compilation of the printers (jfmt.h, decimal.h through dq_java_doubles_to_strings and
    dq_format_values) gives the oracle's text on every case row, so a failure of the device test
    is the device's alone;
  * each edit a wrong printer would make to one row (last digit up or down, ".0" dropped, "E-"
    printed as "E", a digit fewer, the sign dropped) changes some probe's fingerprint, and a pair
    of such edits leaves all seven patterns of
    test_gpu_pattern_quantile.py::test_pattern_match_floating_point_columns_match_oracle as they were;
  * every probe compiles to at most 255 states, is not nullable, and a full scan's worth of them
    fits the plan's explain() text.
"""
import numpy as np
import pytest

import format_cases as FC
import regex_cases as RC
from oracle import deequ_oracle as O

FAMILIES = FC.family_names()
SEVEN_PATTERNS = [r"\d\.\d", r"E-\d+$", r"^-?\d+\.0$", r"\.\d{6,}", r"^(NaN|-?Infinity)$", r"^-0\.0$", r"9{3}"]


@pytest.mark.parametrize("name", FAMILIES)
def test_probes_pin_the_text_of_every_row(name):
    fam = FC.family(name)
    ps = FC.probes(fam.alphabet, fam.lmax)
    tv = {pr: FC.truth(pr, fam.texts) for pr in ps}
    n = len(fam.texts)
    assert fam.cut % 64 and 0 < fam.cut < n
    assert [r for r, t in enumerate(fam.texts) if t is None] == FC.null_rows(n)
    assert {0, n - 1, fam.cut - 1, fam.cut} <= set(FC.null_rows(n))
    assert n < 64 or {63, 64} <= set(FC.null_rows(n))
    assert n < 257 or {255, 256} <= set(FC.null_rows(n))
    longest = max(len(t) for t in fam.texts if t is not None)
    assert fam.lmax == longest + 1 <= (FC.K_MAX_CHARS if fam.alphabet == FC.FLOAT_ALPHABET else FC.K_FMT_MAX)
    for r, text in enumerate(fam.texts):
        if text is None:
            assert all(v[r] == -1 for v in tv.values())
        else:
            assert FC.decode(fam.alphabet, fam.lmax, lambda pr: tv[pr][r] == 1) == text, (r, fam.raw[r])
    alien = tv[ps[-1]]
    assert ps[-1].what == "alien" and not (alien == 1).any()


def test_the_case_lists_hold_what_they_promise():
    d = FC.family("double")
    texts = set(d.texts)
    # (9.999999999999999e-4 is the double below 0.001: its shortest digits end in 8)
    assert {"0.001", "9.999999999999998E-4", "9999999.999999998", "1.0E7", "1.0E-4", "123456.789", "0.0",
            "-0.0", "NaN", "Infinity", "-Infinity", "4.9E-324", "-4.9E-324", "1.7976931348623157E308",
            "2.2250738585072014E-308", "2.225073858507201E-308", "9.007199254740992E15",
            "-1.2345678901234567E-308"} <= texts
    bits = {FC.d_bits(v) for v in d.values if v is not None}
    assert {e << 52 for e in range(1, 2047)} <= {b & ~(1 << 63) for b in bits}       # every binade edge
    assert {1 << k for k in range(52)} <= {b & ~(1 << 63) for b in bits}             # subnormal 2^k
    assert sum(1 for b in bits if (b >> 52) & 0x7ff == 0x7ff and b & ((1 << 52) - 1)) >= 6   # NaN payloads
    f = FC.family("float")
    fbits = {FC.f_bits(v) for v in f.values if v is not None}
    assert {e << 23 for e in range(1, 255)} <= {b & 0x7fffffff for b in fbits}
    assert set(range(1, 65)) <= fbits
    assert {"1.0E7", "9999999.0", "0.001", "9.999999E-4", "1.6777216E7", "1.4E-45", "3.4028235E38"} <= set(f.texts)
    dec = FC.family("decimal(38,10)")
    assert {"0E-10", "1E-10", "0.0000010000", "1.000E-7", "1844674407.3709551616",
            "-9999999999999999999999999999.9999999999"} <= set(dec.texts)
    assert "0.00" in FC.family("decimal(38,2)").texts
    ts = set(FC.family("timestamp").texts)
    assert {"1969-12-31 23:59:59.999999", "1970-01-01 00:00:00", "1970-01-01 00:00:00.000001",
            "1969-12-31 00:00:00.1", "1970-01-02 00:00:00.12", "0001-01-01 00:00:00",
            "9999-12-31 23:59:59.999999", "2024-02-29 00:00:00"} <= ts
    assert {"0001-01-01", "9999-12-31", "1969-12-31", "2000-02-29", "1900-03-01"} <= set(FC.family("date").texts)
    for fam in FC.families():
        assert 100 < len(fam.values) < 6000, fam.name


@pytest.mark.parametrize("name", FAMILIES)
def test_host_printers_match_the_oracle_on_every_row(name):
    from deequ_amd import _native as N
    fam = FC.family(name)
    live = [r for r in fam.results if r is not None]
    want = [t for t in fam.texts if t is not None]
    if fam.prints in ("double", "float"):
        got = N.java_doubles_to_strings(live, fam.prints == "float")
    elif fam.prints == "date":
        got = N.format_values(N.DATE32, [O.days_of(v) for v in live])
    elif fam.prints == "timestamp":
        got = N.format_values(N.TIMESTAMP_US, [O.micros_of(v) for v in live])
    else:
        p, s = O.decimal_ps(fam.prints)
        got = N.format_values(N.decimal_type(p, s), [O.unscaled(v, s) for v in live])
    bad = [(g, w) for g, w in zip(got, want) if g != w]
    assert not bad, bad[:5]
    if fam.kind == "string":        # the device parses s: the host build of that parser reads it back
        for s, r in zip((v for v in fam.values if v is not None), live):
            got_d = N.parse_double_utf8(s.encode())
            assert got_d is not None and (got_d == r or (got_d != got_d and r != r)), s


def _fingerprints(fam, pr, texts):
    return RC.fingerprint(FC.truth(pr, texts), RC.weights(len(texts)))


@pytest.mark.parametrize("name", FAMILIES)
def test_an_edit_to_one_row_changes_a_fingerprint(name):
    fam = FC.family(name)
    ps = FC.probes(fam.alphabet, fam.lmax)
    applied = set()
    for edit in FC.EDITS:
        hit = next(((r, t, edit(t)) for r, t in enumerate(fam.texts) if t is not None and edit(t) is not None), None)
        if hit is None:
            continue
        r, old, new = hit
        assert new != old
        applied.add(edit.__name__)
        changed = [pr for pr in ps if FC.probe_value(pr, old) != FC.probe_value(pr, new)]
        assert changed, (edit.__name__, old, new)
        edited = fam.texts[:r] + (new,) + fam.texts[r + 1:]
        assert _fingerprints(fam, changed[0], edited)[:2] != _fingerprints(fam, changed[0], fam.texts)[:2]
    if fam.name in ("double", "float", "decimal(38,10)"):      # (a date has no sign, a long no "E-")
        assert len(applied) == len(FC.EDITS), applied
    assert {"edit_last_digit_up", "edit_last_digit_down", "edit_one_digit_fewer"} <= applied


def test_two_edits_that_the_seven_count_patterns_cannot_see():
    """123456.789 printed as 123456.788 and -1.2345678901234567E-308 printed with a digit fewer:
    each of the seven patterns gives both rows the verdict it gave before, so every match count of
    the older test stands; the probes tell both."""
    fam = FC.family("double")
    edits = {"123456.789": FC.edit_last_digit_down, "-1.2345678901234567E-308": FC.edit_one_digit_fewer}
    texts = list(fam.texts)
    for old, edit in edits.items():
        new = edit(old)
        assert new in ("123456.788", "-1.234567890123456E-308")
        for p in SEVEN_PATTERNS:
            assert O.regex_find_nonempty(old, p) == O.regex_find_nonempty(new, p), (old, new, p)
        texts[texts.index(old)] = new
    seen = [pr for pr in FC.probes(fam.alphabet, fam.lmax)
            if _fingerprints(fam, pr, tuple(texts))[:2] != _fingerprints(fam, pr, fam.texts)[:2]]
    print(len(seen), "probes differ")
    assert len(seen) >= 2


SHAPES = sorted({(f.alphabet, f.lmax) for f in FC.families()})


@pytest.mark.parametrize("alphabet,lmax", SHAPES)
def test_every_probe_is_small_and_not_nullable(alphabet, lmax):
    ps = FC.probes(alphabet, lmax)
    assert len(ps) == lmax * len(alphabet).bit_length() + lmax + 1
    assert len({pr.pattern for pr in ps}) == len(ps)
    for pr in ps:
        assert RC.n_states(pr.pattern) <= 255, pr
        assert not RC.is_nullable(pr.pattern), pr


@pytest.mark.parametrize("name", FAMILIES)
def test_a_full_scan_of_probes_fits_explain(name):
    """The plan of the widest chunk (the highest positions, the longest SQL) has every line that
    check_plan counts, as written and under the where filter."""
    from deequ_amd.runners.engine import get_plan
    from deequ_amd.table import Table
    fam = FC.family(name)
    schema = Table.from_arrow(FC.arrow_batches(fam)[0].slice(0, 1), device="cpu").schema
    ps = FC.probes(fam.alphabet, fam.lmax)
    chunk = max(FC.chunks(ps), key=lambda c: (len(c), sum(len(pr.pattern) for pr in c)))
    assert len(chunk) == FC.PROBES_PER_SCAN
    for extra in (None, "g = 0", "id BETWEEN 1000 AND 4000"):
        FC.check_plan(get_plan(schema, FC.scan_specs(fam, chunk, extra)).explain(), len(chunk))


@pytest.mark.parametrize("name", FAMILIES)
def test_arrow_columns_hold_the_case_values(name):
    fam = FC.family(name)
    a, b = FC.arrow_batches(fam)
    assert (a.num_rows, a.num_rows + b.num_rows) == (fam.cut, len(fam.values))
    col = a.column(fam.column).to_pylist() + b.column(fam.column).to_pylist()
    assert [v is None for v in col] == [v is None for v in fam.values]
    if fam.kind == "double":
        raw = np.concatenate([t.column("d").to_numpy(zero_copy_only=False) for t in (a, b)]).view(np.uint64)
        assert all(v is None or int(x) == FC.d_bits(v) for x, v in zip(raw, fam.values))
    elif fam.kind == "float":
        raw = np.concatenate([t.column("f").to_numpy(zero_copy_only=False) for t in (a, b)]).view(np.uint32)
        assert all(v is None or int(x) == FC.f_bits(v) for x, v in zip(raw, fam.values))
    elif fam.kind.startswith("decimal"):
        s = O.decimal_ps(fam.kind)[1]
        assert [None if v is None else O.unscaled(v, s) for v in col] == list(fam.values)
    elif fam.kind == "timestamp":
        assert [None if v is None else v.replace(tzinfo=None) for v in col] == list(fam.values)
    else:
        assert col == list(fam.values)
