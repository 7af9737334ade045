"""The correctly rounded Double.parseDouble of csrc/parse_double.h on the host, through
dq_parse_double_utf8 (the complete parser: every form) and dq_cast_parse_utf8 (the string cast's
three-way verdict).  The reference is cast_cases.java_parse_double: float(Decimal(text)) for decimal
forms and float.fromhex for hex forms.

Values: bit equality, the sign of zero and NaN-ness included, over parse_double_cases.ALL -- the
Java forms bare, signed and padded, the window edges, the random tables, exact halfway cases with
their neighbours in plain and exponent form, the classic hard strings, the hex forms.
Verdicts: the cast converts every plain decimal (1), reports every other form Java reads (2), and
both entries give NULL exactly where Java throws.
Fallback coverage: over the random tables the exact fallback is reached, but by fewer than one row
in ten, so neither a broken fallback nor a broken fast path can hide; every halfway string of more
than 19 digits reaches it.  (Measured when the tables were fixed: 5 of 13000 random rows.)  Exponents of twenty digits and
hex strings above DBL_MAX, which the Python reference refuses, have their answers stated with the
reason in parse_double_cases.BEYOND_REFERENCE.
The committed pow5_128.h equals its generator's output.
"""
import os
import sys

import pytest

import cast_cases as CC
import parse_double_cases as PD

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def N():
    from deequ_amd import _native
    return _native


def _check_value(N, b):
    cls, ref = CC.java_parse_double(b)
    got = N.parse_double_utf8(b)
    if cls == CC.NULL:
        assert got is None, (b[:60], got)
    else:
        assert got is not None, (b[:60], "NumberFormatException, Java reads", ref)
        assert PD.same_double(got, ref), (b[:60], len(b), got.hex(), ref.hex())


def test_reference_reads_the_pinned_java_forms():
    """The reference agrees with the hand-derived classes and values in tests/golden."""
    for b, cls in CC.JAVA_FORMS:
        assert CC.java_parse_double(b)[0] == cls, b
    for b, v in CC.JAVA_FORM_VALUES.items():
        assert PD.same_double(CC.java_parse_double(b)[1], float(v)), b


@pytest.mark.parametrize("name", ["java forms", "window edges", *PD.RANDOM, "halfway plain",
                                  "halfway exponent", "hard", "hex"])
def test_values(name, N):
    rows = {"java forms": PD.java_forms_padded(), "window edges": CC.TABLES["window edges"],
            "halfway plain": PD.HALFWAY_PLAIN, "halfway exponent": PD.HALFWAY_EXP,
            "hard": PD.HARD, "hex": PD.HEX, **PD.RANDOM}[name]
    assert len(rows) > 20
    for b in rows:
        _check_value(N, b)


def test_named_answers(N):
    inf = float("inf")
    for text, want in [("2.2250738585072011e-308", 2.225073858507201e-308),
                       ("2.2250738585072012e-308", 2.2250738585072014e-308),
                       ("1.7976931348623158e308", 1.7976931348623157e308),
                       ("1.7976931348623159e308", inf), ("1e309", inf), ("-1e309", -inf),
                       ("1e-324", 0.0), ("-1e-324", -0.0), ("4.9e-324", 5e-324),
                       ("2.4703282292062327e-324", 0.0), ("2.4703282292062328e-324", 5e-324),
                       ("0e99999999999", 0.0), ("-0e99999999999", -0.0), ("1" + "0" * 400, inf),
                       ("0." + "0" * 400 + "1", 0.0), ("0x1p-1074", 5e-324), ("0x1p-1075", 0.0),
                       ("0x1.8p-1075", 5e-324), ("0x1.fffffffffffff8p1023", inf), ("0x.8p1", 1.0),
                       ("0.30000000000000004", 0.1 + 0.2), ("9007199254740993", 9007199254740992.0),
                       ("Infinity", inf), ("-Infinity", -inf), (" 1.5d ", 1.5), ("1e2f", 100.0)]:
        got = N.parse_double_utf8(text.encode())
        assert got is not None and CC.double_bits(got) == CC.double_bits(want), (text[:40], got, want)
    for b, want in PD.BEYOND_REFERENCE:
        got = N.parse_double_utf8(b)
        assert got is not None and CC.double_bits(got) == CC.double_bits(want), (b, got, want)
        assert N.cast_parse_utf8(b, N.FLOAT64) == (2, None)
    assert N.parse_double_utf8(b"NaN") != N.parse_double_utf8(b"NaN")
    for text in ("", " ", "1e", "e5", "0x1", "0x1.p", "1d2", "nan", "inf", "1_0", "1.2.3", "0xp1",
                 "+-1", "1e+", "1 e5", "NaNd", "Infinityf"):
        assert N.parse_double_utf8(text.encode()) is None, text


def test_cast_verdicts(N):
    seen = {0: 0, 1: 0, 2: 0}
    for b in PD.ALL:
        cls, ref = CC.java_parse_double(b)
        res, got = N.cast_parse_utf8(b, N.FLOAT64)
        want = 0 if cls == CC.NULL else 1 if PD.is_plain(b) else 2
        assert res == want, (b[:60], res, want)
        assert (N.parse_double_utf8(b) is None) == (cls == CC.NULL), b[:60]
        if res == 1:
            assert PD.same_double(got, ref), (b[:60], got.hex(), ref.hex())
        else:
            assert got is None
        seen[res] += 1
    print("verdicts:", seen)
    assert min(seen.values()) > 100


def test_fallback_coverage(N):
    def reached(rows):
        before = N.parse_double_fallbacks()
        for b in rows:
            N.parse_double_utf8(b)
        return N.parse_double_fallbacks() - before

    rows = [b for t in PD.RANDOM.values() for b in t]
    n = reached(rows)
    print("random tables:", n, "of", len(rows), "rows through the exact fallback")
    assert 0 < n < len(rows) / 10
    assert reached(CC.TABLES["window edges"] + PD.RANDOM["17 to 19 digits"]) == 0
    # every halfway string here has more than 19 significant digits, and w / w + 1 straddle it
    long_halfway = [b for b in PD.HALFWAY_PLAIN + PD.HALFWAY_EXP
                    if sum(c in b"0123456789" for c in b.split(b"e")[0].lstrip(b"-0.")) > 19
                    and CC.java_parse_double(b)[1] not in (float("inf"), -float("inf"))]
    assert len(long_halfway) > 400
    assert reached(long_halfway) >= len(long_halfway) * 0.9


def test_generated_header_is_current():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        import gen_pow5_128
    finally:
        sys.path.pop(0)
    with open(os.path.join(ROOT, "deequ_amd", "csrc", "pow5_128.h"), encoding="ascii") as f:
        assert f.read() == gen_pow5_128.text()
