"""CPU checks of tests/cast_cases.py (the reference of tests/test_gpu_cast_rows.py) and of the
engine's string-cast parsers run on the host.

  * The restatement's double is the nearest one, ties to even: recomputed for a few thousand
    decimals in exact rational arithmetic, so the reference does not rest on the platform's strtod.
  * Its verdicts on the long edges and the Java forms equal the hand-derived answers of
    tests/golden/cast_known_answers.json.
  * Every row of the window-edge table is tagged in the window, deliberately outside it, or
    rejected by Java, and the tags hold; no table holds a row on which the reference alone breaks a
    rule of cast_cases (a row in the window whose class is not VALUE or whose value is not finite).
  * csrc/cast_parse.h -- the functions cast_utf8_kernel calls per row -- through
    dq_cast_parse_utf8: every table under the rules the device test applies.  This pins the parsing
    and the classification; the device's fp64 multiply and divide are the GPU file's business.
"""
import math
from fractions import Fraction

import numpy as np
import pytest

import cast_cases as CC


def _exact(text: str) -> Fraction:
    """A plain decimal (optional sign, digits, at most one point) as a rational."""
    neg = text[:1] == "-"
    whole, _, fraction = text.lstrip("+-").partition(".")
    q = Fraction(int(whole + fraction), 10 ** len(fraction))
    return -q if neg else q


def _nearest_even(q: Fraction) -> float:
    """The double nearest to q, ties to the even significand, by exact distances: a candidate is
    accepted only when neither of its neighbours is closer."""
    if q == 0:
        return 0.0
    c = q.numerator / q.denominator  # a starting guess only: the loop below corrects it
    for _ in range(4):
        lo, hi = math.nextafter(c, -math.inf), math.nextafter(c, math.inf)
        dc, dlo, dhi = abs(Fraction(c) - q), abs(Fraction(lo) - q), abs(Fraction(hi) - q)
        even = CC.double_bits(c) & 1 == 0
        if dlo < dc or (dlo == dc and not even):
            c = lo
        elif dhi < dc or (dhi == dc and not even):
            c = hi
        else:
            return c
    raise AssertionError(f"no nearest double found for {q}")


def test_nearest_even_helper_on_known_ties():
    assert _nearest_even(Fraction(CC.P53 + 1)) == float(CC.P53)            # tie: even wins (down)
    assert _nearest_even(Fraction(CC.P53 + 3)) == float(CC.P53 + 4)        # tie: even wins (up)
    assert _nearest_even(Fraction(1, 10)) == 0.1
    assert _nearest_even(Fraction(10) ** 23) == 1e23


def test_restatement_value_is_the_nearest_double():
    rows = CC.TABLES["random decimals"] + CC.TABLES["scaled decimals"]
    rows += [b for b, tag in CC.WINDOW_EDGES if tag != CC.REJECTED]
    assert len(rows) > 6000
    for b in rows:
        cls, got = CC.java_parse_double(b)
        assert cls == CC.VALUE, b
        text = b.strip(bytes(range(0x21))).decode("ascii")
        q = _exact(text)
        want = math.copysign(_nearest_even(abs(q)), -1.0 if text[:1] == "-" else 1.0)
        assert CC.double_bits(got) == CC.double_bits(want), (b, got, want)


def test_known_answers():
    for b, want in CC.LONG_EDGES:
        assert CC.spark_to_long(b) == want, b
    for b, cls in CC.JAVA_FORMS:
        assert cls in (CC.NULL, CC.VALUE)
        assert CC.java_parse_double(b)[0] == cls, b
        assert not CC.plain_in_window(b), b
    for b, v in CC.JAVA_FORM_VALUES.items():
        assert CC.java_parse_double(b) == (CC.VALUE, v), b
    assert math.isnan(CC.java_parse_double(b"-NaN")[1])
    assert CC.java_parse_double(b"-Infinity")[1] == -math.inf
    # the issue's list is in the table, with the classes it states
    stated = dict(CC.JAVA_FORMS)
    for text in ("1e", "1e+", "e5", "1.2e.3", "d", "1d2", "fabc", "Nan", "NaNx", "Inf", "0x", "0x1",
                 "1x", "0xp1", "1e5 d"):
        assert stated[text.encode()] == CC.NULL
    for text in ("1e5", "1E-3", "1d", "1f", "NaN", "-NaN", "Infinity", "-Infinity", "0x1p3",
                 "0x1.8p1", "1e5d"):
        assert stated[text.encode()] == CC.VALUE


def test_window_edge_tags_hold():
    tags = {CC.IN: 0, CC.OUT: 0, CC.REJECTED: 0}
    for b, tag in CC.WINDOW_EDGES:
        cls, _ = CC.java_parse_double(b)
        tags[tag] += 1
        if tag == CC.IN:
            assert cls == CC.VALUE and CC.plain_in_window(b), b
        elif tag == CC.OUT:
            assert cls == CC.VALUE and not CC.plain_in_window(b), b
        else:
            assert cls == CC.NULL and not CC.plain_in_window(b), b
    assert min(tags.values()) > 0
    for b in (b"1" + b"0" * 20, b"1" + b"0" * 30 + b".0", str(CC.P53).encode() + b"0" * 22):
        assert (b, CC.IN) in CC.WINDOW_EDGES


@pytest.mark.parametrize("name", list(CC.TABLES))
def test_reference_alone_breaks_no_rule(name):
    for b in CC.TABLES[name]:
        cls, v = CC.java_parse_double(b)
        assert (cls == CC.NULL) == (v is None)
        if CC.plain_in_window(b):
            assert cls == CC.VALUE and math.isfinite(v), b
        # the long and the double agree wherever both read an integer without a point
        n = CC.spark_to_long(b)
        if n is not None and b"." not in b:
            assert cls == CC.VALUE and v == float(n), b


def _host_cast(rows, to_type):
    from deequ_amd import _native as N
    res = [N.cast_parse_utf8(b, to_type) for b in rows]
    valid = [r == 1 for r, _ in res]
    values = np.array([v if r == 1 else 0 for r, v in res],
                      np.int64 if to_type == N.INT64 else np.float64)
    return valid, values, sum(r == 2 for r, _ in res)


@pytest.mark.parametrize("name", list(CC.TABLES))
def test_engine_parsers_on_the_host(name):
    from deequ_amd import _native as N
    rows = CC.TABLES[name]
    valid, values, bad = _host_cast(rows, N.INT64)
    CC.check_long(rows, valid, values, bad)
    valid, values, bad = _host_cast(rows, N.FLOAT64)
    CC.check_double(rows, valid, values, bad)


def test_engine_parsers_tell_null_from_unsupported():
    """Row by row, where the device test can only compare a count: a form Java rejects is 0 (NULL),
    a form it reads is 2 (unsupported) or, should a later build convert it, 1 with Java's value."""
    from deequ_amd import _native as N

    def verdict(b):
        res, got = N.cast_parse_utf8(b, N.FLOAT64)
        cls, ref = CC.java_parse_double(b)
        if res == 1:
            assert cls == CC.VALUE and (CC.double_bits(got) == CC.double_bits(ref) or ref != ref), b
        return res

    for b, cls in CC.JAVA_FORMS:
        for text in (b, b" " + b, b + b"\t", b if b[:1] in (b"+", b"-") else b"-" + b):
            want = CC.java_parse_double(text)[0]
            assert verdict(text) in ((1, 2) if want == CC.VALUE else (0,)), text
    for b, tag in CC.WINDOW_EDGES:
        assert verdict(b) in {CC.IN: (1,), CC.OUT: (1, 2), CC.REJECTED: (0,)}[tag], b
