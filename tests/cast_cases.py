"""Spark 2.2's Cast(StringType -> LongType | DoubleType) restated on the host, the case tables of
the device string cast (dq_cast_utf8, csrc/cast.hip) and the rules a cast's output must obey
(tests/test_cast_cases.py on the host, tests/test_gpu_cast_rows.py on the device).  Everything here
is plain Python, written from the specifications and not from the engine's parsers:

  spark_to_long      UTF8String.toLong (Spark 2.2): an optional sign (a sign alone is NULL), ASCII
                     digits up to an optional '.', after it ASCII digits only (truncated); nothing
                     is trimmed; overflow is NULL; ".", "-." and ".5" are 0, "" is NULL.  Python
                     integers make the bound check exact.
  java_parse_double  the grammar of java.lang.Double.valueOf's documentation (Cast:
                     `s.toString.toDouble`, NumberFormatException -> NULL): characters <= 0x20
                     trimmed at both ends, a sign, then NaN | Infinity | a hex significand with its
                     mandatory p exponent | decimal digits with at most one '.' and at least one
                     digit, an optional e/E exponent (optional sign, at least one digit); the hex
                     and decimal forms take an optional suffix f F d D.  The value of a decimal form
                     is float(Decimal(text)): the double nearest to the decimal, ties to even
                     (test_cast_cases.py checks that against exact rational arithmetic).
  plain_in_window    the floor of what the device converts: a plain decimal (no exponent, no
                     suffix) whose digits without leading and trailing zeros, d, and the matching
                     power of ten, e, satisfy d <= 2^53 and (|e| <= 22, or e > 22 and
                     d * 10^(e - 22) <= 2^53); zero in any spelling.  Such a value is one correctly
                     rounded fp64 multiply or divide of two exact doubles.

The rules (check_long / check_double), for every row of a cast's output:
  long:    value and validity equal spark_to_long; nothing is ever counted unsupported.
  double:  output valid            => its bits equal the reference's, the sign of zero included;
           output NULL, class NULL => the row is not counted as unsupported;
           output NULL, class VALUE => the row is counted, and plain_in_window is false for it;
           n_unsupported is exactly the number of rows of the last kind.
  both:    a NULL input row stays NULL and is never counted; the value at a NULL row is 0.
The double rules are a floor: a converter that reads more forms (exponents, 17 digits) still passes.
"""
import json
import math
import os
import random
import re
import struct
from decimal import Decimal
from functools import lru_cache

NULL, VALUE = "NULL", "VALUE"
INT64_MIN, INT64_MAX = -(1 << 63), (1 << 63) - 1
P53 = 1 << 53

_GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "cast_known_answers.json")


# ------------------------------------------------------------------------------------------------
# The restatements
# ------------------------------------------------------------------------------------------------
def _ascii_digits(b: bytes) -> bool:
    return all(0x30 <= c <= 0x39 for c in b)


def spark_to_long(b: bytes):
    """UTF8String.toLong: the long, or None where Spark's Cast gives NULL."""
    if not b:
        return None
    signed = b[:1] in (b"-", b"+")
    body = b[1:] if signed else b
    if signed and not body:
        return None
    whole, _, fraction = body.partition(b".")
    if not _ascii_digits(whole) or not _ascii_digits(fraction):
        return None
    v = int(whole.decode("ascii")) if whole else 0
    if b[:1] == b"-":
        v = -v
    return v if INT64_MIN <= v <= INT64_MAX else None


_TRIMMED = bytes(range(0x21))
_SUFFIX = rb"[fFdD]?"
_DECIMAL = re.compile(rb"((?:[0-9]+\.?[0-9]*|\.[0-9]+)(?:[eE][+-]?[0-9]+)?)" + _SUFFIX)
_HEX = re.compile(rb"(0[xX](?:[0-9a-fA-F]+\.?|[0-9a-fA-F]*\.[0-9a-fA-F]+)[pP][+-]?[0-9]+)" + _SUFFIX)


@lru_cache(maxsize=None)
def java_parse_double(b: bytes):
    """(class, value): (NULL, None) where Double.parseDouble throws, else (VALUE, the double)."""
    t = b.strip(_TRIMMED)
    sign = -1.0 if t[:1] == b"-" else 1.0
    if t[:1] in (b"-", b"+"):
        t = t[1:]
    if t == b"NaN":
        return VALUE, math.nan
    if t == b"Infinity":
        return VALUE, sign * math.inf
    m = _HEX.fullmatch(t)
    if m:
        return VALUE, sign * float.fromhex(m.group(1).decode("ascii"))
    m = _DECIMAL.fullmatch(t)
    if m:
        return VALUE, math.copysign(float(Decimal(m.group(1).decode("ascii"))), sign)
    return NULL, None


_PLAIN = re.compile(rb"[+-]?([0-9]*)(?:\.([0-9]*))?")


def plain_in_window(b: bytes) -> bool:
    m = _PLAIN.fullmatch(b.strip(_TRIMMED))
    if not m:
        return False
    whole, fraction = m.group(1), m.group(2) or b""
    if not whole and not fraction:
        return False
    digits = (whole + fraction).lstrip(b"0")
    if not digits:
        return True  # zero, however it is spelled
    kept = digits.rstrip(b"0")
    d, e = int(kept.decode("ascii")), len(digits) - len(kept) - len(fraction)
    if d > P53:
        return False
    return -22 <= e <= 22 or (e > 22 and d * 10 ** (e - 22) <= P53)


# ------------------------------------------------------------------------------------------------
# Case tables (bytes)
# ------------------------------------------------------------------------------------------------
with open(_GOLDEN, encoding="utf-8") as _f:
    KNOWN = json.load(_f)

# the long edges and the Java forms with their hand-derived answers (tests/golden)
LONG_EDGES = [(text.encode("utf-8"), want) for text, want in KNOWN["long_edges"]]
JAVA_FORMS = [(text.encode("utf-8"), cls) for text, cls in KNOWN["java_forms"]]
JAVA_FORM_VALUES = {text.encode("utf-8"): v for text, v in KNOWN["java_form_values"].items()}

IN, OUT, REJECTED = "in the window", "outside the window", "rejected by Java"


def _window_edges():
    """(bytes, tag): tag IN = plain_in_window must hold (the device must convert the row), OUT = a
    decimal parseDouble reads that is deliberately outside the window, REJECTED = class NULL.  The
    tags are set by hand, family by family; test_cast_cases.py checks them against the
    restatements."""
    rows = []

    def add(tag, *texts):
        rows.extend((t.encode("latin-1"), tag) for t in texts)

    for n, tag in ((P53, IN), (P53 - 1, IN), (P53 + 1, OUT)):
        s = str(n)
        add(tag, s, "-" + s, "000" + s, "0" * 40 + s, "0.000" + s)
        add(tag, *[s[:k] + "." + s[k:] for k in range(len(s) + 1)])         # the point everywhere
        add(tag, *[s + "." + "0" * z for z in (1, 5, 22)])                  # zeros after a point
        add(tag, s + "0" * 22, s + "0" * 22 + ".0")                         # e = 22
    add(OUT, str(P53) + "0" * 23, str(P53 - 1) + "0" * 23, "2" + "0" * 38)  # e = 23, no exact rescale
    add(IN, "0." + "0" * 21 + "1", "-0." + "0" * 21 + "1", "0." + "0" * 6 + str(P53))   # e = -22
    add(OUT, "0." + "0" * 22 + "1", "0." + "0" * 7 + str(P53))              # e = -23
    for k in (20, 22, 23, 30, 37):                                          # e > 22: the rescale loop
        add(IN, "1" + "0" * k, "1" + "0" * k + ".0", "-1" + "0" * k + ".0")
    add(OUT, "1" + "0" * 38, "1" + "0" * 38 + ".0")                         # 10^16 > 2^53
    add(IN, "9" + "0" * 36, "9007199254740992" + "0" * 21)
    # the 19-significant-digit cut: the 20th digit zero or not
    add(IN, "9007199254740992000", "90071992547409920000", "9007199254740992000.0",
        "9007199254740.992000000", "1000000000000000000", "10000000000000000000",
        "10000000000000000000.000")
    add(OUT, "1234567890123456789", "12345678901234567890", "12345678901234567891",
        "90071992547409920001", "900719925474099200.01", "10000000000000000000.5",
        "1000000000000000000.5", "9223372036854775807", "18446744073709551616")
    add(IN, "0." + "0" * 30, "0" * 40 + "1.5", "0" * 40, "-0", "-0.0", "+.5", "-0." + "0" * 30,
        "\t1.5 ", "1.5\x00", "\x00\x1f 2.25\r\n", "0.1", "0.3", "123456.789", "4.35", "1.", ".5")
    add(REJECTED, "-.", ".", "+.", "- 1.5", "1 .5", "1.5\x7f", "1.2.3", "")
    return rows


WINDOW_EDGES = _window_edges()


def random_decimals(seed: int, n: int):
    """Plain decimals of at most 17 digits: random point position, leading and trailing zeros, a
    sign.  Most are in the window; 17 digits above 2^53 are not."""
    rng = random.Random(seed)
    out = []
    for _ in range(n):
        digits = "".join(rng.choice("0123456789") for _ in range(rng.randint(1, 17)))
        digits = "0" * rng.choice((0, 0, 0, 1, 3, 8)) + digits + "0" * rng.choice((0, 0, 0, 1, 4, 9))
        k = rng.randint(0, len(digits))
        s = digits if rng.random() < 0.15 else digits[:k] + "." + digits[k:]
        out.append((rng.choice(("", "", "-", "+")) + s).encode("ascii"))
    return out


def random_scaled_decimals(seed: int, n: int):
    """Up to 16 digits pushed to both ends of the window: followed by up to 40 zeros (the rescale of
    exponents above 22) or put behind "0." and up to 24 zeros (exponents down to -40)."""
    rng = random.Random(seed)
    out = []
    for _ in range(n):
        d = str(rng.randint(1, P53 + 4) if rng.random() < 0.3 else rng.randint(1, 10 ** rng.randint(1, 16)))
        if rng.random() < 0.5:
            s = d + "0" * rng.randint(0, 40) + rng.choice(("", ".", ".0", ".000"))
        else:
            s = rng.choice(("0.", ".", "00.")) + "0" * rng.randint(0, 24) + d
        out.append((rng.choice(("", "-")) + s).encode("ascii"))
    return out


def random_soups(seed: int, n: int):
    """Random bytes over 0-9 . + - e d x N space, length 0 to 8."""
    rng = random.Random(seed)
    alphabet = b"0123456789.+-edxN "
    return [bytes(rng.choice(alphabet) for _ in range(rng.randint(0, 8))) for _ in range(n)]


# the tables both suites run, by name
TABLES = {
    "long edges": [b for b, _ in LONG_EDGES],
    "window edges": [b for b, _ in WINDOW_EDGES],
    "java forms": [b for b, _ in JAVA_FORMS],
    "random decimals": random_decimals(11, 3000),
    "scaled decimals": random_scaled_decimals(12, 3000),
    "byte soups": random_soups(13, 4000),
}


# ------------------------------------------------------------------------------------------------
# The rules
# ------------------------------------------------------------------------------------------------
def double_bits(x: float) -> int:
    return struct.unpack("<Q", struct.pack("<d", x))[0]


def check_long(rows, valid, values, n_unsupported):
    """rows: bytes or None (a NULL input row); valid / values: the cast's output per row."""
    assert len(valid) == len(values) == len(rows)
    for i, b in enumerate(rows):
        want = None if b is None else spark_to_long(b)
        got = int(values[i]) if valid[i] else None
        assert got == want, (i, b, got, want)
        assert valid[i] or int(values[i]) == 0, (i, b, "the value at a NULL row is 0")
    assert n_unsupported == 0


def check_double(rows, valid, values, n_unsupported):
    assert len(valid) == len(values) == len(rows)
    counted = 0
    for i, b in enumerate(rows):
        got = float(values[i])
        if not valid[i]:
            assert double_bits(got) == 0, (i, b, got, "the value at a NULL row is +0.0")
        if b is None:
            assert not valid[i], (i, "a NULL input row became a value")
            continue
        cls, ref = java_parse_double(b)
        if valid[i]:
            assert cls == VALUE, (i, b, got, "Java throws NumberFormatException")
            assert double_bits(got) == double_bits(ref) or (got != got and ref != ref), \
                (i, b, got.hex(), ref.hex())
        elif cls == VALUE:
            assert not plain_in_window(b), (i, b, ref, "in the window, but not converted")
            counted += 1
    assert n_unsupported == counted, (n_unsupported, counted)
