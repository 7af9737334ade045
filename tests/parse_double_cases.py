"""Case tables for the correctly rounded Double.parseDouble (csrc/parse_double.h), shared by
tests/test_parse_double.py (host) and tests/test_gpu_parse_double.py (device).  Everything is bytes,
built deterministically; the reference for every value is cast_cases.java_parse_double (Python's
float(Decimal(...)) and float.fromhex).

  RANDOM         the three random tables of cast_cases plus random 17- to 19-digit and 20- to 40-digit
                 decimals: mostly rows the fast steps decide, a few that need the exact fallback.
  HALFWAY        for doubles across the exponent range, the midpoint to the next double written out
                 exactly, with its last digit -1 / +1, followed by 50 zeros, followed by 800 zeros and
                 a 1 -- each in plain and in exponent form.
  HARD, HEX      the classic hard strings and the hex forms.
"""
import math
import random
import re
import struct
from decimal import Decimal, getcontext

import cast_cases as CC

getcontext().prec = 2500  # above every exact expansion here (at most 1075 + 17 digits)

_TRIM = bytes(range(0x21))
_PLAIN = re.compile(rb"[+-]?(?:[0-9]+\.?[0-9]*|\.[0-9]+)")


def is_plain(b: bytes) -> bool:
    """A plain decimal: no exponent, no suffix (what the string cast converts)."""
    return _PLAIN.fullmatch(b.strip(_TRIM)) is not None


def same_double(a: float, b: float) -> bool:
    return CC.double_bits(a) == CC.double_bits(b) or (a != a and b != b)


def _from_bits(u: int) -> float:
    return struct.unpack("<d", struct.pack("<Q", u))[0]


def random_long_decimals(seed: int, n: int, lo: int, hi: int):
    """Plain decimals of lo..hi significant digits, the point anywhere (or absent), a sign."""
    rng = random.Random(seed)
    out = []
    for _ in range(n):
        k = rng.randint(lo, hi)
        digits = rng.choice("123456789") + "".join(rng.choice("0123456789") for _ in range(k - 1))
        at = rng.randint(0, k)
        s = digits if rng.random() < 0.2 else digits[:at] + "." + digits[at:]
        out.append((rng.choice(("", "", "-", "+")) + s).encode("ascii"))
    return out


RANDOM = {
    "random decimals": CC.TABLES["random decimals"],
    "scaled decimals": CC.TABLES["scaled decimals"],
    "byte soups": CC.TABLES["byte soups"],
    "17 to 19 digits": random_long_decimals(21, 1500, 17, 19),
    "20 to 40 digits": random_long_decimals(22, 1500, 20, 40),
}


# ------------------------------------------------------------------------------------------------
# Halfway cases
# ------------------------------------------------------------------------------------------------
def halfway_doubles():
    """Positive finite doubles whose upper midpoint is taken: the edges, then random bit patterns
    spread over the exponent range."""
    edges = [5e-324, 1e-323, _from_bits((1 << 52) - 1), _from_bits(1 << 52),           # DBL_MIN
             _from_bits((1 << 52) + 1), 1.0, float(2 ** 53 - 2), float(2 ** 53 - 1),
             float(2 ** 53), float(2 ** 53 + 2), math.nextafter(1.7976931348623157e308, 0.0),
             1.7976931348623157e308, 0.1, 0.3, 1e22, 1e23, 8.41e21, 9e-265]
    rng = random.Random(31)
    rand = [_from_bits((rng.randrange(0, 2047) << 52) | rng.getrandbits(52)) for _ in range(40)]
    rand += [_from_bits(rng.getrandbits(52)) for _ in range(6)]                        # subnormals
    return edges + [d for d in rand if d > 0.0]


def midpoint(d: float):
    """(digits, scale): the midpoint of d and the next double above is int(digits) / 10^scale."""
    up = Decimal(2) ** 1024 if d == 1.7976931348623157e308 else Decimal(math.nextafter(d, math.inf))
    mid = (Decimal(d) + up) / 2
    sign, digits, exp = mid.as_tuple()
    assert sign == 0 and len(digits) < 1200
    text = "".join(map(str, digits))
    if exp > 0:
        text, exp = text + "0" * exp, 0
    return text, -exp


def render_plain(digits: str, scale: int) -> bytes:
    if scale <= 0:
        return (digits + "0" * -scale).encode("ascii")
    digits = digits.rjust(scale + 1, "0")
    return (digits[:-scale] + "." + digits[-scale:]).encode("ascii")


def render_exp(digits: str, scale: int) -> bytes:
    digits = digits.lstrip("0") or "0"
    return f"{digits[0]}.{digits[1:] or '0'}e{len(digits) - 1 - scale}".encode("ascii")


def halfway_variants(d: float):
    """[(digits, scale)]: the exact midpoint above d, its neighbours in the last digit, the same
    midpoint followed by 50 zeros, and by 800 zeros and a 1."""
    digits, scale = midpoint(d)
    return [(digits, scale), (str(int(digits) - 1), scale), (str(int(digits) + 1), scale),
            (digits + "0" * 50, scale + 50), (digits + "0" * 800 + "1", scale + 801)]


def _halfway():
    plain, exp = [], []
    for i, d in enumerate(halfway_doubles()):
        sign = b"-" if i % 3 == 1 else b""
        for digits, scale in halfway_variants(d):
            plain.append(sign + render_plain(digits, scale))
            exp.append(sign + render_exp(digits, scale))
    return plain, exp


HALFWAY_PLAIN, HALFWAY_EXP = _halfway()

_MIN_MID = midpoint(0.0)   # 2^-1075 = 2.4703282292062327...e-324, exactly

HARD = [s.encode("ascii") for s in (
    "2.2250738585072011e-308", "2.2250738585072012e-308", "1.7976931348623158e308",
    "1.7976931348623159e308", "1e309", "1e-324", "4.9e-324", "2.4703282292062327e-324",
    "2.4703282292062328e-324", "0e99999999999", "-0e99999999999", "1" + "0" * 400, "0." + "0" * 400 + "1",
    "-0." + "0" * 400 + "1", "0.30000000000000004", "9007199254740993", "1e23", "8.41e21")]
HARD += [r(*v) for v in halfway_variants(0.0) for r in (render_plain, render_exp)]
assert render_exp(*_MIN_MID).startswith(b"2.4703282292062327208") and \
    render_exp(*_MIN_MID).endswith(b"e-324")

# Exponents that Python's Decimal and float.fromhex refuse, so the reference cannot read them.
# Java has no such limit: a non-zero significand times 10^(+-10^20) or 2^(+-10^20) is out of the
# double range on that side, whatever the significand.
BEYOND_REFERENCE = [(b"1e99999999999999999999", math.inf), (b"1e-99999999999999999999", 0.0),
                    (b"-1e99999999999999999999", -math.inf), (b"-1e-99999999999999999999", -0.0),
                    (b"0." + b"0" * 30 + b"1e+99999999999999999999", math.inf),
                    (b"1" + b"0" * 30 + b"e-99999999999999999999", 0.0),
                    (b"0x1p99999999999999999999", math.inf), (b"0x1p-99999999999999999999", 0.0),
                    (b"-0x.0001p99999999999999999999", -math.inf),
                    (b"0x1000p-99999999999999999999d", 0.0),
                    # float.fromhex raises OverflowError where Java rounds to Infinity: the tie
                    # between DBL_MAX and 2^1024 goes to the even 2^1024, anything above it too
                    (b"0x1.fffffffffffff8p1023", math.inf), (b"-0x1p1024", -math.inf),
                    (b"0x1.fffffffffffff8000001p1023", math.inf)]

HEX = [s.encode("ascii") for s in (
    "0x1p-1074", "0x1p-1075", "0x1.8p-1075", "0x1.0000000001p-1075",
    "0x1.fffffffffffff7ffffp1023", "0x1.fffffffffffffp1023", "0x.8p1", "0X.8P1d", "-0x.8p1f",
    # 20 hex digits: exact ties (to even, both ways), and ties broken by the last digit
    "0x1.00000000000008000000p0", "0x1.00000000000018000000p0", "0x1.00000000000008000001p0",
    "0x1.00000000000017ffffffp0", "0x123456789abcdef08000p0", "0x123456789abcdef18000p0",
    "0x123456789abcdef08001p-300", "0x0.000000000000000000001p0", "0x0p0", "-0x0.0p-5",
    "0x1.8p1", "0x10p-1078",
    "0x1.ffffffffffffep-1023", "0x1.fffffffffffffp-1023", "0x0.fffffffffffff8p-1022")]


def java_forms_padded():
    """Every java_forms entry, bare, signed and padded with bytes <= 0x20."""
    out = []
    for b, _ in CC.JAVA_FORMS:
        out += [b, b" " + b, b + b"\t\n", b"\x00 " + b + b" \x1f", b"-" + b, b" +" + b + b" "]
    return out


ALL = (java_forms_padded() + CC.TABLES["window edges"] + [b for t in RANDOM.values() for b in t]
       + HALFWAY_PLAIN + HALFWAY_EXP + HARD + HEX)
