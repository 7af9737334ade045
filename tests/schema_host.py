"""Plain-Python restatement of RowLevelSchemaValidator (helper, not a test), written from
src/main/scala/com/amazon/deequ/schema/RowLevelSchemaValidator.scala (R/ below) and Spark 2.2's
Cast; the device path (deequ_amd/schema.py over csrc/rowschema.hip) is compared with it row for row.

A schema is a list of dicts as in tests/golden/schema_known_answers.json:
  {"kind": "int", "name", "is_nullable", "min_value", "max_value"}
  {"kind": "string", "name", "is_nullable", "min_length", "max_length", "matches"}
  {"kind": "decimal", "name", "is_nullable", "precision", "scale"}
  {"kind": "timestamp", "name", "is_nullable", "mask"}
Values are Python str or None.  Three-valued logic: True / False / None.
"""
import calendar
import decimal
import re

UNSUPPORTED = "UNSUPPORTED"  # a value whose outcome under Java is not decided (never guessed)


# ------------------------------------------------------------------------------------------------
# Kleene logic (Catalyst's And / Or)
# ------------------------------------------------------------------------------------------------
def k_and(a, b):
    if a is False or b is False:
        return False
    if a is None or b is None:
        return None
    return True


def k_or(a, b):
    if a is True or b is True:
        return True
    if a is None or b is None:
        return None
    return False


# ------------------------------------------------------------------------------------------------
# Casts
# ------------------------------------------------------------------------------------------------
def cast_int(v):
    """Spark 2.2 UTF8String.toInt (Cast StringType -> IntegerType, R/:47, :240): optional sign,
    digits, optionally '.' and digits (truncated), no trimming; None = NULL."""
    if v is None:
        return None
    b = v.encode("utf-8")
    m = re.fullmatch(rb"([+-]?)([0-9]*)(\.[0-9]*)?", b)
    if not m or len(b) == 0 or b in (b"+", b"-"):
        return None
    # a sign must be followed by at least one more byte (checked above); "." alone reads as 0
    n = int(m.group(2) or b"0")
    if m.group(1) == b"-":
        n = -n
    return n if -2**31 <= n <= 2**31 - 1 else None


_DEC_GRAMMAR = re.compile(r"[+-]?([0-9]+(\.[0-9]*)?|\.[0-9]+)([eE][+-]?([0-9]+))?", re.ASCII)
_DEC_CTX = decimal.Context(prec=12000, rounding=decimal.ROUND_HALF_UP, Emax=decimal.MAX_EMAX,
                           Emin=decimal.MIN_EMIN)


def cast_decimal(v, p, s):
    """new java.math.BigDecimal(v) then Decimal.changePrecision(p, s), ROUND_HALF_UP (Cast
    StringType -> DecimalType, R/:57, :255-256): the unscaled int at scale s, None = NULL,
    UNSUPPORTED for a byte >= 0x80 (Java reads Unicode digits) or an exponent of > 4 digits."""
    if v is None:
        return None
    if any(ord(c) >= 0x80 for c in v):
        return UNSUPPORTED
    m = _DEC_GRAMMAR.fullmatch(v)  # gate: Python's Decimal also reads "1_0", " 1", "NaN"
    if not m:
        return None
    if m.group(4) is not None and len(m.group(4)) > 4:
        return UNSUPPORTED
    d = _DEC_CTX.create_decimal(v)
    q = d.scaleb(s, context=_DEC_CTX).to_integral_value(rounding=decimal.ROUND_HALF_UP)
    u = int(q)
    return u if abs(u) < 10**p else None


_FIELDS = {"yyyy": "Y", "MM": "M", "dd": "D", "HH": "h", "mm": "m", "ss": "s"}


def compile_mask(mask):
    """The supported SimpleDateFormat masks as tokens: ("lit", ch) or (field, width).  ValueError
    for anything else (other letters / run lengths, a field twice, no field, non-ASCII or digit
    literals, an unterminated quote)."""
    toks, seen, i = [], set(), 0

    def lit(ch):
        if ord(ch) >= 0x80 or ch in "0123456789":
            raise ValueError(f"mask {mask!r}: literal {ch!r}")
        toks.append(("lit", ch))

    while i < len(mask):
        ch = mask[i]
        if ch == "'":
            if mask[i + 1:i + 2] == "'":
                lit("'")
                i += 2
                continue
            i += 1
            while True:
                if i >= len(mask):
                    raise ValueError(f"mask {mask!r}: unterminated quote")
                if mask[i] == "'":
                    if mask[i + 1:i + 2] == "'":
                        lit("'")
                        i += 2
                        continue
                    i += 1
                    break
                lit(mask[i])
                i += 1
        elif re.fullmatch(r"[A-Za-z]", ch):
            run = re.match(re.escape(ch) + "+", mask[i:]).group(0)
            if run not in _FIELDS or run in seen:
                raise ValueError(f"mask {mask!r}: field {run!r}")
            seen.add(run)
            toks.append((_FIELDS[run], len(run)))
            i += len(run)
        else:
            lit(ch)
            i += 1
    if not seen:
        raise ValueError(f"mask {mask!r}: no field")
    return toks


def parse_ts(v, mask):
    """unix_timestamp(v, mask).cast(TimestampType) (R/:66-68, :275-276) in UTC: microseconds for a
    value in the mask's strict form, None where SimpleDateFormat's lenient parse must fail too,
    UNSUPPORTED for everything else."""
    if v is None:
        return None
    toks = compile_mask(mask)
    b = v.encode("utf-8")
    pos = 0
    f = {"Y": 1970, "M": 1, "D": 1, "h": 0, "m": 0, "s": 0}
    blank = (0x20, 0x09)
    for k, (kind, arg) in enumerate(toks):
        if pos >= len(b):
            return None  # the text has ended at a field or a literal
        c = b[pos]
        if kind == "lit":
            if c != ord(arg):
                return UNSUPPORTED if (c in blank or ord(arg) in blank) else None
            pos += 1
            continue
        if not 0x30 <= c <= 0x39:
            return UNSUPPORTED if (c in b"+-" or c in blank or c >= 0x80) else None
        digits = b[pos:pos + arg]
        if len(digits) < arg or not digits.isdigit():
            return UNSUPPORTED  # too few digits
        pos += arg
        abuts = k + 1 < len(toks) and toks[k + 1][0] != "lit"
        if not abuts and pos < len(b) and 0x30 <= b[pos] <= 0x39:
            return UNSUPPORTED  # too many digits
        f[kind] = int(digits)
    if pos < len(b):
        return UNSUPPORTED  # trailing text
    if not (1583 <= f["Y"] <= 9999 and 1 <= f["M"] <= 12 and f["h"] <= 23 and f["m"] <= 59
            and f["s"] <= 59 and 1 <= f["D"] <= calendar.monthrange(f["Y"], f["M"])[1]):
        return UNSUPPORTED  # lenient mode rolls these over
    return calendar.timegm((f["Y"], f["M"], f["D"], f["h"], f["m"], f["s"])) * 1_000_000


def char_length(v):
    """Spark's length(): characters of the string."""
    return len(v)


# ------------------------------------------------------------------------------------------------
# toCNF (R/:225-281) and validate (R/:183-223)
# ------------------------------------------------------------------------------------------------
def _regex(pattern):
    from deequ_amd.regex import compile_java_regex
    return compile_java_regex(pattern)


def cast_value(d, v):
    """castExpression (R/:29, :47, :57, :66-68) of one value."""
    if d["kind"] == "int":
        return cast_int(v)
    if d["kind"] == "decimal":
        return cast_decimal(v, d["precision"], d["scale"])
    if d["kind"] == "timestamp":
        return parse_ts(v, d["mask"])
    return v


def row_verdict(schema, row, compiled=None):
    """The CNF of one row (dict name -> str | None): True / False / None, or UNSUPPORTED."""
    cnf = True
    for d in schema:
        v = row[d["name"]]
        is_null = v is None
        if not d.get("is_nullable", True):
            cnf = k_and(cnf, not is_null)  # R/:230-232
        if d["kind"] == "int":
            n = cast_int(v)
            cnf = k_and(cnf, k_or(is_null, n is not None))  # R/:243
            if d.get("min_value") is not None:
                # R/:246: colIsNull.isNull is always false
                cnf = k_and(cnf, k_or(False, None if n is None else n >= d["min_value"]))
            if d.get("max_value") is not None:
                cnf = k_and(cnf, k_or(is_null, None if n is None else n <= d["max_value"]))  # R/:250
        elif d["kind"] == "decimal":
            u = cast_decimal(v, d["precision"], d["scale"])
            if u == UNSUPPORTED:
                return UNSUPPORTED
            cnf = k_and(cnf, k_or(is_null, u is not None))  # R/:256
        elif d["kind"] == "string":
            ln = None if is_null else char_length(v)
            if d.get("min_length") is not None:
                cnf = k_and(cnf, k_or(is_null, None if ln is None else ln >= d["min_length"]))  # :261
            if d.get("max_length") is not None:
                cnf = k_and(cnf, k_or(is_null, None if ln is None else ln <= d["max_length"]))  # :265
            if d.get("matches") is not None:
                rx = (compiled or {}).get(d["name"]) or _regex(d["matches"])
                # regexp_extract(v, regex, 0) != "": a non-empty first match (PatternMatch's find)
                cnf = k_and(cnf, k_or(is_null, None if is_null else rx.matches(v)))  # R/:268-271
        elif d["kind"] == "timestamp":
            t = parse_ts(v, d["mask"])
            if t == UNSUPPORTED:
                return UNSUPPORTED
            cnf = k_and(cnf, k_or(is_null, t is not None))  # R/:275-276
        else:
            raise ValueError(d["kind"])
    return cnf


def check_schema(schema, columns):
    """The refusals of validate that need no rows (names of `columns` are the string columns)."""
    seen = set()
    for d in schema:
        if d["name"] in seen:
            raise ValueError(f"column {d['name']} is declared twice")
        seen.add(d["name"])
        if d["name"] not in columns:
            raise ValueError(f"column {d['name']} is missing")
        if d["kind"] == "decimal" and not (1 <= d["precision"] <= 38 and 0 <= d["scale"] <= d["precision"]):
            raise ValueError(f"column {d['name']}: decimal({d['precision']},{d['scale']})")
        if d["kind"] == "timestamp":
            compile_mask(d["mask"])
        if d["kind"] == "string" and d.get("matches") is not None:
            _regex(d["matches"])


def validate(schema, columns):
    """columns: dict name -> list of str | None (every column of the table, declared or not).
    Returns (valid, invalid): two dicts name -> list, the valid one with the declared columns cast
    (int, unscaled decimal int, microseconds, str), both in input order.  Raises
    NotImplementedError when a value is UNSUPPORTED."""
    check_schema(schema, columns)
    names = list(columns)
    n = len(columns[names[0]]) if names else 0
    compiled = {d["name"]: _regex(d["matches"]) for d in schema
                if d["kind"] == "string" and d.get("matches") is not None}
    by_name = {d["name"]: d for d in schema}
    valid = {c: [] for c in names}
    invalid = {c: [] for c in names}
    for r in range(n):
        row = {c: columns[c][r] for c in names}
        verdict = row_verdict(schema, row, compiled)
        if verdict == UNSUPPORTED:
            raise NotImplementedError(f"row {r}: a value in an undecided form")
        if verdict is True:
            for c in names:
                valid[c].append(cast_value(by_name[c], row[c]) if c in by_name else row[c])
        elif verdict is False:
            for c in names:
                invalid[c].append(row[c])
    return valid, invalid


# ------------------------------------------------------------------------------------------------
# The reference's seven tests as data (tests/golden/schema_known_answers.json)
# ------------------------------------------------------------------------------------------------
def load_known_answers():
    import json
    import os
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden",
                        "schema_known_answers.json")
    with open(path) as f:
        return json.load(f)["cases"]


def assert_known_answer(case, valid, invalid, num_valid, num_invalid, valid_types=None,
                        invalid_types=None):
    """Every assertion the reference's test makes, over outputs in validate()'s form (decimals as
    unscaled ints at the declared scale); *_types: column -> Spark type name (device runs only)."""
    e = case["expected"]
    assert num_valid == e["num_valid"], (case["name"], num_valid)
    assert num_invalid == e["num_invalid"], (case["name"], num_invalid)
    for out, n in ((valid, num_valid), (invalid, num_invalid)):
        for col, vals in out.items():
            assert len(vals) == n, (case["name"], col)
    for col, members in e.get("valid_contains", {}).items():
        want = [m[0] if isinstance(m, list) else m for m in members]
        for m in want:
            assert m in valid[col], (case["name"], col, m, valid[col])
    for col, members in e.get("invalid_contains", {}).items():
        for m in members:
            assert m in invalid[col], (case["name"], col, m, invalid[col])
    for col, members in e.get("invalid_excludes", {}).items():
        for m in members:
            assert m not in invalid[col], (case["name"], col, m)
    for col, k in e.get("valid_distinct", {}).items():
        assert len(set(valid[col])) == k, (case["name"], col)
    for col, k in e.get("invalid_distinct", {}).items():
        assert len(set(invalid[col])) == k, (case["name"], col)
    for col in e.get("disjoint", []):
        assert not set(valid[col]) & set(invalid[col]), (case["name"], col)
    for col, counts in e.get("invalid_prefix_counts", {}).items():
        for prefix, k in counts.items():
            assert sum(1 for v in invalid[col] if v is not None and v.startswith(prefix)) == k
    if valid_types is not None:
        for col, t in e.get("valid_types", {}).items():
            assert valid_types[col] == t, (case["name"], col, valid_types[col])
    if invalid_types is not None:
        for col, t in e.get("invalid_types", {}).items():
            assert invalid_types[col] == t, (case["name"], col, invalid_types[col])
