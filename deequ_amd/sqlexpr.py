"""Spark-SQL predicate subset -> engine expression words (include/deequ_amd.h, dq_xop).

deequ passes SQL strings to Spark's ``expr()`` for ``where`` filters and constraints
(``Analyzers.conditionalSelection`` / ``conditionalCount``, Analyzer.scala:385-408; Compliance
Compliance.scala:47-49).  The strings Check generates are (Check.scala):

  * ``satisfies``            any predicate                                           :538-548
  * ``isNonNegative``        ``"c >= 0"``,  ``isPositive`` ``"c > 0"``               :670-686
  * ``isLessThan`` & co.     ``"a < b"``, ``"a <= b"``, ``"a > b"``, ``"a >= b"``    :697-760
  * ``isContainedIn``        ``"c IS NULL OR c IN ('v1','v2')"`` (quotes doubled)    :826-840
  * numeric range            ``"c IS NULL OR (c >= lo AND c <= hi)"``                :853-869

This module parses that grammar (plus NOT, parentheses, <>, !=, <=>, BETWEEN, booleans, NULL,
CAST(x AS DOUBLE / FLOAT / STRING), RLIKE, LIKE, arithmetic, DATE / TIMESTAMP literals, six
scalar and seven date functions) with Spark 2.2's
precedence -- OR < AND < NOT < comparison / IS / IN / BETWEEN / LIKE / RLIKE < ``+ -`` <
``* / %`` < unary ``- +`` < primary -- and applies Spark 2.2's type coercion so the engine only
sees typed operations:

  * numeric vs numeric: compared in the wider type (integral -> int64, else double);
  * string vs numeric: the string side is CAST to DOUBLE (Spark 2.2 ``PromoteStrings``);
  * ``x IN (...)`` with mixed item types: numeric literals in a string list become strings
    (``InConversion`` -> ``findWiderCommonType`` with string promotion); a numeric column or
    cast IN a list of strings, which Spark casts to STRING row by row, raises :class:`SqlError`;
  * ``x [NOT] LIKE 'pattern'`` over a string operand: the literal is unescaped as Spark's
    ``unescapeSQLString`` does (``\\%`` and ``\\_`` keep their backslash) and read as
    ``StringUtils.escapeLikeRegex`` reads it (``%`` any sequence, ``_`` one code point, ``\\%``
    ``\\_`` ``\\\\`` literals, any other escape an error), then compiled into a small pattern
    program (LIT / ANY1 / ANYSEQ tokens) for the device's own matcher -- never into a regex;
  * ``+ - * / %`` and unary ``-``: the result type follows ``numericPrecedence`` (Byte < Short <
    Int < Long < Float < Double; an integer literal is Int if it fits, else Long), integral
    results wrap at that width, ``/`` is always a double division, ``/`` and ``%`` by zero are
    NULL, a string operand is CAST to DOUBLE; a fractional literal without a ``D`` suffix is a
    decimal literal: cast to double against a float / double / string operand, refused against
    an integral or decimal one (Spark does decimal arithmetic there);
  * ``abs``, ``length``, ``coalesce`` (2 to 8 arguments), ``isnan``, ``isnull``, ``isnotnull``;
  * ``CAST(x AS STRING)`` of any value: Spark's text of it (``true``, decimal digits,
    ``Double.toString`` / ``Float.toString``, ``BigDecimal.toString``, ``yyyy-MM-dd``,
    ``yyyy-MM-dd HH:mm:ss[.f]`` in UTC), a string operand wherever one is taken -- comparisons,
    ``IN``, ``LIKE``, ``RLIKE``, ``length``, ``coalesce``, and against a number through the string
    -> double rule.  The implicit casts Spark inserts for ``i32 IN ('1')``, ``i32 LIKE '1%'``,
    ``length(i32)`` and ``coalesce(s, 1)`` are still refused: the cast has to be written;
  * date / timestamp comparisons (``PromoteStrings`` / ``findCommonTypeForBinaryComparison``):

      ====================================  ====================================================
      date vs date, timestamp vs timestamp  as int days / int64 microseconds
      date vs string (any operator)         refused: Spark casts the date to STRING and compares
                                            text; that cast has to be written, ``CAST(d AS
                                            STRING) = '2020-1-1'`` (FALSE for 2020-01-01, unsigned
                                            byte order), or the literal typed, ``DATE '...'``
      timestamp vs string, ``< <= > >=``    the timestamp CAST AS STRING: ``ts >= '2020-01-01'``
                                            is TRUE at midnight (the longer string sorts higher)
      timestamp vs string, ``= <> <=>``     the STRING is cast to timestamp: a literal
                                            ``yyyy-MM-dd`` / ``yyyy-MM-dd HH:mm:ss[.f{1,6}]`` is
                                            folded here (UTC); any other string operand is refused
      date vs timestamp                     both CAST AS STRING
      date / timestamp vs number / boolean  an error (Spark 2.2: type mismatch)
      date / timestamp vs NULL              NULL (``<=>``: FALSE / TRUE)
      ====================================  ====================================================

    ``x IN (...)`` over a date / timestamp ``x``: items of x's own type compare natively, a list
    of strings (and NULLs) casts x to STRING (``InConversion``), any other mix is refused;
    ``BETWEEN`` is its two comparisons;
  * ``DATE 'yyyy-[m]m-[d]d'`` and ``TIMESTAMP 'yyyy-[m]m-[d]d hh:mm:ss[.f{1,6}]'`` literals, read as
    ``java.sql.Date.valueOf`` / ``Timestamp.valueOf`` read them (a day up to 31 rolls into the next
    month), in UTC, on the proleptic Gregorian calendar; what those reject, a signed field, an
    hour above 23 / minute or second above 59, and more than 6 fractional digits raise;
  * ``year``, ``month``, ``dayofmonth``, ``to_date``, ``datediff(end, start)``, ``date_add(x, n)``,
    ``date_sub(x, n)`` over date or timestamp arguments (a timestamp is cast to date first: the
    floor of micros / 86 400 000 000, UTC); ``n`` is a tinyint / smallint / int expression; a
    string argument (Spark's lenient ``stringToDate``) is refused, ``d + 1`` too;
  * every other function raises :class:`SqlError`.

Column names resolve case-insensitively (spark.sql.caseSensitive=false).  Anything outside the
grammar raises :class:`SqlError`, which the runner turns into a failure of the shared scan exactly
like Spark's AnalysisException at ``data.agg`` (AnalysisRunner.scala:310-313).
"""
from __future__ import annotations

import re
import struct
from dataclasses import dataclass, field
from typing import List, Optional

from . import _native as N


class SqlError(Exception):
    pass


# ------------------------------------------------------------------------------------------------
# Tokenizer
# ------------------------------------------------------------------------------------------------
_TOKEN = re.compile(r"""
    \s*(?:
      (?P<num>(?:\d+\.\d*|\.\d+|\d+)(?:[eE][+-]?\d+)?[LDSYlfdsyBD]{0,2})|
      (?P<str>'(?:[^'\\]|''|\\.)*'|"(?:[^"\\]|\\.)*")|
      (?P<bq>`(?:[^`]|``)+`)|
      (?P<op><=>|<=|>=|<>|!=|==|=|<|>|\(|\)|,|\+|-|\*|/|%)|
      (?P<id>[A-Za-z_][A-Za-z0-9_.]*)
    )""", re.VERBOSE)


@dataclass
class Tok:
    kind: str
    text: str


def tokenize(s: str) -> List[Tok]:
    out, pos = [], 0
    s = s.rstrip()
    while pos < len(s):
        m = _TOKEN.match(s, pos)
        if not m or m.end() == pos:
            raise SqlError(f"cannot parse SQL expression at: {s[pos:]!r}")
        pos = m.end()
        for k in ("num", "str", "bq", "op", "id"):
            if m.group(k) is not None:
                out.append(Tok(k, m.group(k)))
                break
    return out


# ------------------------------------------------------------------------------------------------
# AST
# ------------------------------------------------------------------------------------------------
@dataclass
class Node:
    op: str                      # col, lit, isnull, isnotnull, not, and, or, cmp, in, cast, regex,
                                 # like, arith (name = + - * / %), neg, func (name = the function)
    kids: List["Node"] = field(default_factory=list)
    name: Optional[str] = None   # column name / comparison symbol / cast type
    value: object = None         # literal value
    ltype: Optional[str] = None  # literal type: int, float, str, bool, null
    # numeric literals: the exact value (int or decimal.Decimal) and whether Spark 2.2 types it
    # DoubleType (a D suffix; every other fractional / exponent literal is a DecimalType literal)
    exact: object = None
    dbl: bool = False
    suffix: str = ""             # an integral literal's type suffix (L, S, Y)


_KW = {"AND", "OR", "NOT", "IS", "NULL", "IN", "TRUE", "FALSE", "BETWEEN", "CAST", "AS", "RLIKE",
       "LIKE"}
_FUNCS = {"abs": (1, 1), "length": (1, 1), "coalesce": (2, 8), "isnan": (1, 1), "isnull": (1, 1),
          "isnotnull": (1, 1), "year": (1, 1), "month": (1, 1), "dayofmonth": (1, 1),
          "to_date": (1, 1), "datediff": (2, 2), "date_add": (2, 2),
          "date_sub": (2, 2)}   # name -> (fewest, most) arguments
_DATE_FUNCS = ("year", "month", "dayofmonth", "to_date", "datediff", "date_add", "date_sub")

# The engine's spelling of PatternMatch's counted expression,
# when(regexp_extract(x, pattern, 0) != "", 1).otherwise(0) (PatternMatch.scala:44-46): TRUE when
# Java's first find() match exists and is non-empty, FALSE otherwise (a NULL x included).
FIND_NONEMPTY = "dq_find_nonempty"


class _Parser:
    def __init__(self, toks: List[Tok]):
        self.t = toks
        self.i = 0

    def peek(self, k=0) -> Optional[Tok]:
        j = self.i + k
        return self.t[j] if j < len(self.t) else None

    def kw(self, word: str, k=0) -> bool:
        t = self.peek(k)
        return t is not None and t.kind == "id" and t.text.upper() == word

    def sym(self, s: str) -> bool:
        t = self.peek()
        return t is not None and t.kind == "op" and t.text == s

    def take(self) -> Tok:
        t = self.peek()
        if t is None:
            raise SqlError("unexpected end of expression")
        self.i += 1
        return t

    def expect_sym(self, s: str):
        if not self.sym(s):
            raise SqlError(f"expected '{s}'")
        self.i += 1

    def parse(self) -> Node:
        n = self.or_()
        if self.peek() is not None:
            raise SqlError(f"unexpected token {self.peek().text!r}")
        return n

    def or_(self) -> Node:
        n = self.and_()
        while self.kw("OR"):
            self.i += 1
            n = Node("or", [n, self.and_()])
        return n

    def and_(self) -> Node:
        n = self.not_()
        while self.kw("AND"):
            self.i += 1
            n = Node("and", [n, self.not_()])
        return n

    def not_(self) -> Node:
        if self.kw("NOT"):
            self.i += 1
            return Node("not", [self.not_()])
        return self.predicate()

    def predicate(self) -> Node:
        left = self.additive()
        t = self.peek()
        if t is None:
            return left
        if t.kind == "op" and t.text in ("=", "==", "<>", "!=", "<", "<=", ">", ">=", "<=>"):
            self.i += 1
            sym = {"==": "=", "!=": "<>"}.get(t.text, t.text)
            return Node("cmp", [left, self.additive()], name=sym)
        if self.kw("IS"):
            self.i += 1
            neg = False
            if self.kw("NOT"):
                self.i += 1
                neg = True
            if not self.kw("NULL"):
                raise SqlError("expected NULL after IS")
            self.i += 1
            return Node("isnotnull" if neg else "isnull", [left])
        neg = False
        if self.kw("NOT") and (self.kw("RLIKE", 1) or self.kw("LIKE", 1)):
            self.i += 1
            neg = True
        if self.kw("LIKE"):  # x LIKE 'pattern': the whole string must match, NULL on NULL
            self.i += 1
            t = self.peek()
            if t is None or t.kind != "str":
                raise SqlError("LIKE needs a string literal pattern")
            self.i += 1
            pat = _unescape_sql_string(t.text, like=True)
            n = Node("like", [left], name=pat, value=like_program(pat))
            return Node("not", [n]) if neg else n
        if self.kw("RLIKE"):  # x RLIKE 'java regex': find() anywhere, NULL on NULL
            self.i += 1
            pat = self.primary()
            if pat.op != "lit" or pat.ltype != "str":
                raise SqlError("RLIKE needs a string literal pattern")
            n = Node("regex", [left], name="rlike", value=pat.value)
            return Node("not", [n]) if neg else n
        if self.kw("NOT") and (self.kw("IN", 1) or self.kw("BETWEEN", 1)):
            self.i += 1
            neg = True
        if self.kw("IN"):
            self.i += 1
            self.expect_sym("(")
            items = [self.additive()]
            while self.sym(","):
                self.i += 1
                items.append(self.additive())
            self.expect_sym(")")
            n = Node("in", [left] + items)
            return Node("not", [n]) if neg else n
        if self.kw("BETWEEN"):
            self.i += 1
            lo = self.additive()
            if not self.kw("AND"):
                raise SqlError("expected AND in BETWEEN")
            self.i += 1
            hi = self.additive()
            n = Node("and", [Node("cmp", [left, lo], name=">="), Node("cmp", [left, hi], name="<=")])
            return Node("not", [n]) if neg else n
        return left

    def additive(self) -> Node:
        n = self.multiplicative()
        while self.sym("+") or self.sym("-"):
            sym = self.take().text
            n = Node("arith", [n, self.multiplicative()], name=sym)
        return n

    def multiplicative(self) -> Node:
        n = self.unary()
        while self.sym("*") or self.sym("/") or self.sym("%"):
            sym = self.take().text
            n = Node("arith", [n, self.unary()], name=sym)
        return n

    def unary(self) -> Node:
        if self.sym("-") or self.sym("+"):
            t = self.take()
            inner = self.unary()
            if inner.op == "lit" and inner.ltype in ("int", "float"):  # a constant: folded
                if t.text == "-":
                    inner.value = -inner.value
                    inner.exact = -inner.exact if inner.exact is not None else None
                return inner
            return Node("neg", [inner]) if t.text == "-" else inner
        return self.primary()

    def primary(self) -> Node:
        t = self.take()
        if t.kind == "op" and t.text == "(":
            n = self.or_()
            self.expect_sym(")")
            return n
        if t.kind == "op" and t.text in ("-", "+"):
            self.i -= 1
            return self.unary()
        if t.kind == "num":
            return _num_literal(t.text)
        if t.kind == "str":
            return Node("lit", value=_unescape_sql_string(t.text), ltype="str")
        if t.kind == "bq":
            return Node("col", name=t.text[1:-1].replace("``", "`"))
        if t.kind == "id":
            u = t.text.upper()
            if u == "NULL":
                return Node("lit", value=None, ltype="null")
            if u in ("TRUE", "FALSE"):
                return Node("lit", value=(u == "TRUE"), ltype="bool")
            if u == "CAST":
                self.expect_sym("(")
                inner = self.or_()
                if not self.kw("AS"):
                    raise SqlError("expected AS in CAST")
                self.i += 1
                ty = self.take().text.upper()
                self.expect_sym(")")
                return Node("cast", [inner], name=ty)
            nxt = self.peek()
            if u in ("DATE", "TIMESTAMP") and nxt is not None and nxt.kind == "str":
                self.i += 1
                text = _unescape_sql_string(nxt.text)
                if u == "DATE":
                    return Node("lit", value=date_literal(text), ltype="date")
                return Node("lit", value=timestamp_literal(text), ltype="ts")
            if u in _KW:
                raise SqlError(f"unexpected keyword {t.text}")
            if self.sym("(") and t.text.lower() == FIND_NONEMPTY:
                self.expect_sym("(")
                x = self.or_()
                self.expect_sym(",")
                pat = self.primary()
                self.expect_sym(")")
                if pat.op != "lit" or pat.ltype != "str":
                    raise SqlError(f"{FIND_NONEMPTY} needs a string literal pattern")
                return Node("regex", [x], name="nonempty", value=pat.value)
            if self.sym("(") and t.text.lower() in _FUNCS:
                name = t.text.lower()
                self.expect_sym("(")
                args = [self.or_()]
                while self.sym(","):
                    self.i += 1
                    args.append(self.or_())
                self.expect_sym(")")
                lo, hi = _FUNCS[name]
                if not lo <= len(args) <= hi:
                    raise SqlError(f"{name}() takes {lo} argument{'s' if lo > 1 else ''}"
                                   + (f" to {hi}" if hi > lo else "") + f", not {len(args)}")
                if name in ("isnull", "isnotnull"):  # the function spelling of IS [NOT] NULL
                    return Node(name, args)
                return Node("func", args, name=name)
            if self.sym("("):
                raise SqlError(f"function {t.text}() is not supported by the engine")
            return Node("col", name=t.text)
        raise SqlError(f"unexpected token {t.text!r}")


def _unescape_sql_string(text: str, like: bool = False) -> str:
    """The value of a quoted SQL string token.  In a LIKE pattern ``\\%`` and ``\\_`` keep their
    backslash, as Spark's ``unescapeSQLString`` leaves them for ``escapeLikeRegex``."""
    q = text[0]
    body = text[1:-1]
    body = body.replace("''", "'") if q == "'" else body
    esc = {"n": "\n", "t": "\t", "0": "\0"}
    if like:
        esc = dict(esc, **{"%": "\\%", "_": "\\_"})
    return re.sub(r"\\(.)", lambda m: esc.get(m.group(1), m.group(1)), body)


# Tokens of a LIKE pattern program (include/deequ_amd.h, DQ_X_LIKE)
LIKE_LIT, LIKE_ANY1, LIKE_ANYSEQ = 1, 2, 3
LIKE_MAX_BYTES = 4096


def like_program(pattern: str) -> bytes:
    """Compiles an (unescaped) LIKE pattern as Spark 2.2's ``StringUtils.escapeLikeRegex`` reads
    it into the device matcher's token stream: LIT(u16 length, bytes), ANY1 (``_``: one code
    point), ANYSEQ (``%``: any sequence; adjacent ones collapsed)."""
    toks: List[object] = []

    def lit(ch: str):
        if toks and isinstance(toks[-1], bytearray):
            toks[-1] += ch.encode("utf-8")
        else:
            toks.append(bytearray(ch.encode("utf-8")))

    i = 0
    while i < len(pattern):
        c = pattern[i]
        if c == "\\":
            if i + 1 >= len(pattern):
                raise SqlError(f"the pattern '{pattern}' is invalid, it is not allowed to end with "
                               f"the escape character")
            d = pattern[i + 1]
            if d not in "_%\\":
                raise SqlError(f"the pattern '{pattern}' is invalid, the escape character is not "
                               f"allowed to precede '{d}'")
            lit(d)
            i += 2
            continue
        if c == "_":
            toks.append(LIKE_ANY1)
        elif c == "%":
            if not toks or toks[-1] != LIKE_ANYSEQ:
                toks.append(LIKE_ANYSEQ)
        else:
            lit(c)
        i += 1
    out = bytearray()
    for t in toks:
        if isinstance(t, bytearray):
            if len(t) > 0xFFFF:
                raise SqlError("LIKE pattern too long for the engine")
            out += bytes([LIKE_LIT, len(t) & 0xFF, len(t) >> 8]) + t
        else:
            out.append(t)
    if len(out) > LIKE_MAX_BYTES:
        raise SqlError(f"LIKE pattern too long for the engine ({len(out)} > {LIKE_MAX_BYTES} bytes)")
    return bytes(out)


# ------------------------------------------------------------------------------------------------
# Date and timestamp literals, folded on the host (session time zone: UTC)
# ------------------------------------------------------------------------------------------------
# (re.ASCII: \d is [0-9] only, as the JDK's and Spark's byte-wise readers take it)
_DATE_RE = re.compile(r"(\d{4})-(\d{1,2})-(\d{1,2})", re.ASCII)
_TS_RE = re.compile(r"(\d{4})-(\d{1,2})-(\d{1,2}) (\d{1,2}):(\d{1,2}):(\d{1,2})(?:\.(\d+))?", re.ASCII)
_TS_STRING_RE = re.compile(r"(\d{4})-(\d{2})-(\d{2})(?: (\d{2}):(\d{2}):(\d{2})(?:\.(\d{1,6}))?)?", re.ASCII)
_US_PER_DAY = 86_400_000_000


def _days(year: int, month: int, day: int, what: str) -> int:
    """Days since 1970-01-01 of a proleptic-Gregorian date.  java.sql.Date.valueOf checks only
    1 <= month <= 12 and 1 <= day <= 31 and builds the date leniently: day 31 of a 30-day month is
    the first of the next one."""
    import datetime
    if not (1 <= month <= 12 and 1 <= day <= 31) or year < 1:
        raise SqlError(f"{what}: no such date")
    try:
        d = datetime.date(year, month, 1) + datetime.timedelta(days=day - 1)
    except OverflowError as e:
        raise SqlError(f"{what}: no such date") from e
    return d.toordinal() - datetime.date(1970, 1, 1).toordinal()


def date_literal(text: str) -> int:
    """``DATE 'yyyy-[m]m-[d]d'`` as java.sql.Date.valueOf reads it (digits only: a sign before a
    field, which Integer.parseInt would take, is refused), in days since the epoch."""
    m = _DATE_RE.fullmatch(text)
    if not m:
        raise SqlError(f"DATE '{text}': expected yyyy-[m]m-[d]d")
    return _days(int(m.group(1)), int(m.group(2)), int(m.group(3)), f"DATE '{text}'")


def timestamp_literal(text: str) -> int:
    """``TIMESTAMP 'yyyy-[m]m-[d]d hh:mm:ss[.f{1,6}]'`` as java.sql.Timestamp.valueOf reads it
    (surrounding blanks trimmed; hours to 23, minutes and seconds to 59 -- the lenient roll-over of
    larger ones is refused), read in UTC, in microseconds since the epoch.  More than six
    fractional digits do not fit Spark's microseconds and are refused."""
    what = f"TIMESTAMP '{text}'"
    m = _TS_RE.fullmatch(text.strip(" "))
    if not m:
        raise SqlError(f"{what}: expected yyyy-[m]m-[d]d hh:mm:ss[.f]")
    y, mo, d, h, mi, sec = (int(g) for g in m.groups()[:6])
    frac = m.group(7) or ""
    if len(frac) > 6:
        raise SqlError(f"{what}: more than 6 fractional digits")
    if h > 23 or mi > 59 or sec > 59:
        raise SqlError(f"{what}: no such time of day")
    us = int(frac.ljust(6, "0")) if frac else 0
    return _days(y, mo, d, what) * _US_PER_DAY + ((h * 60 + mi) * 60 + sec) * 1_000_000 + us


def timestamp_of_string(text: str) -> Optional[int]:
    """The timestamp Spark's Cast(string AS TIMESTAMP) gives a string of the exact forms
    ``yyyy-MM-dd`` / ``yyyy-MM-dd HH:mm:ss[.f{1,6}]`` (UTC); None for any other string, whose
    reading by DateTimeUtils.stringToTimestamp is not restated."""
    import datetime
    m = _TS_STRING_RE.fullmatch(text)
    if not m:
        return None
    y, mo, d = (int(g) for g in m.groups()[:3])
    h, mi, sec = (int(g) for g in m.groups()[3:6]) if m.group(4) else (0, 0, 0)
    try:
        day = datetime.date(y, mo, d).toordinal() - datetime.date(1970, 1, 1).toordinal()
    except ValueError:
        return None
    if h > 23 or mi > 59 or sec > 59:
        return None
    us = int((m.group(7) or "").ljust(6, "0") or 0)
    return day * _US_PER_DAY + ((h * 60 + mi) * 60 + sec) * 1_000_000 + us


def _num_literal(text: str) -> Node:
    m = re.match(r"^((?:\d+\.\d*|\.\d+|\d+)(?:[eE][+-]?\d+)?)([A-Za-z]*)$", text)
    body, suffix = m.group(1), m.group(2).upper()
    if suffix in ("D", "BD") or any(c in body for c in ".eE"):
        from decimal import Decimal
        return Node("lit", value=float(body), ltype="float", exact=Decimal(body), dbl=suffix == "D")
    if suffix in ("", "L", "S", "Y"):
        return Node("lit", value=int(body), ltype="int", exact=int(body), suffix=suffix)
    raise SqlError(f"bad numeric literal {text}")


def parse(sql: str) -> Node:
    return _Parser(tokenize(sql)).parse()


# ------------------------------------------------------------------------------------------------
# Typing + emission
# ------------------------------------------------------------------------------------------------
_CMP = {"=": N.X_EQ, "<>": N.X_NE, "<": N.X_LT, "<=": N.X_LE, ">": N.X_GT, ">=": N.X_GE,
        "<=>": N.X_EQ_NULL_SAFE}


def _kind_of_type(t: int) -> str:
    if t == N.UTF8:
        return "str"
    if t == N.BOOL:
        return "bool"
    if t in N.INTEGRAL_TYPES:
        return "int"
    if N.is_decimal(t):
        return "dec"
    if t == N.DATE32:
        return "date"
    if t == N.TIMESTAMP_US:
        return "ts"
    if t == N.UNSUPPORTED:
        raise SqlError("a column of a type the engine does not read appears in an expression")
    return "float"


_DEC_LIMIT = 10 ** 38  # |unscaled| of any decimal(38) value is below it


def _dec128_words(v: int) -> List[int]:
    """An unscaled value (clamped to +-10^38: still on the right side of every column value) as
    the [X_DEC128, lo, hi] words (signed int64 each)."""
    v = max(-_DEC_LIMIT, min(_DEC_LIMIT, v)) & ((1 << 128) - 1)
    lo, hi = v & 0xFFFFFFFFFFFFFFFF, v >> 64
    sg = lambda x: x - (1 << 64) if x >= (1 << 63) else x  # noqa: E731
    return [N.X_DEC128, sg(lo), sg(hi)]


def _exact_literal(n: "Node"):
    """The exact value of an int / decimal literal (None for a double literal or a non-number)."""
    if n.op != "lit" or n.ltype not in ("int", "float") or n.dbl or n.exact is None:
        return None
    return n.exact


class _Emitter:
    def __init__(self, schema, col_index):
        self.schema = schema
        self.col_index = col_index  # callable name -> column index in the plan
        self.words: List[int] = []
        self.columns: List[str] = []

    def type_of(self, n: Node) -> str:
        if n.op == "col":
            name = self.schema.resolve(n.name)
            if name is None:
                raise SqlError(f"cannot resolve '`{n.name}`' given input columns: "
                               f"[{', '.join(self.schema.field_names)}]")
            n.name = name
            return _kind_of_type(self.schema[name].dtype)
        if n.op == "lit":
            return n.ltype
        if n.op == "cast":
            return {"DOUBLE": "float", "FLOAT": "float", "STRING": "str", "INT": "int",
                    "BIGINT": "int", "LONG": "int", "BOOLEAN": "bool"}.get(n.name, "?")
        if n.op in ("arith", "neg") or (n.op == "func" and n.name != "isnan"):
            t = self.result_type(n)
            if t == N.DATE32:
                return "date"
            return "str" if t == N.UTF8 else ("int" if t in N.INTEGRAL_TYPES else "float")
        return "bool"

    # -- arithmetic and functions: Spark 2.2 result types, widths included
    def operand_type(self, n: Node, what: str):
        """What an operand of ``what`` (an arithmetic operator or a function) is: a dq_type in
        INT8..FLOAT64, "str", "null" or "declit" (a DecimalType literal).  Anything else has no
        arithmetic in the interpreter and is refused."""
        if n.op == "lit":
            if n.ltype == "int":
                t = {"L": N.INT64, "S": N.INT16, "Y": N.INT8}.get(n.suffix)
                return t or (N.INT32 if -(1 << 31) <= n.value < (1 << 31) else N.INT64)
            if n.ltype == "float":
                return N.FLOAT64 if n.dbl else "declit"
            if n.ltype in ("str", "null"):
                return n.ltype
        elif n.op == "col":
            kind = self.type_of(n)
            if kind in ("int", "float"):
                return self.schema[n.name].dtype
            if kind == "str":
                return "str"
            if kind == "dec":
                raise SqlError(f"{what} over a decimal column: Spark does decimal arithmetic, "
                               f"which is not supported by the engine")
        elif n.op == "cast" and n.name in ("DOUBLE", "FLOAT"):
            return N.FLOAT64 if n.name == "DOUBLE" else N.FLOAT32
        elif n.op == "cast" and n.name == "STRING":
            self.cast_str_kind(n)
            return "str"
        elif n.op in ("arith", "neg", "func") and self.type_of(n) not in ("bool", "date"):
            t = self.result_type(n)
            return "str" if t == N.UTF8 else t
        raise SqlError(f"{what} over a {self.type_of(n)} operand is not supported by the engine")

    def promote(self, types, what: str) -> int:
        """numericPrecedence over operand types: a string is cast to DOUBLE (PromoteStrings), a
        decimal literal to double beside a float / double / string operand."""
        nums = [t for t in types if t not in ("null", "declit", "str")]
        if "declit" in types and not ("str" in types or any(t in (N.FLOAT32, N.FLOAT64) for t in nums)):
            raise SqlError(f"{what} of a fractional (decimal) literal and an integral or decimal "
                           f"operand: Spark does decimal arithmetic, which is not supported by the "
                           f"engine (write the literal with a D suffix for double arithmetic)")
        if "declit" in types or "str" in types:
            return N.FLOAT64
        if not nums:
            raise SqlError(f"{what} over NULL operands only is not supported by the engine")
        return max(nums)  # (the dq_type values ascend Byte < Short < Int < Long < Float < Double)

    def result_type(self, n: Node) -> int:
        """The dq_type an arith / neg / func node evaluates to (UTF8: coalesce over strings)."""
        if n.op == "neg":
            return self.promote([self.operand_type(n.kids[0], "unary -")], "unary -")
        if n.op == "arith":
            t = self.promote([self.operand_type(k, f"'{n.name}'") for k in n.kids], f"'{n.name}'")
            return N.FLOAT64 if n.name == "/" else t  # the Division rule: always a double division
        what = f"{n.name}()"
        if n.name in _DATE_FUNCS:
            return self.date_func_type(n)
        types = [self.operand_type(k, what) for k in n.kids]
        if n.name == "length":
            if types != ["str"]:
                raise SqlError("length() needs a string operand (write CAST(x AS STRING) for the "
                               "length of another value's text)")
            return N.INT32
        if n.name == "isnan":
            if types[0] not in (N.FLOAT32, N.FLOAT64):
                raise SqlError("isnan() needs a float or double operand")
            return N.BOOL
        if n.name == "coalesce" and all(t in ("str", "null") for t in types) and "str" in types:
            return N.UTF8
        if n.name == "coalesce" and "str" in types:
            raise SqlError("coalesce() over string and numeric arguments is not supported by the "
                           "engine (write CAST(x AS STRING) around the numeric ones)")
        return self.promote(types, what)

    # -- dates and timestamps
    def date_func_type(self, n: Node) -> int:
        """Checks a date function's arguments and returns its result type.  A date argument is a
        date or a timestamp (cast to date: its UTC day); a string one, which Spark reads with the
        lenient stringToDate, is refused."""
        what = f"{n.name}()"
        day_count = n.name in ("date_add", "date_sub")
        for k in (n.kids[:1] if day_count else n.kids):
            t = self.type_of(k)
            if t not in ("date", "ts"):
                raise SqlError(f"{what} needs a date or timestamp argument, not a {t} one"
                               + (" (Spark parses the string as a date; write a DATE '...' literal)"
                                  if t == "str" else ""))
        if day_count:
            t = self.type_of(n.kids[1])
            nt = self.operand_type(n.kids[1], what) if t == "int" else None
            if nt not in (N.INT8, N.INT16, N.INT32):
                raise SqlError(f"{what} needs an int number of days (a tinyint, smallint or int "
                               f"expression), as Spark's type check does")
        return N.DATE32 if day_count or n.name == "to_date" else N.INT32

    def cast_str_kind(self, n: Node) -> str:
        t = self.type_of(n.kids[0])
        if t not in ("str", "bool", "int", "float", "dec", "date", "ts", "null"):
            raise SqlError(f"CAST of a {t} value AS STRING is not supported by the engine")
        return t

    def _as_string(self, n: Node) -> Node:
        return Node("cast", [n], name="STRING")

    def _emit_temporal_cmp(self, sym: str, a: Node, ta: str, b: Node, tb: str) -> None:
        """A comparison with a date / timestamp operand, typed as Spark 2.2's PromoteStrings and
        findCommonTypeForBinaryComparison type it."""
        kinds = {ta, tb}
        if ta == tb or "null" in kinds:            # days / microseconds as integers; NULL
            pass
        elif kinds == {"date", "ts"}:              # both sides as strings
            a, b = self._as_string(a), self._as_string(b)
        elif kinds == {"date", "str"}:
            # Spark casts the DATE to string and compares text (d = '2020-1-1' is FALSE for
            # 2020-01-01).  This implicit cast stays refused, as for i32 IN ('1'): the caller says
            # which comparison is meant
            raise SqlError(f"'{sym}' of a date and a string: Spark 2.2 casts the date to STRING and "
                           f"compares text; write CAST(x AS STRING) {sym} '...' for that comparison, "
                           f"or a DATE '...' literal to compare dates")
        elif kinds == {"ts", "str"} and sym in ("<", "<=", ">", ">="):
            if ta == "str":
                b = self._as_string(b)
            else:
                a = self._as_string(a)
        elif kinds == {"ts", "str"}:               # =, <>, <=>: the STRING is cast to timestamp
            s = a if ta == "str" else b
            us = timestamp_of_string(s.value) if s.op == "lit" else None
            if us is None:
                raise SqlError(f"'{sym}' of a timestamp and a string: Spark parses the string as a "
                               f"timestamp, which the engine does only for a literal of the form "
                               f"'yyyy-MM-dd' or 'yyyy-MM-dd HH:mm:ss[.f]' (write a TIMESTAMP '...' "
                               f"literal)")
            lit = Node("lit", value=us, ltype="ts")
            a, b = (lit, b) if ta == "str" else (a, lit)
        else:
            other = tb if ta in ("date", "ts") else ta
            this = ta if ta in ("date", "ts") else tb
            raise SqlError(f"cannot compare a {this} value with a {other} one (Spark 2.2 reports a "
                           f"type mismatch)")
        self.words.append(_CMP[sym])
        self.emit(a)
        self.emit(b)

    def _emit_temporal_in(self, x: Node, tx: str, items: List[Node], tis: List[str]) -> None:
        if all(t in (tx, "null") for t in tis):    # natively
            pass
        elif all(t in ("str", "null") for t in tis):   # InConversion with string promotion
            x = self._as_string(x)
        else:
            raise SqlError(f"a {tx} value IN a list that mixes other types is not supported by the "
                           f"engine")
        self.words += [N.X_IN, len(items)]
        self.emit(x)
        for i in items:
            self.emit(i)

    def emit_operand(self, k: Node, what: str):
        """An operand of an arithmetic operator / numeric function: a string under CAST AS DOUBLE,
        a decimal literal as its double."""
        t = self.operand_type(k, what)
        if t == "str":
            self.words.append(N.X_CAST_F64)
        self.emit(k, "float" if t == "declit" else None)

    def emit(self, n: Node, want: Optional[str] = None):
        w = self.words
        if n.op == "col":
            self.type_of(n)
            w += [N.X_COL, self.col_index(n.name)]
            if n.name not in self.columns:
                self.columns.append(n.name)
            if want == "float" and self.type_of(n) in ("str", "dec"):
                w.insert(len(w) - 2, N.X_CAST_F64)  # (a decimal: Decimal.toDouble)
            return
        if n.op == "lit":
            v, t = n.value, n.ltype
            if want == "str" and t in ("int", "float"):
                v, t = (str(v) if t == "int" else repr(float(v))), "str"
            if want == "float" and t == "int":
                v, t = float(v), "float"
            if t == "null":
                w.append(N.X_NULL)
            elif t == "bool":
                w += [N.X_BOOL, 1 if v else 0]
            elif t == "int":
                if not -(1 << 63) <= v < (1 << 63):
                    raise SqlError(f"integer literal out of range: {v}")
                w += [N.X_I64, v]
            elif t == "float":
                w += [N.X_F64, struct.unpack("<q", struct.pack("<d", v))[0]]
            elif t == "date":
                w += [N.X_DATE, v]
            elif t == "ts":
                w += [N.X_TIMESTAMP, v]
            elif t == "str":
                b = v.encode("utf-8")
                w += [N.X_STR, len(b)]
                padded = b + b"\0" * ((-len(b)) % 8)
                w += list(struct.unpack(f"<{len(padded) // 8}q", padded)) if padded else []
            return
        if n.op == "cast" and n.name == "STRING":
            self.cast_str_kind(n)
            if want == "float":                    # against a number: the text parsed as a double
                w.append(N.X_CAST_F64)
            w.append(N.X_CAST_STR)
            self.emit(n.kids[0])
            return
        if n.op == "cast":
            if n.name not in ("DOUBLE", "FLOAT"):
                raise SqlError(f"CAST AS {n.name} is not supported by the engine")
            if n.name == "FLOAT" and self.type_of(n.kids[0]) == "str":
                # Spark parses with Float.parseFloat (one rounding to float); parse-to-double and
                # then round would round twice -- refused rather than restated approximately
                raise SqlError("CAST(string AS FLOAT) is not supported by the engine")
            w.append(N.X_CAST_F32 if n.name == "FLOAT" else N.X_CAST_F64)
            self.emit(n.kids[0])
            return
        if n.op in ("isnull", "isnotnull", "not"):
            w.append({"isnull": N.X_IS_NULL, "isnotnull": N.X_IS_NOT_NULL, "not": N.X_NOT}[n.op])
            if n.op == "not" and self.type_of(n.kids[0]) not in ("bool", "null"):
                raise SqlError("NOT needs a boolean operand")
            self.emit(n.kids[0])
            return
        if n.op in ("and", "or"):
            for k in n.kids:
                if self.type_of(k) not in ("bool", "null"):
                    raise SqlError(f"{n.op.upper()} needs boolean operands")
            w.append(N.X_AND if n.op == "and" else N.X_OR)
            self.emit(n.kids[0])
            self.emit(n.kids[1])
            return
        if n.op == "cmp":
            a, b = n.kids
            ta, tb = self.type_of(a), self.type_of(b)
            if "dec" in (ta, tb) and self._emit_dec_cmp(n.name, a, ta, b, tb):
                return
            if ta in ("date", "ts") or tb in ("date", "ts"):
                self._emit_temporal_cmp(n.name, a, ta, b, tb)
                return
            target = _common_cmp_type(ta, tb)
            w.append(_CMP[n.name])
            self.emit(a, target)
            self.emit(b, target)
            return
        if n.op == "in":
            x, items = n.kids[0], n.kids[1:]
            tx = self.type_of(x)
            tis = [self.type_of(i) for i in items]
            if tx == "dec":
                self._emit_dec_in(x, items)
                return
            if tx in ("date", "ts"):
                self._emit_temporal_in(x, tx, items, tis)
                return
            if any(t in ("dec", "date", "ts") for t in tis):
                raise SqlError("IN over a date / timestamp / decimal value is not supported by the "
                               "engine")
            target = tx
            if any(t not in (tx, "null") for t in tis):
                kinds = {tx} | {t for t in tis if t != "null"}
                if "str" in kinds:
                    target = "str"
                elif kinds <= {"int", "float"}:
                    target = "float" if "float" in kinds else "int"
                else:
                    raise SqlError("incompatible types in IN list")
            if target == "str" and tx not in ("str", "null") and x.op != "lit":
                # Spark 2.2 InConversion casts the value to STRING (1 IN ('1', '2') is TRUE,
                # 1 IN ('01') FALSE); comparing the number with the strings as they are would make
                # every row FALSE, and the implicit cast is left to be written (CAST AS STRING)
                raise SqlError(f"a {tx} value IN a list of strings (Spark casts the value to "
                               f"STRING) is not supported by the engine as it stands: write "
                               f"CAST(x AS STRING) IN (...)")
            w += [N.X_IN, len(items)]
            self.emit(x, target if target != tx or tx == "str" else None)
            for i in items:
                self.emit(i, target)
            return
        if n.op == "regex":
            tx = self.type_of(n.kids[0])
            # a non-string operand is matched as Spark's cast to string: decimal integers,
            # true / false, Double.toString / Float.toString (csrc/jfmt.h, on the device)
            if tx not in ("str", "int", "float", "bool", "null", "dec", "date", "ts"):
                raise SqlError(f"cannot match a regex against a {tx} value")
            blob = _compiled_regex(n.value, n.name == "rlike")
            w += [N.X_REGEX, 1 if n.name == "nonempty" else 0, len(blob)]
            padded = blob + b"\0" * ((-len(blob)) % 8)
            w += list(struct.unpack(f"<{len(padded) // 8}q", padded))
            self.emit(n.kids[0])
            return
        if n.op == "like":
            if self.type_of(n.kids[0]) != "str":
                # Spark casts the operand to string; the engine leaves that cast to be written
                raise SqlError(f"LIKE over a {self.type_of(n.kids[0])} operand (Spark casts it to "
                               f"STRING) is not supported by the engine as it stands: write "
                               f"CAST(x AS STRING) LIKE ...")
            blob = n.value
            w += [N.X_LIKE, len(blob)]
            padded = blob + b"\0" * ((-len(blob)) % 8)
            w += list(struct.unpack(f"<{len(padded) // 8}q", padded)) if padded else []
            self.emit(n.kids[0])
            return
        if n.op in ("arith", "neg"):
            what = "unary -" if n.op == "neg" else f"'{n.name}'"
            which = N.AR_NEG if n.op == "neg" else _ARITH[n.name]
            w += [N.X_ARITH, which, self.result_type(n)]
            for k in n.kids:
                self.emit_operand(k, what)
            return
        if n.op == "func" and n.name in _DATE_FUNCS:
            w += [N.X_FUNC, _FUNC_CODE[n.name], self.result_type(n), len(n.kids)]
            for k in n.kids:
                self.emit(k)
            return
        if n.op == "func":
            rt = self.result_type(n)
            if n.name == "coalesce":
                w += [N.X_FUNC, N.FN_COALESCE, rt, len(n.kids)]
            else:
                w += [N.X_FUNC, _FUNC_CODE[n.name], rt, 1]
            for k in n.kids:
                if rt == N.UTF8 or n.name in ("length", "isnan"):
                    self.emit(k)
                else:
                    self.emit_operand(k, f"{n.name}()")
            return
        raise SqlError(f"unsupported expression node {n.op}")

    # -- decimal columns (Spark 2.2 DecimalPrecision: exact against integral / decimal literals,
    #    through Cast(AS DOUBLE) against doubles)
    def _scale_of(self, n: Node) -> int:
        return N.decimal_scale(self.schema[self.schema.resolve(n.name)].dtype)

    def _emit_dec_cmp(self, sym: str, a: Node, ta: str, b: Node, tb: str) -> bool:
        """Emits a comparison with a decimal column operand; False when it is not one of the forms
        handled here (the generic path then raises or casts)."""
        if ta == "dec" and tb == "dec":
            raise SqlError("comparisons of two decimal values are not supported by the engine")
        col, lit, op = (a, b, sym) if ta == "dec" else (b, a, _FLIP.get(sym, sym))
        tl = tb if ta == "dec" else ta
        if tl in ("float", "str") and _exact_literal(lit) is None:
            return False  # double / string: both sides as double (Cast(decimal AS DOUBLE))
        if tl == "null":
            self.words.append(_CMP[sym])
            self.emit(a)
            self.emit(b)
            return True
        exact = _exact_literal(lit)
        if exact is None:
            raise SqlError("a decimal column compared with a non-literal value is not supported by "
                           "the engine")
        from fractions import Fraction
        t = Fraction(exact) * 10 ** self._scale_of(col)
        if t.denominator == 1:
            op, v = op, int(t)
        elif op in ("<", "<="):  # x < t  <=>  x <= floor(t)  (x an integer)
            op, v = "<=", t.numerator // t.denominator
        elif op in (">", ">="):
            op, v = ">=", -((-t.numerator) // t.denominator)
        else:  # =, <>, <=> against a value no column value equals
            v = _DEC_LIMIT
        self.words.append(_CMP[op])
        self.emit(col)
        self.words.extend(_dec128_words(v))
        return True

    def _emit_dec_in(self, x: Node, items: List[Node]) -> None:
        from fractions import Fraction
        sc = self._scale_of(x)
        words = []
        for it in items:
            if self.type_of(it) == "null":
                words.append(N.X_NULL)
                continue
            exact = _exact_literal(it)
            if exact is None:
                raise SqlError("a decimal column IN a list of non-literal / double items is not "
                               "supported by the engine")
            t = Fraction(exact) * 10 ** sc
            words.extend(_dec128_words(int(t) if t.denominator == 1 else _DEC_LIMIT))
        self.words += [N.X_IN, len(items)]
        self.emit(x)
        self.words.extend(words)


_FLIP = {"<": ">", "<=": ">=", ">": "<", ">=": "<="}
_ARITH = {"+": N.AR_ADD, "-": N.AR_SUB, "*": N.AR_MUL, "/": N.AR_DIV, "%": N.AR_MOD}
_FUNC_CODE = {"abs": N.FN_ABS, "length": N.FN_LENGTH, "isnan": N.FN_ISNAN, "year": N.FN_YEAR,
              "month": N.FN_MONTH, "dayofmonth": N.FN_DAYOFMONTH, "to_date": N.FN_TO_DATE,
              "datediff": N.FN_DATEDIFF, "date_add": N.FN_DATE_ADD, "date_sub": N.FN_DATE_SUB}


_REGEX_CACHE = {}


def _compiled_regex(pattern: str, any_match: bool) -> bytes:
    """The automaton blob of a Java regex (deequ_amd/regex.py).  RLIKE (any_match) is find()
    including an empty match: a pattern that can match the empty string then matches every row."""
    from .regex import PatternNotSupported, accept_all, compile_java_regex, nullable_pattern
    key = (pattern, any_match)
    if key not in _REGEX_CACHE:
        try:
            if any_match and nullable_pattern(pattern):
                _REGEX_CACHE[key] = accept_all(pattern).blob()
            else:
                _REGEX_CACHE[key] = compile_java_regex(pattern).blob()
        except PatternNotSupported as e:
            raise SqlError(f"regex /{pattern}/: {e}") from e
    return _REGEX_CACHE[key]


def _common_cmp_type(ta: str, tb: str) -> Optional[str]:
    if ta == "null" or tb == "null":
        return None
    if "dec" in (ta, tb) and ({ta, tb} - {"dec"}) <= {"float", "str"}:
        return "float"  # decimal vs double (or a string cast to double): Cast(decimal AS DOUBLE)
    if ta == tb:
        return ta if ta != "int" else None
    if {ta, tb} <= {"int", "float"}:
        return "float"
    if "str" in (ta, tb) and ({ta, tb} & {"int", "float"}):
        return "float"  # Spark 2.2 PromoteStrings: string side cast to double
    if "bool" in (ta, tb):
        raise SqlError(f"cannot compare {ta} with {tb}")
    return None


@dataclass
class CompiledExpr:
    sql: str
    words: List[int]
    columns: List[str]


def compile_expr(sql: str, schema, col_index) -> CompiledExpr:
    """Parses and types ``sql`` against ``schema``; ``col_index(name)`` returns the plan column
    index of a (resolved) column name."""
    node = parse(sql)
    em = _Emitter(schema, col_index)
    t = em.type_of(node) if node.op != "col" else em.type_of(node)
    if t not in ("bool", "null") and node.op in ("col", "lit", "arith", "neg", "func"):
        if t != "bool":
            raise SqlError(f"expression '{sql}' is not a predicate")
    em.emit(node)
    return CompiledExpr(sql, em.words, em.columns)


def referenced_columns(sql: str) -> List[str]:
    out = []

    def walk(n: Node):
        if n.op == "col" and n.name not in out:
            out.append(n.name)
        for k in n.kids:
            walk(k)

    walk(parse(sql))
    return out
