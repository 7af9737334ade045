"""ORACLE -- test infrastructure only.  A CPU restatement of deequ's metric computation over Spark
2.2 semantics, used by tests/ and bench.py's cpu_baseline as the checker.  The product (deequ_amd)
never imports this module.

Each function follows the cited reference file:line (prefix M/ = /root/reference/src/main/scala/
com/amazon/deequ/).  Third-party semantics restated from Spark 2.2.2 (not vendored in the
reference): CentralMomentAgg / Corr update+merge, Count/Sum/Min/Max, XXH64
(checked against the `xxhash` 3.8.1 package), HyperLogLogPlusPlus register update, cast-to-string.

Data model: a table is a dict {column: list of python values, None = NULL} plus a dict of Spark
type names {column: "long" | "int" | "double" | "float" | "string" | "boolean" | "decimal(p,s)" |
"date" | "timestamp"}.  Decimal values are decimal.Decimal, dates datetime.date, timestamps
datetime.datetime (UTC, naive) -- the oracle's own representations, independent of the engine's
unscaled integers / day and microsecond counts.  Rows are
processed sequentially per "partition" (Spark's per-task update loop), and partitions are merged
with the aggregate's merge rule -- so the oracle reproduces Spark's evaluation order, not just its
mathematics.

Parity pinning: tests/test_oracle_golden.py checks this oracle against every known answer the
reference's own tests hold (tests/golden/reference_known_answers.json, each with its file:line).
"""
from __future__ import annotations

import math
import re
import struct
from typing import Dict, List, Optional, Sequence, Tuple

import datetime
import decimal
from decimal import Decimal

import xxhash

INT_TYPES = {"byte", "short", "int", "long"}
NUM_TYPES = INT_TYPES | {"float", "double"}
# exact decimal arithmetic: 100 significant digits hold any sum of decimal(38) values
_DEC_CTX = decimal.Context(prec=100)


def decimal_ps(ty: str):
    """(precision, scale) of an oracle type "decimal(p,s)", else None."""
    m = re.match(r"^decimal\((\d+),(\d+)\)$", ty or "")
    return (int(m.group(1)), int(m.group(2))) if m else None


def unscaled(v: Decimal, scale: int) -> int:
    """The unscaled integer of a decimal value at `scale` (the value must have at most that many
    fraction digits, as a column of that DecimalType holds)."""
    u = v.scaleb(scale, context=_DEC_CTX)
    if u != u.to_integral_value():
        raise ValueError(f"{v} has more than {scale} fraction digits")
    return int(u)

# ------------------------------------------------------------------------------------------------
# SQL predicates (Spark SQL subset, three-valued logic) -- an independent little evaluator
# ------------------------------------------------------------------------------------------------
_TOK = re.compile(r"\s*(?:((?:\d+\.\d*(?:[eE][+-]?\d+)?|\d+(?:[eE][+-]?\d+)?)[dD]?)(?![A-Za-z_])|('(?:[^']|'')*')|"
                  r"(<=>|<=|>=|<>|!=|==|=|<|>|\(|\)|,|-)|([A-Za-z_][A-Za-z0-9_]*))")


def _tokens(s: str):
    pos, out = 0, []
    s = s.strip()
    while pos < len(s):
        m = _TOK.match(s, pos)
        if not m or m.end() == pos:
            raise ValueError(f"oracle cannot parse {s[pos:]!r}")
        pos = m.end()
        num, st, op, ident = m.groups()
        if num is not None:
            # Spark 2.2 types a fractional / exponent literal DecimalType: exact (a double column
            # compares it as a double, _cmp3); a D suffix makes a DoubleType literal
            if num[-1] in "dD":
                out.append(("num", float(num[:-1])))
            else:
                out.append(("num", Decimal(num) if any(c in num for c in ".eE") else int(num)))
        elif st is not None:
            out.append(("str", st[1:-1].replace("''", "'")))
        elif op is not None:
            out.append(("op", op))
        else:
            out.append(("id", ident))
    return out


class _P:
    def __init__(self, toks):
        self.t, self.i = toks, 0

    def peek(self):
        return self.t[self.i] if self.i < len(self.t) else (None, None)

    def kw(self, w):
        k, v = self.peek()
        return k == "id" and v.upper() == w

    def take(self):
        self.i += 1
        return self.t[self.i - 1]

    def expr(self):
        n = self.conj()
        while self.kw("OR"):
            self.take()
            n = ("or", n, self.conj())
        return n

    def conj(self):
        n = self.neg()
        while self.kw("AND"):
            self.take()
            n = ("and", n, self.neg())
        return n

    def neg(self):
        if self.kw("NOT"):
            self.take()
            return ("not", self.neg())
        return self.pred()

    def pred(self):
        a = self.atom()
        k, v = self.peek()
        if k == "op" and v in ("=", "==", "<>", "!=", "<", "<=", ">", ">=", "<=>"):
            self.take()
            return ("cmp", {"==": "=", "!=": "<>"}.get(v, v), a, self.atom())
        if self.kw("IS"):
            self.take()
            neg = False
            if self.kw("NOT"):
                self.take()
                neg = True
            self.take()  # NULL
            return ("isnotnull" if neg else "isnull", a)
        neg = False
        if self.kw("NOT"):
            self.take()
            neg = True
        if self.kw("IN"):
            self.take()
            self.take()  # (
            items = [self.atom()]
            while self.peek() == ("op", ","):
                self.take()
                items.append(self.atom())
            self.take()  # )
            n = ("in", a, items)
            return ("not", n) if neg else n
        if self.kw("BETWEEN"):
            self.take()
            lo = self.atom()
            self.take()  # AND
            hi = self.atom()
            n = ("and", ("cmp", ">=", a, lo), ("cmp", "<=", a, hi))
            return ("not", n) if neg else n
        return a

    def atom(self):
        k, v = self.take()
        if k == "op" and v == "(":
            n = self.expr()
            self.take()
            return n
        if k == "op" and v == "-":
            _, num = self.take()
            return ("lit", -num)
        if k in ("num", "str"):
            return ("lit", v)
        if v.upper() == "NULL":
            return ("lit", None)
        if v.upper() in ("TRUE", "FALSE"):
            return ("lit", v.upper() == "TRUE")
        return ("col", v)


def parse_predicate(sql: str):
    return _P(_tokens(sql)).expr()


_JAVA_DOUBLE = re.compile(r"^[+-]?(?:NaN|Infinity|(?:[0-9]+\.?[0-9]*|\.[0-9]+)(?:[eE][+-]?[0-9]+)?[fFdD]?)\Z")


def _to_double(v):
    """Spark 2.2 Cast(StringType -> DoubleType) is `s.toString.toDouble` with NULL on a
    NumberFormatException, i.e. java.lang.Double.parseDouble: characters <= U+0020 trimmed, an
    optional sign, `NaN` / `Infinity` in exactly that case, decimal digits with an optional
    exponent and an optional f / F / d / D suffix ("1.5d" is 1.5).  Python's float() differs on
    each of these ("nan", "inf", "1_0" parse, "1.5d" does not), so the grammar is restated here;
    Java's hexadecimal floating-point strings are not."""
    if isinstance(v, str):
        s = v.strip("".join(chr(c) for c in range(33)))
        if not _JAVA_DOUBLE.match(s):
            return None
        return float(s.rstrip("fFdD") if s[-1] in "fFdD" else s)
    return float(v)


def _cmp3(a, b) -> Optional[int]:
    """Spark ordering: numbers NaN-safe (NaN largest, NaN = NaN), strings bytewise UTF-8."""
    if isinstance(a, str) and isinstance(b, str):
        ab, bb = a.encode(), b.encode()
        return (ab > bb) - (ab < bb)
    if isinstance(a, str) or isinstance(b, str):
        # Spark 2.2 PromoteStrings: cast the string side to double
        a, b = _to_double(a), _to_double(b)
        if a is None or b is None:
            return None
    if isinstance(a, bool) or isinstance(b, bool):
        return (a > b) - (a < b)
    if isinstance(a, float) or isinstance(b, float):  # (a decimal vs a double: Cast AS DOUBLE)
        a, b = float(a), float(b)
        an, bn = math.isnan(a), math.isnan(b)
        if (an and bn) or a == b:
            return 0
        if an:
            return 1
        if bn:
            return -1
        return 1 if a > b else -1
    return (a > b) - (a < b)


def eval_predicate(node, row: Dict[str, object]):
    """Evaluates to True / False / None (NULL)."""
    op = node[0]
    if op == "lit":
        return node[1]
    if op == "col":
        name = node[1]
        if name not in row:
            low = {k.lower(): k for k in row}
            if name.lower() not in low:
                raise KeyError(f"cannot resolve {name}")
            name = low[name.lower()]
        return row[name]
    if op == "isnull":
        return eval_predicate(node[1], row) is None
    if op == "isnotnull":
        return eval_predicate(node[1], row) is not None
    if op == "not":
        v = eval_predicate(node[1], row)
        return None if v is None else not v
    if op == "and":
        a, b = eval_predicate(node[1], row), eval_predicate(node[2], row)
        if a is False or b is False:
            return False
        if a is None or b is None:
            return None
        return True
    if op == "or":
        a, b = eval_predicate(node[1], row), eval_predicate(node[2], row)
        if a is True or b is True:
            return True
        if a is None or b is None:
            return None
        return False
    if op == "cmp":
        sym, a, b = node[1], eval_predicate(node[2], row), eval_predicate(node[3], row)
        if sym == "<=>":
            if a is None or b is None:
                return a is None and b is None
            return _cmp3(a, b) == 0
        if a is None or b is None:
            return None
        c = _cmp3(a, b)
        if c is None:
            return None
        return {"=": c == 0, "<>": c != 0, "<": c < 0, "<=": c <= 0, ">": c > 0, ">=": c >= 0}[sym]
    if op == "in":
        x = eval_predicate(node[1], row)
        if x is None:
            return None
        items = [eval_predicate(i, row) for i in node[2]]
        saw_null = False
        for it in items:
            if it is None:
                saw_null = True
                continue
            if isinstance(x, str) != isinstance(it, str):
                # Spark 2.2 InConversion (TypeCoercion.scala): findWiderCommonType promotes a
                # numeric / string mix to StringType and casts BOTH sides to it, so a number meets
                # a string item as its cast to string -- 1 IN ('1') is TRUE, 1 IN ('01') and
                # 1 IN ('1.0') are FALSE (a double prints as Double.toString; a float column's
                # Float.toString is not restated: rows carry no column types here)
                if isinstance(x, str):
                    it = str(it)
                elif isinstance(x, bool):
                    raise ValueError("boolean IN (strings): Spark raises an AnalysisException")
                elif isinstance(x, float):
                    if java_double_to_string(x) == it:
                        return True
                    continue
                else:
                    if str(x) == it:
                        return True
                    continue
            if _cmp3(x, it) == 0:
                return True
        return None if saw_null else False
    raise ValueError(op)


# ------------------------------------------------------------------------------------------------
# Table helpers
# ------------------------------------------------------------------------------------------------
class OTable:
    def __init__(self, columns: Dict[str, list], types: Dict[str, str]):
        self.columns = columns
        self.types = types
        self.n = len(next(iter(columns.values()))) if columns else 0

    def rows(self):
        names = list(self.columns)
        for i in range(self.n):
            yield {k: self.columns[k][i] for k in names}

    def partitions(self, k: int) -> List["OTable"]:
        """Contiguous row partitions (Spark's partitions of a parallelized collection)."""
        bounds = [self.n * j // k for j in range(k + 1)]
        return [OTable({c: v[bounds[j]:bounds[j + 1]] for c, v in self.columns.items()}, self.types)
                for j in range(k)]


def _sel(table: OTable, column: str, where: Optional[str]):
    """conditionalSelection (M/analyzers/Analyzer.scala:385-402): when(where, col) -- NULL where
    the filter is not TRUE."""
    pred = parse_predicate(where) if where else None
    vals = table.columns[column]
    if pred is None:
        return list(vals)
    out = []
    for i, r in enumerate(table.rows()):
        out.append(vals[i] if eval_predicate(pred, r) is True else None)
    return out


def _to_long(v):
    return int(v)


def _wrap64(x: int) -> int:
    x &= (1 << 64) - 1
    return x - (1 << 64) if x >= (1 << 63) else x


# ------------------------------------------------------------------------------------------------
# Scan aggregations: one partition's aggregation buffer at a time, then the merge
# ------------------------------------------------------------------------------------------------
def agg_count_all(t: OTable) -> int:
    return t.n


def agg_conditional_count(t: OTable, where: Optional[str]) -> Optional[int]:
    """conditionalCount (Analyzer.scala:404-408): sum(expr(where).cast(Long)) else count(*)."""
    if where is None:
        return t.n
    pred = parse_predicate(where)
    vals = [eval_predicate(pred, r) for r in t.rows()]
    nn = [v for v in vals if v is not None]
    return None if not nn else sum(1 for v in nn if v)


def agg_sum_notnull(t: OTable, column: str, where: Optional[str]) -> Optional[int]:
    """Completeness numerator (Completeness.scala:44): sum(isNotNull(when(where,col)).cast(Int))."""
    if t.n == 0:
        return None
    return sum(1 for v in _sel(t, column, where) if v is not None)


def agg_compliance(t: OTable, predicate: str, where: Optional[str]) -> Optional[int]:
    """Compliance.scala:47-49: sum(when(where, expr(predicate)).cast(Int))."""
    p = parse_predicate(predicate)
    w = parse_predicate(where) if where else None
    vals = []
    for r in t.rows():
        if w is not None and eval_predicate(w, r) is not True:
            vals.append(None)
        else:
            vals.append(eval_predicate(p, r))
    nn = [v for v in vals if v is not None]
    return None if not nn else sum(1 for v in nn if v)


def agg_sum_decimal(t: OTable, column: str, where: Optional[str]) -> Optional[Decimal]:
    """Spark 2.2 Sum over decimal(p, s): the exact sum in the result type decimal(min(p + 10, 38),
    s), NULL when it does not fit (Cast's changePrecision; a per-partition overflow inside Spark
    is not restated -- parity unpinned)."""
    p, sc = decimal_ps(t.types[column])
    vals = [v for v in _sel(t, column, where) if v is not None]
    if not vals:
        return None
    acc = Decimal(0)
    for v in vals:
        acc = _DEC_CTX.add(acc, v)
    rp = min(p + 10, 38)
    if abs(unscaled(acc, sc)) >= 10 ** rp:
        return None
    return acc


def agg_sum(t: OTable, column: str, where: Optional[str]) -> Optional[float]:
    """Sum.scala:35: sum(col).cast(Double); integral columns sum as a wrapping Long first; a
    decimal column sums exactly and casts once (Decimal.toDouble: correctly rounded)."""
    if decimal_ps(t.types[column]):
        d = agg_sum_decimal(t, column, where)
        return None if d is None else float(d)
    vals = [v for v in _sel(t, column, where) if v is not None]
    if not vals:
        return None
    if t.types[column] in INT_TYPES:
        acc = 0
        for v in vals:
            acc = _wrap64(acc + int(v))
        return float(acc)
    acc = 0.0
    for v in vals:
        acc += float(v)
    return acc


def _nan_safe_lt(a: float, b: float) -> bool:
    return _cmp3(a, b) < 0


def agg_min(t: OTable, column: str, where: Optional[str]) -> Optional[float]:
    """Minimum.scala:36 -- Spark's Min in the column type (NaN largest), then cast to double."""
    vals = [v for v in _sel(t, column, where) if v is not None]
    if not vals:
        return None
    m = vals[0]
    for v in vals[1:]:
        if _cmp3(v, m) < 0:
            m = v
    return float(m)


def agg_max(t: OTable, column: str, where: Optional[str]) -> Optional[float]:
    vals = [v for v in _sel(t, column, where) if v is not None]
    if not vals:
        return None
    m = vals[0]
    for v in vals[1:]:
        if _cmp3(v, m) > 0:
            m = v
    return float(m)


def moments_update(state, x: float):
    """Spark 2.2 CentralMomentAgg.updateExpressions (momentOrder 2)."""
    n, avg, m2 = state
    n2 = n + 1.0
    delta = x - avg
    delta_n = delta / n2
    avg2 = avg + delta_n
    m22 = m2 + delta * (delta - delta_n)
    return (n2, avg2, m22)


def moments_merge(a, b):
    """CentralMomentAgg.mergeExpressions == StandardDeviationState.sum
    (M/analyzers/StandardDeviation.scala:37-44)."""
    n1, avg1, m21 = a
    n2, avg2, m22 = b
    n = n1 + n2
    delta = avg2 - avg1
    delta_n = 0.0 if n == 0.0 else delta / n
    return (n, avg1 + delta_n * n2, m21 + m22 + delta * delta_n * n1 * n2)


def agg_stddev(t: OTable, column: str, where: Optional[str], partitions: int = 1):
    """stateful_stddev_pop (M/analyzers/catalyst/StatefulStdDevPop.scala:24-34)."""
    state = (0.0, 0.0, 0.0)
    for p in t.partitions(partitions):
        s = (0.0, 0.0, 0.0)
        for v in _sel(p, column, where):
            if v is not None:
                s = moments_update(s, float(v))
        state = moments_merge(state, s)
    return state


def corr_update(state, x: float, y: float):
    """Spark 2.2 Corr.updateExpressions."""
    n, xa, ya, ck, xmk, ymk = state
    n2 = n + 1.0
    dx = x - xa
    dxn = dx / n2
    dy = y - ya
    dyn = dy / n2
    xa2 = xa + dxn
    ya2 = ya + dyn
    ck2 = ck + dx * (y - ya2)
    xmk2 = xmk + dx * (x - xa2)
    ymk2 = ymk + dy * (y - ya2)
    return (n2, xa2, ya2, ck2, xmk2, ymk2)


def corr_merge(a, b):
    """Corr.mergeExpressions == CorrelationState.sum (M/analyzers/Correlation.scala:37-52)."""
    n1, xa1, ya1, ck1, xm1, ym1 = a
    n2, xa2, ya2, ck2, xm2, ym2 = b
    n = n1 + n2
    dx = xa2 - xa1
    dxn = 0.0 if n == 0.0 else dx / n
    dy = ya2 - ya1
    dyn = 0.0 if n == 0.0 else dy / n
    return (n, xa1 + dxn * n2, ya1 + dyn * n2, ck1 + ck2 + dx * dyn * n1 * n2,
            xm1 + xm2 + dx * dxn * n1 * n2, ym1 + ym2 + dy * dyn * n1 * n2)


def agg_corr(t: OTable, cx: str, cy: str, where: Optional[str], partitions: int = 1):
    state = (0.0,) * 6
    for p in t.partitions(partitions):
        s = (0.0,) * 6
        for x, y in zip(_sel(p, cx, where), _sel(p, cy, where)):
            if x is not None and y is not None:
                s = corr_update(s, float(x), float(y))
        state = corr_merge(state, s)
    return state


# ------------------------------------------------------------------------------------------------
# XXH64 / HLL++ (StatefulHyperloglogPlus.scala:87-146, 150-255)
# ------------------------------------------------------------------------------------------------
P = 9
M = 1 << P
NUM_WORDS = 52


_EPOCH_DATE = datetime.date(1970, 1, 1)
_EPOCH_TS = datetime.datetime(1970, 1, 1)


def days_of(d: datetime.date) -> int:
    return (d - _EPOCH_DATE).days


def micros_of(ts: datetime.datetime) -> int:
    delta = ts - _EPOCH_TS
    return (delta.days * 86400 + delta.seconds) * 1000000 + delta.microseconds


def spark_xxhash64(value, spark_type: str, seed: int = 42) -> int:
    """XxHash64Function.hash(v, type, seed) (Spark 2.2 HashExpression): standard XXH64 over the
    little-endian bytes: long/double as 8 bytes (double via doubleToLongBits, NaN canonical),
    int/short/byte/boolean/float as 4 bytes (float via floatToIntBits), string as its UTF-8; a
    date as its int days (hashInt), a timestamp as its long microseconds (hashLong), a decimal of
    precision <= 18 as its unscaled long (hashLong), above as BigInteger.toByteArray of the unscaled
    value (the minimal big-endian two's complement, hashUnsafeBytes)."""
    ps = decimal_ps(spark_type)
    if ps:
        u = unscaled(value, ps[1])
        if ps[0] <= 18:
            return xxhash.xxh64_intdigest(struct.pack("<q", u), seed=seed)
        n = ((u if u >= 0 else ~u).bit_length()) // 8 + 1
        return xxhash.xxh64_intdigest(u.to_bytes(n, "big", signed=True), seed=seed)
    if spark_type == "date":
        return xxhash.xxh64_intdigest(struct.pack("<i", days_of(value)), seed=seed)
    if spark_type == "timestamp":
        return xxhash.xxh64_intdigest(struct.pack("<q", micros_of(value)), seed=seed)
    if spark_type == "string":
        data = value.encode("utf-8")
    elif spark_type in ("long",):
        data = struct.pack("<q", int(value))
    elif spark_type in ("int", "short", "byte"):
        data = struct.pack("<i", int(value))
    elif spark_type == "boolean":
        data = struct.pack("<i", 1 if value else 0)
    elif spark_type == "double":
        d = float(value)
        data = struct.pack("<Q", 0x7ff8000000000000) if math.isnan(d) else struct.pack("<d", d)
    elif spark_type == "float":
        if math.isnan(value):
            data = struct.pack("<I", 0x7fc00000)
        else:
            data = struct.pack("<f", value)
    else:
        raise ValueError(spark_type)
    return xxhash.xxh64_intdigest(data, seed=seed)


def hll_registers(values, spark_type: str) -> List[int]:
    regs = [0] * M
    for v in values:
        if v is None:
            continue
        x = spark_xxhash64(v, spark_type)
        idx = x >> (64 - P)
        w = ((x << P) & ((1 << 64) - 1)) | (1 << (P - 1))
        pw = 64 - w.bit_length() + 1
        if pw > regs[idx]:
            regs[idx] = pw
    return regs


def hll_words(regs: Sequence[int]) -> List[int]:
    words = []
    for w in range(NUM_WORDS):
        v = 0
        for i in range(10):
            idx = w * 10 + i
            if idx < M:
                v |= (regs[idx] & 0x3F) << (6 * i)
        words.append(_wrap64(v))
    return words


def _jvm_int_one_shl(m: int) -> int:
    """Scala `1 << Midx` with `1: Int` and `Midx: Long` (StatefulHyperloglogPlus.scala:220): the
    JVM shifts the 32-bit int by Midx & 31 (JLS 15.19) and the result wraps to a signed int, so
    1 << 31 == Int.MinValue and 1 << 32 == 1."""
    v = (1 << (m & 31)) & 0xFFFFFFFF
    return v - (1 << 32) if v >= (1 << 31) else v


def hll_count(words: Sequence[int]) -> Tuple[float, bool]:
    """HyperLogLogPlusPlusUtils.count; returns (estimate, needed_bias_tables)."""
    z_inv, V = 0.0, 0.0
    idx = 0
    for word in words:
        word &= (1 << 64) - 1
        for i in range(10):
            if idx >= M:
                break
            m = (word >> (6 * i)) & 0x3F
            z_inv += 1.0 / _jvm_int_one_shl(m)
            if m == 0:
                V += 1.0
            idx += 1
    alpha_m2 = (0.7213 / (1.0 + 1.079 / M)) * M * M
    e = alpha_m2 / z_inv
    biased = e < 5.0 * M
    if V > 0:
        H = M * math.log(M / V)
        if H <= 400.0:
            return java_math_round(H), False
    return java_math_round(e), biased


def java_math_round(a: float) -> float:
    """JDK 8 Math.round(double) as a double: (long) floor(a + 0.5), except 0.49999999999999994
    rounds to 0; the (long) cast saturates and maps NaN to 0 (JLS 5.1.3)."""
    if a != a:
        return 0.0
    if a == 0.49999999999999994:
        return 0.0
    f = a + 0.5
    if f >= 2.0 ** 63:
        return float(2 ** 63 - 1)
    if f <= -(2.0 ** 63):
        return float(-(2 ** 63))
    return float(math.floor(f))


def agg_hll(t: OTable, column: str, where: Optional[str]) -> List[int]:
    return hll_words(hll_registers(_sel(t, column, where), t.types[column]))


# ------------------------------------------------------------------------------------------------
# Frequencies (GroupingAnalyzers.scala:53-80) and the aggregations over them
# ------------------------------------------------------------------------------------------------
def _group_key(v, spark_type):
    if spark_type in ("double", "float") and v is not None:
        return struct.pack("<d", float(v))  # Spark 2.2 groups by binary value
    return v


def frequencies(t: OTable, columns: Sequence[str]) -> Dict[tuple, int]:
    freq: Dict[tuple, int] = {}
    cols = [t.columns[c] for c in columns]
    for i in range(t.n):
        key = tuple(c[i] for c in cols)
        if any(k is None for k in key):
            continue
        key = tuple(_group_key(k, t.types[c]) for k, c in zip(key, columns))
        freq[key] = freq.get(key, 0) + 1
    return freq


def uniqueness(freq, num_rows):
    """Uniqueness.scala:29 (None == NULL -> empty state)."""
    if not freq:
        return None
    return float(sum(1 for c in freq.values() if c == 1)) / num_rows


def distinctness(freq, num_rows):
    if not freq:
        return None
    return float(sum(1 for c in freq.values() if c >= 1)) / num_rows


def unique_value_ratio(freq):
    if not freq:
        return None
    return float(sum(1 for c in freq.values() if c == 1)) / float(len(freq))


def count_distinct(freq):
    return float(len(freq))


def entropy(freq, num_rows):
    """Entropy.scala:33-40 (summed in sorted-key order)."""
    if not freq:
        return None
    total = 0.0
    for c in freq.values():
        p = c / num_rows
        total += -p * math.log(p) if c else 0.0
    return total


def _java_layout(sign: str, digits: str, e10: int) -> str:
    """java.lang.Double.toString's layout of a shortest digit string whose leading digit has
    exponent e10: plain ddd.ddd for e10 in [-3, 6], else d.dddE<e10>; one fraction digit at least."""
    digits = digits.rstrip("0") or "0"
    if 0 <= e10 < 7:
        ip = (digits + "0" * 7)[:e10 + 1]
        return sign + ip + "." + (digits[e10 + 1:] or "0")
    if -3 <= e10 < 0:
        return sign + "0." + "0" * (-e10 - 1) + digits
    return sign + digits[0] + "." + (digits[1:] or "0") + "E" + str(e10)


def java_double_to_string(d: float) -> str:
    """Double.toString (Spark 2.2 Cast(DoubleType -> StringType)): Python's repr gives the shortest
    round-trip digits (David Gay's dtoa), laid out as Java does.  Double.MIN_VALUE prints 4.9E-324
    (FloatingDecimal's two-digit estimate); JDK 8's other non-shortest outputs are unpinned."""
    if math.isnan(d):
        return "NaN"
    if math.isinf(d):
        return "Infinity" if d > 0 else "-Infinity"
    if d == 0.0:
        return "-0.0" if math.copysign(1.0, d) < 0 else "0.0"
    if abs(d) == 5e-324:
        return ("-" if d < 0 else "") + "4.9E-324"
    from decimal import Decimal
    t = Decimal(repr(abs(d))).as_tuple()
    return _java_layout("-" if d < 0 else "", "".join(map(str, t.digits)),
                        t.exponent + len(t.digits) - 1)


def java_float_to_string(f: float) -> str:
    """Float.toString (Cast(FloatType -> StringType)): numpy's shortest float32 digits (Dragon4
    unique mode), Java's layout; Float.MIN_VALUE prints 1.4E-45."""
    import numpy as np
    if math.isnan(f):
        return "NaN"
    if math.isinf(f):
        return "Infinity" if f > 0 else "-Infinity"
    if f == 0.0:
        return "-0.0" if math.copysign(1.0, f) < 0 else "0.0"
    if abs(f) == float(np.float32(1e-45)):
        return ("-" if f < 0 else "") + "1.4E-45"
    sci = np.format_float_scientific(np.float32(abs(f)), unique=True, trim="-")
    mant, _, exp = sci.partition("e")
    return _java_layout("-" if f < 0 else "", mant.replace(".", ""), int(exp))


def java_bigdecimal_to_string(v: Decimal, scale: int) -> str:
    """java.math.BigDecimal.toString (Spark 2.2 Decimal.toString) of a value at `scale`: the
    unscaled digits, plain when the adjusted exponent (digits - 1 - scale) >= -6 (with a '.'
    before the last `scale` digits), else one digit, '.', the rest, 'E' and the exponent."""
    u = unscaled(v, scale)
    digits = str(abs(u))
    sign = "-" if u < 0 else ""
    adjusted = len(digits) - 1 - scale
    if scale == 0:
        return sign + digits
    if adjusted >= -6:
        if len(digits) > scale:
            return sign + digits[:-scale] + "." + digits[-scale:]
        return sign + "0." + "0" * (scale - len(digits)) + digits
    body = digits[0] + ("." + digits[1:] if len(digits) > 1 else "")
    return sign + body + "E" + str(adjusted)


def java_date_to_string(d: datetime.date) -> str:
    """DateTimeUtils.dateToString: yyyy-MM-dd (years 1..9999)."""
    return f"{d.year:04d}-{d.month:02d}-{d.day:02d}"


def java_timestamp_to_string(ts: datetime.datetime) -> str:
    """DateTimeUtils.timestampToString in UTC: yyyy-MM-dd HH:mm:ss, then java.sql.Timestamp's
    fraction (the nanoseconds, trailing zeros dropped) unless it is ".0"."""
    base = f"{ts.year:04d}-{ts.month:02d}-{ts.day:02d} {ts.hour:02d}:{ts.minute:02d}:{ts.second:02d}"
    if ts.microsecond:
        return base + "." + f"{ts.microsecond * 1000:09d}".rstrip("0")
    return base


def java_to_string(v, ty: str) -> str:
    """Spark's cast to string of a non-NULL value of oracle type `ty`."""
    ps = decimal_ps(ty)
    if ps:
        return java_bigdecimal_to_string(v, ps[1])
    if ty == "date":
        return java_date_to_string(v)
    if ty == "timestamp":
        return java_timestamp_to_string(v)
    if ty == "string":
        return v
    if ty == "boolean":
        return "true" if v else "false"
    if ty == "double":
        return java_double_to_string(float(v))
    if ty == "float":
        return java_float_to_string(float(v))
    return str(int(v))


def histogram(t: OTable, column: str) -> Tuple[Dict[str, int], int]:
    """Histogram.scala:54-79: cast(col as string), NULL -> "NullValue", group, count."""
    ty = t.types[column]
    out: Dict[str, int] = {}
    for v in t.columns[column]:
        s = "NullValue" if v is None else java_to_string(v, ty)
        out[s] = out.get(s, 0) + 1
    return out, t.n


# ------------------------------------------------------------------------------------------------
# PatternMatch (M/analyzers/PatternMatch.scala:41-53): Java's Pattern.find() restated with
# Python's backtracking `re` (same leftmost-first semantics), the pattern translated from Java
# syntax where the two differ.  Test infrastructure only.
# ------------------------------------------------------------------------------------------------
_JAVA_DOLLAR = "(?:\\Z|(?=\\r\\n\\Z)|(?<!\\r)(?=\\n\\Z)|(?=[\\r\\x85\\u2028\\u2029]\\Z))"


def _java_word_class() -> str:
    """Java's Bound.isWord (Pattern.java, JDK 8): '_' or Character.isLetterOrDigit -- Unicode
    categories L* and Nd -- as a Python character class over every code point."""
    import unicodedata
    parts, start = [], None
    for cp in range(0x110000):
        cat = unicodedata.category(chr(cp))
        w = cp == 95 or cat[0] == "L" or cat == "Nd"
        if w and start is None:
            start = cp
        elif not w and start is not None:
            parts.append((start, cp - 1))
            start = None
    if start is not None:
        parts.append((start, 0x10FFFF))
    esc = lambda c: "\\U%08x" % c  # noqa: E731
    return "[" + "".join(esc(a) if a == b else esc(a) + "-" + esc(b) for a, b in parts) + "]"


_JAVA_WORD = None


_PY_DOT = {"": "[^\\n\\r\\u0085\\u2028\\u2029]", "d": "[^\\n]"}
# Pattern.java (JDK 8): Caret / UnixCaret (MULTILINE ^: the start, or after a line terminator --
# never between "\r\n" -- and never at the end), Dollar(true) / UnixDollar(true) (MULTILINE $:
# before a line terminator -- never between "\r\n" -- or at the end), UnixDollar(false)
_PY_CARET_M = "(?:\\A|(?<=[\\n\\x85\\u2028\\u2029])|(?<=\\r)(?!\\n))(?!\\Z)"
_PY_CARET_MD = "(?:\\A|(?<=\\n))(?!\\Z)"
_PY_DOLLAR_M = "(?:(?<!\\r)(?=\\n)|(?=[\\r\\x85\\u2028\\u2029])|\\Z)"
_PY_DOLLAR_MD = "(?=\\n|\\Z)"
_PY_DOLLAR_D = "(?:\\Z|(?=\\n\\Z))"


# Pattern.java (JDK 8): the US-ASCII POSIX classes of \p{...}, \h / \v
_JAVA_POSIX = {"Lower": "a-z", "Upper": "A-Z", "ASCII": "\\x00-\\x7f", "Alpha": "a-zA-Z",
               "Digit": "0-9", "Alnum": "0-9a-zA-Z", "Punct": "!-/:-@\\[-`{-~", "Graph": "!-~",
               "Print": " -~", "Blank": " \\t", "Cntrl": "\\x00-\\x1f\\x7f",
               "XDigit": "0-9a-fA-F", "Space": " \\t\\n\\x0b\\f\\r"}
_HSP = " \\t\\xa0\\u1680\\u180e\\u2000-\\u200a\\u202f\\u205f\\u3000"
_VSP = "\\n\\x0b\\f\\r\\x85\\u2028\\u2029"
_JAVA_HV = {"\\h": _HSP, "\\H": _HSP, "\\v": _VSP, "\\V": _VSP}


def _java_class_has_ops(p: str, i: int) -> bool:
    """Whether the class opening at p[i] holds a nested class or && (Java class set operations)."""
    j = i + 1
    if p.startswith("^", j):
        j += 1
    first = True
    while j < len(p):
        c = p[j]
        if c == "\\":
            j += 2
        elif c == "]" and not first:
            return False
        elif c == "[" or p.startswith("&&", j):
            return True
        else:
            j += 1
        first = False
    return False


def _java_class_to_py(p: str, i: int):
    """A Java class with nested classes / && (JDK 8 Pattern.clazz, non-negated) at p[i] -> a
    Python one-character expression: a union as an alternation of classes, A && B as the
    lookahead (?=A) before B.  Returns (expression, index after the class)."""
    i += 1
    assert not p.startswith("^", i), "a negated class with set operations is not restated"
    alts, plain, first = [], [], True

    def item(i):
        if p[i] != "\\":
            return p[i], i + 1
        e = p[i:i + 2]
        if e in ("\\p", "\\P"):
            j = p.index("}", i) if p.startswith("{", i + 2) else i + 2
            name = p[i + 3:j] if p.startswith("{", i + 2) else p[i + 2]
            assert e == "\\p", "\\P inside a class with set operations"
            return _JAVA_POSIX[name], j + 1
        if e in _JAVA_HV:
            assert e[1].islower()
            return _JAVA_HV[e], i + 2
        return e, i + 2

    def union(alts, plain):
        parts = list(alts) + (["[" + "".join(plain) + "]"] if plain else [])
        return "(?:" + "|".join(parts) + ")" if parts else None

    while True:
        c = p[i]
        if c == "]" and not first:
            i += 1
            break
        first = False
        if c == "[":
            sub, i = _java_class_to_py(p, i) if _java_class_has_ops(p, i) else _py_plain_class(p, i)
            alts.append(sub)
        elif p.startswith("&&", i):
            left = union(alts, plain)
            i += 2
            if p[i] == "[":
                right, i = (_java_class_to_py(p, i) if _java_class_has_ops(p, i)
                            else _py_plain_class(p, i))
            else:
                items = []
                while p[i] != "]" and not p.startswith("&&", i):
                    x, i = item(i)
                    items.append(x)
                right = "[" + "".join(items) + "]"
            alts, plain = [right if left is None else f"(?:(?={left}){right})"], []
        else:
            x, i = item(i)
            plain.append(x)
    return union(alts, plain) or "[^\\s\\S]", i


def _py_plain_class(p: str, i: int):
    """A plain Java class (no set operations) at p[i], copied as a Python class."""
    j = i + 1
    if p.startswith("^", j):
        j += 1
    first = True
    while True:
        if p[j] == "\\":
            j += 2
        elif p[j] == "]" and not first:
            return p[i:j + 1], j + 1
        else:
            j += 1
        first = False


def _java_remove_qe(p: str) -> str:
    """Pattern.java's RemoveQEQuoting: \\Q...\\E becomes its characters, each escaped."""
    out, i = [], 0
    while i < len(p):
        if p.startswith("\\Q", i):
            j = p.find("\\E", i + 2)
            j = len(p) if j < 0 else j
            out.append("".join(re.escape(ch) for ch in p[i + 2:j]))
            i = j + 2
        elif p[i] == "\\":
            out.append(p[i:i + 2])
            i += 2
        else:
            out.append(p[i])
            i += 1
    return "".join(out)


def java_regex_to_python(pattern: str) -> str:
    """Java -> Python `re` (used with re.ASCII, which gives Java's ASCII \\d \\w \\s):
    `.` outside a class excludes every Java line terminator (Python's excludes only \\n); `$` and
    `\\Z` are Java's Dollar (end, or before one final terminator, "\\r\\n" included, never
    between "\\r\\n"); `\\z` is the strict end; `\\b` is Java's Bound over Unicode letters and
    digits (Python's ASCII \\b would call every non-ASCII code point a non-word one).  Embedded
    flags i d m s x (and u without i) are tracked here with Java's scoping and each construct they
    change is written out explicitly, so Python's own flag semantics never apply."""
    global _JAVA_WORD
    pattern = _java_remove_qe(pattern)
    out, i, in_class = [], 0, False
    # Java's inline flags apply to the end of the enclosing group, alternatives included (Python's
    # apply to the whole pattern).  (?i) is restated as scoped (?i:...) groups closed at each '|'
    # and ')' of that group and re-opened after a '|' -- ASCII-only in Java without UNICODE_CASE,
    # as in Python under re.ASCII; d m s x are applied by the translation itself.
    scopes = [[]]
    fl = {"i": False, "d": False, "m": False, "s": False, "x": False, "u": False}
    saved = []  # the flags at each open group
    atom_at, n_atomic = None, 0  # where the last one-character atom's output starts
    closers = []  # per open group: what follows its ')' (an atomic group's backreference)
    while i < len(pattern):
        c = pattern[i]
        if fl["x"] and c in " \t\n\x0b\f\r":  # COMMENTS: white space ignored, classes too
            i += 1
            continue
        if fl["x"] and c == "#":  # ... and a comment up to the end of the line
            while i < len(pattern):
                i += 1
                if pattern[i - 1] == "\n" or (not fl["d"] and pattern[i - 1] in "\r\x85\u2028\u2029"):
                    break
            continue
        if not in_class:
            m = re.match(r"\(\?([idmsux]*)(?:-([idmsux]*))?([):])", pattern[i:])
            if m and (m.group(1) or m.group(2) is not None):
                new = dict(fl)
                for f in m.group(1):
                    new[f] = True
                for f in m.group(2) or "":
                    new[f] = False
                assert not (new["i"] and new["u"]), "UNICODE_CASE is not restated"
                opener = None
                if new["i"] != fl["i"]:
                    opener = "(?i:" if new["i"] else "(?-i:"
                if m.group(3) == ")":
                    if opener:
                        out.append(opener)
                        scopes[-1].append(opener)
                else:  # (?flags:...): a group of its own
                    saved.append(fl)
                    scopes.append([])
                    closers.append("")
                    out.append("(?:")
                    if opener:
                        out.append(opener)
                        scopes[-1].append(opener)
                fl = new
                i += m.end()
                continue
            if pattern.startswith("(?<", i) and pattern[i + 3:i + 4].isalpha():  # named group
                scopes.append([])
                saved.append(dict(fl))
                closers.append("")
                out.append("(?P<")
                i += 3
                continue
            if pattern.startswith("(?>", i):  # atomic group: the lookahead-and-backreference idiom
                scopes.append([])
                saved.append(dict(fl))
                closers.append(f"))(?P=_ag{n_atomic}))")  # (one group: a quantifier repeats it all)
                out.append(f"(?:(?=(?P<_ag{n_atomic}>(?:")
                n_atomic += 1
                atom_at = None
                i += 3
                continue
            if c == "(":
                scopes.append([])
                saved.append(dict(fl))
                closers.append("")
            elif c == ")" and len(scopes) > 1:
                out.append(")" * len(scopes.pop()))
                fl = saved.pop()
                out.append(")" + closers.pop())
                atom_at = None
                i += 1
                continue
            elif c == "|":
                out.append(")" * len(scopes[-1]))
                out.append("|")
                out.extend(scopes[-1])
                i += 1
                continue
        if not in_class:  # a possessive quantifier over the last atom: Python 3.10 has none, so
            # the atomic-group idiom (?=(?P<a>X*))(?P=a) -- the lookahead's preferred match, kept
            q = re.match(r"(?:[*+?]|\{\d+(?:,\d*)?\})\+", pattern[i:])
            if q and i > 0 and pattern[i - 1] != "(":
                assert atom_at is not None, "possessive quantifier over a group is not restated"
                atom = "".join(out[atom_at:])
                del out[atom_at:]
                out.append(f"(?=(?P<_pq{n_atomic}>{atom}{q.group(0)[:-1]}))(?P=_pq{n_atomic})")
                n_atomic += 1
                atom_at = None
                i += q.end()
                continue
            if c == "\\" or c == "[" or c == "." or c not in "()|*+?{}^$":
                atom_at = len(out)
            elif c in ")|(":
                atom_at = None
        if c == "\\":
            e = pattern[i:i + 2]
            if not in_class and e == "\\b":
                if _JAVA_WORD is None:
                    _JAVA_WORD = _java_word_class()
                w = _JAVA_WORD
                out.append(f"(?:(?<!{w})(?={w})|(?<={w})(?!{w}))")
            elif not in_class and e == "\\Z":
                out.append(_PY_DOLLAR_D if fl["d"] else _JAVA_DOLLAR)
            elif not in_class and e == "\\z":
                out.append("\\Z")
            elif e in ("\\p", "\\P"):  # the POSIX classes (US-ASCII)
                if pattern.startswith("{", i + 2):
                    j = pattern.index("}", i)
                    name = pattern[i + 3:j]
                else:
                    j, name = i + 2, pattern[i + 2]
                body = _JAVA_POSIX[name]
                assert not (in_class and e == "\\P"), "a negated property inside a class"
                out.append(body if in_class else ("[" if e == "\\p" else "[^") + body + "]")
                i = j + 1
                continue
            elif e in _JAVA_HV:
                body = _JAVA_HV[e]
                assert not (in_class and e[1].isupper()), "\\H / \\V inside a class"
                out.append(body if in_class else ("[^" if e[1].isupper() else "[") + body + "]")
            elif e == "\\R" and not in_class:  # LineEnding (JDK 8): atomic \r\n | one terminator
                out.append(f"(?:(?=(?P<_ag{n_atomic}>(?:\\r\\n|[{_VSP}])))(?P=_ag{n_atomic}))")
                n_atomic += 1
            elif e == "\\k":  # \k<name>
                j = pattern.index(">", i)
                out.append(f"(?P={pattern[i + 3:j]})")
                i = j + 1
                continue
            else:
                out.append(e)
            i += 2
            continue
        if in_class:
            if c == "]" and not (out and out[-1] in ("[", "[^")):
                in_class = False
            out.append(c)
        elif c == "[" and _java_class_has_ops(pattern, i):  # class set operations
            expr, i = _java_class_to_py(pattern, i)
            out.append(expr)
            continue
        elif c == "[":
            in_class = True
            if pattern.startswith("[^", i):
                out.append("[^")
                i += 2
                continue
            out.append(c)
        elif c == ".":
            out.append("(?s:.)" if fl["s"] else _PY_DOT["d" if fl["d"] else ""])
        elif c == "^":
            out.append((_PY_CARET_MD if fl["d"] else _PY_CARET_M) if fl["m"] else "\\A")
        elif c == "$":
            if fl["m"]:
                out.append(_PY_DOLLAR_MD if fl["d"] else _PY_DOLLAR_M)
            else:
                out.append(_PY_DOLLAR_D if fl["d"] else _JAVA_DOLLAR)
        else:
            out.append(c)
        i += 1
    out.append(")" * len(scopes[0]))
    return "".join(out)


def regex_find_nonempty(value, pattern: str) -> bool:
    """regexp_extract(value, pattern, 0) != "" (a NULL value gives False: otherwise(0))."""
    import re
    if value is None:
        return False
    m = re.search(java_regex_to_python(pattern), str(value), re.ASCII)
    return bool(m) and m.group(0) != ""


def agg_pattern_match(t: OTable, column: str, pattern: str, where: Optional[str]):
    """(sum of matches over the where-rows, conditionalCount(where)) -- the PatternMatch state."""
    vals = _sel(t, column, where)
    n = agg_conditional_count(t, where)
    if not n:
        return None
    pred = parse_predicate(where) if where else None
    hits = 0
    for i, r in enumerate(t.rows()):
        if pred is not None and eval_predicate(pred, r) is not True:
            continue
        v = vals[i]
        hits += regex_find_nonempty(None if v is None else java_to_string(v, t.types[column]),
                                    pattern)
    return hits, n


# ------------------------------------------------------------------------------------------------
# ApproxQuantile (M/analyzers/ApproxQuantile.scala:41-104) -> Spark 2.2 ApproximatePercentile:
# QuantileSummaries(relativeError) fed one value at a time; below its 50000-value head buffer the
# summary is one sorted-buffer insert followed by compress, then query.  Restated for tests.
# ------------------------------------------------------------------------------------------------
def spark_approx_quantile(values, quantile: float, relative_error: float = 0.01):
    """The reference's result for at most 50000 non-NULL values (None when there are none)."""
    import math
    # Java's Double.compare order: -0.0 before 0.0, NaN after everything
    xs = sorted((float(v) for v in values if v is not None),
                key=lambda x: (math.isnan(x), 0.0 if math.isnan(x) else x, math.copysign(1.0, x)))
    n = len(xs)
    if n == 0:
        return None
    assert n <= 50000, "beyond one head buffer the result depends on Spark's row order"
    # insert: (value, g, delta); delta = floor(2 eps i) except the first and the last
    s = [(x, 1, 0 if i in (0, n - 1) else int(math.floor(2 * relative_error * (i + 1))))
         for i, x in enumerate(xs)]
    # compress from the right with threshold 2 eps n, keeping the minimum
    thr = 2 * relative_error * n
    head = s[-1]
    kept = []
    for i in range(n - 2, 0, -1):
        if s[i][1] + head[1] + head[2] < thr:
            head = (head[0], head[1] + s[i][1], head[2])
        else:
            kept.append(head)
            head = s[i]
    kept.append(head)
    kept.reverse()
    if n > 1 and s[0][0] <= head[0]:
        kept.insert(0, s[0])
    if quantile <= relative_error:
        return kept[0][0]
    if quantile >= 1 - relative_error:
        return kept[-1][0]
    rank = math.ceil(quantile * n)
    err = math.ceil(relative_error * n)
    lo = 0
    for v, g, d in kept[1:-1]:
        lo += g
        if lo + d - err <= rank <= lo + err:
            return v
    return kept[-1][0]


def quantile_rank_error(values, quantile: float, result: float) -> int:
    """How many ranks `result` is from the target rank ceil(q n) of the sorted non-NULL values
    (0 when a copy of `result` sits at the target rank)."""
    import bisect
    import math
    xs = sorted(float(v) for v in values if v is not None)
    n = len(xs)
    target = max(1, math.ceil(quantile * n))
    lo = bisect.bisect_left(xs, result) + 1   # 1-based rank range of `result`
    hi = bisect.bisect_right(xs, result)
    if lo <= target <= hi:
        return 0
    return min(abs(target - lo), abs(target - hi))


# ------------------------------------------------------------------------------------------------
# DataType (M/analyzers/catalyst/StatefulDataType.scala:36-69): Scala `x match { case R(_) => }`
# is a full match; each value of when(where, col) cast to string is classified in order.
# ------------------------------------------------------------------------------------------------
def datatype_counts(t: OTable, column: str, where: Optional[str]) -> Tuple[int, ...]:
    """(NULL, Fractional, Integral, Boolean, String) counts."""
    import re
    frac = re.compile(r"(-|\+)? ?[0-9]*\.[0-9]*")
    integral = re.compile(r"(-|\+)? ?[0-9]*")
    boolean = re.compile(r"(true|false)")
    ty = t.types[column]
    out = [0, 0, 0, 0, 0]
    for v in _sel(t, column, where):
        if v is None:
            out[0] += 1
            continue
        s = java_to_string(v, ty)
        if frac.fullmatch(s):
            out[1] += 1
        elif integral.fullmatch(s):
            out[2] += 1
        elif boolean.fullmatch(s):
            out[3] += 1
        else:
            out[4] += 1
    return tuple(out)


# ------------------------------------------------------------------------------------------------
# MutualInformation (M/analyzers/MutualInformation.scala:41-84): joint frequencies (both keys
# non-NULL), marginals re-aggregated from them, joined, summed per joint group.
# ------------------------------------------------------------------------------------------------
def mutual_information(t: OTable, c1: str, c2: str) -> Optional[float]:
    import math
    joint = frequencies(t, [c1, c2])
    if not joint:
        return None
    px: Dict = {}
    py: Dict = {}
    for (x, y), c in joint.items():
        px[x] = px.get(x, 0) + c
        py[y] = py.get(y, 0) + c
    total = t.n
    # Spark sums the per-group terms in partition order, which no fixed order reproduces: the
    # oracle takes the exactly rounded sum of the same terms (fsum), the reference point every
    # summation order is within its own rounding error of
    return math.fsum((c / total) * math.log((c / total) / ((px[x] / total) * (py[y] / total)))
                     for (x, y), c in joint.items())
