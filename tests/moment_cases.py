"""Ill-conditioned and poisoned inputs for the moment / co-moment tests, their exact reference and
the error bound (tests/test_moment_cases.py on the host, tests/test_gpu_moments_conditioning.py on
the device).  Everything here runs on the host: numpy, pyarrow and the oracle only.

The fused scan computes (n, avg, m2) and (n, xAvg, yAvg, ck, xMk, yMk) as per-lane two-pass blocks
followed by Chan merges; Spark updates row by row.  Both are backward stable, so on a column with
condition number kappa = sqrt(sum x^2 / m2) their second moments carry a relative error of a small
multiple of kappa * 2^-52, while the textbook form  sum x^2 - (sum x)^2 / n  is off by kappa^2 *
2^-52.  The random tables of the parity tests have kappa ~ 4, where the two cannot be told apart;
the families below have kappa between 1e5 and 1e11.

The bound ("Moment conditioning"):

    |got - exact| <= max(1e-12, C * kappa * 2^-52) * scale

scale = sum|x| / n for an average, sum|x| for a sum, sum|dx * dy| for ck and the moment itself for
m2 / xMk / yMk (the scales of test_moments_against_exact_arithmetic); kappa = 1 for averages and
sums, kappa_x for m2 / xMk, kappa_y for yMk, kappa_x + kappa_y for ck and for the correlation
(ck's terms dx * dy inherit the error eps * |mean x| = eps * kappa_x * sd_x of dx and likewise of
dy).  C is measured on the REFERENCE, never on the device: the largest error / (kappa * 2^-52 *
scale) that the oracle's row-sequential agg_stddev / agg_corr show on the second-moment components
over every case below whose kappa * 2^-52 reaches 1e-12 (below that the 1e-12 contract governs and
the ratio only counts ulps), times 4 for the device's different merge order, and at least 1.
test_moment_cases.py measures it and asserts that the figure recorded here bounds it.

    measured oracle ratio: 34.60 (ORACLE_RATIO = 34.61), so C = 4 * 34.61 = 138.44

The figure is set by one family, the ramp 1e9 + i at 1023 rows: Spark's running average carries
a random walk of rounding errors e_k ~ sqrt(k) ulp(1e9), and the ramp's growing deltas (i / 2)
multiply it into m2 (2 * delta * e_k per row, all of one sign while the walk stays on one side).
Every other family stays below 0.90 (the normal columns about 0.3, as a two-pass scheme does).
The textbook form is off by kappa^2 * 2^-52, so with kappa >= 1e6 it still misses C * kappa * 2^-52
by more than 1e3 (asserted on every float64 / int64 case).

The averages and sums keep the 1e-12 contract as it is (C * 2^-52 stays far below 1e-12).
"""
import math
from collections import namedtuple
from decimal import Decimal
from fractions import Fraction as F
from functools import lru_cache

import numpy as np
import pyarrow as pa

ORACLE_RATIO = 34.61                # the largest ratio the oracle shows; see the docstring
C = max(1.0, 4.0 * ORACLE_RATIO)
EPS = F(1, 2 ** 52)

WHERE = "g < 5"                     # the side column g = row % 8
NP = {"i8": np.int8, "i16": np.int16, "i32": np.int32, "i64": np.int64, "f32": np.float32,
      "f64": np.float64}
SPARK = {"i8": "byte", "i16": "short", "i32": "int", "i64": "long", "f32": "float", "f64": "double",
         "d20": "decimal(20,4)", "g": "int"}
NUMERIC = list(NP)


# ------------------------------------------------------------------------------------------------
# The exact reference
# ------------------------------------------------------------------------------------------------
def _ints(xs):
    """The doubles xs as integers over one power-of-two denominator (exact)."""
    ratios = [float(x).as_integer_ratio() for x in xs]
    den = max((d for _, d in ratios), default=1)
    return [p * (den // d) for p, d in ratios], den


def exact_moments(xs, ys=None):
    """Population moments in exact rational arithmetic over the double inputs: the value both
    Spark's row-sequential update (Correlation.scala:37-52 merge, Corr update) and the device's
    blocked two-pass + Chan merges approximate.  (Integer arithmetic over the common power-of-two
    denominator: the same numbers as Fractions, a hundred times faster.)"""
    if ys is None:
        ys = xs
    n = len(xs)
    X, dx = _ints(xs)
    Y, dy = (X, dx) if ys is xs else _ints(ys)
    sx, sy = sum(X), sum(Y)
    cx, cy = [n * v - sx for v in X], [n * v - sy for v in Y]      # n * (x - mean) * den
    nn = n * n
    return dict(n=n, mx=F(sx, n * dx), my=F(sy, n * dy),
                ck=F(sum(a * b for a, b in zip(cx, cy)), nn * dx * dy),
                xm=F(sum(a * a for a in cx), nn * dx * dx), ym=F(sum(b * b for b in cy), nn * dy * dy),
                sx=F(sum(abs(v) for v in X), n * dx), sy=F(sum(abs(v) for v in Y), n * dy),
                sck=F(sum(abs(a * b) for a, b in zip(cx, cy)), nn * dx * dy),
                sxx=F(sum(v * v for v in X), dx * dx), syy=F(sum(v * v for v in Y), dy * dy))


def _sqrt(q):
    """sqrt of a positive Fraction as a float, without overflow in the conversion."""
    return math.sqrt(q.numerator // q.denominator) if q > 2 ** 60 else math.sqrt(float(q))


def kappa(e):
    """(kappa_x, kappa_y) of exact_moments' result: sqrt(sum x^2 / m2), inf on a constant column."""
    kx = _sqrt(e["sxx"] / e["xm"]) if e["xm"] else math.inf
    ky = _sqrt(e["syy"] / e["ym"]) if e["ym"] else math.inf
    return kx, ky


def rel_bound(k, c=None):
    """max(1e-12, C * kappa * 2^-52) as a Fraction (kappa = inf: the moment is 0, any factor)."""
    c = C if c is None else c
    if math.isinf(k):
        return F(1)
    return max(F(1, 10 ** 12), F(c) * F(k) * EPS)


def component_bounds(e, c=None):
    """name -> (exact value, allowed |error|) for the six state components and the correlation."""
    kx, ky = kappa(e)
    out = {"xAvg": (e["mx"], F(1, 10 ** 12) * e["sx"]), "yAvg": (e["my"], F(1, 10 ** 12) * e["sy"]),
           "ck": (e["ck"], rel_bound(kx + ky, c) * e["sck"]),
           "xMk": (e["xm"], rel_bound(kx, c) * e["xm"]), "yMk": (e["ym"], rel_bound(ky, c) * e["ym"])}
    return out


def exact_corr(e):
    """(the exact correlation as a float, its allowed error), None on a constant side.  The bound
    of ck propagated: corr = ck / sqrt(xMk yMk), so a relative error b on each of the three gives
    |d corr| <= b * sck / sqrt(xm ym) + |corr| * b to first order, b the bound at kappa_x + kappa_y
    (which is at least the bounds of xMk and of yMk)."""
    if not e["xm"] or not e["ym"]:
        return None
    den = _sqrt(e["xm"] * e["ym"])
    corr = float(e["ck"] / F(den))
    kx, ky = kappa(e)
    b = float(rel_bound(kx + ky))
    return corr, b * float(e["sck"] / F(den)) + abs(corr) * b


def ratios(state, e):
    """error / (kappa * 2^-52 * scale) of the second-moment components of a state
    (n, avg, m2) or (n, xAvg, yAvg, ck, xMk, yMk) against exact_moments' e."""
    kx, ky = kappa(e)
    if len(state) == 3:
        parts = [(state[2], e["xm"], kx, e["xm"])]
    else:
        parts = [(state[3], e["ck"], kx + ky, e["sck"]), (state[4], e["xm"], kx, e["xm"]),
                 (state[5], e["ym"], ky, e["ym"])]
    out = []
    for got, exact, k, scale in parts:
        if scale == 0 or math.isinf(k):
            out.append(0.0 if F(got) == exact else math.inf)
        elif F(k) * EPS < F(1, 10 ** 12):
            out.append(0.0)         # well conditioned: the 1e-12 contract governs, not kappa
        else:
            out.append(float(abs(F(got) - exact) / (F(k) * EPS * scale)))
    return out


def naive_moments(xs, ys=None):
    """NEGATIVE CONTROL ONLY: the textbook sum x^2 - (sum x)^2 / n (and sum xy) in fp64."""
    ys = xs if ys is None else ys
    n = float(len(xs))
    sx = sy = sxx = syy = sxy = 0.0
    for x, y in zip(xs, ys):
        sx += x
        sy += y
        sxx += x * x
        syy += y * y
        sxy += x * y
    return (n, sx / n, sy / n, sxy - sx * sy / n, sxx - sx * sx / n, syy - sy * sy / n)


# ------------------------------------------------------------------------------------------------
# Ill-conditioned families
# ------------------------------------------------------------------------------------------------
Family = namedtuple("Family", "name type")
FAMILIES = [Family("f64_1e6_sd1", "f64"), Family("f64_1e9_sd1", "f64"), Family("f64_1e12_sd3", "f64"),
            Family("f64_m1e9_sd001", "f64"), Family("f64_halves_pm1e9", "f64"), Family("f64_ramp_1e9", "f64"),
            Family("i64_2p53_steps", "i64"), Family("i64_1e15", "i64"), Family("i32_2e9", "i32"),
            Family("i16_top", "i16"), Family("i8_top", "i8"), Family("f32_2p24_m512", "f32"),
            Family("d20_1e12", "d20")]
FAMILY = {f.name: f for f in FAMILIES}
ROWS = [1, 7, 8, 9, 1023, 1024, 1025, 4097]
ROWS_BATCHED = (20_011, 4096)       # rows, max_batch_rows
ROWS_ITEMS = 33_000                 # > one 256 KiB item of 8-byte values


def family_values(name, n, seed=0):
    """The n values of a family in the column's numpy dtype (d20: unscaled int64 at scale 4)."""
    rng = np.random.default_rng([seed, n, sum(name.encode())])
    z = rng.normal(0.0, 1.0, n)
    if name == "f64_1e6_sd1":
        return 1e6 + z
    if name == "f64_1e9_sd1":
        return 1e9 + z
    if name == "f64_1e12_sd3":
        return 1e12 + 3.0 * z
    if name == "f64_m1e9_sd001":
        return -1e9 + 0.01 * z
    if name == "f64_halves_pm1e9":
        return np.where(np.arange(n) < n // 2, 1e9, -1e9) + z
    if name == "f64_ramp_1e9":
        return 1e9 + np.arange(n, dtype=np.float64)
    if name == "i64_2p53_steps":          # (double)x rounds to even above 2^53, as Spark's cast does
        return 2 ** 53 + rng.integers(0, 4000, n, dtype=np.int64)
    if name == "i64_1e15":
        return 10 ** 15 + np.rint(3.0 * z).astype(np.int64)
    if name == "i32_2e9":
        return (2_000_000_000 + np.rint(30.0 * z)).astype(np.int32)
    if name == "i16_top":
        return (32767 - rng.integers(0, 200, n)).astype(np.int16)
    if name == "i8_top":
        return (127 - rng.integers(0, 20, n)).astype(np.int8)
    if name == "f32_2p24_m512":           # unit steps below 2^24: every value exact in float32
        return (16_777_216 - 512 + rng.integers(0, 512, n)).astype(np.float32)
    if name == "d20_1e12":                # decimal(20, 4) around 1e12 +- 3
        return 10 ** 16 + np.rint(30_000.0 * z).astype(np.int64)
    raise KeyError(name)


def _valid(n, null_rate, rng):
    return rng.random(n) >= null_rate if null_rate else np.ones(n, bool)


def arrow_array(values, valid):
    """A fixed-width Arrow array over exactly these value bytes: whatever sits in a NULL slot stays
    there (pa.array(values, mask=) makes no such promise)."""
    values = np.ascontiguousarray(values)
    n = len(values)
    nulls = int(n - valid.sum())
    bitmap = pa.py_buffer(np.packbits(valid, bitorder="little").tobytes()) if nulls else None
    return pa.Array.from_buffers(pa.from_numpy_dtype(values.dtype), n,
                                 [bitmap, pa.py_buffer(values.tobytes())], nulls)


def column_arrow(ty, values, valid):
    if ty == "d20":
        vals = [Decimal(int(v)).scaleb(-4) if ok else None for v, ok in zip(values, valid)]
        return pa.array(vals, type=pa.decimal128(20, 4))
    return arrow_array(values, valid)


def side_column(n):
    return pa.array((np.arange(n) % 8).astype(np.int32))


def doubles(ty, values):
    """The doubles the device sees: (double)x of every value (d20: the correctly rounded cast)."""
    if ty == "d20":
        return [float(Decimal(int(v)).scaleb(-4)) for v in values]
    return [float(v) for v in values]


def oracle_table(t, types):
    from oracle.deequ_oracle import OTable
    return OTable({k: t.column(k).to_pylist() for k in t.column_names}, {k: SPARK[v] for k, v in types.items()})


MomentCase = namedtuple("MomentCase", "family n batch arrow otable sel exact")


@lru_cache(maxsize=None)
def moment_case(name, n, batch=None, null_rate=0.05):
    """One family at n rows with 5 % NULLs: the Arrow table (x, g), the oracle's table, and per
    where in (None, WHERE) the selected doubles with their exact moments (None: no row selected)."""
    ty = FAMILY[name].type
    values = family_values(name, n)
    rng = np.random.default_rng([7, n])
    valid = _valid(n, null_rate if n > 1 else 0.0, rng)
    t = pa.table({"x": column_arrow(ty, values, valid), "g": side_column(n)})
    xs = np.array(doubles(ty, values))
    g = np.arange(n) % 8
    sel, exact = {}, {}
    for w, m in ((None, valid), (WHERE, valid & (g < 5))):
        sel[w] = [float(v) for v in xs[m]]
        exact[w] = exact_moments(sel[w]) if m.any() else None
    return MomentCase(name, n, batch, t, oracle_table(t, {"x": ty, "g": "g"}), sel, exact)


def moment_cases(name):
    ty = FAMILY[name].type
    out = [(n, None) for n in ROWS] + [ROWS_BATCHED]
    if ty in ("i64", "f64"):
        out.append((ROWS_ITEMS, None))
    return out


# ------------------------------------------------------------------------------------------------
# Correlated pairs on the ill-conditioned columns
# ------------------------------------------------------------------------------------------------
PAIRS = [("f64", "f64"), ("i64", "f64"), ("i64", "i64"), ("i32", "f64"), ("f32", "f64"), ("f32", "i16"),
         ("i8", "i32"), ("i16", "i64")]
WIDE_PAIRS = PAIRS[:3]              # both sides 8 bytes: the vector and the fused-HLL paths
RHOS = [0.8, -0.99]
PAIR_ROWS = [1, 2, 511, 512, 513, 1024, 1025, 4097]
# (centre, spread) of a side by type: x sides and y sides differ, so (i64, i64) is no copy
_SIDE = {("f64", 0): (1e9, 1.0), ("f64", 1): (1e8, 1.0), ("i64", 0): (2.0 ** 53 + 4000, 800.0),
         ("i64", 1): (1e15, 3.0), ("i32", 0): (2e9, 30.0), ("i32", 1): (2e9, 30.0),
         ("i16", 0): (32_000.0, 150.0), ("i16", 1): (32_000.0, 150.0), ("i8", 0): (100.0, 8.0),
         ("f32", 0): (16_777_216.0 - 256, 40.0)}


def _side_values(ty, role, u):
    centre, spread = _SIDE[(ty, role)]
    if ty == "f64":
        return centre + spread * u
    v = np.rint(spread * u).astype(np.int64) + int(centre)
    if ty == "f32":
        return np.clip(v, 0, 16_777_215).astype(np.float32)
    if ty == "i64":
        return v
    info = np.iinfo(NP[ty])
    return np.clip(v, info.min, info.max).astype(NP[ty])


def asymmetric_nulls(n, rng, rate=0.03):
    """Validity of x and of y: independent 3 % NULLs, and rows 992..1055 (a run of 64 across the
    1024-row chunk edge; rows 480..543 across the 512-row step of the scalar loop) with x NULL on
    the even rows and y NULL on the odd ones -- never both, so every row of the run is dropped
    through one side alone."""
    vx, vy = rng.random(n) >= rate, rng.random(n) >= rate
    r = np.arange(n)
    for lo in (480, 992):
        run = (r >= lo) & (r < lo + 64)
        vx = np.where(run, r % 2 == 1, vx)
        vy = np.where(run, r % 2 == 0, vy)
    if n <= 2:
        vx[:] = True
        vy[:] = True
    return vx, vy


PairCase = namedtuple("PairCase", "tx ty rho n batch arrow otable sel exact")


@lru_cache(maxsize=None)
def pair_case(tx, ty, rho, n, batch=None):
    rng = np.random.default_rng([11, n, int(abs(rho) * 100), sum((tx + ty).encode())])
    z, e = rng.normal(0.0, 1.0, n), rng.normal(0.0, 1.0, n)
    x = _side_values(tx, 0, z)
    y = _side_values(ty, 1, rho * z + math.sqrt(1.0 - rho * rho) * e)
    vx, vy = asymmetric_nulls(n, rng)
    t = pa.table({"x": arrow_array(x, vx), "y": arrow_array(y, vy), "g": side_column(n)})
    g = np.arange(n) % 8
    xd, yd = x.astype(np.float64), y.astype(np.float64)
    sel, exact = {}, {}
    for w, m in ((None, vx & vy), (WHERE, vx & vy & (g < 5))):
        sel[w] = ([float(v) for v in xd[m]], [float(v) for v in yd[m]])
        exact[w] = exact_moments(*sel[w]) if m.any() else None
    return PairCase(tx, ty, rho, n, batch, t, oracle_table(t, {"x": tx, "y": ty, "g": "g"}), sel, exact)


def pair_rows():
    return [(n, None) for n in PAIR_ROWS] + [ROWS_BATCHED]


# ------------------------------------------------------------------------------------------------
# Poison
# ------------------------------------------------------------------------------------------------
def _nan(bits, dtype):
    return np.array([bits], np.uint64 if dtype == np.float64 else np.uint32).view(dtype)[0]


POISON = {
    "f64": [_nan(0x7ff8000000000000, np.float64), _nan(0x7ff0000000000123, np.float64), np.inf, -np.inf,
            1.797e308, -0.0],
    "f32": [_nan(0x7fc00000, np.float32), _nan(0x7f800123, np.float32), np.float32(np.inf),
            np.float32(-np.inf), np.float32(3.4e38), np.float32(-0.0)],
    "i8": [-128, 127], "i16": [-32768, 32767], "i32": [-2 ** 31, 2 ** 31 - 1],
    "i64": [-2 ** 63, 2 ** 63 - 1, 2 ** 53 + 1],
}


def benign_values(ty, n, rng):
    """Well-conditioned visible values: the hidden-row tests are about the slots, not the moments."""
    if ty in ("f64", "f32"):
        return rng.normal(100.0, 30.0, n).astype(NP[ty])
    hi = {"i8": 100, "i16": 30_000, "i32": 10 ** 6, "i64": 10 ** 9}[ty]
    return rng.integers(-hi, hi, n).astype(NP[ty])


def poisoned(values, slots, ty, zero=False):
    """values with the type's poison cycled through `slots` (zero: with zeros there instead)."""
    out = values.copy()
    idx = np.flatnonzero(slots)
    out[idx] = 0 if zero else np.resize(np.array(POISON[ty], dtype=values.dtype), len(idx))
    return out


HiddenCase = namedtuple("HiddenCase", "ty n poison zeros otable")


@lru_cache(maxsize=None)
def hidden_case(ty, n, null_rate=0.3):
    """Two Arrow tables (x, y, z, g, f) that differ only in hidden slots.
    x: NULL slots hold poison / zeros.  y: a benign float64 partner for Correlation, NULLs of its
    own.  z: no NULLs, but poison / zeros on the rows where f = 0 (hidden by the where "f = 1"
    only).  otable is the oracle's view of the poison version; where-less aggregates run on x,
    filtered ones on x and z."""
    rng = np.random.default_rng([13, n, sum(ty.encode())])
    base = benign_values(ty, n, rng)
    valid = rng.random(n) >= null_rate
    f = (rng.random(n) < 0.7).astype(np.int32)
    y = rng.normal(50.0, 10.0, n)
    vy = rng.random(n) >= 0.1
    tabs = []
    for zero in (False, True):
        tabs.append(pa.table({
            "x": arrow_array(poisoned(base, ~valid, ty, zero), valid),
            "y": arrow_array(poisoned(y, ~vy, "f64", zero), vy),
            "z": arrow_array(poisoned(base, f == 0, ty, zero), np.ones(n, bool)),
            "g": side_column(n), "f": pa.array(f)}))
    types = {"x": ty, "y": "f64", "z": ty, "g": "g", "f": "g"}
    return HiddenCase(ty, n, tabs[0], tabs[1], oracle_table(tabs[0], types))
