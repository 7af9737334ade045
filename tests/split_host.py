"""Host restatement of dq_split_rows' draw (include/deequ_amd.h), shared by the CPU and GPU tests:

    z = seed + (r + 1) * 0x9E3779B97F4A7C15        (mod 2^64; r = the table-global row index)
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9
    z = (z ^ (z >> 27)) * 0x94D049BB133111EB
    z =  z ^ (z >> 31)
    u = (z >> 11) * 2^-53
    split(r) = the first k with u < bound[k],  bound = cumsum(w) / sum(w), the last forced to 1
"""
import numpy as np

GAMMA = 0x9E3779B97F4A7C15
M1 = 0xBF58476D1CE4E5B9
M2 = 0x94D049BB133111EB
MASK = (1 << 64) - 1


def bounds(weights):
    """cumsum(w) / sum(w) in fp64, in that order of operations; the last entry exactly 1.0."""
    acc, cum = 0.0, []
    for w in weights:
        acc += float(w)
        cum.append(acc)
    out = [c / acc for c in cum]
    out[-1] = 1.0
    return out


def draw_int(seed: int, r: int) -> float:
    """u(seed, r) in plain Python integers."""
    z = (seed + (r + 1) * GAMMA) & MASK
    z = ((z ^ (z >> 30)) * M1) & MASK
    z = ((z ^ (z >> 27)) * M2) & MASK
    z ^= z >> 31
    return (z >> 11) * 2.0 ** -53


def split_int(seed: int, r: int, bnd) -> int:
    u = draw_int(seed % (1 << 64), r)
    for k, b in enumerate(bnd):
        if u < b:
            return k
    raise AssertionError("the last bound is 1 > u")


def draw(seed: int, row_base: int, rows: int) -> np.ndarray:
    """u for the rows [row_base, row_base + rows), vectorised (uint64 arithmetic wraps)."""
    with np.errstate(over="ignore"):
        r1 = np.arange(rows, dtype=np.uint64) + np.uint64((row_base + 1) & MASK)
        z = np.uint64(seed % (1 << 64)) + r1 * np.uint64(GAMMA)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(M1)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(M2)
        z = z ^ (z >> np.uint64(31))
    return (z >> np.uint64(11)).astype(np.float64) * 2.0 ** -53


def assign(seed: int, row_base: int, rows: int, weights) -> np.ndarray:
    """split(r) of every row of a batch, int64."""
    u = draw(seed, row_base, rows)
    bnd = np.asarray(bounds(weights), np.float64)
    # the first k with u < bound[k] = the number of bounds u has reached (bounds never decrease)
    return (u[:, None] >= bnd[None, :-1]).sum(axis=1).astype(np.int64)


def bitmaps(seed: int, row_base: int, rows: int, weights):
    """(one uint64 word array per split in dq_select_plan's layout, counts)."""
    a = assign(seed, row_base, rows, weights)
    words = (rows + 63) // 64
    out, counts = [], []
    for k in range(len(weights)):
        bits = np.zeros(words * 64, np.uint8)
        bits[:rows] = a == k
        out.append(np.packbits(bits, bitorder="little").view("<u8").astype(np.uint64))
        counts.append(int((a == k).sum()))
    return out, counts
