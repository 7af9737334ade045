"""CPU checks of tests/repartition_cases.py, the reference of tests/test_gpu_repartition.py:

  * the reference's groups and counts equal oracle.deequ_oracle.frequencies (groupings) or
    histogram (null_as_group) on every case that has rows -- the synthetic tables have none, their
    reference is the sum of the groups they are loaded from;
  * no case leaves an output of the reference empty, and every case holds what it is named for
    (all 256 int8 values, the int64 edges, three NaN payloads, the string lengths, the hot counts,
    the empty and the all-NULL shard, ...);
  * every case x world size is either run or left out with a reason.
"""
import math

import numpy as np
import pytest

import repartition_cases as RC
from deequ_amd import _native as N
from oracle import deequ_oracle as O

ROW_CASES = [c.name for c in RC.CASES.values() if c.synthetic is None]


def _pylists(case):
    return [c.to_pylist() for c in case.columns]


@pytest.mark.parametrize("name", ROW_CASES)
def test_reference_agrees_with_the_oracle(name):
    case = RC.CASES[name]
    ref = RC.reference(case)
    cols = _pylists(case)
    names = case.key_columns
    types = dict(zip(names, case.oracle_types))
    ot = O.OTable(dict(zip(names, cols)), types)
    assert ref.num_rows == ot.n
    mine = RC.row_keys(case)
    if not case.null_as_group:
        freq = O.frequencies(ot, names)
        seen = {}
        for k, row in zip(mine, zip(*cols)):
            if None in k:
                continue
            ok = tuple(O._group_key(v, t) for v, t in zip(row, case.oracle_types))
            assert seen.setdefault(k, ok) == ok  # one reference group, one oracle group
        assert len(set(seen.values())) == len(seen) == len(freq) == ref.n_groups
        for k, ok in seen.items():
            assert ref.groups[k] == freq[ok], k
        assert ref.null_key_rows == ot.n - sum(freq.values()) and ref.null_group_rows == 0
        assert ref.n_unique == sum(1 for c in freq.values() if c == 1)
        want = O.entropy(freq, ot.n)
        assert abs(ref.entropy - want) <= 1e-12 * abs(want)
        return
    hist, n = O.histogram(ot, names[0])
    assert n == ref.num_rows and ref.null_key_rows == 0
    ty = case.oracle_types[0]
    text = {}
    for k, v in zip(mine, cols[0]):
        s = "NullValue" if v is None else O.java_to_string(v, ty)
        assert text.setdefault(k, s) == s
    got = {}
    for k, c in ref.groups.items():
        got[text[k]] = got.get(text[k], 0) + c
    assert got == hist
    # the groups are the string groups, but for the NULL group a string table keeps apart
    folded = ref.folded() if ty == "string" else ref.groups
    assert len(folded) == len(hist)
    assert ref.null_group_rows == sum(v is None for v in cols[0])


@pytest.mark.parametrize("name", list(RC.CASES))
def test_no_output_of_the_reference_is_empty(name):
    case = RC.CASES[name]
    for w in case.worlds:
        ref = RC.reference(case, w)
        assert ref.n_groups > 0 and ref.num_rows >= sum(ref.groups.values()) > 0
        assert ref.entropy > 0.0 and math.isfinite(ref.entropy)
        assert ref.top_counts[0] >= 1 and len(ref.top_counts) == ref.n_groups
        shards = RC.shard_reference(case, w)
        assert len(shards) == w
        assert RC.merge(shards).groups == ref.groups
        assert sum(s.num_rows for s in shards) == ref.num_rows < 1 << 63
        assert all(c < 1 << 63 for c in ref.groups.values())
        if case.synthetic is None:
            break  # (rows: the whole-table reference does not depend on W)


def test_some_case_fills_every_output():
    refs = [RC.reference(c) for c in RC.CASES.values()]
    assert sum(r.n_unique > 0 for r in refs) >= 10
    assert sum(r.null_key_rows > 0 for r in refs) >= 10
    assert sum(r.null_group_rows > 0 for r in refs) >= 6
    assert sum(r.literal_rows > 0 and r.null_group_rows > 0 for r in refs) >= 2


def test_every_pair_is_run_or_left_out_with_a_reason():
    for c in RC.CASES.values():
        assert set(c.worlds) | set(c.left_out) == set(RC.WORLDS), c.name
        assert not set(c.worlds) & set(c.left_out), c.name
        assert all(len(why) > 20 for why in c.left_out.values()), c.name
        if c.synthetic is None:
            assert len(c.weights) >= 3 and len(set(c.weights)) > 1, c.name
            assert 20_000 <= c.n_rows <= 70_000, c.name
        assert c.null_as_group is False or len(c.key_types) == 1
        assert c.raw is False or (len(c.key_types) == 1 and c.synthetic is None)
    for w in RC.WORLDS:  # every world size runs both key modes and both paths
        assert any(w in c.worlds and c.key_types == [N.INT64] for c in RC.CASES.values())
        assert any(w in c.worlds and c.key_types == [N.UTF8] for c in RC.CASES.values())
        assert any(w == pw for _, pw in RC.RAW_PAIRS)
    assert len(RC.RECORD_PAIRS) == len(set(RC.RECORD_PAIRS))


def _key(v):
    return (int(v) & RC.MASK64,)


def test_cases_hold_what_they_are_named_for():
    C = RC.CASES
    g = RC.reference(C["int8_all_values"]).groups
    assert {_key(v) for v in range(-128, 128)} == set(g)
    g = RC.reference(C["int64_edges_consecutive"]).groups
    for v in (-(1 << 63), (1 << 63) - 1, 0, -1):
        assert g[_key(v)] > 1
    for name in ("int64_edges_consecutive", "int32_consecutive", "utf8_near_unique"):
        assert RC.reference(C[name]).n_groups >= RC.BALANCE_MIN_KEYS, name
    ids = sorted(k[0] for k in g if 1_000_000 <= k[0] < 1_026_000)
    assert len(ids) >= RC.BALANCE_MIN_KEYS and ids[-1] - ids[0] < 26_000  # consecutive ids

    f32 = {"nan": (0x7FC00000, 0x7FC00001, 0xFFC12345), "zero": (0x0, 0x80000000),
           "inf": (0x7F800000, 0xFF800000), "sub": (0x1,)}
    f64 = {"nan": (0x7FF8000000000000, 0x7FF8000000000001, 0xFFF8000000ABCDEF),
           "zero": (0x0, 0x8000000000000000), "inf": (0x7FF0000000000000, 0xFFF0000000000000),
           "sub": (0x1,)}
    for width, bits in (("float32", f32), ("float64", f64)):
        grouping = RC.reference(C[f"{width}_grouping"]).groups
        histogram = RC.reference(C[f"{width}_histogram"]).groups
        for kind in ("nan", "zero", "inf", "sub"):
            for b in bits[kind]:
                assert grouping[(b,)] > 10, (width, hex(b))  # by bits: every payload, both zeros
        for b in bits["zero"] + bits["inf"] + bits["sub"]:
            assert histogram[(b,)] == grouping[(b,)]
        # NaN payloads are one group only where null_as_group is set
        assert histogram[(bits["nan"][0],)] == sum(grouping[(b,)] for b in bits["nan"])
        assert all((b,) not in histogram for b in bits["nan"][1:])
        assert histogram[(None,)] > 0 and (None,) not in grouping
        assert len(grouping) > 500  # and ordinary values

    for name in ("utf8_lengths_grouping", "utf8_lengths_histogram"):
        ref = RC.reference(C[name])
        lengths = {len(k[0]) for k in ref.groups if k[0] is not None}
        assert {0, 3, 4, 5, 7, 8, 15, 16, 17, 300} <= lengths
        assert any(max(k[0]) > 0x7F for k in ref.groups if k[0])  # non-ASCII bytes
        assert ref.literal_rows > 0
    ref = RC.reference(C["utf8_lengths_histogram"])
    assert ref.null_group_rows == ref.groups[(None,)] > 0
    assert ref.folded()[(RC.NULL_LITERAL,)] == ref.null_group_rows + ref.literal_rows
    assert len(ref.folded()) == ref.n_groups - 1
    ref = RC.reference(C["utf8_lengths_grouping"])
    assert ref.null_key_rows > 0 and (None,) not in ref.groups

    for name in ("composite_int64_utf8", "composite_int32_float64_utf8"):
        case = C[name]
        keys = RC.row_keys(case)
        for pos in range(len(case.key_types)):  # NULL in each position, alone and together
            assert any(k[pos] is None and sum(e is None for e in k) == 1 for k in keys)
        assert any(sum(e is None for e in k) >= 2 for k in keys)
        assert all(None not in k for k in RC.reference(case).groups)

    hot = C["hot_key_0x5555"]
    for w in hot.worlds:
        shards = RC.shard_reference(hot, w)
        assert shards[0].groups[_key(-77)] == 0x5555
        assert all(_key(-77) not in s.groups for s in shards[1:])
    hot = C["hot_key_sum_over_65535"]
    key = (b"hot key of 23 bytes ...",)
    for w in hot.worlds:
        per = [s.groups[key] for s in RC.shard_reference(hot, w)]
        assert max(per) <= 65_535 < sum(per) and min(per) > 0

    for name in ("synthetic_int64", "synthetic_utf8", "synthetic_utf8_histogram"):
        case = C[name]
        for w in case.worlds:
            shards = RC.shard_reference(case, w)
            counts = {c for s in shards for c in s.groups.values()}
            assert set(RC.SYNTH_COUNTS) <= counts | {RC.SYNTH_BIG}
            assert RC.SYNTH_BIG in counts
            if w >= 3:  # a key's big counts meet on its owner
                assert max(RC.reference(case, w).groups.values()) >= 2 * RC.SYNTH_BIG
    assert bin(RC.SYNTH_BIG).count("1") == 31 and RC.SYNTH_BIG.bit_length() == 61

    for name in ("empty_shard_grouping", "empty_shard_histogram"):
        for w in C[name].worlds:
            rows = [s.num_rows for s in RC.shard_reference(C[name], w)]
            assert rows[1] == 0 and rows[0] > 0 and rows[2] > 0
    for name in ("all_null_shard_grouping", "all_null_shard_histogram"):
        s = RC.shard_reference(C[name], 3)[1]
        assert s.num_rows == 6_000 == s.null_key_rows + s.null_group_rows
        assert set(s.groups) <= {(None,)}
    assert RC.reference(C["five_keys"]).n_groups == 5 and 64 in C["five_keys"].worlds

    for name, p in (("decimal_9_2", 9), ("decimal_18_4", 18), ("decimal_38_10", 38)):
        case = C[name]
        assert N.decimal_precision(case.key_types[0]) == p
        assert RC.reference(case).n_groups > 1_000
    wide = RC.reference(C["decimal_38_10"]).groups
    low7 = [k for k in wide if k[0][:8] == (7).to_bytes(8, "little")]
    assert len(low7) == 4  # equal low words, different high words: four groups


def test_shard_bounds():
    assert RC.shard_bounds(100, [5, 1, 3], 1) == [0, 100]
    assert RC.shard_bounds(90, [5, 1, 3], 3) == [0, 50, 60, 90]
    assert RC.shard_bounds(110, [4, 0, 2, 5], 4) == [0, 40, 40, 60, 110]
    b = RC.shard_bounds(20_000, [5, 1, 3], 64)
    assert len(b) == 65 and b[0] == 0 and b[-1] == 20_000 and np.all(np.diff(b) > 0)
