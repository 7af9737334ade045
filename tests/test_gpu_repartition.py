"""The multi-GPU group-by repartition at any world size, row-exact, in one process.

distributed.freq_partition / freq_add_records (freq_owner_count / freq_owner_scatter and the
records insert of csrc/freq.hip) and raw_key_partition / raw_key_count (key_owner_count /
key_owner_scatter of csrc/key_partition.hip) are pure functions of (table, n_parts), and the
all-to-all between them is a concatenation in rank order, so one process plays the W ranks exactly:
one table per shard, its W owner segments copied to the host and checked (A1-A5 / C1-C3), segment
j of every shard concatenated for owner j, the owners' tables checked against the reference of
tests/repartition_cases.py (B1-B5 / C4-C5).  Counts, groups and owners exact; the entropy within
1e-12 relative (dist_suite.close); the balance bound of A5 is the binomial's six standard
deviations, 6 sqrt(n (W - 1)) / W around n / W, which a uniform hash misses with probability below
1e-8 per segment.

The two-rank test (test_gpu_distributed.py) still covers the collectives themselves, the
_raw_keys_pay decision and DistributedFrequencies' reductions.
"""
import ctypes
import math
from collections import Counter
from functools import lru_cache

import numpy as np
import pytest

import repartition_cases as RC
from deequ_amd import _native as N

pytestmark = pytest.mark.gpu

REC = np.dtype([("key", "<u8"), ("count", "<u8"), ("enc_off", "<u8")])
assert REC.itemsize == N.FREQ_RECORD_BYTES
REL = 1e-12
BATCH_ROWS = 6_001  # a shard is added in several batches, cut off any bitmap byte
GUARD = 256
GUARD_BYTE = 0xA5


# ------------------------------------------------------------------------------------------------
# Decoding
# ------------------------------------------------------------------------------------------------
def _u32(data, pos):
    return int.from_bytes(data[pos: pos + 4], "little")


def _decode_enc(data: bytes, pos: int, types):
    """(key, size in bytes) of the encoded key at data[pos:] (freq_codec.h: per column a tag, then
    8 value bytes or a length and the bytes zero-padded to 4)."""
    start, key = pos, []
    for t in types:
        tag = _u32(data, pos)
        pos += 4
        if tag == 0:
            key.append(None)
            continue
        assert tag == 1, tag
        if RC.string_like(t):
            ln = _u32(data, pos)
            pos += 4
            key.append(data[pos: pos + ln])
            padded = (ln + 3) & ~3
            assert data[pos + ln: pos + padded] == b"\0" * (padded - ln), "string padding"
            pos += padded
        else:
            key.append(int.from_bytes(data[pos: pos + 8], "little"))
            pos += 8
    return tuple(key), pos - start


def _one_fixed(types) -> bool:
    return len(types) == 1 and not RC.string_like(types[0])


def _decode_groups(types, counts, offs, raw) -> Counter:
    """dq_freq_export / dq_freq_topk arrays as {key: count}, keys by bits; no key twice."""
    n = len(counts)
    if n and _one_fixed(types):
        words = np.frombuffer(bytes(raw) + b"\0" * 8, np.uint32)
        at = np.asarray(offs[:n], np.int64) // 4
        tags = words[at].tolist()
        bits = (words[at + 1].astype(np.uint64) | (words[at + 2].astype(np.uint64) << np.uint64(32))).tolist()
        keys = [(b,) if tg else (None,) for b, tg in zip(bits, tags)]
    else:
        data = bytes(raw)
        keys = [_decode_enc(data, int(offs[g]), types)[0] for g in range(n)]
    out = Counter(dict(zip(keys, (int(c) for c in counts))))
    assert len(out) == n, "a key appears twice"
    return out


def _export(table, types) -> Counter:
    return _decode_groups(types, *table.export_raw())


def _segments(rec, var, rc, vb):
    """The host copies of a partition's W segments: [(records as REC, var bytes)]."""
    rec_h = rec.cpu().numpy().view(REC) if rec.numel() else np.zeros(0, REC)
    var_h = var.cpu().numpy().tobytes()
    r0 = np.concatenate([[0], np.cumsum(rc)]).astype(np.int64)
    v0 = np.concatenate([[0], np.cumsum(vb)]).astype(np.int64)
    return [(rec_h[r0[j]: r0[j + 1]], var_h[v0[j]: v0[j + 1]]) for j in range(len(rc))]


def _decode_segment(recs, var: bytes, types, exact: bool):
    """[(key, count)] of one segment; hashed mode checks A3 on the way: every enc_off a multiple of
    8, the padded regions disjoint and tiling the segment's var bytes exactly, the pad word zero."""
    counts = recs["count"].tolist()
    if exact:
        assert not var
        return list(zip(((k,) for k in recs["key"].tolist()), counts))
    offs = recs["enc_off"].tolist()
    out, regions = [], []
    for off, c in zip(offs, counts):
        assert off % 8 == 0 and off + 4 <= len(var), (off, len(var))
        key, size = _decode_enc(var, off, types)
        padded = (size + 7) & ~7
        assert off + padded <= len(var)
        if size & 4:
            assert var[off + size: off + padded] == b"\0\0\0\0", "pad word"
        regions.append((off, off + padded))
        out.append((key, c))
    regions.sort()
    end = 0
    for lo, hi in regions:
        assert lo == end, f"var regions overlap or leave a gap at {lo} (expected {end})"
        end = hi
    assert end == len(var), (end, len(var))
    return out


# ------------------------------------------------------------------------------------------------
# One run of the records path
# ------------------------------------------------------------------------------------------------
def _device_shards(case, world, device):
    from deequ_amd.table import Table
    arrow = case.arrow()
    b = RC.shard_bounds(case.n_rows, case.weights, world)
    return [Table.from_arrow(arrow.slice(b[r], b[r + 1] - b[r]), device=device,
                             max_batch_rows=BATCH_ROWS) for r in range(world)]


def _local_tables(case, world, device):
    from deequ_amd.analyzers.grouping import FrequencyTable
    cols, types, nag = case.key_columns, case.key_types, case.null_as_group
    if case.synthetic is not None:
        return [FrequencyTable.from_groups(cols, types, 0, groups, num_rows,
                                           null_key_rows=null_key_rows, null_as_group=nag)
                for groups, num_rows, null_key_rows in case.synthetic(world)]
    out = []
    for shard in _device_shards(case, world, device):
        ft = FrequencyTable(cols, types, 0)
        for batch in shard.batches:
            ft.add([batch[c] for c in cols], null_as_group=nag)
        out.append(ft)
    return out


def _balanced(counts, n, world, what):
    """A5: every count within six standard deviations of binomial(n, 1 / W)."""
    bound = 6.0 * math.sqrt(n * (world - 1)) / world
    for j, c in enumerate(counts):
        assert abs(c - n / world) <= bound, (what, j, int(c), n / world, bound)


def _check_owners(case, world, owners, ref, topk=True):
    """B1-B4 on the owners' tables; returns the union of their groups."""
    types = case.key_types
    union, nullg, lit = Counter(), [], []
    g = u = nk = 0
    entropy = 0.0
    exports = [_export(owned, types) for owned in owners]
    for j, (owned, got) in enumerate(zip(owners, exports)):
        assert not set(got) & set(union), f"groups on two owners ({j})"      # B1
        union.update(got)
        assert owned.num_rows == ref.num_rows                                 # B2
        s = owned.summarize()
        assert s.n_groups == len(got) == owned.count()
        g, u, nk = g + s.n_groups, u + s.n_unique, nk + s.n_null_key_rows
        entropy += s.entropy                                                  # rank order
        a, b = owned.null_literal()
        nullg.append(a)
        lit.append(b)
    assert union == ref.groups                                                # B1
    assert (g, u, nk) == (ref.n_groups, ref.n_unique, ref.null_key_rows)      # B2
    assert sum(nullg) == nullg[0] == ref.null_group_rows
    one_utf8 = types == [N.UTF8] and case.null_as_group
    assert sum(lit) == (ref.literal_rows if one_utf8 else 0)
    assert sum(1 for v in lit if v) <= 1
    want = ref.entropy
    assert entropy == want or abs(entropy - want) <= REL * max(abs(entropy), abs(want)), \
        (entropy, want)                                                       # B3
    if topk:                                                                  # B4
        for k in (1, 10, 1000):
            merged = []
            for owned, got in zip(owners, exports):
                top = _decode_groups(types, *owned.topk_raw(k))
                counts = [c for _, c in sorted(top.items(), key=lambda kv: -kv[1])]
                assert counts == sorted(got.values(), reverse=True)[:k]
                for key, c in top.items():
                    assert ref.groups[key] == c
                merged += list(top.items())
            merged.sort(key=lambda kv: -kv[1])  # stable: ties keep rank order
            assert [c for _, c in merged[:k]] == ref.top_counts[:k], k
    if ref.n_groups >= RC.BALANCE_MIN_KEYS and 1 < world <= 8:                # A5, summed
        keyed = [len([k for k in got if k != (None,)]) for got in exports]
        _balanced(keyed, sum(keyed), world, "owners")
    return union


def _records_run(name, world, device):
    import torch

    from deequ_amd.analyzers.grouping import FrequencyTable, _decode_fixed
    from deequ_amd.distributed import freq_add_records, freq_partition
    case = RC.CASES[name]
    cols, types, nag = case.key_columns, case.key_types, case.null_as_group
    exact = _one_fixed(types)
    shard_refs = RC.shard_reference(case, world)
    ref = RC.merge(shard_refs)
    locals_ = _local_tables(case, world, device)
    owner_of, parts, special = {}, [], np.zeros(3, np.int64)
    for r, (local, sref) in enumerate(zip(locals_, shard_refs)):
        assert local.num_rows == sref.num_rows
        exported = _export(local, types)
        assert exported == sref.groups, f"shard {r}: the local table"
        keyed = {k: c for k, c in exported.items() if k != (None,)}
        rec, var, rc, vb, sp = freq_partition(local, world)
        assert len(rc) == len(vb) == world
        # A1
        assert int(rc.sum()) == len(keyed) and rec.numel() == len(keyed) * REC.itemsize
        assert sp.tolist() == [0, sref.null_group_rows, sref.null_key_rows]
        assert var.numel() == int(vb.sum()) and (exact or len(keyed) == 0 or var.numel() > 0)
        got = Counter()
        segs = _segments(rec, var, rc, vb)
        for j, (recs, vbytes) in enumerate(segs):
            assert len(recs) == rc[j] and len(vbytes) == vb[j] and vb[j] % 8 == 0
            for key, c in _decode_segment(recs, vbytes, types, exact):     # A3
                assert key not in got, f"shard {r}: {key} written twice"    # A2
                got[key] = c
                assert owner_of.setdefault(key, j) == j, f"{key}: owners {owner_of[key]} and {j}"  # A4
        assert got == keyed, f"shard {r}: records != export"               # A2
        if exact and types[0] not in (N.FLOAT32, N.FLOAT64):
            # the same through the product's decoder of a fixed-width key
            mine = {((_decode_fixed(types[0], k[0]),), c) for k, c in got.items()}
            assert mine == {kc for kc in local.export() if kc[0] != (None,)}
        if ref.n_groups >= RC.BALANCE_MIN_KEYS and 1 < world <= 8 and len(keyed) >= 1_000:
            _balanced(rc, len(keyed), world, f"shard {r}")                  # A5
        special += sp
        parts.append((rec, var, rc, vb))
    # the all-to-all: segment j of every shard, in rank order, to owner j
    rb = REC.itemsize
    owners = []
    for j in range(world):
        recs, vars_ = [], []
        for rec, var, rc, vb in parts:
            r0, v0 = int(rc[:j].sum()) * rb, int(vb[:j].sum())
            recs.append(rec[r0: r0 + int(rc[j]) * rb])
            vars_.append(var[v0: v0 + int(vb[j])])
        src_rc = np.array([p[2][j] for p in parts], np.int64)
        src_vb = np.array([p[3][j] for p in parts], np.int64)
        owned = FrequencyTable(cols, types, 0, capacity_hint=int(src_rc.sum()))
        freq_add_records(owned, torch.cat(recs), torch.cat(vars_), src_rc, src_vb, ref.num_rows,
                         special if j == 0 else np.zeros(3, np.int64), nag)
        owners.append(owned)
    union = _check_owners(case, world, owners, ref)
    held = {}  # A4 once more: a key's segment is the owner that holds it
    for j, owned in enumerate(owners):
        for key in _export(owned, types):
            if key != (None,):
                held[key] = j
    assert held == owner_of
    # B5: the owner with the most groups, partitioned again with W = 1 and inserted afresh
    big = max(range(world), key=lambda j: owners[j].count())
    rec, var, rc, vb, sp = freq_partition(owners[big], 1)
    again = FrequencyTable(cols, types, 0)
    freq_add_records(again, rec, var, rc, vb, owners[big].num_rows, sp, nag)
    assert _export(again, types) == _export(owners[big], types)
    assert again.num_rows == owners[big].num_rows
    assert again.null_literal() == owners[big].null_literal()
    return union


@lru_cache(maxsize=None)
def _records_union(name, world, device):
    return _records_run(name, world, device)


@pytest.mark.parametrize("name,world", RC.RECORD_PAIRS)
def test_records_path(name, world, gpu_device):
    ref = RC.reference(RC.CASES[name], world)
    assert _records_union(name, world, gpu_device) == ref.groups


# ------------------------------------------------------------------------------------------------
# The raw-key path
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,world", RC.RAW_PAIRS)
def test_raw_key_path(name, world, gpu_device):
    import torch

    from deequ_amd.distributed import RAW_KEY_ELEM, raw_key_count, raw_key_partition
    case = RC.CASES[name]
    col, dtype, nag = case.key_columns[0], case.key_types[0], case.null_as_group
    elem = RAW_KEY_ELEM[dtype]
    npt = {1: np.uint8, 2: np.uint16, 4: np.uint32, 8: np.uint64}[elem]
    raw_all = RC._fixed_buffer(case.columns[0], npt)
    keys_all = RC.row_keys(case)
    bounds = RC.shard_bounds(case.n_rows, case.weights, world)
    ref = RC.reference(case)
    owner_of, parts, tot_nulls = {}, [], 0
    for r, shard in enumerate(_device_shards(case, world, gpu_device)):
        lo, hi = bounds[r], bounds[r + 1]
        rows = hi - lo
        keys = keys_all[lo:hi]
        valid = np.array([k[0] is not None for k in keys], bool)
        buf = torch.full((rows * elem + GUARD,), GUARD_BYTE, dtype=torch.uint8, device=gpu_device)
        out, counts, nulls = raw_key_partition(shard, col, dtype, world, nag, out=buf)
        assert out is buf and len(counts) == world
        n_valid = int(valid.sum())
        assert int(counts.sum()) == n_valid and nulls == rows - n_valid                # C1
        host = buf.cpu().numpy()
        assert np.all(host[n_valid * elem:] == GUARD_BYTE), "written past the segments"  # C2
        sent = host[: n_valid * elem].view(npt)
        want = raw_all[lo:hi][valid]
        assert np.array_equal(np.sort(sent), np.sort(want))                             # C2
        canon = dict(zip(want.tolist(), (k[0] for k, ok in zip(keys, valid) if ok)))
        at = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
        for j in range(world):                                                          # C3
            for v in np.unique(sent[at[j]: at[j + 1]]).tolist():
                key = (canon[v],)
                assert owner_of.setdefault(key, j) == j, f"{key}: owners {owner_of[key]} and {j}"
        tot_nulls += nulls
        parts.append((buf, counts, at))
    owners = []
    for j in range(world):
        recv = torch.cat([buf[int(at[j]) * elem: int(at[j + 1]) * elem] for buf, _, at in parts])
        n_recv = sum(int(c[j]) for _, c, _ in parts)
        assert recv.numel() == n_recv * elem
        owners.append(raw_key_count(recv, n_recv, col, dtype, 0, j, world, case.n_rows, tot_nulls,
                                    nag))
    union = _check_owners(case, world, owners, ref, topk=False)                         # C4
    held = {k: j for j, o in enumerate(owners) for k in _export(o, case.key_types) if k != (None,)}
    assert held == owner_of                                                             # C3
    assert union == _records_union(name, world, gpu_device)                             # C5


# ------------------------------------------------------------------------------------------------
# Argument checks: refused before any kernel runs, the table left as it was
# ------------------------------------------------------------------------------------------------
def _small_table(device, utf8=False):
    from deequ_amd.analyzers.grouping import FrequencyTable
    from deequ_amd.table import Table
    vals = ["a", "bb", None, "a"] if utf8 else [1, 2, None, 1]
    t = Table.from_pydict({"k": vals}, {"k": "string" if utf8 else "int64"}, device=device)
    ft = FrequencyTable(["k"], [t.schema["k"].dtype], 0)
    ft.add([t.batches[0]["k"]])
    return t, ft


def _refused(code, fn, *args):
    with pytest.raises(N.EngineError) as e:
        fn(*args)
    assert e.value.code == code, (e.value.code, str(e.value))


def _untouched(ft):
    s = ft.summarize()
    return (ft.num_rows, s.n_groups, s.n_unique, s.n_null_key_rows, ft.null_literal())


@pytest.mark.parametrize("n_parts", [0, 65])
def test_bad_world_sizes_are_unsupported(n_parts, gpu_device):
    import torch

    from deequ_amd.distributed import freq_add_records, freq_partition, raw_key_partition
    t, ft = _small_table(gpu_device)
    _refused(N.ERR_UNSUPPORTED, freq_partition, ft, n_parts)
    out = torch.full((64,), GUARD_BYTE, dtype=torch.uint8, device=gpu_device)
    stream = ctypes.c_void_p(torch.cuda.current_stream(gpu_device).cuda_stream)
    assert N.lib.dq_freq_partition(ft.handle, n_parts, out.data_ptr(), out.data_ptr(),
                                   stream) == N.ERR_UNSUPPORTED
    _refused(N.ERR_UNSUPPORTED, raw_key_partition, t, "k", N.INT64, n_parts, False, out)
    assert np.all(out.cpu().numpy() == GUARD_BYTE)
    fresh = _small_table(gpu_device)[1]
    before = _untouched(fresh)
    rec = torch.zeros(24 * max(1, n_parts), dtype=torch.uint8, device=gpu_device)
    sizes = np.ones(n_parts, np.int64)
    _refused(N.ERR_UNSUPPORTED, freq_add_records, fresh, rec, rec[:0], sizes, 0 * sizes, 5,
             np.zeros(3, np.int64))
    assert _untouched(fresh) == before


def test_bad_segment_sizes_and_special_are_refused(gpu_device):
    import torch

    from deequ_amd.distributed import freq_add_records, freq_partition
    _, src = _small_table(gpu_device, utf8=True)
    rec, var, rc, vb, sp = freq_partition(src, 1)
    assert vb[0] % 8 == 0 and vb[0] > 0
    _, ft = _small_table(gpu_device, utf8=True)
    before = _untouched(ft)
    exported = _export(ft, [N.UTF8])
    _refused(N.ERR_INVALID_ARGUMENT, freq_add_records, ft, rec, var, rc, vb - 4, 4, sp)
    _refused(N.ERR_INVALID_ARGUMENT, freq_add_records, ft, rec, var, rc, -vb, 4, sp)
    _refused(N.ERR_INVALID_ARGUMENT, freq_add_records, ft, rec, var, -rc, vb, 4, sp)
    assert _untouched(ft) == before
    # special[0] was a count once; a non-zero value is refused with nothing inserted or counted
    _refused(N.ERR_INVALID_ARGUMENT, freq_add_records, ft, rec, var, rc, vb, 4,
             np.array([1, 0, 7], np.int64))
    assert _untouched(ft) == before and _export(ft, [N.UTF8]) == exported
    freq_add_records(ft, rec, var, rc, vb, 4, sp)  # and the table still takes a good call
    assert ft.num_rows == 8 and _export(ft, [N.UTF8]) == Counter({(b"a",): 4, (b"bb",): 2})
    assert ft.summarize().n_null_key_rows == 2


@pytest.mark.parametrize("values,arrow_type", [(["a", None, "bc"], "string"),
                                               ([True, None, False], "bool_")])
def test_raw_keys_need_a_fixed_width_column(values, arrow_type, gpu_device):
    import torch

    from deequ_amd.table import Table
    t = Table.from_pydict({"k": values}, {"k": arrow_type}, device=gpu_device)
    arr = (N.dq_column * 1)(t.batches[0]["k"].to_c())
    out = torch.full((64,), GUARD_BYTE, dtype=torch.uint8, device=gpu_device)
    counts = np.full(2, -1, np.int64)
    nulls = ctypes.c_int64(-1)
    stream = ctypes.c_void_p(torch.cuda.current_stream(gpu_device).cuda_stream)
    status = N.lib.dq_key_partition(arr, 1, 2, 0, out.data_ptr(), counts.ctypes.data,
                                    ctypes.byref(nulls), stream)
    assert status == N.ERR_WRONG_TYPE
    torch.cuda.synchronize()
    assert np.all(out.cpu().numpy() == GUARD_BYTE) and counts.tolist() == [-1, -1]
    assert nulls.value == -1
