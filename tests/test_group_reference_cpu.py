"""tests/group_reference.py without a GPU: every mirror against a second implementation in plain Python integers, the table
geometry at the two specs and at every dense size of the GPU cases, and every case builder's claims -- group counts, partitions,
probe distances, wraps, rows per tile, heavy-hitter counts -- from the mirrors and np.unique alone.  The oracle is run over every case
of at most 300 000 rows: it must return the np.unique number of groups and count exactly the rows the Filter keeps.

What cannot be checked here is that the device hashes as the mirrors say: that takes a GPU, where the stage_info facts of the cases
fail if it does not (tests/test_sizes_group_forms_gpu.py)."""
import numpy as np
import pytest

import group_reference as gr
from oracle import oracle

M64, M32 = (1 << 64) - 1, (1 << 32) - 1


# ---- second implementations ----------------------------------------------------------------------------------------------------------
def py_hash_local(k):
    h = (k & M32) ^ (((k >> 32) * 0x9E3779B1) & M32)
    h ^= h >> 15
    h = (h * 0x85EBCA77) & M32
    return h ^ (h >> 13)


def py_part_of(k, parts):
    h = (py_hash_local(k) * 0x2C1B3C6D) & M32
    h ^= h >> 16
    return (((h * 0x297A2D39) & M32) * parts) >> 32


def py_hash64(k):
    k ^= k >> 33
    k = (k * 0xff51afd7ed558ccd) & M64
    k ^= k >> 33
    k = (k * 0xc4ceb9fe1a85ec53) & M64
    return (k ^ (k >> 33)) & M32


def py_pack(fields, values):
    """values[k]: an int, or None for NULL (nullable keys are those with a None somewhere in `nullable`)."""
    key, shift = 0, 0
    for (t, nullable), v in zip(fields, values):
        bits = {"BOOL": 8, "INT32": 32, "INT64": 64}[t]
        key |= ((1 << bits) if v is None else (v & ((1 << bits) - 1))) << shift
        shift += bits + (1 if nullable else 0)
    return key


SAMPLE = [0, 1, 2, M64, M64 - 1, 1 << 32, (1 << 32) - 1, 1 << 63, 0x0123456789ABCDEF] + [int(x) for x in np.random.default_rng(1).integers(0, 1 << 64, 500, dtype=np.uint64)]


def test_hashes_against_python_integers():
    keys = np.array(SAMPLE, dtype=np.uint64)
    assert gr.hash_local(keys).tolist() == [py_hash_local(k) for k in SAMPLE]
    for parts in (1, 2, 7, 16, 32, 256, 8192):
        assert gr.part_of(keys, parts).tolist() == [py_part_of(k, parts) for k in SAMPLE]
        assert (gr.part_of(keys, 2 * parts) // np.uint64(2) == gr.part_of(keys, parts)).all()      # doubling the partitions splits each in two
    for C in (1, 64, 65, 1100, 4954):
        assert gr.local_home(keys, C).tolist() == [(py_hash_local(k) * C) >> 32 for k in SAMPLE]
    assert gr.home_slot(64, keys).tolist() == [py_hash64(k) & 63 for k in SAMPLE]


def test_key_packing_against_python_integers():
    rng = np.random.default_rng(2)
    a, b = rng.integers(-(1 << 31), 1 << 31, 300).astype(np.int32), rng.integers(-(1 << 31), 1 << 31, 300).astype(np.int32)
    a[:4], b[:4] = [-1, -1, 0, -2], [-1, 0, -1, -1]
    z = rng.random(300) < 0.3
    w = rng.integers(-(1 << 63), 1 << 63, 300)
    got = gr.pack_group_key(["INT32", "INT32"], [a, b], [None, None])
    assert got.tolist() == [py_pack([("INT32", False)] * 2, [int(x), int(y)]) for x, y in zip(a, b)] and got[0] == gr.ALL_ONES
    t = b > 0
    got = gr.pack_group_key(["INT32", "BOOL"], [a, t], [z, None])           # the NULL bit of the first key sits at bit 32, the second key above it
    assert got.tolist() == [py_pack([("INT32", True), ("BOOL", False)], [None if n else int(x), int(y)]) for x, y, n in zip(a, t, z)]
    assert int(got[z][0]) & ((1 << 33) - 1) == 1 << 32
    got = gr.pack_group_key(["INT64"], [w], [None])
    assert got.tolist() == [int(x) & M64 for x in w]
    got = gr.pack_group_key(["INT32"], [a], [z])
    assert got.tolist() == [(1 << 32) if n else int(x) & M32 for x, n in zip(a, z)]


def test_table_entries_at_the_two_specs():
    assert gr.acc_words("SMALL") == (3, False) and gr.acc_words("WIDE") == (16, False)
    assert gr.table_entries(3, False, 80 * 1024)[1:] == (32, 4260)
    assert gr.PART_AGG_LDS == 4260 + 64 * 32 == 6308 and gr.C_SMALL == 64
    assert gr.table_entries(3, False, gr.PART_AGG_LDS - 1)[0] == 63          # one byte less: below the fewest entries the runtime accepts
    assert gr.table_entries(16, False, 80 * 1024)[1:] == (8 + 17 * 8, 8 + 17 * 8 + 4100 + 128)
    assert gr.C_FULL == (159 * 1024 - 4372) // 144 == 1100 and gr.C_FULL < gr.TILE
    assert gr.table_entries(3, True, 80 * 1024)[1] == 8 + 3 * 8 + 3 * 4 and gr.table_entries(4, True, 80 * 1024)[1] == 8 + 5 * 8 + 5 * 4


def test_dense_geometry_at_every_size_of_the_dense_cases():
    wide, small = gr.acc_words("WIDE"), gr.acc_words("SMALL")
    geo = gr.dense_geometry
    # D1: one table up to C_FULL slots, then 17 partitions (slots / 64) of 65 entries
    assert geo([gr.C_FULL], [False], 4 * gr.C_FULL + 3, *wide, options={}) == (True, 1100, True, 1, 1100)
    assert geo([gr.C_FULL + 1], [False], 4 * gr.C_FULL + 7, *wide, options={}) == (True, 1101, False, 17, 65)
    assert geo([gr.C_FULL], [False], 4403, *wide, options={"group_resident": 0})[2] is False
    # D2: slots <= rows / 4
    assert geo([5000], [False], 20000, *small, options={}) == (True, 5000, False, 78, 65)
    assert geo([5000], [False], 19999, *small, options={})[0] is False
    assert geo([4096], [False], 1, *small, options={})[0] is True and geo([4097], [False], 16387, *small, options={})[0] is False     # (the floor of 4096 slots)
    # D3: 2^21 slots
    rows = gr.DENSE_ROWS_AT_MAX
    assert rows == 8388608
    assert geo([1 << 21], [False], rows, *small, options={}) == (True, 1 << 21, False, 1024, 2048)
    assert geo([1 << 21], [False], rows - 4, *small, options={})[0] is False
    assert geo([(1 << 21) + 1], [False], rows, *small, options={})[0] is False
    assert geo([2048, 1024], [False, False], rows, *small, options={}) == (True, 1 << 21, False, 1024, 2048)
    assert geo([2049, 1024], [False, False], rows, *small, options={})[0] is False
    # D4 / D5
    assert geo([1008], [True], 3000, *small, options={}) == (True, 1009, True, 1, 1009)
    assert geo([1008], [True], 3000, *small, options={"dense_parts": 7, "group_resident": 0}) == (True, 1009, False, 7, 145)
    assert geo([0], [True], 3000, *small, options={}) == (True, 1, True, 1, 1)
    assert geo([0, 2], [True, False], 3000, *small, options={}) == (True, 2, True, 1, 2)
    assert geo([700], [False], 3000, *small, options={"dense_parts": 7, "group_resident": 0}) == (True, 700, False, 7, 100)
    assert geo([16384], [False], 65536, *small, options={"dense_parts": 256, "group_resident": 0}) == (True, 16384, False, 256, 64)
    assert geo([16384], [False], 65535, *small, options={"dense_parts": 256, "group_resident": 0})[0] is False


def test_hot_thresholds():
    assert gr.hot_min_count(1 << 18, 256) == 256 and gr.hot_min_count(1000, 256) == 16
    assert gr.hot_keys_reported(np.array([5243] * 32 + [19]), 256) == 32
    assert gr.hot_keys_reported(np.array([5243] * 33 + [19]), 256) == 0        # the doubling passes 5243 before fewer than 33 keys are left
    assert gr.hot_keys_reported(np.array([6000 - 60 * h for h in range(33)]), 256) == 32      # at 4096 the smallest (4080) drops out


def test_probe_distances_and_keys_with():
    rng = np.random.default_rng(3)
    keys = gr.keys_with(16, 5, 64, 63, 4, rng)
    assert len(np.unique(keys)) == 4 and [py_part_of(int(k), 16) for k in keys] == [5] * 4 and [(py_hash_local(int(k)) * 64) >> 32 for k in keys] == [63] * 4
    assert gr.probe_distances(keys, 16, 64).tolist() == [0, 1, 2, 3]          # 63, then 0, 1, 2: across the table's end
    other = gr.keys_with(16, None, 64, None, 50, rng, avoid_part=5)
    assert 5 not in gr.part_of(other, 16).tolist() and not (other == gr.ALL_ONES).any()
    assert gr.probe_distances(np.array([gr.ALL_ONES] * 3, dtype=np.uint64), 16, 64).tolist() == [0, 0, 0]
    # a table of 3 entries, by hand: homes in insertion order and the entries they end on
    three = gr.keys_with(1, 0, 3, 2, 3, rng)
    assert gr.probe_distances(three, 1, 3).tolist() == [0, 1, 2]


# ---- the cases ---------------------------------------------------------------------------------------------------------------------------
def check_oracle(case):
    """The oracle over a case: the np.unique number of groups, COUNT(*) (SMALL) summing to the rows the Filter keeps."""
    assert case.rows <= 300000
    view = case.view()
    _schema, cols = oracle.run(case.op(view))
    n_keys = len(case.keys)
    assert len(cols) == n_keys + len(gr.SPECS[case.spec][0])
    assert len(cols[0][0]) == len(case.groups()), case.name
    if case.spec == "SMALL":
        assert int(cols[n_keys][0].sum()) == int(case.kept().sum()), case.name
    return cols


@pytest.mark.parametrize("local", [1, 0])
@pytest.mark.parametrize("kind", gr.DIRECT_KINDS)
def test_direct_cases(kind, local):
    case = gr.direct_case(kind, local)
    groups = case.groups()
    want = {"full": 64, "full_and_all_ones": 65, "one_past_full": 65, "one_chain": 64, "all_ones_1_row": 1, "all_ones_3000_rows": 1, "all_filtered": 0}[kind]
    assert len(groups) == want
    ordinary = groups[groups != gr.ALL_ONES]
    assert len(ordinary) == {"full_and_all_ones": 64, "all_ones_1_row": 0, "all_ones_3000_rows": 0}.get(kind, want)
    if kind == "one_chain":
        assert [py_hash64(int(k)) & 63 for k in ordinary] == [gr.DIRECT_CHAIN_HOME] * 64 and gr.DIRECT_CHAIN_HOME > 0      # 64 slots from 61 on: wraps
    assert case.rows == {"all_ones_1_row": 1, "all_ones_3000_rows": 3000, "all_filtered": 70000}.get(kind, 5 * want)
    if local:
        check_oracle(case)


@pytest.mark.parametrize("rows", [65536, 65535])
@pytest.mark.parametrize("kind", gr.PARTITION_KINDS)
def test_partition_cases(kind, rows):
    case = gr.partition_case(kind, rows)
    keys = case.groups()
    part = gr.part_of(keys, gr.PART_N).astype(np.int64)
    target = keys[part == gr.TARGET]
    ordinary = target[target != gr.ALL_ONES]
    filler = keys[part != gr.TARGET]
    assert case.facts["plain_scatter"] == (1 if rows == 65536 and kind != "one_partition" else 0)
    if kind == "one_partition":
        assert case.rows == 80 and len(keys) == len(target) == 40 and (np.unique(case.packed(), return_counts=True)[1] == 2).all()
        assert gr.probe_distances(target, gr.PART_N, 64).max() < gr.PROBE_LIMIT
        check_oracle(case)
        return
    assert case.rows == rows
    # filler: 8 keys in each of the 15 other partitions (4 in either half), every one on its home entry, under 16 and under 32 partitions
    assert np.bincount(part[part != gr.TARGET], minlength=16).tolist() == [0 if p == gr.TARGET else 8 for p in range(16)]
    assert np.bincount(gr.part_of(filler, 32).astype(np.int64), minlength=32).tolist() == [0 if p // 2 == gr.TARGET else 4 for p in range(32)]
    assert gr.probe_distances(filler, 16, 64).max() == 0 and gr.probe_distances(filler, 32, 64).max() == 0
    # every partition's rows: an even share of every run of 2048 rows (no segment runs full)
    per_tile = np.array([np.bincount(gr.part_of(case.packed()[s:s + 2048], 16).astype(np.int64), minlength=16) for s in range(0, rows - 2047, 2048)])
    assert per_tile.min() == per_tile.max() == 128
    distance = gr.probe_distances(ordinary, 16, 64)
    homes = gr.local_home(ordinary, 64).astype(np.int64)
    if kind in ("chain32", "chain32_and_all_ones"):
        assert len(ordinary) == 32 and set(homes) == {gr.CHAIN_HOME} and distance.max() == 31 == gr.PROBE_LIMIT - 1
        assert (gr.ALL_ONES in target) == (kind == "chain32_and_all_ones") and py_part_of(M64, 16) == gr.TARGET
    elif kind == "chain33":
        assert len(ordinary) == 33 and set(homes) == {gr.CHAIN_HOME} and distance.max() == 32 == gr.PROBE_LIMIT
        assert sorted(gr.probe_distances(ordinary, 32, 64).tolist()) == sorted(list(range(17)) + list(range(16)))      # under 32 partitions: chains of 17 and 16
    elif kind == "wrap5":
        assert homes.tolist() == [63] * 5 and sorted((homes + distance) % 64) == [0, 1, 2, 3, 63]
    else:
        assert sorted(homes.tolist()) == [62] * 3 + [63] * 4 and sorted((homes + distance) % 64) == [0, 1, 2, 3, 4, 62, 63]
    check_oracle(case)


@pytest.mark.parametrize("rows", gr.LAST_TILE_ROWS)
def test_last_tile_cases(rows):
    assert gr.LAST_TILE_ROWS == (65536, 67583, 67584, 67585)
    case = gr.last_tile_case(rows)
    keys, counts = np.unique(case.packed(), return_counts=True)
    assert case.rows == rows and len(keys) == 500 and counts.max() - counts.min() <= 1 and gr.ALL_ONES not in keys
    if rows == 65536:
        check_oracle(case)


@pytest.mark.parametrize("shape", ["partitions", "one_table", "dense"])
def test_filtered_cases(shape):
    case = gr.filtered_case(shape)
    assert case.rows == 70000 and not case.kept().any() and len(case.groups()) == 0 and len(np.unique(case.packed())) == 700
    cols = check_oracle(case)
    assert all(len(d) == 0 for d, _z in cols)


@pytest.mark.parametrize("resident", [1, 0])
@pytest.mark.parametrize("kind", gr.ONE_TABLE_KINDS)
def test_one_table_cases(kind, resident):
    case = gr.one_table_case(kind, resident)
    g = case.notes["group_ids"]
    assert len(case.groups()) == len(np.unique(g)) == {"full": gr.C_FULL, "one_past_full": gr.C_FULL + 1, "three_tiles": gr.C_FULL + 1}[kind]
    assert gr.ALL_ONES not in case.groups()
    if kind == "three_tiles":
        per_tile = [len(np.unique(g[s:s + 512])) for s in range(0, len(g), 512)]       # whatever tile of 512, 1024 or 2048 rows a workgroup takes
        assert case.rows == 3 * gr.TILE and max(len(np.unique(g[s:s + gr.TILE])) for s in range(0, len(g), gr.TILE)) == gr.C_FULL - 100 and max(per_tile) <= 512
    else:
        assert case.rows == len(case.groups()) <= gr.TILE
    if resident:
        check_oracle(case)


def test_dense_cases():
    cases = [gr.dense_table_edge_case(gr.C_FULL), gr.dense_table_edge_case(gr.C_FULL + 1), gr.dense_rows_bound_case(20000), gr.dense_rows_bound_case(19999)]
    assert [c.facts["dense_slots"] for c in cases] == [gr.C_FULL, gr.C_FULL + 1, 5000, 0]
    assert [c.facts.get("group_shape") for c in cases] == [3, 1, 1, None]
    assert [len(c.groups()) for c in cases] == [gr.C_FULL, gr.C_FULL + 1, 5000, 5000] and cases[0].rows == 4 * gr.C_FULL + 3
    for partitioned in (False, True):
        c = gr.dense_span_edge_case("span_edges", partitioned)
        cases.append(c)
        assert c.facts == {"dense_slots": 1009, "group_shape": 1 if partitioned else 3} and len(c.groups()) == 3
        assert sorted(c.groups().tolist()) == sorted([py_pack([("INT32", True)], [v]) for v in (-7, 1000, None)])
    c = gr.dense_span_edge_case("all_null", False)
    assert c.facts == {"dense_slots": 1, "group_shape": 3} and c.groups().tolist() == [1 << 32]
    cases.append(c)
    c = gr.dense_span_edge_case("all_null_and_ordinary", False)
    assert c.facts == {"dense_slots": 2, "group_shape": 3} and c.groups().tolist() == [1 << 32, (1 << 32) | (1 << 33)]
    cases.append(c)
    for parts in (7, 256):
        c = gr.dense_partition_corner_case(parts)
        cap = c.notes["cap"]
        assert c.facts == {"dense_slots": parts * cap, "group_shape": 1, "reruns": [0, 0]} and c.notes["geometry"] == (True, parts * cap, False, parts, cap)
        idx = c.groups().astype(np.int64)                                  # (a single key from 0: the packed key is the slot index)
        assert sorted(zip((idx % parts).tolist(), (idx // parts).tolist())) == [(0, 0), (0, cap - 1), (parts - 1, 0), (parts - 1, cap - 1)]
        assert int(c.kept().sum()) == 200 and np.unique(c.packed()[c.kept()], return_counts=True)[1].tolist() == [50] * 4
        cases.append(c)
    for rows in gr.DENSE_PARTITION_ROWS:
        c = gr.dense_partitioned_rows_case(rows)
        assert c.facts == {"dense_slots": 700, "group_shape": 1} and len(c.groups()) == 700 and c.notes["geometry"][3:] == (7, 100)
        cases.append(c)
    assert gr.DENSE_PARTITION_ROWS == (2047, 2048, 2049, 16384, 16385)
    for c in cases:
        check_oracle(c)


@pytest.mark.parametrize("kind", gr.DENSE_MAX_KINDS)
def test_dense_cases_at_the_slot_limit(kind):
    # (8 388 608 rows: past what the oracle is asked to run here)
    c = gr.dense_max_slots_case(kind)
    at_max = kind.endswith("at_max")
    assert c.rows == 8388608 and c.facts["dense_slots"] == ((1 << 21) if at_max else 0)
    corners = c.notes["corners"]
    assert corners == (2 if kind.startswith("one_key") else 4)
    assert np.unique(c.packed()[c.kept()], return_counts=True)[1].tolist() == [64] * corners and len(np.unique(c.packed())) == corners
    spans = [int(d.max()) - int(d.min()) + 1 for _t, d, _z in c.keys]
    assert spans == {"one_key_at_max": [1 << 21], "one_key_past_max": [(1 << 21) + 1], "two_keys_at_max": [2048, 1024], "two_keys_past_max": [2049, 1024]}[kind]


@pytest.mark.parametrize("kind", gr.HOT_KINDS)
def test_hot_cases(kind):
    c = gr.hot_case(kind)
    threshold = gr.hot_min_count(gr.HOT_ROWS, gr.HOT_PARTS)
    assert c.rows == 262144 and threshold == 256
    keys, counts = np.unique(c.packed(), return_counts=True)
    hot = counts >= threshold
    if kind == "all_ones_half":
        assert keys[hot].tolist() == [M64] and counts[hot].tolist() == [131072] and c.facts["hot_keys"] == 0
        assert len(keys) == 5001
    else:
        assert sorted(counts[hot].tolist(), reverse=True) == sorted(c.notes["counts"], reverse=True) and len(keys) == 5000 + len(c.notes["counts"])
        assert c.facts["hot_keys"] == {"32_keys": 32, "33_equal_keys": 0, "33_falling_keys": 32}[kind]
        assert gr.ALL_ONES not in keys
    assert counts[~hot].max() < threshold and (~hot).sum() == 5000
    # hot rows lie everywhere: every tile of 2048 rows has some (kind 32_keys: about 1300), no partition's segment is spared
    if kind == "32_keys":
        is_hot = np.isin(c.packed(), keys[hot])
        per_tile = is_hot.reshape(-1, 2048).sum(axis=1)
        assert per_tile.min() > 1100 and per_tile.max() < 1500
    check_oracle(c)
