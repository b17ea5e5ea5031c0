"""Mirrors of GroupAggregate's table geometry and the inputs that put every execution shape on its table and row edges
(tests/test_group_reference_cpu.py checks both without a GPU; tests/test_sizes_group_forms_gpu.py runs the device over them).

The expected rows of every case come from the oracle (`oracle.run(op)`: the reference's hash aggregate restated on the CPU, which
shares nothing with the device's tables), compared after `sort_rows` on both sides, bit for bit: every DOUBLE input is a multiple of
0.25 of small magnitude, so every partial sum is exact under any order and no tolerance appears anywhere.

The mirrors below restate the code their docstrings cite.  They are used only to BUILD inputs -- keys that share a partition and a
home entry, ranges that end on a slot limit -- and never to compute expected rows.  Were the device to hash differently, the layouts
would degrade to ordinary keys: the rows would still compare exactly, but the `stage_info` facts of the cases (reruns, part_n,
hot_keys, dense_slots ...) would not hold.  That is how the GPU run checks the mirrors.

Out of reach at test sizes: part_n reaching 8192 (run_group_agg_partitioned gives up there: 8192 partitions of 64 entries need more than
2^18 groups clustered 33 deep), part_seg_growth reaching 64 through the VM scatter, and the 2^32-record limit of the segments."""
import numpy as np

from join_reference import ALL_ONES, U64, hash64, home_slot    # the global table homes keys as the join index does (pipeline_kernels.hip: hash64)

M32 = U64(0xFFFFFFFF)
NP_OF = {"INT64": np.int64, "INT32": np.int32, "BOOL": np.bool_}
TILE = 2048                      # rows of a tile of the plain scatter and of the resident kernel (1024 threads x 2 rows)
PLAIN_ROWS = 1 << 16             # run_group_agg_partitioned: the plain scatter runs from this many rows (or under dense slots)
HOT_MAX = 32                     # launch.h: SSGPU_HOT_MAX
DENSE_MAX_SLOTS = 1 << 21        # launch.h: SSGPU_DENSE_MAX_SLOTS
PROBE_LIMIT = 32                 # ssgpu_part_agg_kernel: probes of a hash partition's LDS table


# ---- mirrors -----------------------------------------------------------------------------------------------------------------------
def pack_group_key(fields, cols, nulls):
    """lower.cpp, lower_group_stage ("pack the key columns into one 64-bit word") and KEY_APPEND_* (pipeline_kernels.hip): fields fill
    from bit 0 in key order; a nullable key (nulls[k] is not None) takes one more bit directly above its value bits; a NULL has value
    bits zero and that bit set."""
    out = np.zeros(len(cols[0]), dtype=U64)
    shift = 0
    for t, col, z in zip(fields, cols, nulls):
        bits = np.dtype(NP_OF[t]).itemsize * 8
        v = np.ascontiguousarray(col, dtype=NP_OF[t]).view({8: np.uint8, 32: np.uint32, 64: np.uint64}[bits]).astype(U64)
        if z is not None:
            assert bits < 64
            v = np.where(np.asarray(z, dtype=bool), U64(1) << U64(bits), v)
        assert shift + bits + (z is not None) <= 64
        out |= v << U64(shift)
        shift += bits + (z is not None)
    return out


def hash_local(key):
    """hash_local of pipeline_kernels.hip / group_scatter_kernel.hip: 32 bits, as uint64."""
    k = np.asarray(key, dtype=U64)
    h = (k & M32) ^ (((k >> U64(32)) * U64(0x9E3779B1)) & M32)
    h ^= h >> U64(15)
    h = (h * U64(0x85EBCA77)) & M32
    h ^= h >> U64(13)
    return h


def local_home(key, C):
    """The entry of an LDS table of C entries (any number) where a key is looked for first: __umulhi(hash_local(key), C)."""
    return (hash_local(key) * U64(C)) >> U64(32)


def part_of(key, NP):
    """part_of of pipeline_kernels.hip / group_scatter_kernel.hip: the hash partition of a packed key among NP."""
    h = (hash_local(key) * U64(0x2C1B3C6D)) & M32
    h ^= h >> U64(16)
    return (((h * U64(0x297A2D39)) & M32) * U64(NP)) >> U64(32)


def table_entries(ng, any_cnt, budget):
    """(C, entry, fixed) of run_group_agg_partitioned (runtime.cpp): the LDS entries a table gets out of `budget` bytes -- 80 KiB or
    part_agg_lds for a hash partition, 159 KiB for the one-table form."""
    stw = ng | 1
    entry = 8 + 8 * stw + (4 * stw if any_cnt else 0)
    fixed = entry + 1025 * 4 + 128
    return (budget - fixed) // entry, entry, fixed


SPECS = {   # name -> ([(aggregation, input or "", output)], value columns)
    "SMALL": ([("COUNT", "", "n"), ("SUM", "v", "s"), ("MIN", "v", "mn")], [("v", "INT64")]),
    "WIDE": ([(f, c, "%s_%s" % (f.lower(), c)) for c in ("d0", "d1", "d2", "d3") for f in ("SUM", "MIN", "MAX")], [(c, "DOUBLE") for c in ("d0", "d1", "d2", "d3")]),
}


def acc_words(spec):
    """(ng, any_cnt) of the end of lower_group_stage (lower.cpp) for SPECS: a DOUBLE SUM takes two accumulator words (sum and
    compensation), everything else one; counts are kept when an aggregate's input is nullable -- no column of SPECS is."""
    aggs, values = SPECS[spec]
    types = dict(values)
    return sum(2 if f == "SUM" and types.get(c) == "DOUBLE" else 1 for f, c, _o in aggs), False


ONE_TABLE_BUDGET = 159 * 1024
C_MIN = 64                                                              # the fewest entries run_group_agg_partitioned accepts
_SMALL_ENTRY, _SMALL_FIXED = table_entries(*acc_words("SMALL"), budget=80 * 1024)[1:]
PART_AGG_LDS = _SMALL_FIXED + C_MIN * _SMALL_ENTRY                      # 6308: a partition table of exactly 64 entries for SMALL
C_SMALL = table_entries(*acc_words("SMALL"), budget=PART_AGG_LDS)[0]    # 64
C_FULL = table_entries(*acc_words("WIDE"), budget=ONE_TABLE_BUDGET)[0]  # about 1100: below one 2048-row tile
C_FULL_SMALL = table_entries(*acc_words("SMALL"), budget=ONE_TABLE_BUDGET)[0]


def dense_geometry(spans, nullable, rows, ng, any_cnt, options):
    """dense_configure (runtime.cpp) for one input of `rows` rows: spans[k] = distinct values hi - lo + 1 of key k's range (0: the key
    has no value at all), nullable[k] adds the NULL offset.  Returns (usable, slots, resident, np, cap)."""
    slots = 1
    for values, z in zip(spans, nullable):
        if values and values - 1 >= DENSE_MAX_SLOTS:
            return (False, 0, False, 0, 0)
        slots *= max(values + (1 if z else 0), 1)
        if slots > DENSE_MAX_SLOTS:
            return (False, 0, False, 0, 0)
    if rows > 0 and slots > max(rows // 4, 4096):
        return (False, 0, False, 0, 0)
    budget80 = options.get("part_agg_lds", 0) or 80 * 1024
    _c, entry, fixed = table_entries(ng, any_cnt, budget80)
    if fixed + 64 * entry > budget80:
        return (False, 0, False, 0, 0)
    cmax, cfull = (budget80 - fixed) // entry, (ONE_TABLE_BUDGET - fixed) // entry
    if slots <= cfull and options.get("group_slab", 1) != 0 and options.get("group_resident", 1) != 0:
        return (True, slots, True, 1, slots)
    np_min = (slots + cmax - 1) // cmax
    if options.get("dense_parts", 0) > 0:
        parts = max(options["dense_parts"], np_min)
    else:
        parts = 256
        while parts < np_min:
            parts *= 2
    parts = max(min(parts, max(np_min, max(slots // 64, 1))), 2)
    if parts > 4096:
        return (False, 0, False, 0, 0)
    return (True, slots, False, parts, (slots + parts - 1) // parts)


def hot_min_count(n_sample, NP):
    """run_group_agg_partitioned: a key is hot from a quarter of a partition's expected share of the sample, at least 16."""
    return max(n_sample // (4 * NP), 16)


def hot_keys_reported(counts, min_count):
    """ssgpu_hot_keys_kernel over exact per-key counts: the threshold doubles until at most HOT_MAX keys reach it."""
    thr = max(min_count, 1)
    for _round in range(24):
        if int((np.asarray(counts) >= thr).sum()) <= HOT_MAX:
            break
        thr *= 2
    return min(int((np.asarray(counts) >= thr).sum()), HOT_MAX)


def probe_distances(keys, NP, C):
    """The linear-probing distance (entries past its home, modulo C) of every key in its partition's table of C entries, keys inserted
    in the given order; the all-ones key takes no entry (distance 0).  The SET of taken entries -- and so the longest distance of a
    cluster from one home -- does not depend on the order."""
    keys = np.asarray(keys, dtype=U64)
    part, home = part_of(keys, NP), local_home(keys, C)
    taken = {}
    out = np.zeros(len(keys), dtype=np.int64)
    for j in range(len(keys)):
        if keys[j] == ALL_ONES:
            continue
        used = taken.setdefault(int(part[j]), set())
        assert len(used) < C
        e = int(home[j])
        while e in used:
            e = 0 if e + 1 == C else e + 1
        used.add(e)
        out[j] = (e - int(home[j])) % C
    return out


def keys_with(NP, part, C, home, count, rng, avoid_part=None):
    """`count` distinct random packed keys of partition `part` among NP (None: any but `avoid_part`) that home on entry `home` of a
    table of C entries (None: anywhere); never the all-ones word.  Random keys are drawn until enough of them do (keys_homing_at)."""
    found = np.zeros(0, dtype=U64)
    while len(found) < count:
        k = rng.integers(0, 1 << 64, 1 << 16, dtype=U64)
        ok = k != ALL_ONES
        if part is not None:
            ok &= part_of(k, NP) == U64(part)
        elif avoid_part is not None:
            ok &= part_of(k, NP) != U64(avoid_part)
        if home is not None:
            ok &= local_home(k, C) == U64(home)
        fresh = k[ok]
        _u, first = np.unique(np.concatenate([found, fresh]), return_index=True)
        found = np.concatenate([found, fresh])[np.sort(first)]
    return found[:count]


# ---- cases -------------------------------------------------------------------------------------------------------------------------
class GroupCase(object):
    """One GroupAggregate input.  keys: [(type, data, nulls or None)] in key order; spec: a name of SPECS; keep: bool per row (the
    rows a Filter `a > 0` lets through) or None (no Filter); options: the context's; facts: what stage_info must say -- a value, or a
    list with one value per run; notes: what the layout tells its checks."""

    def __init__(self, name, keys, spec, options, facts, keep=None, **notes):
        self.name, self.keys, self.spec, self.options, self.facts, self.keep, self.notes = name, keys, spec, options, facts, keep, notes
        self.rows = len(keys[0][1])

    def packed(self):
        return pack_group_key([t for t, _d, _z in self.keys], [d for _t, d, _z in self.keys], [z for _t, _d, z in self.keys])

    def kept(self):
        return np.ones(self.rows, bool) if self.keep is None else np.asarray(self.keep, dtype=bool)

    def value_columns(self):
        """[(name, type, data)]: v INT64 in [-50, 50); d0..d3 DOUBLE, multiples of 0.25 in [-16, 16) -- sums of 2^23 of them are exact."""
        i = np.arange(self.rows, dtype=np.int64)
        if self.spec == "SMALL":
            return [("v", "INT64", (i * 7919 + 13) % 100 - 50)]
        return [("d%d" % j, "DOUBLE", (((i * (31 + 2 * j) + 5 * j) % 128) - 64) * 0.25) for j in range(4)]

    def view(self):
        import supersonic_amd as ss
        types = {"INT64": ss.INT64, "INT32": ss.INT32, "BOOL": ss.BOOL, "DOUBLE": ss.DOUBLE}
        attrs = [ss.Attribute("k%d" % j, types[t], ss.NULLABLE if z is not None else ss.NOT_NULLABLE) for j, (t, _d, z) in enumerate(self.keys)]
        cols = [ss.Column(np.ascontiguousarray(d, dtype=NP_OF[t]), np.asarray(z, dtype=bool)) if z is not None else np.ascontiguousarray(d, dtype=NP_OF[t])
                for t, d, z in self.keys]
        for name, t, data in self.value_columns():
            attrs.append(ss.Attribute(name, types[t]))
            cols.append(data)
        if self.keep is not None:
            attrs.append(ss.Attribute("a", ss.INT64))
            cols.append(self.kept().astype(np.int64))
        return ss.View(ss.TupleSchema(attrs), cols)

    def op(self, view):
        import supersonic_amd as ss
        spec = ss.AggregationSpecification()
        for f, c, o in SPECS[self.spec][0]:
            spec.AddAggregation(getattr(ss, f), c, o)
        child = ss.ScanView(view)
        if self.keep is not None:
            child = ss.Filter(ss.Greater(ss.NamedAttribute("a"), ss.ConstInt64(0)), ss.ProjectAllAttributes(), child)
        return ss.GroupAggregate(ss.ProjectNamedAttributes(["k%d" % j for j in range(len(self.keys))]), spec, None, child)

    def groups(self):
        """Distinct packed keys of the rows the Filter keeps (np.unique alone: the packed key is injective over the key columns)."""
        return np.unique(self.packed()[self.kept()])


def _i64(packed):
    return [("INT64", np.asarray(packed, dtype=U64).view(np.int64).copy(), None)]


def _i32_pair(g, width):
    g = np.asarray(g, dtype=np.int64)
    return [("INT32", (g // width).astype(np.int32), None), ("INT32", (g % width).astype(np.int32), None)]


def _ordinary_keys(rng, count):
    out = np.unique(rng.integers(0, 1 << 64, count + 8, dtype=U64))
    out = out[out != ALL_ONES]
    assert len(out) >= count
    return rng.permutation(out)[:count]


# A. direct shape
DIRECT_CAPACITY = 64
DIRECT_KINDS = ("full", "full_and_all_ones", "one_past_full", "one_chain", "all_ones_1_row", "all_ones_3000_rows", "all_filtered")
DIRECT_CHAIN_HOME = 61


def direct_case(kind, local):
    """A. group_partition = 0, a global table of 64 slots (+ the slot of the all-ones key) behind the LDS table (local = 1) or alone."""
    rng = np.random.default_rng(DIRECT_KINDS.index(kind) + 100)
    options = {"group_partition": 0, "group_capacity": DIRECT_CAPACITY, "group_local": local, "group_dense": 0}
    facts, keep, reps = {"group_shape": 0, "reruns": [0, 0]}, None, 5
    if kind == "full":
        keys = _ordinary_keys(rng, 64)
    elif kind == "full_and_all_ones":
        keys = np.concatenate([_ordinary_keys(rng, 64), [ALL_ONES]])
    elif kind == "one_past_full":
        keys, facts = _ordinary_keys(rng, 65), {"group_shape": 0, "reruns": [1, 0]}
    elif kind == "one_chain":                                            # every key homes on ONE slot: a chain of 64 that wraps the table's end
        keys = keys_with(1, None, 1, None, 1 << 13, rng)
        keys = keys[home_slot(DIRECT_CAPACITY, keys) == U64(DIRECT_CHAIN_HOME)][:64]
        assert len(keys) == 64
    elif kind in ("all_ones_1_row", "all_ones_3000_rows"):
        keys, reps = np.array([ALL_ONES], dtype=U64), 1 if kind == "all_ones_1_row" else 3000
    else:
        keys, reps, keep = _ordinary_keys(rng, 700), 100, np.zeros(70000, bool)
    rows = rng.permutation(np.tile(keys, reps))
    return GroupCase("direct-%s-local%d" % (kind, local), _i64(rows), "SMALL", options, facts, keep)


# B. hash partitions
PART_N = 16
PARTITION_OPTIONS = {"group_partition": 2, "part_n": PART_N, "part_agg_lds": PART_AGG_LDS, "group_slab": 0, "group_dense": 0}
TARGET = int(part_of(np.array([ALL_ONES]), PART_N)[0])                   # the partition the all-ones key is routed to
PARTITION_KINDS = ("chain32", "chain32_and_all_ones", "chain33", "wrap5", "wrap3_4", "one_partition")
CHAIN_HOME = 20


def filler_keys(rng):
    """8 keys for each of the 16 partitions but TARGET, on the home entries 0, 8, .. 56 of a 64-entry table (probe distance 0), four in
    either half of the partition (the partitions 2 p and 2 p + 1 of 32): {partition: keys}."""
    return {p: np.concatenate([keys_with(2 * PART_N, 2 * p + (j & 1), C_SMALL, 8 * j, 1, rng) for j in range(8)]) for p in range(PART_N) if p != TARGET}


def _dealt(by_part, rows):
    """Row i carries a key of partition order[i % len]: its keys in turn.  Every run of rows holds every partition's even share, so
    no (partition, workgroup) or (partition, XCD) segment runs full."""
    order = sorted(by_part)
    i = np.arange(rows)
    which, turn = i % len(order), i // len(order)
    out = np.zeros(rows, dtype=U64)
    for j, p in enumerate(order):
        mine = which == j
        out[mine] = by_part[p][turn[mine] % len(by_part[p])]
    return out


def partition_case(kind, rows):
    """B. 16 hash partitions of 64-entry tables; rows = 65536: the plain scatter, 65535: the VM scatter."""
    rng = np.random.default_rng(PARTITION_KINDS.index(kind) + 200)
    facts = {"group_shape": 1, "reruns": [0, 0], "part_n": [PART_N, PART_N], "hot_keys": 0, "plain_scatter": int(rows >= PLAIN_ROWS)}
    by_part = filler_keys(rng)
    if kind in ("chain32", "chain32_and_all_ones"):                        # 32 keys on one home entry: the last one is found by the 32nd probe
        by_part[TARGET] = keys_with(PART_N, TARGET, C_SMALL, CHAIN_HOME, 32, rng)
        if kind == "chain32_and_all_ones":
            by_part[TARGET] = np.concatenate([by_part[TARGET], [ALL_ONES]])
    elif kind == "chain33":                                               # 33: one too many; halves of 17 and 16 under 32 partitions
        by_part[TARGET] = np.concatenate([keys_with(2 * PART_N, 2 * TARGET, C_SMALL, CHAIN_HOME, 17, rng), keys_with(2 * PART_N, 2 * TARGET + 1, C_SMALL, CHAIN_HOME, 16, rng)])
        facts["part_n"], facts["reruns"] = [2 * PART_N, 2 * PART_N], [">=1", 0]
    elif kind == "wrap5":
        by_part[TARGET] = keys_with(PART_N, TARGET, C_SMALL, C_SMALL - 1, 5, rng)
    elif kind == "wrap3_4":
        by_part[TARGET] = np.concatenate([keys_with(PART_N, TARGET, C_SMALL, C_SMALL - 2, 3, rng), keys_with(PART_N, TARGET, C_SMALL, C_SMALL - 1, 4, rng)])
    else:                                                                 # every row in ONE partition: 40 keys anywhere in its table, 2 rows each
        by_part, rows = {TARGET: keys_with(PART_N, TARGET, C_SMALL, None, 40, rng)}, 80
        facts = {"group_shape": 1, "part_n": [PART_N, PART_N], "hot_keys": 0, "plain_scatter": 0}
    return GroupCase("partitions-%s-%d" % (kind, rows), _i64(_dealt(by_part, rows)), "SMALL", PARTITION_OPTIONS, facts, by_part=by_part)


LAST_TILE_ROWS = tuple(PLAIN_ROWS + extra for extra in (0, TILE - 1, TILE, TILE + 1))


def last_tile_case(rows):
    """B5. 500 groups dealt evenly over `rows` rows: the plain scatter's last tile holds 0 / 2047 / 2048 / 1 rows more."""
    keys = _ordinary_keys(np.random.default_rng(250), 500)
    facts = {"group_shape": 1, "plain_scatter": 1, "hot_keys": 0}
    return GroupCase("partitions-500-groups-%d" % rows, _i64(keys[np.arange(rows) % 500]), "SMALL", PARTITION_OPTIONS, facts)


def filtered_case(shape):
    """A5 in the other shapes: a Filter drops every one of 70 000 rows."""
    rows = 70000
    g = np.arange(rows) % 700
    if shape == "partitions":
        return GroupCase("partitions-all-filtered", _i64(_ordinary_keys(np.random.default_rng(5), 700)[g]), "SMALL", PARTITION_OPTIONS, {}, np.zeros(rows, bool))
    if shape == "one_table":
        return GroupCase("one-table-all-filtered", _i32_pair(g, 40), "WIDE", dict(ONE_TABLE_OPTIONS, group_resident=1), {}, np.zeros(rows, bool))
    return GroupCase("dense-all-filtered", [("INT32", g.astype(np.int32), None)], "SMALL", dict(DENSE_OPTIONS), {}, np.zeros(rows, bool))


# C. one-table form
ONE_TABLE_OPTIONS = {"group_partition": 2, "group_slab": 2, "group_dense": 0}
ONE_TABLE_KINDS = ("full", "one_past_full", "three_tiles")


def one_table_case(kind, resident):
    """C. ONE LDS table of C_FULL entries per aggregation workgroup, fed from the columns (resident: tiles of 2048 rows, one workgroup
    each) or from records.  The records come from the VM scatter, whose tiles (512, 1024 or 2048 rows) may be smaller than C_FULL rows,
    one aggregation workgroup per tile: grid_limit = 1 gives the records of `full` and `one_past_full` to ONE workgroup, whatever the tile."""
    options = dict(ONE_TABLE_OPTIONS, group_resident=resident)
    if not resident and kind != "three_tiles":
        options["grid_limit"] = 1
    shape = 3 if resident else 2
    if kind == "full":                                                    # one tile, one row per group: the table is exactly full
        g, facts = np.arange(C_FULL), {"group_shape": [shape, shape], "reruns": [0, 0]}
    elif kind == "one_past_full":                                         # one group more: on to the hash partitions, for good
        g, facts = np.arange(C_FULL + 1), {"group_shape": [1, 1], "reruns": [">=1", 0]}
    else:                                                                 # C_FULL + 1 groups, no tile with more than C_FULL - 100 of them
        i, width = np.arange(TILE), C_FULL - 100
        g = np.concatenate([i % width, 101 + i % width, 50 + i % width])
        facts = {"group_shape": [shape, shape], "reruns": [0, 0]}
    return GroupCase("one-table-%s-resident%d" % (kind, resident), _i32_pair(g, 40), "WIDE", options, facts, group_ids=g)


# D. dense slots
DENSE_OPTIONS = {"group_dense": 1, "dense_min_rows": 1}
DENSE_ROWS_AT_MAX = 4 * DENSE_MAX_SLOTS                                  # the fewest rows for which 2^21 slots pass the rows / 4 bound
DENSE_PARTITION_ROWS = (TILE - 1, TILE, TILE + 1, 8 * TILE, 8 * TILE + 1)


def _dense_facts(case_keys, rows, spec, options):
    spans = []
    for _t, d, z in case_keys:
        live = np.asarray(d)[~np.asarray(z, dtype=bool)] if z is not None else np.asarray(d)
        spans.append(int(live.max()) - int(live.min()) + 1 if len(live) else 0)
    usable, slots, resident, parts, cap = dense_geometry(spans, [z is not None for _t, _d, z in case_keys], rows, *acc_words(spec), options=options)
    return usable, slots, resident, parts, cap


def dense_case(name, keys, spec, options, keep=None, **facts):
    """A dense-slot case: dense_slots (and group_shape, when the slots are usable) as dense_geometry gives them."""
    options = dict(DENSE_OPTIONS, **options)
    rows = len(keys[0][1])
    usable, slots, resident, parts, cap = _dense_facts(keys, rows, spec, options)
    expect = {"dense_slots": slots if usable else 0}
    if usable:
        expect["group_shape"] = 3 if resident else 1
    expect.update(facts)
    return GroupCase("dense-" + name, keys, spec, options, expect, keep, geometry=(usable, slots, resident, parts, cap))


def dense_table_edge_case(D):
    """D1. WIDE, one INT32 key 0 .. D - 1 on 4 D + 3 rows: D = C_FULL is one table, C_FULL + 1 partitions."""
    rows = 4 * D + 3
    return dense_case("wide-%d-slots" % D, [("INT32", (np.arange(rows) % D).astype(np.int32), None)], "WIDE", {}, reruns=[0, 0])


def dense_rows_bound_case(rows, D=5000):
    """D2. SMALL, 5000 slots: usable from 20 000 rows (slots <= rows / 4)."""
    return dense_case("small-%d-slots-%d-rows" % (D, rows), [("INT32", (np.arange(rows) % D).astype(np.int32), None)], "SMALL", {})


DENSE_MAX_KINDS = ("one_key_at_max", "one_key_past_max", "two_keys_at_max", "two_keys_past_max")


def dense_max_slots_case(kind):
    """D3. SMALL over 8 388 608 rows whose keys take only the corner values of ranges spanning 2^21 slots, or one value more.  A Filter
    keeps 64 rows of each corner: all rows bound the ranges (the key ranges are taken ahead of the Filter), while the few kept ones
    cannot fill a partition's segments -- millions of rows on two slots would send the stage back to the hashed shapes."""
    rows = DENSE_ROWS_AT_MAX
    i = np.arange(rows)
    if kind.startswith("one_key"):
        top = DENSE_MAX_SLOTS - 1 if kind == "one_key_at_max" else DENSE_MAX_SLOTS
        keys = [("INT32", np.where(i % 2 == 0, 0, top).astype(np.int32), None)]
        corner = i % 2
    else:
        wide = 2048 if kind == "two_keys_at_max" else 2049
        keys = [("INT32", np.where(i % 2 == 0, 0, wide - 1).astype(np.int32), None), ("INT32", np.where((i // 2) % 2 == 0, 0, 1023).astype(np.int32), None)]
        corner = i % 4
    keep = i < 64 * (int(corner.max()) + 1)
    case = dense_case(kind, keys, "SMALL", {}, keep)
    case.notes["corners"] = int(corner.max()) + 1
    return case


def dense_span_edge_case(kind, partitioned):
    """D4. SMALL.  span_edges: a nullable key with its lowest value, its highest value and NULL only; all_null / all_null_and_ordinary:
    a nullable key that is NULL on every row (a span of one offset), alone and in front of an ordinary BOOL key (a NULLABLE INT32 leaves
    31 bits of the packed word)."""
    rows = 3000
    i = np.arange(rows)
    options = {"dense_parts": 7, "group_resident": 0} if partitioned else {}
    if kind == "span_edges":
        keys = [("INT32", np.where(i % 3 == 0, -7, 1000).astype(np.int32), i % 3 == 2)]
    elif kind == "all_null":
        keys = [("INT32", (i % 5).astype(np.int32), np.ones(rows, bool))]
    else:
        keys = [("INT32", (i % 5).astype(np.int32), np.ones(rows, bool)), ("BOOL", i % 2 == 1, None)]
    return dense_case("%s-%s" % (kind, "parts7" if partitioned else "one-table"), keys, "SMALL", options)


def dense_partition_corner_case(parts):
    """D4. The first and last entry of the first and last partition: slots = parts x cap, keys on the indices 0, (cap - 1) parts,
    parts - 1 and parts cap - 1 only (index % parts is the partition, index / parts the entry); a Filter keeps 50 rows of each."""
    cap = {7: 100, 256: 64}[parts]
    rows = {7: 3000, 256: 4 * parts * cap}[parts]
    corners = np.array([0, (cap - 1) * parts, parts - 1, parts * cap - 1])
    i = np.arange(rows)
    case = dense_case("corners-of-%d-partitions" % parts, [("INT32", corners[i % 4].astype(np.int32), None)], "SMALL", {"dense_parts": parts, "group_resident": 0},
                      i < 200, reruns=[0, 0])
    case.notes.update(parts=parts, cap=cap, corners=corners)
    return case


def dense_partitioned_rows_case(rows):
    """D5. 700 slots in 7 partitions over one to nine scatter tiles (one to eight XCD segment sets)."""
    return dense_case("parts7-%d-rows" % rows, [("INT32", (np.arange(rows) % 700).astype(np.int32), None)], "SMALL", {"dense_parts": 7, "group_resident": 0})


# E. heavy hitters
HOT_ROWS = 1 << 18
HOT_OPTIONS = {"group_partition": 2, "group_dense": 0}
HOT_PARTS = 256                                                          # run_group_agg_partitioned's default without an estimate
HOT_KINDS = ("32_keys", "33_equal_keys", "33_falling_keys", "all_ones_half")
COLD_GROUPS = 5000


def hot_case(kind):
    """E. 262 144 rows (the sample is every row), two INT32 keys, WIDE: hot keys (1000 + h, 7) with the counts of `kind`, the other rows
    dealt over 5000 cold groups (c // 100, c % 100), all in random order."""
    rng = np.random.default_rng(HOT_KINDS.index(kind) + 500)
    counts = {"32_keys": [5243] * 32, "33_equal_keys": [5243] * 33, "33_falling_keys": [6000 - 60 * h for h in range(33)], "all_ones_half": []}[kind]
    k0 = np.concatenate([np.full(c, 1000 + h, dtype=np.int32) for h, c in enumerate(counts)] + [np.zeros(0, np.int32)])
    k1 = np.full(len(k0), 7, dtype=np.int32)
    if kind == "all_ones_half":
        k0 = k1 = np.full(HOT_ROWS // 2, -1, dtype=np.int32)
    cold = np.arange(HOT_ROWS - len(k0)) % COLD_GROUPS
    order = rng.permutation(HOT_ROWS)
    k0, k1 = np.concatenate([k0, (cold // 100).astype(np.int32)])[order], np.concatenate([k1, (cold % 100).astype(np.int32)])[order]
    hot = hot_keys_reported(np.array(counts + [-(-len(cold) // COLD_GROUPS)]), hot_min_count(HOT_ROWS, HOT_PARTS))
    facts = {"hot_keys": hot, "plain_scatter": 1}
    if kind == "32_keys":
        facts.update(group_shape=1, part_seg_growth=1, reruns=[1, 0])
    return GroupCase("hot-" + kind, [("INT32", k0, None), ("INT32", k1, None)], "WIDE", HOT_OPTIONS, facts, counts=counts)
