"""ForeignFilter and RowidMergeJoin on the device, against the numpy model (structured_filter_reference, itself pinned on the
reference's vectors by tests/test_structured_filter_cpu.py): same rows, same order, bit for bit.

ForeignFilter is VM_JOIN_SEARCH -- a lower bound over the filter's sorted key column whose trip count depends on the table's row
count alone -- plus the match filter and the compaction of a materialising stage; RowidMergeJoin is VM_JOIN_ROWID, a range check on
the 64-bit key in front of the HashJoin's gathers (supersonic_amd/csrc/vm_body.inc).  The sizes here sit where those change shape:
table sizes around the powers of two of the halving, input sizes around the tile (VM_TILE_UNIT rows, vm.h; a stage may pick tiles of
up to four units) and past three tiles, so that kept rows cross tile and workgroup borders."""
import os
import re

import numpy as np
import pytest

import structured_filter_reference as sfr
import supersonic_amd as ss

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
I64_MIN, I64_MAX = np.iinfo(np.int64).min, np.iinfo(np.int64).max
GOLDEN = sfr.golden()


def vm_tile_unit():
    with open(os.path.join(ROOT, "supersonic_amd", "csrc", "vm.h")) as f:
        text = f.read()
    threads = int(re.search(r"#define VM_THREADS (\d+)", text).group(1))
    assert re.search(r"#define VM_TILE_UNIT \(2 \* VM_THREADS\)", text)
    return 2 * threads


U = vm_tile_unit()
INPUT_SIZES = [0, 1, U - 1, U, U + 1, 3 * U + 1, 12 * U + 1]      # (12 U + 1: three tiles and a row of the largest tile, 4 units)
TABLE_SIZES = [0, 1, 2, 3, 63, 64, 65, 4095, 4096, 4097]


def bits_of(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize])       # floats as integers


def assert_result(got, want, context):
    """Every column of the fetched View `got` against `want` ([(data, nulls or None), ...]): the same rows in the same order, NULL
    masks exactly (and exactly the columns that should have one), data bit for bit wherever the expected row is not NULL."""
    assert got.column_count() == len(want), (context, got.column_count(), len(want))
    for i, (wd, wz) in enumerate(want):
        where = "%s, column %d (%s)" % (context, i, got.schema().attribute(i).name())
        gd, gz = got.column(i).data, got.column(i).is_null
        assert len(gd) == len(wd) == got.row_count(), "%s: %d rows, expected %d" % (where, len(gd), len(wd))
        assert (gz is None) == (wz is None), "%s: NULL mask %s" % (where, "missing" if gz is None else "unexpected")
        live = np.ones(len(wd), bool)
        if wz is not None:
            bad = np.nonzero(gz != wz)[0]
            assert len(bad) == 0, "%s: NULL masks differ in %d rows, first at %s" % (where, len(bad), bad[:8])
            live = ~wz
        if wd.dtype == object:
            g, w = gd[live], wd[live]
        else:
            g, w = bits_of(gd)[live], bits_of(wd)[live]
            assert g.dtype == w.dtype, (where, gd.dtype, wd.dtype)
        bad = np.nonzero(g != w)[0]
        assert len(bad) == 0, "%s: %d rows differ, first at %s: got %s want %s" % (where, len(bad), np.flatnonzero(live)[bad[:8]], g[bad[:8]], w[bad[:8]])


def run_twice(plan, want, context):
    for run in range(2):
        plan.run()
        assert_result(plan.fetch(), want, "%s, run %d" % (context, run))


def run_fails(plan, code, text=None):
    for _run in range(2):
        with pytest.raises(ss.SupersonicException) as e:
            plan.run()
            plan.fetch()
        assert e.value.return_code == code, e.value
        if text is not None:
            assert text in str(e.value), e.value


# ---- tables ------------------------------------------------------------------------------------------------------------------------
NANS = np.array([0x7FF8000000000000, 0x7FF8000000000001, 0xFFF8000000000000, 0x7FF0000000000001, 0xFFFFFFFFFFFFFFFF], dtype=np.uint64).view(np.float64)
CHILD_TYPES = ["INT32", "INT64", "INT64", "DOUBLE", "STRING"]
CHILD_NAMES = ["i32", "fk", "i64", "d", "s"]
FK = 1
PARENT_TYPES = ["INT64", "DOUBLE", "STRING", "INT32"]
PARENT_NAMES = ["ri", "rd", "rs", "rn"]


def child_table(keys, seed=0):
    """i32 INT32 NULLABLE, fk INT64 (the key), i64 INT64 NULLABLE, d DOUBLE NULLABLE with NaNs of several bit patterns, s STRING."""
    keys = np.ascontiguousarray(keys, dtype=np.int64)
    n = len(keys)
    rng = np.random.default_rng(1000 + seed + n)
    d = rng.integers(-8, 8, n) * 0.125
    d[rng.random(n) < 0.2] = -0.0
    at = np.flatnonzero(rng.random(n) < 0.2)
    d[at] = NANS[at % len(NANS)]
    s = np.empty(n, dtype=object)
    s[:] = [b"row%d" % (i % 37) for i in range(n)]
    return [(rng.integers(-2**31, 2**31, n).astype(np.int32), rng.random(n) < 0.25), (keys, None),
            (rng.integers(I64_MIN, I64_MAX, n, dtype=np.int64), rng.random(n) < 0.25), (d, rng.random(n) < 0.25), (s, None)]


def parent_table(m, seed=0):
    """ri INT64, rd DOUBLE NULLABLE (NULLs and NaNs), rs STRING, rn INT32 NULLABLE without a single NULL."""
    rng = np.random.default_rng(2000 + seed + m)
    d = rng.integers(-100, 100, m) * 0.25
    at = np.flatnonzero(rng.random(m) < 0.2)
    d[at] = NANS[at % len(NANS)]
    s = np.empty(m, dtype=object)
    s[:] = [b"p%d" % (i % 53) for i in range(m)]
    return [(np.arange(m, dtype=np.int64) * 3 + 1, None), (d, rng.random(m) < 0.3), (s, None), (rng.integers(-5, 5, m).astype(np.int32), np.zeros(m, bool))]


RMJ_PROJECTOR = [(0, 0), (0, 3), (0, 4), (1, 0), (1, 1), (1, 2), (1, 3)]


def rmj_op(left_op, right_view):
    proj = ss.CompoundMultiSourceProjector().add(0, ss.ProjectNamedAttributes(["i32", "d", "s"])).add(1, ss.ProjectAllAttributes())
    return ss.RowidMergeJoin(ss.ProjectNamedAttribute("fk"), proj, left_op, ss.ScanView(right_view))


def ff_op(filter_view, input_op):
    return ss.ForeignFilter(ss.ProjectNamedAttribute("id"), ss.ProjectNamedAttribute("fk"), ss.ScanView(filter_view), input_op)


def filter_view(keys):
    """w DOUBLE, id INT64: the key is not the first column."""
    keys = np.ascontiguousarray(keys, dtype=np.int64)
    return sfr.view(["DOUBLE", "INT64"], [(np.arange(len(keys)) * 0.5, None), (keys, None)], ["w", "id"])


def filter_keys(m, seed=0):
    """m strictly ascending keys with gaps between them; from four keys on INT64 min, -1, 0 and INT64 max are among them."""
    rng = np.random.default_rng(3000 + seed + m)
    forced = [I64_MIN, -1, 0, I64_MAX][:m] if m < 4 else [I64_MIN, -1, 0, I64_MAX]
    keys = set(forced)
    while len(keys) < m:
        keys.update((rng.integers(-2**40, 2**40, m - len(keys) + 8) * 4).tolist())      # multiples of 4: key +- 1 is never a key
    extra = sorted(keys - set(forced))[:m - len(forced)]
    return np.array(sorted(set(forced) | set(extra)), dtype=np.int64)


def probing_keys(fkeys, n, seed=0):
    """n input keys around the table: every key itself (the edge keys too), its neighbours +-1 (between two keys, below the first,
    above the last), runs of equal keys, far misses -- shuffled, so the input is not ascending."""
    rng = np.random.default_rng(4000 + seed + n + len(fkeys))
    edges = [I64_MIN, I64_MIN + 1, -2, -1, 0, 1, 2, I64_MAX - 1, I64_MAX, 1 << 32, -(1 << 32)]
    if len(fkeys):
        edges += [fkeys[0], fkeys[-1]]
    always = np.array(edges, dtype=np.int64)[:n]          # (the edge keys are in every input that has room for them)
    pool = [always]
    if len(fkeys):
        pool += [fkeys, fkeys[fkeys < I64_MAX] + 1, fkeys[fkeys > I64_MIN] - 1, np.repeat(fkeys[:: max(1, len(fkeys) // 16)], 5)]
    pool = np.concatenate(pool)
    keys = np.concatenate([always, pool[rng.integers(0, len(pool), n - len(always))]]) if n else always
    return keys[rng.permutation(n)]


# ---- a. the reference's own vectors --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", GOLDEN["foreign_filter"], ids=[c["name"] for c in GOLDEN["foreign_filter"]])
def test_reference_foreign_filter_vector(gpu_ctx, case):
    filt, inp = sfr.table(case["filter_types"], case["filter"]), sfr.table(case["input_types"], case["input"])
    want = sfr.table(case["input_types"], case["expected"])
    assert sfr.same_table(sfr.foreign_filter(filt[case["filter_key"]][0], inp, case["foreign_key"]), want)
    plan = ss.Plan(sfr.foreign_filter_op(case, sfr.view(case["filter_types"], filt), sfr.view(case["input_types"], inp)), gpu_ctx)
    run_twice(plan, want, case["name"])


@pytest.mark.parametrize("case", GOLDEN["rowid_merge_join"], ids=[c["name"] for c in GOLDEN["rowid_merge_join"]])
def test_reference_rowid_merge_join_vector(gpu_ctx, case):
    left, right = sfr.table(case["left_types"], case["left"]), sfr.table(case["right_types"], case["right"])
    plan = ss.Plan(sfr.rowid_merge_join_op(case, sfr.view(case["left_types"], left), sfr.view(case["right_types"], right)), gpu_ctx)
    if "expected_error" in case:
        run_fails(plan, case["expected_error"], "No parent record with ID > %d" % len(case["right"]))
        return
    want = sfr.rowid_merge_join(left, case["left_key"], right, [(s, p) for s, p, _n in case["projector"]])
    golden = sfr.table(case["expected_types"], case["expected"])
    for (wd, wz), (gd, gz) in zip(want, golden):        # the model's rows are the golden rows (its NULL masks: wherever the source is NULLABLE)
        assert list(wd[~wz] if wz is not None else wd) == list(gd[~gz] if gz is not None else gd)
    run_twice(plan, want, case["name"])


# ---- b. ForeignFilter: the search ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m", TABLE_SIZES)
def test_search_table_sizes_and_edge_keys(gpu_ctx, m):
    fkeys = filter_keys(m)
    assert len(fkeys) == m and sfr.strictly_ascending(fkeys)
    child = child_table(probing_keys(fkeys, 3 * U + 1 if m > 64 else 700))
    want = sfr.foreign_filter(fkeys, child, FK)
    if m >= 4:
        hit = set(fkeys[want[FK][0]].tolist())
        assert {I64_MIN, -1, 0, I64_MAX} <= hit and 0 < len(want[FK][0]) < len(child[FK][0])
        assert not sfr.strictly_ascending(child[FK][0])
    plan = ss.Plan(ff_op(filter_view(fkeys), ss.ScanView(sfr.view(CHILD_TYPES, child, CHILD_NAMES))), gpu_ctx)
    run_twice(plan, want, "%d filter keys" % m)


def test_search_compares_signed(gpu_ctx):
    # as unsigned values -1 and INT64 min sort behind INT64 max: a search with unsigned compares misses them
    fkeys = np.array([I64_MIN, -1, 0, I64_MAX], dtype=np.int64)
    keys = np.array([I64_MAX, 0, -1, I64_MIN, I64_MIN + 1, -2, 1, I64_MAX - 1, -1, I64_MIN], dtype=np.int64)
    child = child_table(keys)
    want = sfr.foreign_filter(fkeys, child, FK)
    assert list(want[FK][0]) == [3, 2, 1, 0, 1, 0]
    run_twice(ss.Plan(ff_op(filter_view(fkeys), ss.ScanView(sfr.view(CHILD_TYPES, child, CHILD_NAMES))), gpu_ctx), want, "signed")


@pytest.mark.parametrize("m", [1, 2, 5, 64, 65, 4097])
def test_keys_below_the_first_and_above_the_last(gpu_ctx, m):
    # filter_keys() always holds INT64 min (and max from four keys on), so nothing lies outside those tables: this one spans
    # [100, 100 + 10 (m - 1)] and is probed below it, above it, at both ends and on both sides of every key
    fkeys = 100 + 10 * np.arange(m, dtype=np.int64)
    first, last = int(fkeys[0]), int(fkeys[-1])
    around = np.concatenate([fkeys - 1, fkeys, fkeys + 1])
    outside = np.array([I64_MIN, -1, 0, 99, first - 10, last + 1, last + 10, 1 << 32, I64_MAX], dtype=np.int64)
    keys = np.concatenate([outside, [first, last], around[np.random.default_rng(m).permutation(len(around))][: 3 * U], outside[::-1]])
    child = child_table(keys)
    want = sfr.foreign_filter(fkeys, child, FK)
    below, above = int((keys < first).sum()), int((keys > last).sum())
    assert below >= 10 and above >= 8 and set(want[FK][0].tolist()) >= {0, m - 1}
    assert len(want[FK][0]) == int(np.isin(keys, fkeys).sum()) <= len(keys) - below - above
    run_twice(ss.Plan(ff_op(filter_view(fkeys), ss.ScanView(sfr.view(CHILD_TYPES, child, CHILD_NAMES))), gpu_ctx), want, "keys outside [%d, %d]" % (first, last))


@pytest.mark.parametrize("which", ["every_row_matches", "no_row_matches", "runs_of_equal_keys"])
def test_all_none_and_one_to_many(gpu_ctx, which):
    fkeys = filter_keys(65)
    rng = np.random.default_rng(7)
    n = 3 * U + 1
    if which == "every_row_matches":
        keys = fkeys[rng.integers(0, len(fkeys), n)]
    elif which == "no_row_matches":
        keys = fkeys[rng.integers(4, len(fkeys) - 4, n)] + 2          # between two keys: the keys are multiples of 4, -1 and 0
    else:
        keys = np.repeat(fkeys[rng.integers(0, len(fkeys), n // 7 + 1)], 7)[:n]        # ascending nowhere, equal keys in runs of 7
    child = child_table(keys)
    want = sfr.foreign_filter(fkeys, child, FK)
    assert len(want[FK][0]) == {"every_row_matches": n, "no_row_matches": 0, "runs_of_equal_keys": n}[which]
    run_twice(ss.Plan(ff_op(filter_view(fkeys), ss.ScanView(sfr.view(CHILD_TYPES, child, CHILD_NAMES))), gpu_ctx), want, which)


# ---- c. input sizes, both operators ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", INPUT_SIZES)
def test_foreign_filter_input_sizes(gpu_ctx, n):
    fkeys = filter_keys(300)
    child = child_table(probing_keys(fkeys, n, seed=1))
    assert len(child[FK][0]) == n
    want = sfr.foreign_filter(fkeys, child, FK)
    assert n < U - 1 or 0 < len(want[FK][0]) < n
    run_twice(ss.Plan(ff_op(filter_view(fkeys), ss.ScanView(sfr.view(CHILD_TYPES, child, CHILD_NAMES))), gpu_ctx), want, "%d input rows" % n)


@pytest.mark.parametrize("n", INPUT_SIZES)
def test_rowid_merge_join_input_sizes(gpu_ctx, n):
    m = 300
    rng = np.random.default_rng(n)
    keys = rng.integers(0, m, n)
    keys[: min(n, 2)] = [0, m - 1][: min(n, 2)]                    # the first and the last right row
    child, parent = child_table(keys), parent_table(m)
    want = sfr.rowid_merge_join(child, FK, parent, RMJ_PROJECTOR)
    plan = ss.Plan(rmj_op(ss.ScanView(sfr.view(CHILD_TYPES, child, CHILD_NAMES)), sfr.view(PARENT_TYPES, parent, PARENT_NAMES)), gpu_ctx)
    run_twice(plan, want, "%d left rows" % n)
    schema = plan.result_schema
    assert [schema.attribute(i).name() for i in range(7)] == ["i32", "d", "s", "ri", "rd", "rs", "rn"]
    assert [schema.attribute(i).is_nullable() for i in range(7)] == [True, True, False, False, True, False, True]       # rn: NULLABLE without a NULL


# ---- d. a filter table that is not strictly ascending ---------------------------------------------------------------------------------
@pytest.mark.parametrize("fault", ["duplicate", "descending_pair", "duplicate_at_the_end_of_4097"])
def test_an_unordered_filter_table_fails_the_run_and_a_good_one_rebinds(gpu_ctx, fault):
    good = filter_keys(4097 if fault.endswith("4097") else 300)
    bad = good.copy()
    if fault == "duplicate":
        bad[150] = bad[149]
    elif fault == "descending_pair":
        bad[[10, 11]] = bad[[11, 10]]
    else:
        bad[-1] = bad[-2]
    assert not sfr.strictly_ascending(bad)
    child = child_table(probing_keys(good, 700))
    plan = ss.Plan(ff_op(filter_view(bad), ss.ScanView(sfr.view(CHILD_TYPES, child, CHILD_NAMES))), gpu_ctx)
    run_fails(plan, ss.ERROR_INVALID_ARGUMENT_VALUE, "unique and ascending")
    plan.aux_input = filter_view(good)                 # the same plan, a correct table bound
    run_twice(plan, sfr.foreign_filter(good, child, FK), "rebound after %s" % fault)


# ---- e. RowidMergeJoin: the key range ----------------------------------------------------------------------------------------------------
def small_join(gpu_ctx, keys, m=3, below=None):
    child, parent = child_table(keys), parent_table(m)
    left = ss.ScanView(sfr.view(CHILD_TYPES, child, CHILD_NAMES))
    if below is not None:
        left = ss.Filter(below, ss.ProjectAllAttributes(), left)
    return ss.Plan(rmj_op(left, sfr.view(PARENT_TYPES, parent, PARENT_NAMES)), gpu_ctx), child, parent


def test_keys_zero_and_last_are_rows(gpu_ctx):
    plan, child, parent = small_join(gpu_ctx, [0, 2, 2, 0, 1])
    run_twice(plan, sfr.rowid_merge_join(child, FK, parent, RMJ_PROJECTOR), "0 and n - 1")


@pytest.mark.parametrize("bad", [3, -1, I64_MIN, 1 << 32, (1 << 32) + 1, I64_MAX], ids=["n", "minus_one", "int64_min", "two_to_32", "two_to_32_plus_1", "int64_max"])
@pytest.mark.parametrize("n", [5, 3 * U + 1])
def test_a_key_outside_the_right_table_fails_the_run(gpu_ctx, n, bad):
    keys = np.arange(n, dtype=np.int64) % 3
    keys[n - 2] = bad                                   # 2^32 narrows to row 0, 2^32 + 1 to row 1: the compare is on the 64-bit value
    plan, _child, _parent = small_join(gpu_ctx, keys)
    run_fails(plan, ss.ERROR_FOREIGN_KEY_INVALID, "No parent record with ID > 3")
    assert ss.ERROR_FOREIGN_KEY_INVALID == 501


def test_an_empty_right_table(gpu_ctx):
    plan, child, parent = small_join(gpu_ctx, [], m=0)
    run_twice(plan, sfr.rowid_merge_join(child, FK, parent, RMJ_PROJECTOR), "0 left rows, 0 right rows")
    plan, _child, _parent = small_join(gpu_ctx, [0], m=0)
    run_fails(plan, ss.ERROR_FOREIGN_KEY_INVALID, "No parent record with ID > 0")


@pytest.mark.parametrize("bad", [3, -1, 1 << 32], ids=["n", "minus_one", "two_to_32"])
def test_a_row_the_filter_below_drops_is_not_checked(gpu_ctx, bad):
    n = 3 * U + 1
    keys = np.arange(n, dtype=np.int64) % 3
    keys[[7, n - 2]] = bad
    below = ss.And(ss.Less(ss.ConstInt64(-1), ss.NamedAttribute("fk")), ss.Less(ss.NamedAttribute("fk"), ss.ConstInt64(3)))
    plan, child, parent = small_join(gpu_ctx, keys, below=below)
    selected = (child[FK][0] > -1) & (child[FK][0] < 3)
    assert selected.sum() == n - 2
    run_twice(plan, sfr.rowid_merge_join(child, FK, parent, RMJ_PROJECTOR, selected=selected), "offending rows dropped below")
    # a Filter ABOVE the join does not excuse them: the join sees every row
    above = ss.Filter(ss.Less(ss.NamedAttribute("ri"), ss.ConstInt64(0)), ss.ProjectAllAttributes(),
                      rmj_op(ss.ScanView(sfr.view(CHILD_TYPES, child, CHILD_NAMES)), sfr.view(PARENT_TYPES, parent, PARENT_NAMES)))
    run_fails(ss.Plan(above, gpu_ctx), ss.ERROR_FOREIGN_KEY_INVALID)
    # ... nor does one that reads LEFT columns only and drops every row: nothing of the join is read by the count pass or by the
    # predicate, so the check is the one the store pass emits on the join's own account
    proj = ss.CompoundMultiSourceProjector().add(0, ss.ProjectNamedAttributes(["i32", "fk", "s"]))
    left_only = ss.RowidMergeJoin(ss.ProjectNamedAttribute("fk"), proj, ss.ScanView(sfr.view(CHILD_TYPES, child, CHILD_NAMES)), ss.ScanView(sfr.view(PARENT_TYPES, parent, PARENT_NAMES)))
    none_left = ss.Filter(ss.Less(ss.NamedAttribute("fk"), ss.ConstInt64(I64_MIN)), ss.ProjectAllAttributes(), left_only)
    run_fails(ss.Plan(none_left, gpu_ctx), ss.ERROR_FOREIGN_KEY_INVALID, "No parent record with ID > 3")
    # (the same plan over keys that are all rows of the table: green, and empty)
    good = child_table(np.arange(n, dtype=np.int64) % 3)
    ok = ss.Filter(ss.Less(ss.NamedAttribute("fk"), ss.ConstInt64(I64_MIN)), ss.ProjectAllAttributes(),
                   ss.RowidMergeJoin(ss.ProjectNamedAttribute("fk"), proj, ss.ScanView(sfr.view(CHILD_TYPES, good, CHILD_NAMES)), ss.ScanView(sfr.view(PARENT_TYPES, parent, PARENT_NAMES))))
    run_twice(ss.Plan(ok, gpu_ctx), [sfr.take(good[c], np.zeros(0, int)) for c in (0, 1, 4)], "a left-column Filter above drops every row")


def test_a_key_is_checked_even_when_no_right_column_is_kept(gpu_ctx):
    child, parent = child_table([0, 1, 5, 2]), parent_table(3)
    proj = ss.CompoundMultiSourceProjector().add(0, ss.ProjectNamedAttributes(["i32", "s"]))
    op = ss.RowidMergeJoin(ss.ProjectNamedAttribute("fk"), proj, ss.ScanView(sfr.view(CHILD_TYPES, child, CHILD_NAMES)), ss.ScanView(sfr.view(PARENT_TYPES, parent, PARENT_NAMES)))
    run_fails(ss.Plan(op, gpu_ctx), ss.ERROR_FOREIGN_KEY_INVALID, "No parent record with ID > 3")
    spec = ss.AggregationSpecification().AddAggregation(ss.COUNT, "", "n")
    run_fails(ss.Plan(ss.ScalarAggregate(spec, op), gpu_ctx), ss.ERROR_FOREIGN_KEY_INVALID)


# ---- f. fusion -----------------------------------------------------------------------------------------------------------------------
def test_scalar_aggregate_over_foreign_filter_over_filter(gpu_ctx):
    fkeys = filter_keys(4097)
    child = child_table(probing_keys(fkeys, 12 * U + 1, seed=2))
    below = ss.Less(ss.NamedAttribute("fk"), ss.ConstInt64(0))
    spec = (ss.AggregationSpecification().AddAggregation(ss.COUNT, "", "n").AddAggregation(ss.SUM, "fk", "sum_fk").AddAggregation(ss.COUNT, "i32", "n_i32"))
    op = ss.ScalarAggregate(spec, ff_op(filter_view(fkeys), ss.Filter(below, ss.ProjectAllAttributes(), ss.ScanView(sfr.view(CHILD_TYPES, child, CHILD_NAMES)))))
    plan = ss.Plan(op, gpu_ctx)
    assert len(plan.stage_info()) == 1                  # Filter, search, match filter and the aggregate: one pipeline
    selected = child[FK][0] < 0
    kept = sfr.foreign_filter(fkeys, [sfr.take(c, np.flatnonzero(selected)) for c in child], FK)
    want = [(np.array([len(kept[FK][0])], dtype=np.uint64), None), (np.array([kept[FK][0].sum()], dtype=np.int64), np.array([False])),
            (np.array([int((~kept[0][1]).sum())], dtype=np.uint64), None)]
    assert want[0][0][0] > 0
    run_twice(plan, want, "ScalarAggregate over ForeignFilter over Filter")


def test_group_aggregate_keyed_by_a_gathered_column(gpu_ctx):
    m, n = 300, 12 * U + 1
    rng = np.random.default_rng(11)
    child, parent = child_table(rng.integers(0, m, n)), parent_table(m)
    spec = ss.AggregationSpecification().AddAggregation(ss.COUNT, "", "n").AddAggregation(ss.SUM, "i32", "sum_i32")
    op = ss.GroupAggregate(ss.ProjectNamedAttributes(["rs"]), spec, None,
                           rmj_op(ss.ScanView(sfr.view(CHILD_TYPES, child, CHILD_NAMES)), sfr.view(PARENT_TYPES, parent, PARENT_NAMES)))
    plan = ss.Plan(op, gpu_ctx)
    joined = sfr.rowid_merge_join(child, FK, parent, RMJ_PROJECTOR)
    rs, (i32, i32_null) = joined[5][0], joined[0]
    expected = {}
    for g, v, z in zip(rs.tolist(), i32.tolist(), i32_null.tolist()):
        e = expected.setdefault(g, [0, 0, 0])
        e[0] += 1
        if not z:
            e[1] += v
            e[2] += 1
    for run in range(2):
        plan.run()
        got = plan.fetch()
        rows = {g: (int(c), None if sz else int(s)) for g, c, s, sz in zip(got.column(0).data.tolist(), got.column(1).data.tolist(), got.column(2).data.tolist(), got.column(2).is_null.tolist())}
        assert got.row_count() == len(expected) == len(rows) == 53
        assert got.column(2).data.dtype == np.int32                        # SUM keeps the input's type: the sum wraps like the reference's int32 +=
        assert rows == {g: (e[0], (e[1] + 2**31) % 2**32 - 2**31 if e[2] else None) for g, e in expected.items()}, run


def test_sort_over_foreign_filter(gpu_ctx):
    fkeys = filter_keys(300)
    child = child_table(probing_keys(fkeys, 3 * U + 1, seed=3))
    child[2] = (np.random.default_rng(5).permutation(len(child[2][0])).astype(np.int64), None)       # i64: a unique sort key
    view = sfr.view(CHILD_TYPES, child, CHILD_NAMES)
    op = ss.Sort(ss.SortOrder().add("i64", ss.ASCENDING), None, 0, ff_op(filter_view(fkeys), ss.ScanView(view)))
    kept = sfr.foreign_filter(fkeys, child, FK)
    order = np.argsort(kept[2][0], kind="stable")
    run_twice(ss.Plan(op, gpu_ctx), [sfr.take(c, order) for c in kept], "Sort over ForeignFilter")


def test_the_structured_filter_chain_as_two_plans(gpu_ctx):
    # parents filtered on the host side of the test; the children keep the rows of surviving parents, renumbered (plan 1), and
    # fetch their parent's columns by the new key (plan 2 scans plan 1's device result)
    m, n = 4097, 12 * U + 1
    rng = np.random.default_rng(13)
    parent = parent_table(m)
    surviving = np.flatnonzero(rng.random(m) < 0.5).astype(np.int64)
    filtered_parent = [sfr.take(c, surviving) for c in parent]
    types, names = ["INT32", "INT64", "INT64", "DOUBLE"], ["i32", "fk", "i64", "d"]
    child = child_table(rng.integers(0, m, n))[:4]                    # numeric columns: a device result carries no dictionary
    first = ss.Plan(ss.ForeignFilter(ss.ProjectNamedAttribute("id"), ss.ProjectNamedAttribute("fk"), ss.ScanView(filter_view(surviving)),
                                     ss.ScanView(sfr.view(types, child, names))), gpu_ctx)
    kept = sfr.foreign_filter(surviving, child, FK)
    proj = ss.CompoundMultiSourceProjector().add(0, ss.ProjectNamedAttributes(["i32", "d"])).add(1, ss.ProjectAllAttributes())
    want = sfr.rowid_merge_join(kept, FK, filtered_parent, [(0, 0), (0, 3), (1, 0), (1, 1), (1, 2), (1, 3)])
    for run in range(2):
        first.run()
        mid = first.result_device_view()
        assert mid.row_count() == len(kept[FK][0]) > 0
        second = ss.Plan(ss.RowidMergeJoin(ss.ProjectNamedAttribute("fk"), proj, ss.ScanView(mid), ss.ScanView(sfr.view(PARENT_TYPES, filtered_parent, PARENT_NAMES))), gpu_ctx)
        second.run()
        assert_result(second.fetch(), want, "chain, run %d" % run)
    assert np.array_equal(want[2][0], parent[0][0][child[FK][0][np.isin(child[FK][0], surviving)]])      # ri of the ORIGINAL parent row


# ---- g. the compiled kernels and chunked staging -------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def specialising_ctx():
    ctx = ss.Context(0)
    ctx.set_option("specialize", 1)
    return ctx


def test_foreign_filter_specialised(specialising_ctx):
    fkeys = filter_keys(4097)
    child = child_table(probing_keys(fkeys, 12 * U + 1, seed=4))
    plan = ss.Plan(ff_op(filter_view(fkeys), ss.ScanView(sfr.view(CHILD_TYPES, child, CHILD_NAMES))), specialising_ctx)
    run_twice(plan, sfr.foreign_filter(fkeys, child, FK), "ForeignFilter, compiled kernel")
    assert plan.specialized() >= 1, plan.specialize_reason()


def test_rowid_merge_join_specialised(specialising_ctx):
    m, n = 300, 12 * U + 1
    child, parent = child_table(np.random.default_rng(17).integers(0, m, n)), parent_table(m)
    plan = ss.Plan(rmj_op(ss.ScanView(sfr.view(CHILD_TYPES, child, CHILD_NAMES)), sfr.view(PARENT_TYPES, parent, PARENT_NAMES)), specialising_ctx)
    run_twice(plan, sfr.rowid_merge_join(child, FK, parent, RMJ_PROJECTOR), "RowidMergeJoin, compiled kernel")
    assert plan.specialized() >= 1, plan.specialize_reason()
    child[FK][0][n - 3] = 1 << 32
    bad = ss.Plan(rmj_op(ss.ScanView(sfr.view(CHILD_TYPES, child, CHILD_NAMES)), sfr.view(PARENT_TYPES, parent, PARENT_NAMES)), specialising_ctx)
    run_fails(bad, ss.ERROR_FOREIGN_KEY_INVALID, "No parent record with ID > 300")


def test_foreign_filter_through_run_host(gpu_ctx):
    fkeys = filter_keys(300)
    child = child_table(probing_keys(fkeys, 12 * U + 1, seed=5))
    plan = ss.Plan(ff_op(filter_view(fkeys), ss.ScanView(sfr.view(CHILD_TYPES, child, CHILD_NAMES))), gpu_ctx)
    assert plan.chunked_form()[0] == 2
    for _run in range(2):
        plan.run_host(chunk_rows=1000)                 # seven chunks, none of them a whole number of tiles
        assert_result(plan.fetch(), sfr.foreign_filter(fkeys, child, FK), "ForeignFilter, chunked")


def test_rowid_merge_join_through_run_host(gpu_ctx):
    m, n = 300, 12 * U + 1
    child, parent = child_table(np.random.default_rng(19).integers(0, m, n)), parent_table(m)
    view = sfr.view(CHILD_TYPES, child, CHILD_NAMES)
    plan = ss.Plan(rmj_op(ss.ScanView(view), sfr.view(PARENT_TYPES, parent, PARENT_NAMES)), gpu_ctx)
    assert plan.chunked_form()[0] == 2
    for _run in range(2):
        plan.run_host(chunk_rows=1000)
        assert_result(plan.fetch(), sfr.rowid_merge_join(child, FK, parent, RMJ_PROJECTOR), "RowidMergeJoin, chunked")
    child[FK][0][n - 3] = m                             # in the last chunk: the run fails as a whole
    bad = ss.Plan(rmj_op(ss.ScanView(sfr.view(CHILD_TYPES, child, CHILD_NAMES)), sfr.view(PARENT_TYPES, parent, PARENT_NAMES)), gpu_ctx)
    with pytest.raises(ss.SupersonicException) as e:
        bad.run_host(chunk_rows=1000)
    assert e.value.return_code == ss.ERROR_FOREIGN_KEY_INVALID and "No parent record with ID > 300" in str(e.value)
