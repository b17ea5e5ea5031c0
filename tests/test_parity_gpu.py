"""GPU parity tests: the HIP path (through the C ABI) against the CPU oracle on the same
seeded inputs.  Bit-exact for integer / index / BOOL columns; DOUBLE data is chosen so that
every partial sum is exact, which makes DOUBLE aggregates bit-exact too.

Row counts follow the reference's block-size cross product idea
(supersonic/testing/operation_testing.cc:350-352), restated as launch-geometry / tile-boundary
cases: around one wave (64), one tile (512/1024/2048) and many tiles.
"""
import os

import numpy as np
import pytest

import supersonic_amd as ss
from helpers import run_both, to_cols, sort_rows, assert_cols_equal
from oracle import oracle as _oracle_mod


def oracle_run(op):
    return _oracle_mod.run(op)

pytestmark = pytest.mark.gpu

ROWS = [0, 1, 63, 64, 65, 511, 512, 513, 1023, 1024, 1025, 2047, 2048, 2049, 10001, 100003]
NA = ss.NamedAttribute


def make_view(n, seed=42, nullable=False):
    rng = np.random.default_rng(seed)
    N = ss.NULLABLE if nullable else ss.NOT_NULLABLE
    schema = ss.TupleSchema([ss.Attribute("a", ss.INT64, N), ss.Attribute("b", ss.INT64), ss.Attribute("c", ss.INT64),
                             ss.Attribute("d", ss.INT64, N), ss.Attribute("k1", ss.INT32, N), ss.Attribute("k2", ss.INT32),
                             ss.Attribute("d0", ss.DOUBLE, N), ss.Attribute("d1", ss.DOUBLE),
                             ss.Attribute("d2", ss.DOUBLE), ss.Attribute("d3", ss.DOUBLE),
                             ss.Attribute("u", ss.UINT32), ss.Attribute("f", ss.FLOAT), ss.Attribute("t", ss.BOOL, N)])
    g = rng.integers(0, 1000, n)

    def nl():
        return (rng.random(n) < 0.1) if nullable else None
    cols = [ss.Column(rng.integers(0, 1000, n), nl()), rng.integers(0, 1000, n), np.arange(n) % 100000,
            ss.Column(rng.integers(-(1 << 62), 1 << 62, n), nl()), ss.Column(g // 31, nl()), g % 31,
            ss.Column(rng.integers(-1000000, 1000001, n).astype(np.float64), nl()), rng.integers(0, 4000, n) * 0.25,
            rng.integers(0, 64, n).astype(np.float64), rng.integers(0, 64, n).astype(np.float64),
            rng.integers(0, 1 << 32, n).astype(np.uint32), (rng.integers(0, 64, n) * 0.5).astype(np.float32),
            ss.Column(rng.integers(0, 2, n).astype(bool), nl())]
    return ss.View(schema, cols)


def fpa_narrow(view):
    return ss.ScalarAggregate(
        ss.AggregationSpecification().AddAggregation(ss.SUM, "s", "sum_s").AddAggregation(ss.COUNT, "a", "cnt"),
        ss.Filter(ss.Greater(NA("a"), ss.ConstInt64(499)), ss.ProjectAllAttributes(),
                  ss.Compute(ss.CompoundExpression().Add(NA("a")).AddAs("s", ss.Plus(NA("a"), NA("b"))), ss.ScanView(view))))


def fpa_wide(view):
    compute = (ss.CompoundExpression().Add(NA("a")).AddAs("s", ss.Plus(NA("a"), NA("b"))).Add(NA("c")).Add(NA("d"))
               .Add(NA("d0")).Add(NA("d1")).AddAs("p", ss.Multiply(NA("d2"), NA("d3"))))
    spec = (ss.AggregationSpecification().AddAggregation(ss.SUM, "s", "sum_s").AddAggregation(ss.COUNT, "", "cnt")
            .AddAggregation(ss.SUM, "c", "sum_c").AddAggregation(ss.MIN, "d", "min_d").AddAggregation(ss.MAX, "d0", "max_d0")
            .AddAggregation(ss.SUM, "d1", "sum_d1").AddAggregation(ss.SUM, "p", "sum_p"))
    return ss.ScalarAggregate(spec, ss.Filter(ss.Greater(NA("a"), ss.ConstInt64(499)), ss.ProjectAllAttributes(),
                                              ss.Compute(compute, ss.ScanView(view))))


@pytest.mark.parametrize("n", ROWS)
def test_fpa_narrow(gpu_ctx, n):
    run_both(fpa_narrow(make_view(n)), gpu_ctx)


@pytest.mark.parametrize("n", ROWS)
def test_fpa_wide(gpu_ctx, n):
    run_both(fpa_wide(make_view(n)), gpu_ctx)


@pytest.mark.parametrize("n", [0, 1, 65, 1025, 100003])
def test_fpa_wide_nullable(gpu_ctx, n):
    run_both(fpa_wide(make_view(n, nullable=True)), gpu_ctx)


@pytest.mark.parametrize("tile", [512, 1024, 2048])
def test_fpa_tile_sizes(tile, n=100003):
    ctx = ss.Context(0)
    ctx.set_option("tile_rows", tile)
    run_both(fpa_wide(make_view(n)), ctx)
    run_both(fpa_narrow(make_view(n)), ctx)


def all_aggs(view):
    spec = ss.AggregationSpecification()
    for col in ["a", "d", "k1", "d0", "u", "f", "t"]:
        for agg, nm in [(ss.MIN, "min"), (ss.MAX, "max"), (ss.FIRST, "first"), (ss.LAST, "last")]:
            spec.AddAggregation(agg, col, "%s_%s" % (nm, col))
        if col != "t":
            spec.AddAggregation(ss.SUM, col, "sum_%s" % col)
        spec.AddAggregation(ss.COUNT, col, "cnt_%s" % col)
    spec.AddAggregationWithDefinedOutputType(ss.SUM, "k1", "sum_k1_64", ss.INT64)
    spec.AddAggregationWithDefinedOutputType(ss.SUM, "k1", "sum_k1_f64", ss.DOUBLE)
    spec.AddAggregationWithDefinedOutputType(ss.COUNT, "", "cnt32", ss.INT32)
    return ss.ScalarAggregate(spec, ss.ScanView(view))


@pytest.mark.parametrize("n", [0, 1, 64, 1000, 100003])
@pytest.mark.parametrize("nullable", [False, True])
def test_scalar_aggregate_matrix(gpu_ctx, n, nullable):
    run_both(all_aggs(make_view(n, nullable=nullable)), gpu_ctx)


def compute_exprs(view):
    e = (ss.CompoundExpression()
         .AddAs("sum", ss.Plus(NA("a"), NA("b")))
         .AddAs("mixed", ss.Plus(NA("a"), NA("k1")))            # INT64 + INT32 -> cast
         .AddAs("dbl", ss.Multiply(NA("d0"), NA("k2")))         # DOUBLE * INT32
         .AddAs("neg", ss.Negate(NA("u")))                      # UINT32 -> INT32
         .AddAs("div", ss.DivideNulling(NA("d1"), NA("k2")))
         .AddAs("cmp", ss.LessOrEqual(NA("k1"), NA("d")))       # INT32 vs INT64, no cast
         .AddAs("ucmp", ss.Less(NA("u"), NA("k2")))             # UINT32 vs INT32
         .AddAs("logic", ss.Or(ss.And(NA("t"), ss.Greater(NA("a"), ss.ConstInt64(300))), ss.Less(NA("f"), ss.ConstDouble(10.0))))
         .AddAs("isnull", ss.IsNull(NA("d0")))
         .AddAs("ifnull", ss.IfNull(NA("a"), NA("c")))
         .AddAs("iff", ss.If(NA("t"), NA("a"), NA("k1")))
         .AddAs("sub", ss.Minus(NA("f"), NA("u")))
         .AddAs("c5", ss.Plus(ss.ConstInt32(2), ss.ConstInt32(3)))
         .Add(NA("d")))
    return ss.Compute(e, ss.ScanView(view))


@pytest.mark.parametrize("n", [0, 1, 65, 513, 2049, 100003])
@pytest.mark.parametrize("nullable", [False, True])
def test_compute_materialize(gpu_ctx, n, nullable):
    run_both(compute_exprs(make_view(n, nullable=nullable)), gpu_ctx)


@pytest.mark.parametrize("n", ROWS + [1000003])
@pytest.mark.parametrize("k", [-1, 499, 989, 1000])   # all / half / 1% / none pass
def test_filter_materialize(gpu_ctx, n, k):
    op = ss.Filter(ss.Greater(NA("a"), ss.ConstInt64(k)), ss.ProjectAllAttributes(), ss.ScanView(make_view(n)))
    run_both(op, gpu_ctx)


@pytest.mark.parametrize("n", [0, 65, 1025, 100003])
def test_filter_nullable_predicate_and_project(gpu_ctx, n):
    view = make_view(n, nullable=True)
    pred = ss.And(ss.Greater(NA("a"), ss.ConstInt64(300)), NA("t"))
    op = ss.Filter(pred, ss.ProjectNamedAttributes(["d", "k1", "a", "d0"]), ss.ScanView(view))
    run_both(op, gpu_ctx)


@pytest.mark.parametrize("n", [0, 65, 1025, 100003])
def test_filter_nullable_and_computed_columns(gpu_ctx, n):
    view = make_view(n, nullable=True)
    pred = ss.And(ss.Greater(NA("a"), ss.ConstInt64(300)), NA("t"))
    run_both(ss.Filter(pred, ss.ProjectNamedAttributes(["d", "k1", "a", "d0", "t"]), ss.ScanView(view)), gpu_ctx)
    # 24 computed columns besides nullable and constant ones
    e = ss.CompoundExpression()
    for i in range(24):
        e.AddAs("x%d" % i, ss.Plus(NA("b"), ss.ConstInt64(i)))
    e.AddAs("h", ss.DivideNulling(NA("d0"), NA("d1"))).Add(NA("k1")).AddAs("five", ss.ConstInt32(5)).Add(NA("c"))
    run_both(ss.Filter(ss.Less(NA("c"), ss.ConstInt64(40000)), ss.ProjectAllAttributes(), ss.Compute(e, ss.ScanView(view))), gpu_ctx)


def test_filter_reuses_the_plan(gpu_ctx):
    # a second run over other data must not see the first run's tile counts
    views = [make_view(100003, seed=s) for s in (1, 2, 3)]
    op = ss.Filter(ss.Greater(NA("a"), ss.ConstInt64(499)), ss.ProjectAllAttributes(), ss.ScanView(views[0]))
    plan = ss.Plan(op, gpu_ctx)
    assert "SEL_COUNT" in plan.describe()
    for v in views:
        plan.run(v)
        got = plan.fetch()
        _, want = oracle_run(ss.Filter(ss.Greater(NA("a"), ss.ConstInt64(499)), ss.ProjectAllAttributes(), ss.ScanView(v)))
        assert_cols_equal(to_cols(got), want)


def group_query(view, with_filter, keys=("k1", "k2")):
    spec = ss.AggregationSpecification()
    for col in ["d0", "d1", "d2", "d3"]:
        spec.AddAggregation(ss.SUM, col, "sum_" + col).AddAggregation(ss.MIN, col, "min_" + col).AddAggregation(ss.MAX, col, "max_" + col)
    spec.AddAggregation(ss.COUNT, "", "n").AddAggregation(ss.SUM, "a", "sum_a").AddAggregation(ss.MAX, "k2", "max_k2")
    child = ss.ScanView(view)
    if with_filter:
        child = ss.Filter(ss.Greater(NA("b"), ss.ConstInt64(499)), ss.ProjectAllAttributes(), child)
    return ss.GroupAggregate(ss.ProjectNamedAttributes(list(keys)), spec, None, child)


@pytest.mark.parametrize("n", [0, 1, 65, 1025, 100003])
@pytest.mark.parametrize("with_filter", [False, True])
@pytest.mark.parametrize("nullable", [False, True])
def test_group_aggregate(gpu_ctx, n, with_filter, nullable):
    # one packed 64-bit key word here (a NULLABLE INT32 key takes 33 bits); wider keys: test_group_aggregate_wide_keys
    keys = ("k1",) if nullable else ("k1", "k2")
    run_both(group_query(make_view(n, nullable=nullable), with_filter, keys), gpu_ctx, ignore_order=True)


@pytest.mark.parametrize("part_plain", [1, 0])
@pytest.mark.parametrize("dense", [0, 1])
def test_group_aggregate_count_only_has_one_word_records(part_plain, dense):
    # COUNT(*) alone: a partition record is the key word and nothing else -- the word -> record division by multiplication
    # (floor(2^32 / words) + 1) has no 32-bit form for ONE word (found by the dense fuzz: groups merged into each other)
    n = 100003
    view = make_view(n, nullable=True)
    ctx = ss.Context(0)
    for k, v in (("group_partition", 2), ("part_plain", part_plain), ("group_dense", dense), ("group_resident", 0), ("group_slab", 0)):
        ctx.set_option(k, v)
    for keys in (["k1"], ["k2", "t"]):
        spec = ss.AggregationSpecification().AddAggregation(ss.COUNT, "", "rows")
        run_both(ss.GroupAggregate(ss.ProjectNamedAttributes(keys), spec, None, ss.ScanView(view)), ctx, ignore_order=True)
        run_both(ss.GroupAggregate(ss.ProjectNamedAttributes(keys), spec, None,
                                   ss.Filter(ss.Greater(NA("b"), ss.ConstInt64(499)), ss.ProjectAllAttributes(), ss.ScanView(view))), ctx, ignore_order=True)


@pytest.mark.parametrize("n", [0, 1000, 100003])
def test_group_aggregate_int64_key(gpu_ctx, n):
    view = make_view(n)
    spec = ss.AggregationSpecification().AddAggregation(ss.SUM, "a", "s").AddAggregation(ss.MIN, "d", "mn").AddAggregation(ss.MAX, "d", "mx")
    run_both(ss.GroupAggregate(ss.ProjectNamedAttributes(["c"]), spec, None, ss.ScanView(view)), gpu_ctx, ignore_order=True)


@pytest.mark.parametrize("n", [0, 1, 65, 1025, 100003])
@pytest.mark.parametrize("with_filter", [False, True])
def test_group_aggregate_wide_keys(gpu_ctx, n, with_filter):
    # keys that do not pack into 64 bits run as materialise -> radix sort -> clustered aggregation:
    # two NULLABLE INT32 keys (66 bits), a NULLABLE INT64 key (65 bits), INT64 + INT32 + BOOL (104 bits)
    view = make_view(n, nullable=True)
    run_both(group_query(view, with_filter, ("k1", "k2")), gpu_ctx, ignore_order=True)
    spec = ss.AggregationSpecification().AddAggregation(ss.SUM, "b", "s").AddAggregation(ss.MIN, "d0", "mn").AddAggregation(ss.COUNT, "d0", "c").AddAggregation(ss.COUNT, "", "n")
    child = ss.ScanView(view)
    if with_filter:
        child = ss.Filter(ss.Greater(NA("b"), ss.ConstInt64(499)), ss.ProjectAllAttributes(), child)
    run_both(ss.GroupAggregate(ss.ProjectNamedAttributes(["a"]), spec, None, child), gpu_ctx, ignore_order=True)
    child = ss.Compute(ss.CompoundExpression().AddAs("k64", ss.Plus(NA("a"), NA("k1"))).Add(NA("k2")).Add(NA("t")).Add(NA("b")).Add(NA("d0")), child)
    run_both(ss.GroupAggregate(ss.ProjectNamedAttributes(["k64", "k2", "t"]), spec, None, child), gpu_ctx, ignore_order=True)


def first_last_spec():
    return (ss.AggregationSpecification().AddAggregation(ss.FIRST, "d0", "f_d0").AddAggregation(ss.LAST, "d0", "l_d0")
            .AddAggregation(ss.FIRST, "c", "f_c").AddAggregation(ss.LAST, "u", "l_u").AddAggregation(ss.LAST, "t", "l_t")
            .AddAggregation(ss.SUM, "b", "s").AddAggregation(ss.COUNT, "", "n"))


@pytest.mark.parametrize("n", [0, 1, 65, 1025, 100003])
@pytest.mark.parametrize("with_filter", [False, True])
@pytest.mark.parametrize("partition", [0, 2])
def test_group_aggregate_first_last(n, with_filter, partition):
    # FIRST / LAST per group (aggregation_operators.h:290-320): first / last non-NULL value in input order
    ctx = ss.Context(0)
    ctx.set_option("group_partition", partition)
    view = make_view(n, nullable=True)
    child = ss.ScanView(view)
    if with_filter:
        child = ss.Filter(ss.Greater(NA("b"), ss.ConstInt64(499)), ss.ProjectAllAttributes(), child)
    run_both(ss.GroupAggregate(ss.ProjectNamedAttributes(["k2"]), first_last_spec(), None, child), ctx, ignore_order=True)
    # wide keys and a computed FIRST input: materialise + sort + clustered aggregation
    run_both(ss.GroupAggregate(ss.ProjectNamedAttributes(["k1", "k2"]), first_last_spec(), None, child), ctx, ignore_order=True)
    spec = ss.AggregationSpecification().AddAggregation(ss.FIRST, "x", "fx").AddAggregation(ss.LAST, "x", "lx").AddAggregation(ss.MAX, "x", "mx")
    computed = ss.Compute(ss.CompoundExpression().Add(NA("k2")).AddAs("x", ss.Plus(NA("a"), NA("c"))), child)
    run_both(ss.GroupAggregate(ss.ProjectNamedAttributes(["k2"]), spec, None, computed), ctx, ignore_order=True)


@pytest.mark.parametrize("n", [0, 1, 1025, 100003])
def test_aggregate_clusters_first_last(gpu_ctx, n):
    view = make_view(n, nullable=True)
    order = np.argsort(view.column(5).data, kind="stable")      # rows clustered by k2
    cols = [ss.Column(view.column(i).data[order], None if view.column(i).is_null is None else view.column(i).is_null[order])
            for i in range(view.column_count())]
    clustered = ss.View(view.schema(), cols)
    run_both(ss.AggregateClusters(ss.ProjectNamedAttributes(["k2"]), first_last_spec(), ss.ScanView(clustered)), gpu_ctx)


def test_group_table_regrow():
    ctx = ss.Context(0)
    ctx.set_option("group_capacity", 64)   # 1000 groups do not fit: forces the regrow + rerun path
    run_both(group_query(make_view(50000), False), ctx, ignore_order=True)


@pytest.mark.parametrize("n", [0, 1, 65, 1025, 100003])
@pytest.mark.parametrize("with_filter", [False, True])
@pytest.mark.parametrize("nullable", [False, True])
def test_group_aggregate_partitioned(n, with_filter, nullable):
    # the hash-partitioned execution (normally chosen by run feedback when the group count is large)
    ctx = ss.Context(0)
    ctx.set_option("group_partition", 2)
    keys = ("k1",) if nullable else ("k1", "k2")
    run_both(group_query(make_view(n, nullable=nullable), with_filter, keys), ctx, ignore_order=True)


def test_group_aggregate_partitioned_many_groups():
    # more groups than one partition's on-chip table holds at 512 partitions x 100 k groups:
    # exercises the "partition finer and rerun" path as well as the EMPTY-valued key
    n = 300000
    rng = np.random.default_rng(7)
    key = rng.integers(0, 120000, n).astype(np.int64)
    key[::1000] = -1          # packed key 0xFFFF...: the table's EMPTY sentinel value
    val = rng.integers(-1000, 1000, n).astype(np.int64)
    schema = ss.TupleSchema([ss.Attribute("k", ss.INT64), ss.Attribute("v", ss.INT64)])
    view = ss.View(schema, [ss.Column(key), ss.Column(val)], n)
    spec = ss.AggregationSpecification().AddAggregation(ss.SUM, "v", "s").AddAggregation(ss.COUNT, "", "c").AddAggregation(ss.MIN, "v", "mn")
    op = ss.GroupAggregate(ss.ProjectNamedAttributes(["k"]), spec, None, ss.ScanView(view))
    ctx = ss.Context(0)
    ctx.set_option("group_partition", 2)
    run_both(op, ctx, ignore_order=True)
    # adaptive: repeated runs of ONE plan walk through the fed-back configurations (smaller
    # residency / larger LDS table, then hash partitioning); every one must give the same rows
    from helpers import to_cols, sort_rows, assert_cols_equal
    from oracle import oracle
    _, want = oracle.run(op, 1024)
    plan = ss.Plan(op, ss.Context(0))
    for _ in range(6):
        plan.run()
        assert_cols_equal(sort_rows(to_cols(plan.fetch())), sort_rows(want), context="adaptive group run")


@pytest.mark.parametrize("shape", ["uniform", "pairs", "long_runs", "sorted_high"])
@pytest.mark.parametrize("payload", [0, 4])
def test_sort_wide_keys_high_half_first(gpu_ctx, shape, payload):
    # INT64 keys whose eight digits all vary: the sort orders them by the high half and fixes up runs of equal high halves
    # by the low half ("pairs": many runs of 2-3), or -- when a run is long ("long_runs") -- falls back to all eight passes;
    # either way the result is the stable order by the whole key, with 0 or 4 payload columns (records)
    rng = np.random.default_rng(21)
    n = 200003
    lo = rng.integers(0, 1 << 32, n, dtype=np.uint64)
    if shape == "uniform":
        hi = rng.integers(0, 1 << 32, n, dtype=np.uint64)
    elif shape == "pairs":
        hi = rng.integers(0, 1 << 32, n // 2, dtype=np.uint64)[rng.integers(0, n // 2, n)]
    elif shape == "long_runs":
        hi = rng.integers(0, 1 << 32, 300, dtype=np.uint64)[rng.integers(0, 300, n)]
    else:
        hi = np.sort(rng.integers(0, 1 << 32, n // 3, dtype=np.uint64)[rng.integers(0, n // 3, n)])
    key = ((hi << np.uint64(32)) | lo).view(np.int64)
    key[::97] = key[5]                                   # exact duplicates: their input order must survive
    cols = [ss.Column(key), ss.Column(np.arange(n, dtype=np.int64))] + [ss.Column(rng.integers(-9, 9, n) * 0.5) for _ in range(payload)]
    schema = ss.TupleSchema([ss.Attribute("k", ss.INT64), ss.Attribute("id", ss.INT64)] + [ss.Attribute("p%d" % i, ss.DOUBLE) for i in range(payload)])
    view = ss.View(schema, cols, n)
    got = ss.drain(ss.Sort(ss.SortOrder().add("k", ss.ASCENDING), None, 0, ss.ScanView(view)).CreateCursor(gpu_ctx), 1 << 20)
    order = np.argsort(key, kind="stable")
    assert np.array_equal(got.column(0).data, key[order])
    assert np.array_equal(got.column(1).data, order)
    for i in range(payload):
        assert np.array_equal(got.column(2 + i).data, cols[2 + i].data[order])


@pytest.mark.parametrize("shape", ["uniform", "pairs", "long_runs"])
@pytest.mark.parametrize("kind", ["int_desc", "double", "minor_key"])
def test_sort_wide_keys_as_one_word_per_row(gpu_ctx, shape, kind):
    # the (high half << 32 | row id) form of the high-half-first sort (runtime.cpp: run_sort, `compact`): descending integer keys,
    # DOUBLE keys (never read back from the sorted words) and a wide key that is the LEAST significant of two
    rng = np.random.default_rng(33)
    n = 150001
    lo = rng.integers(0, 1 << 32, n, dtype=np.uint64)
    if shape == "uniform":
        hi = rng.integers(0, 1 << 32, n, dtype=np.uint64)
    elif shape == "pairs":
        hi = rng.integers(0, 1 << 32, n // 2, dtype=np.uint64)[rng.integers(0, n // 2, n)]
    else:
        hi = rng.integers(0, 1 << 32, 300, dtype=np.uint64)[rng.integers(0, 300, n)]
    bits = (hi << np.uint64(32)) | lo
    bits[::89] = bits[7]
    payload = [rng.integers(-9, 9, n) * 0.5 for _ in range(3)]
    rowid = np.arange(n, dtype=np.int64)
    if kind == "double":
        key = bits.view(np.float64).copy()
        key[~np.isfinite(key)] = 1.5                      # NaN ordering is a separate test
        kcol, ktype = key, ss.DOUBLE
    else:
        key = bits.view(np.int64)
        kcol, ktype = key, ss.INT64
    g = (np.arange(n) % 3).astype(np.int32)
    schema = ss.TupleSchema([ss.Attribute("k", ktype), ss.Attribute("id", ss.INT64), ss.Attribute("g", ss.INT32)] + [ss.Attribute("p%d" % i, ss.DOUBLE) for i in range(3)])
    view = ss.View(schema, [ss.Column(kcol), ss.Column(rowid), ss.Column(g)] + [ss.Column(x) for x in payload], n)
    if kind == "int_desc":
        order_spec = ss.SortOrder().add("k", ss.DESCENDING)
        want = np.array(sorted(range(n), key=lambda i: (-int(key[i]), i)), dtype=np.int64)
    elif kind == "double":
        order_spec = ss.SortOrder().add("k", ss.ASCENDING)
        want = np.argsort(key, kind="stable")
    else:
        order_spec = ss.SortOrder().add("g", ss.ASCENDING).add("k", ss.ASCENDING)
        want = np.lexsort((rowid, key, g))
    got = ss.drain(ss.Sort(order_spec, None, 0, ss.ScanView(view)).CreateCursor(gpu_ctx), 1 << 20)
    assert np.array_equal(got.column(1).data, want)
    assert np.array_equal(got.column(0).data.view(np.uint64), np.asarray(kcol)[want].view(np.uint64))
    assert np.array_equal(got.column(2).data, g[want])
    for i in range(3):
        assert np.array_equal(got.column(3 + i).data, payload[i][want])


@pytest.mark.parametrize("n", [0, 1, 1025, 60013])
@pytest.mark.parametrize("nullable", [False, True])
def test_distinct_aggregates(gpu_ctx, n, nullable):
    # SUM / COUNT of the DISTINCT values of a group (column_aggregator.cc:308-376), next to plain aggregates of the same and of
    # other columns; MIN / MAX DISTINCT are the plain ones.  Device: materialise -> sort by (keys, column) -> first-of-run flags.
    view = make_view(n, nullable=nullable)
    spec = (ss.AggregationSpecification().AddDistinctAggregation(ss.COUNT, "a", "cd").AddDistinctAggregation(ss.SUM, "a", "sd")
            .AddAggregation(ss.SUM, "a", "s").AddAggregation(ss.COUNT, "a", "c").AddAggregation(ss.COUNT, "", "n")
            .AddDistinctAggregation(ss.MAX, "d0", "mx").AddAggregation(ss.MIN, "d1", "mn"))
    run_both(ss.ScalarAggregate(spec, ss.ScanView(view)), gpu_ctx)
    run_both(ss.GroupAggregate(ss.ProjectNamedAttributes(["k2"]), spec, None, ss.ScanView(view)), gpu_ctx, ignore_order=True)
    run_both(ss.GroupAggregate(ss.ProjectNamedAttributes(["k1", "t"]), spec, None,
                               ss.Filter(ss.Greater(NA("b"), ss.ConstInt64(499)), ss.ProjectAllAttributes(), ss.ScanView(view))), gpu_ctx, ignore_order=True)
    # a DISTINCT aggregate of a computed column, DOUBLE values (sums of small multiples of 0.5: exact in any order)
    e = ss.CompoundExpression().Add(NA("k2")).AddAs("x", ss.Multiply(NA("d2"), ss.ConstDouble(0.5)))
    spec2 = ss.AggregationSpecification().AddDistinctAggregation(ss.SUM, "x", "sx").AddDistinctAggregation(ss.COUNT, "x", "cx")
    run_both(ss.GroupAggregate(ss.ProjectNamedAttributes(["k2"]), spec2, None, ss.Compute(e, ss.ScanView(view))), gpu_ctx, ignore_order=True)


@pytest.mark.parametrize("n", [0, 3, 700, 40001])
@pytest.mark.parametrize("nullable", [False, True])
def test_distinct_aggregates_over_several_columns(gpu_ctx, n, nullable):
    # DISTINCT aggregations over two and three different columns of one specification (hybrid_aggregate_test.cc:652-720 has
    # the two-column shape): every further column costs one more sort + flag pass whose flags ride along as payload
    view = make_view(n, nullable=nullable)
    spec = (ss.AggregationSpecification().AddDistinctAggregation(ss.COUNT, "a", "cda").AddDistinctAggregation(ss.SUM, "k1", "sdk")
            .AddAggregation(ss.SUM, "a", "s").AddDistinctAggregation(ss.SUM, "a", "sda").AddDistinctAggregation(ss.COUNT, "t", "cdt")
            .AddAggregation(ss.COUNT, "", "n").AddDistinctAggregation(ss.COUNT, "k1", "cdk").AddAggregation(ss.MIN, "d1", "mn"))
    run_both(ss.ScalarAggregate(spec, ss.ScanView(view)), gpu_ctx)
    run_both(ss.GroupAggregate(ss.ProjectNamedAttributes(["k2"]), spec, None, ss.ScanView(view)), gpu_ctx, ignore_order=True)
    run_both(ss.GroupAggregate(ss.ProjectNamedAttributes(["k2", "t"]), spec, None,
                               ss.Filter(ss.Greater(NA("b"), ss.ConstInt64(499)), ss.ProjectAllAttributes(), ss.ScanView(view))), gpu_ctx, ignore_order=True)


@pytest.mark.parametrize("n", [0, 5, 1025, 60013])
@pytest.mark.parametrize("nullable", [False, True])
def test_first_last_next_to_distinct_aggregates(gpu_ctx, n, nullable):
    # FIRST / LAST follow the INPUT order (aggregation_operators.h:290-320) although the DISTINCT shape re-orders the rows by
    # (keys, distinct column): the input row id is stored as one more column, carried through the sorts, and the clustered
    # aggregate picks by (row id << 32 | position), the scalar sinks by the row id.  One and two DISTINCT columns; NULL inputs never
    # count; with a filter.
    view = make_view(n, nullable=nullable)
    spec = (ss.AggregationSpecification().AddDistinctAggregation(ss.SUM, "a", "sd").AddAggregation(ss.FIRST, "d0", "fd").AddAggregation(ss.LAST, "d", "ld")
            .AddAggregation(ss.FIRST, "b", "fb").AddAggregation(ss.LAST, "t", "lt").AddAggregation(ss.COUNT, "", "n").AddAggregation(ss.LAST, "a", "la"))
    run_both(ss.GroupAggregate(ss.ProjectNamedAttributes(["k2"]), spec, None, ss.ScanView(view)), gpu_ctx, ignore_order=True)
    spec.AddDistinctAggregation(ss.COUNT, "k1", "cdk")
    run_both(ss.GroupAggregate(ss.ProjectNamedAttributes(["k2", "t"]), spec, None,
                               ss.Filter(ss.Greater(NA("b"), ss.ConstInt64(499)), ss.ProjectAllAttributes(), ss.ScanView(view))), gpu_ctx, ignore_order=True)
    run_both(ss.ScalarAggregate(spec, ss.ScanView(view)), gpu_ctx)    # the scalar sinks take their order from that column too
    run_both(ss.ScalarAggregate(spec, ss.Filter(ss.Less(NA("b"), ss.ConstInt64(300)), ss.ProjectAllAttributes(), ss.ScanView(view))), gpu_ctx)


def test_plan_restages_every_new_host_view(gpu_ctx):
    # one Plan run over a stream of temporary host Views (a per-batch loop): CPython reuses the id() of a freed View, so
    # the staged device block must be keyed on the object itself -- never on its id
    schema = ss.TupleSchema([ss.Attribute("a", ss.INT64)])
    op = ss.ScalarAggregate(ss.AggregationSpecification().AddAggregation(ss.SUM, "a", "s"), ss.ScanView(ss.View(schema, [np.zeros(8, np.int64)])))
    plan = ss.Plan(op, gpu_ctx)
    for batch in range(20):
        data = np.full(1000 + batch, batch, dtype=np.int64)
        plan.run(ss.View(schema, [data]))               # the View is garbage as soon as run() returns
        assert plan.fetch().column(0).data[0] == batch * (1000 + batch)


def test_device_view_of_a_failed_run_reports_the_evaluation_error(gpu_ctx):
    # result_device_view (what the sharded sort / group aggregate consume) must not hand out the buffers of a run that
    # hit a signaling division
    schema = ss.TupleSchema([ss.Attribute("a", ss.INT64), ss.Attribute("b", ss.INT64)])
    view = ss.View(schema, [np.arange(1, 2001), np.where(np.arange(2000) == 777, 0, 3)])
    plan = ss.Plan(ss.Compute(ss.CompoundExpression().AddAs("q", ss.CppDivideSignaling(NA("a"), NA("b"))), ss.ScanView(view)), gpu_ctx)
    plan.run()
    with pytest.raises(ss.SupersonicException) as e:
        plan.result_device_view()
    assert e.value.return_code == ss.ERROR_EVALUATION_ERROR


@pytest.mark.parametrize("nullable", [False, True])
def test_guarded_signaling_operators_do_not_fail_on_rows_they_are_not_evaluated_on(gpu_ctx, nullable):
    # the canonical guards: IF(b <> 0, a / b, x), (b <> 0) AND (a / b > 1), IFNULL, CASE, a NULL earlier argument --
    # the reference evaluates the failing child under a skip vector (elementary_bound_expressions.cc:279-318,935-955)
    rng = np.random.default_rng(3)
    n = 5000
    N = ss.NULLABLE if nullable else ss.NOT_NULLABLE
    schema = ss.TupleSchema([ss.Attribute("a", ss.INT64, N), ss.Attribute("b", ss.INT64), ss.Attribute("x", ss.DOUBLE, N)])
    nl = (lambda: rng.random(n) < 0.2) if nullable else (lambda: None)
    view = ss.View(schema, [ss.Column(rng.integers(-50, 50, n), nl()), rng.integers(0, 3, n), ss.Column(rng.integers(-9, 9, n) * 0.5, nl())])
    nz = ss.NotEqual(NA("b"), ss.ConstInt64(0))
    e = (ss.CompoundExpression()
         .AddAs("g1", ss.If(nz, ss.CppDivideSignaling(NA("a"), NA("b")), ss.ConstInt64(-1)))
         .AddAs("g2", ss.And(nz, ss.Greater(ss.DivideSignaling(NA("a"), NA("b")), ss.ConstDouble(1.0))))
         .AddAs("g3", ss.Or(ss.Equal(NA("b"), ss.ConstInt64(0)), ss.Less(ss.ModulusSignaling(NA("a"), NA("b")), ss.ConstInt64(1))))
         .AddAs("g4", ss.If(ss.GreaterOrEqual(NA("x"), ss.ConstDouble(0.0)), ss.SqrtSignaling(NA("x")), ss.ConstDouble(0.0)))
         .AddAs("g5", ss.Case([NA("b"), ss.ConstInt64(7), ss.ConstInt64(1), ss.CppDivideSignaling(NA("a"), NA("b")),
                               ss.ConstInt64(2), ss.ModulusSignaling(NA("a"), NA("b"))])))
    run_both(ss.Compute(e, ss.ScanView(view)), gpu_ctx)
    # and the unguarded forms still fail
    for bad in (ss.CppDivideSignaling(NA("a"), NA("b")), ss.If(nz, ss.ConstInt64(1), ss.ModulusSignaling(ss.ConstInt64(5), NA("b")))):
        with pytest.raises(ss.SupersonicException) as err:
            ss.drain(ss.Compute(ss.CompoundExpression().AddAs("q", bad), ss.ScanView(view)).CreateCursor(gpu_ctx))
        assert err.value.return_code == ss.ERROR_EVALUATION_ERROR


def test_group_aggregate_partitioned_skewed_keys():
    # one hot key takes 90 % of the rows: its (partition, workgroup) segments run full, the stage reruns with larger
    # segments (x4 per attempt) and, if that is not enough, falls back to the direct path -- the rows never change
    n = 300000
    rng = np.random.default_rng(9)
    key = np.where(rng.random(n) < 0.9, 77, rng.integers(0, 50000, n)).astype(np.int64)
    val = rng.integers(-1000, 1000, n).astype(np.int64)
    d = rng.integers(-4000, 4000, n) * 0.25
    schema = ss.TupleSchema([ss.Attribute("k", ss.INT64), ss.Attribute("v", ss.INT64), ss.Attribute("d", ss.DOUBLE)])
    view = ss.View(schema, [ss.Column(key), ss.Column(val), ss.Column(d)], n)
    spec = (ss.AggregationSpecification().AddAggregation(ss.SUM, "v", "s").AddAggregation(ss.COUNT, "", "c").AddAggregation(ss.MIN, "v", "mn")
            .AddAggregation(ss.SUM, "d", "sd").AddAggregation(ss.MAX, "d", "mxd"))
    op = ss.GroupAggregate(ss.ProjectNamedAttributes(["k"]), spec, None, ss.ScanView(view))
    ctx = ss.Context(0)
    ctx.set_option("group_partition", 2)
    run_both(op, ctx, ignore_order=True)


def test_sharded_group_aggregate_merge_plan_on_device(gpu_ctx):
    # the multi-GPU GroupAggregate (per-shard aggregate -> all-gather -> merge aggregate) with the
    # device executor; one rank here, the world_size-2 exchange is covered on CPU (gloo)
    import socket
    import torch.distributed as dist
    from supersonic_amd.distributed import sharded_group_aggregate, device_executor
    from helpers import to_cols, sort_rows, assert_cols_equal
    from oracle import oracle
    s = socket.socket(); s.bind(("127.0.0.1", 0)); port = s.getsockname()[1]; s.close()
    dist.init_process_group("gloo", init_method="tcp://127.0.0.1:%d" % port, rank=0, world_size=1)
    try:
        view = make_view(50000)
        spec = (ss.AggregationSpecification().AddAggregation(ss.SUM, "d0", "s0").AddAggregation(ss.MIN, "d1", "mn1")
                .AddAggregation(ss.MAX, "d2", "mx2").AddAggregation(ss.COUNT, "", "n"))
        child = ss.Filter(ss.Greater(NA("a"), ss.ConstInt64(499)), ss.ProjectAllAttributes(), ss.ScanView(view))
        out = sharded_group_aggregate(["k1", "k2"], spec, child, device_executor(gpu_ctx))
        _schema, want = oracle.run(ss.GroupAggregate(ss.ProjectNamedAttributes(["k1", "k2"]), spec, None, child))
        assert_cols_equal(sort_rows(to_cols(out)), sort_rows(want), context="sharded group aggregate on device")
        # what is not a partial result: DISTINCT aggregates travel as distinct (keys, value) pairs stacked under the partial table,
        # CONCAT and the row-after-row SUM as the rows themselves -- the shard plans and the merge plans run on the device here
        hard = [ss.AggregationSpecification().AddDistinctAggregation(ss.COUNT, "b", "cb").AddAggregation(ss.SUM, "d0", "s0").AddDistinctAggregation(ss.SUM, "u", "su")
                .AddAggregation(ss.COUNT, "", "n").AddAggregation(ss.LAST, "t", "lt"),
                ss.AggregationSpecification().AddAggregation(ss.CONCAT, "t", "ct").AddAggregation(ss.SUM, "d0", "s0").AddDistinctAggregation(ss.COUNT, "b", "cb"),
                ss.AggregationSpecification().AddAggregationWithDefinedOutputType(ss.SUM, "d1", "q", ss.INT64).AddAggregation(ss.MAX, "b", "mb")]
        small = ss.Filter(ss.Greater(NA("a"), ss.ConstInt64(499)), ss.ProjectAllAttributes(), ss.ScanView(make_view(4000, nullable=True)))
        for hspec in hard:
            for key_range in (False, True):
                out = sharded_group_aggregate(["k1", "k2"], hspec, small, device_executor(gpu_ctx), key_range=key_range)
                _schema, want = oracle.run(ss.GroupAggregate(ss.ProjectNamedAttributes(["k1", "k2"]), hspec, None, small))
                assert_cols_equal(sort_rows(to_cols(out)), sort_rows(want), context="sharded hard aggregates on device")
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("n", [0, 1, 1025, 20011])
@pytest.mark.parametrize("nullable", [False, True])
def test_case_and_in_expressions(gpu_ctx, n, nullable):
    # CASE (elementary_bound_expressions.cc:542-760) and IN (comparison_expressions.h:75-89) over
    # columns, constants and NULL literals, with type promotion of the WHEN / THEN / list elements
    view = make_view(n, nullable=nullable)
    case1 = ss.Case([NA("k2"), NA("d0"), ss.ConstInt32(1), NA("d1"), NA("k1"), ss.ConstDouble(-1.5), ss.ConstInt64(7), ss.Null(ss.DOUBLE)])
    case2 = ss.Case([NA("t"), NA("a"), ss.ConstBool(True), NA("b")])
    in1 = ss.In(NA("k2"), [ss.ConstInt32(3), NA("k1"), ss.ConstInt64(11)])
    in2 = ss.In(NA("a"), [ss.ConstInt64(5), ss.Null(ss.INT64), NA("b")])
    in3 = ss.In(NA("d2"), [ss.ConstDouble(3.0), NA("d3")])
    e = (ss.CompoundExpression().AddAs("c1", case1).AddAs("c2", case2).AddAs("i1", in1).AddAs("i2", in2).AddAs("i3", in3)
         .AddAs("i0", ss.In(NA("a"), [])))
    run_both(ss.Compute(e, ss.ScanView(view)), gpu_ctx)
    # as a filter predicate and inside an aggregate
    spec = ss.AggregationSpecification().AddAggregation(ss.SUM, "c1", "s").AddAggregation(ss.COUNT, "c2", "n")
    run_both(ss.ScalarAggregate(spec, ss.Compute(e, ss.Filter(in1, ss.ProjectAllAttributes(), ss.ScanView(view)))), gpu_ctx)


@pytest.mark.parametrize("n", [0, 3, 1025, 40013])
@pytest.mark.parametrize("nullable", [False, True])
def test_exact_math_family(gpu_ctx, n, nullable):
    # ABS / ROUND / CEIL / FLOOR / TRUNC / *_TO_INT / SQRT / IS_* : every one is an exact or
    # correctly rounded IEEE operation, so the device must match libm bit for bit
    rng = np.random.default_rng(3)
    N = ss.NULLABLE if nullable else ss.NOT_NULLABLE
    schema = ss.TupleSchema([ss.Attribute("x", ss.DOUBLE, N), ss.Attribute("f", ss.FLOAT, N), ss.Attribute("i", ss.INT32, N),
                             ss.Attribute("l", ss.INT64), ss.Attribute("u", ss.UINT64), ss.Attribute("p", ss.DOUBLE)])
    x = rng.standard_normal(n) * np.exp(rng.integers(-20, 20, n))
    special = np.array([0.0, -0.0, 0.5, -0.5, 1.5, 2.5, -2.5, np.inf, -np.inf, np.nan, 4.9e-324, 1e308, -1e-310])
    x[: min(n, len(special))] = special[: min(n, len(special))]

    def nl():
        return (rng.random(n) < 0.15) if nullable else None
    view = ss.View(schema, [ss.Column(x, nl()), ss.Column((rng.standard_normal(n) * 1000).astype(np.float32), nl()),
                            ss.Column(rng.integers(-2**31, 2**31, n).astype(np.int32), nl()), rng.integers(-2**63, 2**63 - 1, n),
                            rng.integers(0, 2**63, n).astype(np.uint64) * np.uint64(2) + np.uint64(1), np.where(np.isfinite(x), np.abs(x), np.nan)])
    small = ss.Multiply(NA("p"), ss.ConstDouble(1e-280))    # keeps *_TO_INT inside the int64 range
    e = (ss.CompoundExpression()
         .AddAs("abs_x", ss.Abs(NA("x"))).AddAs("abs_f", ss.Abs(NA("f"))).AddAs("abs_i", ss.Abs(NA("i"))).AddAs("abs_l", ss.Abs(NA("l"))).AddAs("abs_u", ss.Abs(NA("u")))
         .AddAs("round_x", ss.Round(NA("x"))).AddAs("round_f", ss.Round(NA("f"))).AddAs("ceil_x", ss.Ceil(NA("x"))).AddAs("ceil_f", ss.Ceil(NA("f")))
         .AddAs("floor_x", ss.Floor(NA("x"))).AddAs("floor_f", ss.Floor(NA("f"))).AddAs("trunc_x", ss.Trunc(NA("x"))).AddAs("trunc_f", ss.Trunc(NA("f")))
         .AddAs("ceil_i", ss.Ceil(NA("i"))))
    run_both(ss.Compute(e, ss.ScanView(view)), gpu_ctx)
    e = (ss.CompoundExpression()     # (the oracle's expression lists hold 16 entries)
         .AddAs("c2i", ss.CeilToInt(small)).AddAs("f2i", ss.FloorToInt(small)).AddAs("r2i", ss.RoundToInt(small)).AddAs("f2i_f", ss.FloorToInt(NA("f")))
         .AddAs("sqrt_q", ss.SqrtQuiet(NA("x"))).AddAs("sqrt_n", ss.SqrtNulling(NA("x"))).AddAs("sqrt_p", ss.SqrtSignaling(NA("p"))).AddAs("sqrt_i", ss.SqrtNulling(NA("i")))
         .AddAs("fin", ss.IsFinite(NA("x"))).AddAs("inf", ss.IsInf(NA("x"))).AddAs("nan", ss.IsNaN(NA("x"))).AddAs("nrm", ss.IsNormal(NA("x"))).AddAs("fin_f", ss.IsFinite(NA("f")))
         .AddAs("odd_i", ss.IsOdd(NA("i"))).AddAs("even_l", ss.IsEven(NA("l"))).AddAs("odd_u", ss.IsOdd(NA("u"))))
    run_both(ss.Compute(e, ss.ScanView(view)), gpu_ctx)


def test_sqrt_signaling_fails_on_selected_negative_rows(gpu_ctx):
    view = make_view(5000)
    op = ss.Compute(ss.SqrtSignaling(NA("d0")), ss.ScanView(view))      # d0 has negative values
    r = op.CreateCursor(gpu_ctx).Next(1024)
    assert r.is_failure() and r.exception().return_code == 104
    op = ss.Compute(ss.SqrtSignaling(NA("d0")),
                    ss.Filter(ss.GreaterOrEqual(NA("d0"), ss.ConstDouble(0.0)), ss.ProjectAllAttributes(), ss.ScanView(view)))
    run_both(op, gpu_ctx)


@pytest.mark.parametrize("n", [0, 7, 1025, 30011])
def test_string_columns_through_the_pipeline(gpu_ctx, n):
    # STRING columns are dictionary codes on the device (include/ssgpu.h); everything the path
    # does with them -- compare, IN / CASE, filter payload, group key, MIN / MAX, sort key -- must
    # return the same byte strings as the oracle
    rng = np.random.default_rng(17)
    words = [b"", b"a", b"aa", b"ab", b"b", b"apple", b"apples", b"Zebra", b"zebra", b"\xff\x00", b"pear", b"fig"]
    schema = ss.TupleSchema([ss.Attribute("s", ss.STRING, ss.NULLABLE), ss.Attribute("t", ss.STRING), ss.Attribute("v", ss.INT64),
                             ss.Attribute("k", ss.INT32)])
    view = ss.View(schema, [ss.Column([words[i] for i in rng.integers(0, len(words), n)], rng.random(n) < 0.15),
                            [words[i] for i in rng.integers(0, len(words), n)], rng.integers(-100, 100, n), rng.integers(0, 5, n).astype(np.int32)])
    e = (ss.CompoundExpression().AddAs("lt", ss.Less(NA("s"), NA("t"))).AddAs("eq", ss.Equal(NA("s"), ss.ConstString("apple")))
         .AddAs("ge", ss.GreaterOrEqual(NA("t"), ss.ConstString("b"))).AddAs("in", ss.In(NA("s"), [ss.ConstString("fig"), NA("t"), ss.ConstString("nope")]))
         .AddAs("cs", ss.Case([NA("k"), NA("t"), ss.ConstInt32(1), ss.ConstString("one"), ss.ConstInt32(2), NA("s")]))
         .AddAs("nv", ss.IfNull(NA("s"), ss.ConstString("<null>"))).Add(NA("s")))
    run_both(ss.Compute(e, ss.ScanView(view)), gpu_ctx)
    flt = ss.Filter(ss.Less(NA("s"), ss.ConstString("b")), ss.ProjectAllAttributes(), ss.ScanView(view))
    run_both(flt, gpu_ctx)
    spec = (ss.AggregationSpecification().AddAggregation(ss.SUM, "v", "sv").AddAggregation(ss.MIN, "t", "mn").AddAggregation(ss.MAX, "s", "mx")
            .AddAggregation(ss.COUNT, "s", "c"))
    run_both(ss.GroupAggregate(ss.ProjectNamedAttributes(["s"]), spec, None, ss.ScanView(view)), gpu_ctx, ignore_order=True)
    run_both(ss.ScalarAggregate(spec, flt), gpu_ctx)
    srt = ss.Sort(ss.SortOrder().add("s", ss.DESCENDING).add("t", ss.ASCENDING).add("v", ss.ASCENDING), ss.ProjectAllAttributes(), 0, ss.ScanView(view))
    got = ss.drain(srt.CreateCursor(gpu_ctx), 1024)
    _schema, want = oracle_run(srt)
    # Sort is not stable in the reference either: compare the key sequence and the row multiset
    for c in (0, 1, 2):
        assert_cols_equal([to_cols(got)[c]], [want[c]], context="sort key column %d" % c)
    assert_cols_equal(sort_rows(to_cols(got)), sort_rows(want), context="sorted rows as a multiset")
    with pytest.raises(ss.SupersonicException):      # arithmetic on STRING is a bind error (402), as in the reference
        ss.Compute(ss.Plus(NA("s"), ss.ConstInt32(1)), ss.ScanView(view)).CreateCursor(gpu_ctx)


def _join_views(n, m, seed=23):
    rng = np.random.default_rng(seed)
    ls = ss.TupleSchema([ss.Attribute("fk", ss.INT64, ss.NULLABLE), ss.Attribute("fk2", ss.INT32), ss.Attribute("v", ss.DOUBLE), ss.Attribute("a", ss.INT64)])
    rs = ss.TupleSchema([ss.Attribute("id", ss.INT64, ss.NULLABLE), ss.Attribute("id2", ss.INT32), ss.Attribute("name", ss.STRING),
                         ss.Attribute("w", ss.DOUBLE, ss.NULLABLE), ss.Attribute("g", ss.INT32)])
    ids = rng.permutation(4 * m)[:m].astype(np.int64) - m          # unique, includes negatives and -1 (the EMPTY sentinel value)
    if m > 3:
        ids[3] = -1
    rview = ss.View(rs, [ss.Column(ids, np.arange(m) % 17 == 5), (np.arange(m) % 3).astype(np.int32), ["n%d" % (i % 37) for i in range(m)],
                         ss.Column(rng.integers(-100, 100, m) * 0.5, rng.random(m) < 0.2), rng.integers(0, 9, m).astype(np.int32)])
    lview = ss.View(ls, [ss.Column(rng.integers(-m, 3 * m + 1, n), rng.random(n) < 0.1), rng.integers(0, 3, n).astype(np.int32),
                         rng.integers(-4000, 4000, n) * 0.25, rng.integers(0, 1000, n)])
    return lview, rview


@pytest.mark.parametrize("n,m", [(0, 5), (7, 0), (1025, 40), (30011, 300)])
@pytest.mark.parametrize("join_type", [ss.INNER, ss.LEFT_OUTER])
def test_hash_join_fused_into_the_pipeline(gpu_ctx, n, m, join_type):
    # HashJoinOperation (hash_join.h:37-56), UNIQUE rhs keys: probe + rhs gathers inside the lhs program
    lview, rview = _join_views(n, m)
    proj = (ss.CompoundMultiSourceProjector().add(0, ss.ProjectAllAttributes("L."))
            .add(1, ss.ProjectNamedAttributes(["name", "w", "g"])).add(1, ss.ProjectNamedAttributeAs("id", "rid")))

    def join(lhs_op):
        return ss.HashJoin(join_type, ss.ProjectNamedAttribute("fk"), ss.ProjectNamedAttribute("id"), proj, ss.UNIQUE, lhs_op, ss.ScanView(rview))
    run_both(join(ss.ScanView(lview)), gpu_ctx)                                     # materialised join, lhs order
    flt = ss.Filter(ss.Greater(NA("a"), ss.ConstInt64(499)), ss.ProjectAllAttributes(), ss.ScanView(lview))
    run_both(join(flt), gpu_ctx)                                                    # under a filter
    spec = (ss.AggregationSpecification().AddAggregation(ss.SUM, "w", "sw").AddAggregation(ss.COUNT, "name", "c")
            .AddAggregation(ss.MIN, "name", "mn").AddAggregation(ss.SUM, "L.v", "sv"))
    run_both(ss.ScalarAggregate(spec, join(flt)), gpu_ctx)                          # join -> aggregate, one kernel
    run_both(ss.GroupAggregate(ss.ProjectNamedAttributes(["g"]), spec, None,
                               ss.Filter(ss.IsNull(NA("w")), ss.ProjectAllAttributes(), join(ss.ScanView(lview)))), gpu_ctx, ignore_order=True)
    expr = ss.CompoundExpression().AddAs("x", ss.Plus(NA("L.v"), ss.IfNull(NA("w"), ss.ConstDouble(0.0)))).Add(NA("name"))
    run_both(ss.Compute(expr, join(ss.ScanView(lview))), gpu_ctx)                    # expressions over joined columns


@pytest.mark.parametrize("n,m", [(0, 5), (7, 0), (1025, 40), (30011, 300)])
@pytest.mark.parametrize("join_type", [ss.INNER, ss.LEFT_OUTER])
def test_hash_join_not_unique(gpu_ctx, n, m, join_type):
    # NOT_UNIQUE rhs keys multiply rows (hash_join_test.cc:240-300): rhs keys repeat (id2 has 3 values, id // 4
    # runs of up to 4), lhs order is kept and the matches of one lhs row come in rhs order
    lview, rview = _join_views(n, m)
    proj = (ss.CompoundMultiSourceProjector().add(0, ss.ProjectAllAttributes("L."))
            .add(1, ss.ProjectNamedAttributes(["name", "w", "g"])).add(1, ss.ProjectNamedAttributeAs("id", "rid")))
    narrow = ss.Filter(ss.Less(NA("a"), ss.ConstInt64(40)), ss.ProjectAllAttributes(), ss.ScanView(lview))   # ~4 % of the lhs: fk2 fans out m / 3 ways

    def join(lhs_op, lk="fk2", rk="id2"):
        return ss.HashJoin(join_type, ss.ProjectNamedAttribute(lk), ss.ProjectNamedAttribute(rk), proj, ss.NOT_UNIQUE, lhs_op, ss.ScanView(rview))
    run_both(join(narrow), gpu_ctx)
    # a NULLABLE INT64 key with NULLs on both sides and the EMPTY-sentinel value (-1); keys made to repeat
    rdup = ss.View(rview.schema(), [ss.Column(rview.column(0).data // 4, rview.column(0).is_null)] + [rview.column(i) for i in range(1, 5)])
    ldup = ss.View(lview.schema(), [ss.Column(lview.column(0).data // 4, lview.column(0).is_null)] + [lview.column(i) for i in range(1, 4)])
    op = ss.HashJoin(join_type, ss.ProjectNamedAttribute("fk"), ss.ProjectNamedAttribute("id"), proj, ss.NOT_UNIQUE, ss.ScanView(ldup), ss.ScanView(rdup))
    run_both(op, gpu_ctx)
    spec = (ss.AggregationSpecification().AddAggregation(ss.SUM, "w", "sw").AddAggregation(ss.COUNT, "name", "c")
            .AddAggregation(ss.MIN, "name", "mn").AddAggregation(ss.SUM, "L.v", "sv").AddAggregation(ss.COUNT, "", "n"))
    run_both(ss.ScalarAggregate(spec, op), gpu_ctx)                                   # the joined rows feed a new pipeline
    run_both(ss.GroupAggregate(ss.ProjectNamedAttributes(["g"]), spec, None, join(narrow)), gpu_ctx, ignore_order=True)
    # a UNIQUE-declared join below a NOT_UNIQUE one: the first stays fused in the lhs pipeline of the second
    inner = ss.HashJoin(ss.LEFT_OUTER, ss.ProjectNamedAttribute("fk"), ss.ProjectNamedAttribute("id"),
                        ss.CompoundMultiSourceProjector().add(0, ss.ProjectAllAttributes()).add(1, ss.ProjectNamedAttributeAs("g", "g1")),
                        ss.UNIQUE, narrow, ss.ScanView(rview))
    outer = ss.HashJoin(join_type, ss.ProjectNamedAttribute("fk2"), ss.ProjectNamedAttribute("id2"),
                        ss.CompoundMultiSourceProjector().add(0, ss.ProjectNamedAttributes(["fk", "g1", "v"])).add(1, ss.ProjectNamedAttributes(["w"])),
                        ss.NOT_UNIQUE, inner, ss.ScanView(rview))
    run_both(outer, gpu_ctx)


def test_hash_join_two_key_columns_and_errors(gpu_ctx):
    rng = np.random.default_rng(4)
    m, n = 200, 7000
    rs = ss.TupleSchema([ss.Attribute("x", ss.INT32), ss.Attribute("y", ss.INT32, ss.NULLABLE), ss.Attribute("name", ss.STRING)])
    ls = ss.TupleSchema([ss.Attribute("p", ss.INT32, ss.NULLABLE), ss.Attribute("q", ss.INT32), ss.Attribute("big", ss.INT64)])
    rview = ss.View(rs, [(np.arange(m) // 10).astype(np.int32), ss.Column((np.arange(m) % 10).astype(np.int32), np.arange(m) % 41 == 7), ["r%d" % i for i in range(m)]])
    lview = ss.View(ls, [ss.Column(rng.integers(-2, 24, n).astype(np.int32), rng.random(n) < 0.1), rng.integers(-1, 11, n).astype(np.int32), rng.integers(0, 5, n)])
    proj = ss.CompoundMultiSourceProjector().add(0, ss.ProjectAllAttributes()).add(1, ss.ProjectNamedAttributes(["name"]))
    for jt in (ss.INNER, ss.LEFT_OUTER):     # (x, y) is unique; NULL y rows can never match
        op = ss.HashJoin(jt, ss.ProjectNamedAttributes(["p", "q"]), ss.ProjectNamedAttributes(["x", "y"]), proj, ss.UNIQUE,
                         ss.ScanView(lview), ss.ScanView(rview))
        run_both(op, gpu_ctx)
    # key type mismatch is a bind error
    bad = ss.HashJoin(ss.INNER, ss.ProjectNamedAttribute("big"), ss.ProjectNamedAttribute("x"), proj, ss.UNIQUE, ss.ScanView(lview), ss.ScanView(rview))
    with pytest.raises(ss.SupersonicException):
        bad.CreateCursor(gpu_ctx)
    # duplicate rhs keys under a UNIQUE declaration are reported, not silently resolved
    dup = ss.HashJoin(ss.INNER, ss.ProjectNamedAttribute("q"), ss.ProjectNamedAttribute("x"), proj, ss.UNIQUE, ss.ScanView(lview), ss.ScanView(rview))
    r = dup.CreateCursor(gpu_ctx).Next(1024)
    assert r.is_failure()


@pytest.mark.parametrize("n,m", [(0, 5), (9, 0), (2049, 60), (30011, 700)])
@pytest.mark.parametrize("join_type", [ss.INNER, ss.LEFT_OUTER])
@pytest.mark.parametrize("uniq", [ss.UNIQUE, ss.NOT_UNIQUE])
def test_hash_join_keys_of_two_words(gpu_ctx, n, m, join_type, uniq):
    # keys that pack into 65..128 bits -- (INT64, STRING) as in hash_join_test.cc:305-382, (INT64, INT64), (INT32, INT64, BOOL):
    # a two-word index whose slots are claimed by row (ssgpu_join_build_kernel)
    rng = np.random.default_rng(n + m)
    words = np.array([b"", b"a", b"ab", b"b", b"zz"], dtype=object)
    rs = ss.TupleSchema([ss.Attribute("id", ss.INT64, ss.NULLABLE), ss.Attribute("tag", ss.STRING, ss.NULLABLE), ss.Attribute("id2", ss.INT64),
                         ss.Attribute("flag", ss.BOOL), ss.Attribute("small", ss.INT32), ss.Attribute("w", ss.DOUBLE)])
    ls = ss.TupleSchema([ss.Attribute("fk", ss.INT64, ss.NULLABLE), ss.Attribute("ftag", ss.STRING, ss.NULLABLE), ss.Attribute("fk2", ss.INT64),
                         ss.Attribute("fflag", ss.BOOL), ss.Attribute("fsmall", ss.INT32), ss.Attribute("v", ss.INT64)])
    # rhs: (id, tag), (id, id2) and (small, id2, flag) are unique when uniq == UNIQUE; values straddle 2^32 and include -1 / 0
    base = (np.arange(m, dtype=np.int64) // 5) * ((1 << 33) + 7) - 1
    if uniq == ss.NOT_UNIQUE:
        base = base // 3
    rview = ss.View(rs, [ss.Column(base, np.arange(m) % 19 == 4), ss.Column(words[np.arange(m) % 5], np.arange(m) % 23 == 7),
                         (np.arange(m, dtype=np.int64) % 5) * -(1 << 40), (np.arange(m) % 2).astype(bool), (np.arange(m) // 10).astype(np.int32),
                         rng.integers(-50, 50, m) * 0.5])
    pick = rng.integers(0, max(m, 1), n)
    hit = rng.random(n) < 0.7
    def like(col, miss):
        r = np.asarray(col)[pick] if m else np.zeros(n, dtype=np.asarray(miss).dtype)
        return np.where(hit, r, miss) if m else np.full(n, miss)
    lview = ss.View(ls, [ss.Column(like(rview.column(0).data, np.int64(12345)).astype(np.int64), rng.random(n) < 0.08),
                         ss.Column(np.array(list(like(rview.column(1).data, b"q")), dtype=object) if n else np.zeros(0, dtype=object), rng.random(n) < 0.08),
                         like(rview.column(2).data, np.int64(3)).astype(np.int64), like(rview.column(3).data, False).astype(bool),
                         like(rview.column(4).data, np.int32(-7)).astype(np.int32), rng.integers(0, 1000, n)])
    proj = (ss.CompoundMultiSourceProjector().add(0, ss.ProjectAllAttributes("L.")).add(1, ss.ProjectNamedAttributes(["w", "tag", "id"])))
    for lk, rk in ((["fk", "ftag"], ["id", "tag"]), (["fk", "fk2"], ["id", "id2"]), (["fsmall", "fk2", "fflag"], ["small", "id2", "flag"])):
        op = ss.HashJoin(join_type, ss.ProjectNamedAttributes(lk), ss.ProjectNamedAttributes(rk), proj, uniq, ss.ScanView(lview), ss.ScanView(rview))
        run_both(op, gpu_ctx)
        spec = ss.AggregationSpecification().AddAggregation(ss.SUM, "w", "sw").AddAggregation(ss.COUNT, "tag", "c").AddAggregation(ss.COUNT, "", "n")
        run_both(ss.ScalarAggregate(spec, op), gpu_ctx)


@pytest.mark.parametrize("join_type", [ss.INNER, ss.LEFT_OUTER])
def test_filters_above_a_join_are_evaluated_ahead_of_the_probe(gpu_ctx, join_type):
    # a Filter written above the join that reads only lhs columns is evaluated first and its rows are not probed (lower.cpp:
    # join_index) -- invisible in the result, also with NULL predicates, LEFT_OUTER NULL padding and filters on both sides
    lview, rview = _join_views(30011, 300)
    proj = (ss.CompoundMultiSourceProjector().add(0, ss.ProjectAllAttributes("L.")).add(1, ss.ProjectNamedAttributes(["name", "w", "g"])))
    join = lambda lhs: ss.HashJoin(join_type, ss.ProjectNamedAttribute("fk"), ss.ProjectNamedAttribute("id"), proj, ss.UNIQUE, lhs, ss.ScanView(rview))
    below = ss.Filter(ss.Less(NA("a"), ss.ConstInt64(700)), ss.ProjectAllAttributes(), ss.ScanView(lview))
    above = ss.Filter(ss.Greater(NA("L.fk"), ss.ConstInt64(10)), ss.ProjectAllAttributes(), join(below))           # NULLABLE predicate
    run_both(above, gpu_ctx)
    both = ss.Filter(ss.Or(ss.IsNull(NA("w")), ss.Less(NA("w"), ss.ConstDouble(20.0))), ss.ProjectAllAttributes(), above)   # reads the join: stays behind it
    run_both(both, gpu_ctx)
    spec = ss.AggregationSpecification().AddAggregation(ss.SUM, "w", "sw").AddAggregation(ss.COUNT, "name", "c").AddAggregation(ss.COUNT, "", "n")
    run_both(ss.ScalarAggregate(spec, above), gpu_ctx)
    run_both(ss.GroupAggregate(ss.ProjectNamedAttributes(["g"]), spec, None, both), gpu_ctx, ignore_order=True)


def test_a_failing_expression_keeps_filters_behind_the_probe(gpu_ctx):
    # The reference evaluates Compute(1000 / w) on EVERY joined row before the Filter above it sees them: a zero w on a row that
    # filter would drop is still an evaluation error.  Probing fewer rows must not hide it.
    ls = ss.TupleSchema([ss.Attribute("fk", ss.INT64), ss.Attribute("a", ss.INT64)])
    rs = ss.TupleSchema([ss.Attribute("id", ss.INT64), ss.Attribute("w", ss.INT64)])
    n = 5000
    lview = ss.View(ls, [np.arange(n) % 50, np.arange(n)])
    proj = ss.CompoundMultiSourceProjector().add(0, ss.ProjectAllAttributes()).add(1, ss.ProjectNamedAttributes(["w"]))

    def query(w):
        rview = ss.View(rs, [np.arange(50), w])
        j = ss.HashJoin(ss.INNER, ss.ProjectNamedAttribute("fk"), ss.ProjectNamedAttribute("id"), proj, ss.UNIQUE, ss.ScanView(lview), ss.ScanView(rview))
        e = ss.CompoundExpression().Add(NA("a")).AddAs("q", ss.DivideSignaling(ss.ConstInt64(1000), NA("w")))
        return ss.Filter(ss.Less(NA("a"), ss.ConstInt64(10)), ss.ProjectAllAttributes(), ss.Compute(e, j))
    ok = np.arange(50) + 1
    run_both(query(ok), gpu_ctx)
    bad = ok.copy(); bad[40] = 0           # fk == 40 first occurs at a == 40: a row the filter drops
    r = query(bad).CreateCursor(gpu_ctx).Next(1024)
    assert r.is_failure() and r.exception().return_code == 104


def test_hash_join_wide_key_errors(gpu_ctx):
    s3 = ss.TupleSchema([ss.Attribute("a", ss.INT64), ss.Attribute("b", ss.INT64), ss.Attribute("c", ss.INT64)])
    v = ss.View(s3, [np.arange(4), np.arange(4), np.arange(4)])
    proj = ss.CompoundMultiSourceProjector().add(0, ss.ProjectAllAttributes("L.")).add(1, ss.ProjectAllAttributes("R."))
    three = ss.HashJoin(ss.INNER, ss.ProjectNamedAttributes(["a", "b", "c"]), ss.ProjectNamedAttributes(["a", "b", "c"]), proj, ss.UNIQUE, ss.ScanView(v), ss.ScanView(v))
    with pytest.raises(ss.SupersonicException) as e:      # three words: refused loudly, never computed elsewhere
        three.CreateCursor(gpu_ctx)
    assert e.value.return_code == 103          # ERROR_NOT_IMPLEMENTED
    # duplicate two-word keys under a UNIQUE declaration are reported
    d = ss.View(s3, [np.array([1, 1, 2, 2]), np.array([5, 5, 6, 7]), np.arange(4)])
    dup = ss.HashJoin(ss.INNER, ss.ProjectNamedAttributes(["a", "b"]), ss.ProjectNamedAttributes(["a", "b"]), proj, ss.UNIQUE, ss.ScanView(v), ss.ScanView(d))
    assert dup.CreateCursor(gpu_ctx).Next(1024).is_failure()


def test_signaling_division_fails_only_on_selected_rows(gpu_ctx):
    n = 5000
    view = make_view(n)
    # k2 == 0 exists; dividing over all rows must fail ...
    op = ss.Compute(ss.DivideSignaling(NA("d1"), NA("k2")), ss.ScanView(view))
    r = op.CreateCursor(gpu_ctx).Next(1024)
    assert r.is_failure() and r.exception().return_code == 104
    # ... but not when the zero divisors are filtered out first
    op = ss.Compute(ss.DivideSignaling(NA("d1"), NA("k2")),
                    ss.Filter(ss.Greater(NA("k2"), ss.ConstInt32(0)), ss.ProjectAllAttributes(), ss.ScanView(view)))
    run_both(op, gpu_ctx)


def test_evaluation_error_is_ordered_behind_the_run(gpu_ctx):
    # The error word is written by kernels on the context's (non-blocking) stream; reading it must be ordered
    # behind the run that sets or clears it, also when that run is long and the only failing row is the last.
    n = 12_000_000
    a = np.arange(n, dtype=np.int64)
    b_ok = np.ones(n, dtype=np.int64)
    b_bad = b_ok.copy(); b_bad[-1] = 0
    schema = ss.TupleSchema([ss.Attribute("a", ss.INT64, ss.NOT_NULLABLE), ss.Attribute("b", ss.INT64, ss.NOT_NULLABLE)])
    spec = ss.AggregationSpecification().AddAggregation(ss.SUM, "q", "s")
    for _ in range(4):
        for b, fails in ((b_bad, True), (b_ok, False)):
            view = ss.View(schema, [a, b])
            op = ss.ScalarAggregate(spec, ss.Compute(ss.CompoundExpression().AddAs("q", ss.DivideSignaling(NA("a"), NA("b"))),
                                                     ss.ScanView(view)))
            r = op.CreateCursor(gpu_ctx).Next(16)
            if fails:
                assert r.is_failure() and r.exception().return_code == 104
            else:
                assert not r.is_failure() and r.view().column(0).data[0] == float(n) * (n - 1) / 2


def test_chained_stages(gpu_ctx):
    # Compute over a GroupAggregate result: two pipeline stages
    view = make_view(20000)
    grouped = group_query(view, True)
    op = ss.Compute(ss.CompoundExpression().Add(NA("k1")).Add(NA("k2")).AddAs("range", ss.Minus(NA("max_d0"), NA("min_d0"))), grouped)
    run_both(op, gpu_ctx, ignore_order=True)


# ---- Sort (cursor/core/sort.cc): unique trailing key -> the order is fully determined ----------
def sort_view(n, nullable):
    rng = np.random.default_rng(7)
    N = ss.NULLABLE if nullable else ss.NOT_NULLABLE
    schema = ss.TupleSchema([ss.Attribute("k", ss.INT64, N), ss.Attribute("g", ss.INT32, N), ss.Attribute("x", ss.DOUBLE, N),
                             ss.Attribute("f", ss.FLOAT), ss.Attribute("u", ss.UINT32), ss.Attribute("t", ss.BOOL),
                             ss.Attribute("id", ss.INT64)])

    def nl():
        return (rng.random(n) < 0.1) if nullable else None
    cols = [ss.Column(rng.integers(-(1 << 62), 1 << 62, n), nl()), ss.Column(rng.integers(-50, 50, n), nl()),
            ss.Column(rng.integers(-1000, 1000, n) * 0.5, nl()), (rng.integers(-100, 100, n) * 0.25).astype(np.float32),
            rng.integers(0, 1 << 32, n).astype(np.uint32), rng.integers(0, 2, n).astype(bool), rng.permutation(n)]
    return ss.View(schema, cols)


SORT_ORDERS = [
    [("k", ss.ASCENDING), ("id", ss.ASCENDING)],
    [("g", ss.DESCENDING), ("id", ss.ASCENDING)],
    [("g", ss.ASCENDING), ("x", ss.DESCENDING), ("id", ss.DESCENDING)],
    [("f", ss.ASCENDING), ("t", ss.DESCENDING), ("u", ss.ASCENDING), ("id", ss.ASCENDING)],
]


@pytest.mark.parametrize("n", [0, 1, 65, 4095, 4096, 4097, 100003])
@pytest.mark.parametrize("order", range(len(SORT_ORDERS)))
@pytest.mark.parametrize("nullable", [False, True])
def test_sort(gpu_ctx, n, order, nullable):
    so = ss.SortOrder()
    for name, o in SORT_ORDERS[order]:
        so.add(name, o)
    run_both(ss.Sort(so, ss.ProjectAllAttributes(), 0, ss.ScanView(sort_view(n, nullable))), gpu_ctx)


def test_sort_after_filter_with_projection(gpu_ctx):
    view = sort_view(50000, True)
    so = ss.SortOrder().add("k", ss.DESCENDING).add("id", ss.ASCENDING)
    child = ss.Filter(ss.Greater(NA("g"), ss.ConstInt32(0)), ss.ProjectAllAttributes(), ss.ScanView(view))
    run_both(ss.Sort(so, ss.ProjectNamedAttributes(["id", "k", "x"]), 0, child), gpu_ctx)


def test_sort_then_group(gpu_ctx):
    # Sort over a GroupAggregate result (the reference's group_sort guide example shape)
    view = make_view(30000)
    grouped = group_query(view, False)
    so = ss.SortOrder().add("k1", ss.ASCENDING).add("k2", ss.DESCENDING)
    run_both(ss.Sort(so, ss.ProjectAllAttributes(), 0, grouped), gpu_ctx)


# ---- AggregateClusters (cursor/core/aggregate_clusters.cc) ---------------------------------------
@pytest.mark.parametrize("n", [0, 1, 2, 511, 512, 513, 10001, 100003])
@pytest.mark.parametrize("nullable", [False, True])
def test_aggregate_clusters(gpu_ctx, n, nullable):
    rng = np.random.default_rng(11)
    N = ss.NULLABLE if nullable else ss.NOT_NULLABLE
    # runs of random length 1..9 with a key that changes at every run boundary (keys may repeat later)
    key = np.cumsum(rng.integers(0, 9, n) == 0) % 13 if n else np.zeros(0, np.int64)
    key2 = (np.arange(n) // 1000).astype(np.int32)
    schema = ss.TupleSchema([ss.Attribute("k", ss.INT64, N), ss.Attribute("k2", ss.INT32), ss.Attribute("v", ss.INT64, N),
                             ss.Attribute("d", ss.DOUBLE)])
    knull = (key % 5 == 0) if nullable else None      # whole runs NULL: NULL keys cluster together
    vnull = (rng.random(n) < 0.2) if nullable else None
    view = ss.View(schema, [ss.Column(key, knull), key2, ss.Column(rng.integers(-100, 100, n), vnull), rng.integers(0, 64, n) * 0.5])
    spec = (ss.AggregationSpecification().AddAggregation(ss.SUM, "v", "sv").AddAggregation(ss.MIN, "v", "mn")
            .AddAggregation(ss.MAX, "d", "mx").AddAggregation(ss.SUM, "d", "sd").AddAggregation(ss.COUNT, "v", "cv")
            .AddAggregation(ss.COUNT, "", "n"))
    run_both(ss.AggregateClusters(ss.ProjectNamedAttributes(["k", "k2"]), spec, ss.ScanView(view)), gpu_ctx)


@pytest.mark.parametrize("n", [0, 1, 2, 513, 10001, 100003])
@pytest.mark.parametrize("nullable", [False, True])
def test_aggregate_clusters_with_distinct_aggregates(gpu_ctx, n, nullable):
    # DISTINCT aggregates of clusters (Aggregator::Create, aggregator.cc:88-101, serves AggregateClusters as every aggregating
    # cursor; a cluster is always aggregated inside one ProcessInput call, aggregate_clusters.cc:436-520): the DISTINCT shape with
    # the cluster's number as the sort key -- equal keys of different clusters stay apart, the clusters keep their input order.
    # Long runs (many repeats of few values), one and two DISTINCT columns, FIRST / LAST next to them, below a Filter / Compute.
    rng = np.random.default_rng(12)
    N = ss.NULLABLE if nullable else ss.NOT_NULLABLE
    key = np.cumsum(rng.integers(0, 40, n) == 0) % 7 if n else np.zeros(0, np.int64)      # runs of ~40 rows; 7 keys that come back
    schema = ss.TupleSchema([ss.Attribute("k", ss.INT64, N), ss.Attribute("v", ss.INT64, N), ss.Attribute("w", ss.INT32), ss.Attribute("d", ss.DOUBLE)])
    knull = (key % 5 == 0) if nullable else None
    vnull = (rng.random(n) < 0.2) if nullable else None
    view = ss.View(schema, [ss.Column(key, knull), ss.Column(rng.integers(-6, 6, n), vnull), rng.integers(0, 5, n).astype(np.int32), rng.integers(0, 8, n) * 0.5])
    spec = (ss.AggregationSpecification().AddDistinctAggregation(ss.SUM, "v", "sdv").AddDistinctAggregation(ss.COUNT, "v", "cdv").AddAggregation(ss.SUM, "v", "sv")
            .AddAggregation(ss.COUNT, "", "n").AddAggregation(ss.MAX, "d", "mx"))
    run_both(ss.AggregateClusters(ss.ProjectNamedAttributes(["k"]), spec, ss.ScanView(view)), gpu_ctx)
    spec.AddDistinctAggregation(ss.COUNT, "w", "cdw").AddDistinctAggregation(ss.SUM, "d", "sdd").AddAggregation(ss.FIRST, "v", "fv").AddAggregation(ss.LAST, "d", "ld")
    run_both(ss.AggregateClusters(ss.ProjectNamedAttributes(["k"]), spec, ss.ScanView(view)), gpu_ctx)
    # below a Filter and a Compute (the pipeline is flushed first), and a consumer above (the segment id is projected away)
    e = ss.CompoundExpression().Add(NA("k")).Add(NA("v")).AddAs("w", ss.Plus(NA("w"), ss.ConstInt32(1))).Add(NA("d"))
    child = ss.Compute(e, ss.Filter(ss.Less(NA("d"), ss.ConstDouble(3.0)), ss.ProjectAllAttributes(), ss.ScanView(view)))
    agg = ss.AggregateClusters(ss.ProjectNamedAttributes(["k"]), spec, child)
    run_both(agg, gpu_ctx)
    run_both(ss.ScalarAggregate(ss.AggregationSpecification().AddAggregation(ss.SUM, "sdv", "t").AddAggregation(ss.COUNT, "k", "c").AddAggregation(ss.SUM, "cdw", "u"), agg), gpu_ctx)
    # WITHOUT a clustering column the whole input is one cluster (aggregate_clusters_test.cc:105-121): the stage still stores a
    # segment number -- of zero key columns (round 5: the derived golden case of this shape met an unset column pointer)
    run_both(ss.AggregateClusters(ss.CompoundSingleSourceProjector(), spec, ss.ScanView(view)), gpu_ctx)
    run_both(ss.AggregateClusters(ss.CompoundSingleSourceProjector(), spec, child), gpu_ctx)


@pytest.mark.parametrize("n", [0, 1, 1025, 100003])
def test_date_and_datetime(gpu_ctx, n):
    # DATE (days, INT32) / DATETIME (microseconds, INT64): the DATE -> DATETIME cast multiplies by the
    # microseconds of a day (cast_bound_expression.cc:129-136); IFNULL / IF / CASE promote DATE to DATETIME through it,
    # comparisons of the two need the explicit cast (comparison_bound_expressions.cc:613)
    rng = np.random.default_rng(3)
    schema = ss.TupleSchema([ss.Attribute("day", ss.DATE, ss.NULLABLE), ss.Attribute("ts", ss.DATETIME), ss.Attribute("v", ss.INT64)])
    view = ss.View(schema, [ss.Column(rng.integers(-20000, 20000, n).astype(np.int32), rng.random(n) < 0.1),
                            rng.integers(-20000, 20000, n) * 86400000000 + rng.integers(0, 86400000000, n), rng.integers(0, 1000, n)])
    e = (ss.CompoundExpression().AddAs("dt", ss.CastTo(ss.DATETIME, NA("day"))).AddAs("before", ss.Less(ss.CastTo(ss.DATETIME, NA("day")), NA("ts")))
         .AddAs("filled", ss.IfNull(NA("day"), NA("ts"))).AddAs("c", ss.CastTo(ss.DATETIME, ss.ConstDate(14600))).Add(NA("v")))
    run_both(ss.Compute(e, ss.ScanView(view)), gpu_ctx)
    spec = ss.AggregationSpecification().AddAggregation(ss.MIN, "ts", "first_ts").AddAggregation(ss.MAX, "dt", "last_day").AddAggregation(ss.SUM, "v", "s")
    q = ss.GroupAggregate(ss.ProjectNamedAttributes(["before"]), spec, None,
                          ss.Compute(ss.CompoundExpression().AddAs("dt", ss.CastTo(ss.DATETIME, NA("day"))).AddAs("before", ss.Less(ss.CastTo(ss.DATETIME, NA("day")), NA("ts"))).Add(NA("ts")).Add(NA("v")),
                                     ss.ScanView(view)))
    run_both(q, gpu_ctx, ignore_order=True)


@pytest.mark.parametrize("descending", [False, True])
def test_sample_sort_range_filters(gpu_ctx, descending):
    # the per-destination range Filters of supersonic_amd.distributed.sharded_sort (the N > 1 Sort) on the device:
    # parity with the oracle, and every row lands on exactly one of 4 ranks
    from supersonic_amd.distributed import _range_predicate
    view = make_view(100003, nullable=True)
    total = 0
    for d in range(4):
        pred = _range_predicate("a", ss.INT64, True, [120, 500, 500], d, 4, descending)
        op = ss.Filter(pred, ss.ProjectNamedAttributes(["a", "d", "d0"]), ss.ScanView(view))
        run_both(op, gpu_ctx)
        total += ss.drain(op.CreateCursor(gpu_ctx), 1 << 20).row_count()
    assert total == 100003


@pytest.mark.parametrize("descending", [False, True])
def test_device_sharded_sort_single_rank_exchange(descending):
    # the device-resident sample sort (local sort -> range Filters -> RCCL all_to_all_single over the plans' own
    # result buffers -> local sort) with the exchange forced on a 1-rank process group
    import socket
    import torch
    import torch.distributed as dist
    from supersonic_amd.distributed import device_sharded_sort
    s = socket.socket(); s.bind(("127.0.0.1", 0)); port = s.getsockname()[1]; s.close()
    os.environ["MASTER_ADDR"] = "127.0.0.1"; os.environ["MASTER_PORT"] = str(port)
    torch.cuda.set_device(0)
    dist.init_process_group("nccl", rank=0, world_size=1)
    try:
        ctx = ss.Context(0)
        view = make_view(100003, nullable=True)
        so = ss.SortOrder().add("a", ss.DESCENDING if descending else ss.ASCENDING).add("k2", ss.ASCENDING)
        plan, _dv = device_sharded_sort(ctx, so, view, always_exchange=True)
        got = plan.fetch()
        _schema, want = oracle_run(ss.Sort(so, None, 0, ss.ScanView(view)))
        assert_cols_equal([(got.column(i).data, got.column(i).is_null) for i in range(got.column_count())], want, context="device sharded sort")
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("fused", [False, True])
@pytest.mark.parametrize("n,shards", [(100003, 3), (2000, 4), (5, 3)])
def test_partial_state_fold_across_shards(gpu_ctx, n, shards, fused):
    # the N > 1 ScalarAggregate protocol on one GPU: every shard runs ssgpu_plan_run_partial with its global row
    # offset, the shards' partial states are laid out as an all-gather would (consecutive images), folded with
    # ssgpu_plan_fold_partials and finalised -- the result must be the single-plan answer (FIRST / LAST included)
    import torch
    from supersonic_amd.distributed import _bytes_over
    view = make_view(n, nullable=True)
    bounds = [n * i // shards for i in range(shards + 1)]
    bounds[1] = bounds[0]                                   # an empty shard
    spec = (ss.AggregationSpecification().AddAggregation(ss.SUM, "a", "sa").AddAggregation(ss.SUM, "d0", "sd").AddAggregation(ss.MIN, "d", "mn")
            .AddAggregation(ss.MAX, "d0", "mx").AddAggregation(ss.MIN, "f", "mf").AddAggregation(ss.COUNT, "k1", "c").AddAggregation(ss.COUNT, "", "n")
            .AddAggregation(ss.FIRST, "d", "fd").AddAggregation(ss.LAST, "k1", "lk"))

    def query(v):
        return ss.ScalarAggregate(spec, ss.Filter(ss.Greater(NA("b"), ss.ConstInt64(300)), ss.ProjectAllAttributes(), ss.ScanView(v)))
    device = torch.device("cuda", 0)
    plans, images = [], []
    for i in range(shards):
        lo, hi = bounds[i], bounds[i + 1]
        shard = ss.View(view.schema(), [ss.Column(view.column(c).data[lo:hi], None if view.column(c).is_null is None else view.column(c).is_null[lo:hi])
                                        for c in range(view.column_count())])
        plan = ss.Plan(query(shard), gpu_ctx)
        segs = plan.run_partial(shard, lo)
        gpu_ctx.synchronize()
        total = sum(count for (_p, count, _d, _r) in segs)
        images.append(_bytes_over(torch, device, segs[0][0], total * 8).clone())
        plans.append(plan)
    gathered = torch.cat(images)
    torch.cuda.synchronize()
    if fused:                                               # ssgpu_plan_fold_finalize: the same two steps as one launch
        plans[0].fold_finalize(gathered.data_ptr(), shards)
    else:
        plans[0].fold_partials(gathered.data_ptr(), shards)
        plans[0].finalize()
    got = plans[0].fetch()
    _schema, want = oracle_run(query(view))
    assert_cols_equal([(got.column(i).data, got.column(i).is_null) for i in range(got.column_count())], want, context="folded partial state")


@pytest.mark.parametrize("n,with_filter", [(100003, True), (2000, False), (0, False)])
def test_device_sharded_group_aggregate_single_rank(n, with_filter):
    # BASELINE config #4's protocol with the tables staying in HBM (per-shard GroupAggregate -> RCCL all-gather of the
    # plan's own result buffers -> merge plan), on a 1-rank process group
    import socket
    import torch
    import torch.distributed as dist
    from supersonic_amd.distributed import device_sharded_group_aggregate
    s = socket.socket(); s.bind(("127.0.0.1", 0)); port = s.getsockname()[1]; s.close()
    os.environ["MASTER_ADDR"] = "127.0.0.1"; os.environ["MASTER_PORT"] = str(port)
    torch.cuda.set_device(0)
    dist.init_process_group("nccl", rank=0, world_size=1)
    try:
        ctx = ss.Context(0)
        view = make_view(n, nullable=True)
        spec = (ss.AggregationSpecification().AddAggregation(ss.SUM, "a", "sa").AddAggregation(ss.MIN, "d0", "mn").AddAggregation(ss.MAX, "d1", "mx")
                .AddAggregation(ss.COUNT, "d0", "c").AddAggregation(ss.COUNT, "", "n").AddAggregation(ss.FIRST, "d", "fd"))
        child = ss.ScanView(view)
        if with_filter:
            child = ss.Filter(ss.Greater(NA("b"), ss.ConstInt64(499)), ss.ProjectAllAttributes(), child)
        plan, _dv = device_sharded_group_aggregate(ctx, ["k2", "t"], spec, child)
        assert plan._sharded_job.collectives == 1          # ONE all-gather of the packed partial tables per step
        got = plan.fetch()
        schema, want = oracle_run(ss.GroupAggregate(ss.ProjectNamedAttributes(["k2", "t"]), spec, None, child))
        gs = plan.result_schema
        assert [(gs.attribute(i).name(), gs.attribute(i).type(), gs.attribute(i).is_nullable()) for i in range(gs.attribute_count())] == [tuple(x) for x in schema]
        assert_cols_equal(sort_rows([(got.column(i).data, got.column(i).is_null) for i in range(got.column_count())]), sort_rows(want),
                          context="device sharded group aggregate")
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("exchange", ["all_gather", "key_range"])
def test_device_sharded_group_aggregate_skips_nans_in_float_min_max(exchange):
    # A NaN in a floating MIN / MAX column sets the stage's NaN bit next to its evaluation-error code (SSGPU_FLAG_NAN_IN_MINMAX).
    # The bit is no error: it must not travel in the image headers as one (round 3's headers carried the raw word and a
    # sharded job with a NaN anywhere failed with ERROR_EVALUATION_ERROR).  Across shards NaNs are skipped (ssgpu.h); with no
    # NaN as a group's first value that is the reference's answer too, so the oracle is the check.  Merge large enough for
    # the partitioned merge shape as well (>= 64 K rows of images).
    import socket
    import torch
    import torch.distributed as dist
    from supersonic_amd.distributed import DeviceShardedGroupAggregate
    s = socket.socket(); s.bind(("127.0.0.1", 0)); port = s.getsockname()[1]; s.close()
    os.environ["MASTER_ADDR"] = "127.0.0.1"; os.environ["MASTER_PORT"] = str(port)
    torch.cuda.set_device(0)
    dist.init_process_group("nccl", rank=0, world_size=1)
    try:
        ctx = ss.Context(0)
        rng = np.random.default_rng(77)
        n = 400003
        k = rng.integers(0, 90000, n).astype(np.int32)
        x = rng.integers(-1000, 1000, n) * 0.5
        first_of_group = np.zeros(n, bool)
        first_of_group[np.unique(k, return_index=True)[1]] = True
        x[(rng.random(n) < 0.05) & ~first_of_group] = np.nan          # NaNs, never as a group's first value
        f = x.astype(np.float32)
        schema = ss.TupleSchema([ss.Attribute("k", ss.INT32), ss.Attribute("x", ss.DOUBLE), ss.Attribute("f", ss.FLOAT)])
        view = ss.View(schema, [k, x, f])
        spec = (ss.AggregationSpecification().AddAggregation(ss.MIN, "x", "mn").AddAggregation(ss.MAX, "x", "mx").AddAggregation(ss.MAX, "f", "mf")
                .AddAggregation(ss.COUNT, "", "n"))
        job = DeviceShardedGroupAggregate(ctx, ["k"], spec, ss.ScanView(view), exchange=exchange)
        for _ in range(4):                                                  # the steady (lazily checked) steps too
            job.step()
            while not job.check():                                          # raises on an (alleged) evaluation error
                job.step()
        got = job.result()[0].fetch()
        _schema, want = oracle_run(ss.GroupAggregate(ss.ProjectNamedAttributes(["k"]), spec, None, ss.ScanView(view)))
        assert_cols_equal(sort_rows(to_cols(got)), sort_rows(want), context="sharded MIN / MAX over a column with NaNs (%s)" % exchange)
    finally:
        dist.destroy_process_group()


def test_device_sharded_jobs_carry_string_columns():
    # STRING group keys / MIN / MAX results and STRING sort payloads cross shards as the INT32 codes of ONE job-wide
    # dictionary (distributed.job_strings); exchange forced on a 1-rank process group
    import socket
    import torch
    import torch.distributed as dist
    from supersonic_amd.distributed import device_sharded_group_aggregate, device_sharded_sort
    s = socket.socket(); s.bind(("127.0.0.1", 0)); port = s.getsockname()[1]; s.close()
    os.environ["MASTER_ADDR"] = "127.0.0.1"; os.environ["MASTER_PORT"] = str(port)
    torch.cuda.set_device(0)
    dist.init_process_group("nccl", rank=0, world_size=1)
    try:
        ctx = ss.Context(0)
        rng = np.random.default_rng(4)
        n = 20011
        words = [b"pear", b"apple", b"fig", b"", b"kiwi\x00k", b"zebra", b"apple pie"]
        schema = ss.TupleSchema([ss.Attribute("name", ss.STRING, ss.NULLABLE), ss.Attribute("v", ss.INT64), ss.Attribute("tag", ss.STRING)])
        names = np.empty(n, dtype=object); names[:] = [words[i] for i in rng.integers(0, len(words), n)]
        tags = np.empty(n, dtype=object); tags[:] = [words[i] for i in rng.integers(0, len(words), n)]
        view = ss.View(schema, [ss.Column(names, rng.random(n) < 0.1), rng.integers(-50, 50, n), tags])
        spec = (ss.AggregationSpecification().AddAggregation(ss.SUM, "v", "sv").AddAggregation(ss.MIN, "tag", "lo")
                .AddAggregation(ss.MAX, "tag", "hi").AddAggregation(ss.COUNT, "", "n"))
        child = ss.Filter(ss.NotEqual(NA("tag"), ss.ConstString("fig")), ss.ProjectAllAttributes(), ss.ScanView(view))
        plan, _dv = device_sharded_group_aggregate(ctx, ["name"], spec, child)
        got = plan.fetch()
        _schema, want = oracle_run(ss.GroupAggregate(ss.ProjectNamedAttributes(["name"]), spec, None, child))
        assert_cols_equal(sort_rows(to_cols(got)), sort_rows(want), context="device sharded group aggregate, STRING key")
        so = ss.SortOrder().add("v", ss.ASCENDING).add("name", ss.DESCENDING)
        plan, _dv = device_sharded_sort(ctx, so, view, always_exchange=True)
        _schema, want = oracle_run(ss.Sort(so, None, 0, ss.ScanView(view)))
        sorted_view = plan.fetch()
        # ties on (v, name) keep their input order on the device (stable) but not in the oracle's qsort: compare the keys
        # in order and the rows as a multiset
        assert_cols_equal(to_cols(sorted_view)[:2], want[:2], context="device sharded sort, STRING second key")
        assert_cols_equal(sort_rows(to_cols(sorted_view)), sort_rows(want), context="device sharded sort, STRING payload")
    finally:
        dist.destroy_process_group()


def test_device_sharded_group_aggregate_regrows_its_images():
    # an image capacity the partial table outgrows: truncated + flagged in the header, check() regrows, the repeat is right;
    # steady-state steps reuse the merge plan and issue exactly one collective
    import socket
    import torch
    import torch.distributed as dist
    from supersonic_amd.distributed import DeviceShardedGroupAggregate
    s = socket.socket(); s.bind(("127.0.0.1", 0)); port = s.getsockname()[1]; s.close()
    os.environ["MASTER_ADDR"] = "127.0.0.1"; os.environ["MASTER_PORT"] = str(port)
    torch.cuda.set_device(0)
    dist.init_process_group("nccl", rank=0, world_size=1)
    try:
        ctx = ss.Context(0)
        view = make_view(50021, nullable=False)
        spec = (ss.AggregationSpecification().AddAggregation(ss.SUM, "d0", "s").AddAggregation(ss.MIN, "d1", "mn")
                .AddAggregation(ss.MAX, "d0", "mx").AddAggregation(ss.COUNT, "", "n"))
        child = ss.ScanView(view)
        job = DeviceShardedGroupAggregate(ctx, ["c"], spec, child, capacity_rows=1024)   # `c` has far more than 1024 groups
        job.step()
        assert not job.check() and job.capacity > 1024
        first_merge = None
        for _ in range(3):
            merge = job.step()
            assert job.collectives == 1
            first_merge = first_merge or merge
            assert merge is first_merge
        assert job.check()
        got = job.result()[0].fetch()
        _schema, want = oracle_run(ss.GroupAggregate(ss.ProjectNamedAttributes(["c"]), spec, None, child))
        assert_cols_equal(sort_rows([(got.column(i).data, got.column(i).is_null) for i in range(got.column_count())]), sort_rows(want),
                          context="regrown images")
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("descending", [False, True])
def test_sort_negative_zero_ties_keep_their_order(gpu_ctx, descending):
    # -0.0 and +0.0 compare equal in the reference (ThreeWayCompare): a stable sort must not separate them
    rng = np.random.default_rng(12)
    n = 20011
    pool = np.array([-0.0, 0.0, -1.5, 2.25, 0.0, -0.0, 7.0])
    d = pool[rng.integers(0, len(pool), n)]
    f = d.astype(np.float32)
    schema = ss.TupleSchema([ss.Attribute("d", ss.DOUBLE), ss.Attribute("f", ss.FLOAT, ss.NULLABLE), ss.Attribute("id", ss.INT64)])
    view = ss.View(schema, [d, ss.Column(f, rng.random(n) < 0.05), np.arange(n)])
    order = ss.DESCENDING if descending else ss.ASCENDING
    run_both(ss.Sort(ss.SortOrder().add("d", order), None, 0, ss.ScanView(view)), gpu_ctx)
    run_both(ss.Sort(ss.SortOrder().add("f", order), None, 0, ss.ScanView(view)), gpu_ctx)


@pytest.mark.parametrize("n", [0, 1, 4097, 100003])
@pytest.mark.parametrize("descending", [False, True])
def test_sort_key_column_read_back_from_the_sorted_keys(gpu_ctx, n, descending):
    # the major key's column comes from the sorted radix keys when that is lossless (integer, no NULLs): alone
    # (keys-only sort, no row ids), next to payload columns, as the first of two keys, and not at all for a
    # key with NULLs or a floating-point key
    view = make_view(n, nullable=False)
    order = ss.DESCENDING if descending else ss.ASCENDING
    for key in ("d", "k2", "u"):
        run_both(ss.Sort(ss.SortOrder().add(key, order), ss.ProjectNamedAttributes([key]), 0, ss.ScanView(view)), gpu_ctx)
        run_both(ss.Sort(ss.SortOrder().add(key, order), ss.ProjectNamedAttributes(["a", key, "d0"]), 0, ss.ScanView(view)), gpu_ctx)
    run_both(ss.Sort(ss.SortOrder().add("k2", order).add("a", ss.ASCENDING), ss.ProjectNamedAttributes(["k2", "a", "c"]), 0, ss.ScanView(view)), gpu_ctx)
    nullable = make_view(n, nullable=True)
    run_both(ss.Sort(ss.SortOrder().add("d", order), ss.ProjectNamedAttributes(["d"]), 0, ss.ScanView(nullable)), gpu_ctx)
    run_both(ss.Sort(ss.SortOrder().add("d1", order), ss.ProjectNamedAttributes(["d1"]), 0, ss.ScanView(view)), gpu_ctx)


LIBM_ULP = 4   # device libm vs the host's (the reference calls glibc): tolerance of the libm family, DESIGN section 4


@pytest.mark.parametrize("n", [0, 1, 513, 100003])
def test_libm_family_within_a_few_ulp(gpu_ctx, n):
    # EXP / LN / LOG10 / LOG2 / LOG / POW / trigonometric / hyperbolic functions (math_expressions.h:30-140): the NULL and
    # failure rules are exact, the values agree with the host libm within LIBM_ULP units in the last place
    rng = np.random.default_rng(21)
    schema = ss.TupleSchema([ss.Attribute("x", ss.DOUBLE, ss.NULLABLE), ss.Attribute("u", ss.DOUBLE), ss.Attribute("p", ss.DOUBLE),
                             ss.Attribute("k", ss.INT32), ss.Attribute("f", ss.FLOAT)])
    x = rng.standard_normal(n) * 50.0
    x[::7] = 0.0
    view = ss.View(schema, [ss.Column(x, rng.random(n) < 0.1), rng.random(n) * 2.0 - 1.0, rng.integers(-6, 7, n) * 0.5,
                            rng.integers(-5, 40, n).astype(np.int32), (rng.random(n) * 8.0).astype(np.float32)])
    X, U, P_, K, F = NA("x"), NA("u"), NA("p"), NA("k"), NA("f")
    groups = [
        [("exp", ss.Exp(U)), ("exp_i", ss.Exp(K)), ("ln_n", ss.LnNulling(X)), ("ln_q", ss.LnQuiet(ss.Abs(X))), ("l10", ss.Log10Nulling(X)),
         ("l2", ss.Log2Nulling(F)), ("l2q", ss.Log2Quiet(ss.Plus(F, ss.ConstDouble(1.0))))],
        [("log_n", ss.LogNulling(ss.ConstDouble(10.0), X)), ("log_b", ss.LogNulling(F, K)), ("pow_n", ss.PowerNulling(X, P_)),
         ("pow_q", ss.PowerQuiet(ss.Abs(X), U)), ("pow_i", ss.PowerNulling(K, ss.ConstInt32(3)))],
        [("sin", ss.Sin(X)), ("cos", ss.Cos(X)), ("tan", ss.Tan(U)), ("cot", ss.Cot(ss.Plus(U, ss.ConstDouble(2.0)))), ("asin", ss.Asin(U)),
         ("acos", ss.Acos(U)), ("atan", ss.Atan(X)), ("atan2", ss.Atan2(X, U))],
        [("sinh", ss.Sinh(U)), ("cosh", ss.Cosh(U)), ("tanh", ss.Tanh(X)), ("asinh", ss.Asinh(X)), ("acosh", ss.Acosh(ss.Plus(ss.Abs(X), ss.ConstDouble(1.0)))),
         ("atanh", ss.Atanh(ss.Multiply(U, ss.ConstDouble(0.99)))), ("deg", ss.ToDegrees(X)), ("rad", ss.ToRadians(K)), ("pi", ss.Multiply(ss.Pi(), U))],
    ]
    for g in groups:
        e = ss.CompoundExpression()
        for name, expr in g:
            e.AddAs(name, expr)
        run_both(ss.Compute(e, ss.ScanView(view)), gpu_ctx, max_ulp=LIBM_ULP)
    # inside a filter and an aggregate (MIN / MAX / COUNT: order-independent)
    spec = ss.AggregationSpecification().AddAggregation(ss.MAX, "y", "mx").AddAggregation(ss.MIN, "y", "mn").AddAggregation(ss.COUNT, "y", "c")
    q = ss.ScalarAggregate(spec, ss.Compute(ss.CompoundExpression().AddAs("y", ss.LnNulling(X)),
                                            ss.Filter(ss.Greater(ss.Sin(U), ss.ConstDouble(0.25)), ss.ProjectAllAttributes(), ss.ScanView(view))))
    run_both(q, gpu_ctx, max_ulp=LIBM_ULP)


def test_power_signaling_fails_on_a_negative_base_with_a_fractional_exponent(gpu_ctx):
    schema = ss.TupleSchema([ss.Attribute("b", ss.DOUBLE), ss.Attribute("e", ss.DOUBLE)])
    ok = ss.View(schema, [np.array([1.0, 2.0, -1.0, 0.5]), np.array([0.0, 2.0, 2.0, -1.0])])
    run_both(ss.Compute(ss.PowerSignaling(NA("b"), NA("e")), ss.ScanView(ok)), gpu_ctx, max_ulp=LIBM_ULP)
    bad = ss.View(schema, [np.array([1.0, -1.0]), np.array([0.5, 0.5])])
    r = ss.Compute(ss.PowerSignaling(NA("b"), NA("e")), ss.ScanView(bad)).CreateCursor(gpu_ctx).Next(1024)
    assert r.is_failure() and r.exception().return_code == 104


@pytest.mark.parametrize("n", [0, 513, 100003])
def test_round_with_precision(gpu_ctx, n):
    # round(x * 10^p) / 10^p (math_bound_expressions.cc:341-382): a constant precision folds 10^p on the host, exactly as
    # the reference does, and the rest is three IEEE operations -> bit-exact; a precision column goes through the device POW
    rng = np.random.default_rng(5)
    schema = ss.TupleSchema([ss.Attribute("x", ss.DOUBLE, ss.NULLABLE), ss.Attribute("p", ss.INT32), ss.Attribute("f", ss.FLOAT)])
    view = ss.View(schema, [ss.Column(rng.standard_normal(n) * 1000.0, rng.random(n) < 0.1), rng.integers(-3, 6, n).astype(np.int32),
                            (rng.random(n) * 100.0).astype(np.float32)])
    e = (ss.CompoundExpression().AddAs("r2", ss.RoundWithPrecision(NA("x"), ss.ConstInt32(2))).AddAs("rm1", ss.RoundWithPrecision(NA("x"), ss.ConstInt64(-1)))
         .AddAs("rf", ss.RoundWithPrecision(NA("f"), ss.ConstInt32(1))))
    run_both(ss.Compute(e, ss.ScanView(view)), gpu_ctx)
    run_both(ss.Compute(ss.CompoundExpression().AddAs("rp", ss.RoundWithPrecision(NA("x"), NA("p"))), ss.ScanView(view)), gpu_ctx, max_ulp=LIBM_ULP)


@pytest.mark.parametrize("n", [9, 1025, 200003])
@pytest.mark.parametrize("partition", [1, 2])
def test_float_min_max_keep_a_leading_nan_like_the_reference(n, partition):
    """aggregation_operators.h:189-228: a group's first non-NULL value is assigned, later values replace it only when
    `val < result` -- so a NaN that comes FIRST stays (nothing compares less than NaN) and later NaNs are skipped.  The kernels
    skip every NaN; a run that met one in a floating MIN / MAX is repeated in the plan's NaN-exact form (hidden FIRST of the
    column, IF(IS_NAN(first), first, min)) -- bit-identical to the oracle, which restates the reference's fold."""
    rng = np.random.default_rng(n)
    nan = float("nan")
    schema = ss.TupleSchema([ss.Attribute("g", ss.INT32), ss.Attribute("x", ss.DOUBLE), ss.Attribute("f", ss.FLOAT, ss.NULLABLE), ss.Attribute("v", ss.INT64)])
    if n == 9:
        g = np.array([0, 0, 0, 1, 1, 1, 2, 2, 3], np.int32)
        x = np.array([nan, 2.0, -1.0, 5.0, nan, 7.0, nan, nan, 4.0])
        f = x.astype(np.float32)
        fz = np.array([False, False, False, False, False, True, True, False, False])
    else:
        g = rng.integers(0, 700, n).astype(np.int32)
        x = rng.integers(-1000, 1000, n) * 0.5
        x[rng.random(n) < 0.02] = nan                # many groups start with a NaN, many meet one later, many never do
        f = x.astype(np.float32)
        fz = rng.random(n) < 0.1
    view = ss.View(schema, [g, x, ss.Column(f, fz), rng.integers(0, 100, n)])
    spec = (ss.AggregationSpecification().AddAggregation(ss.MIN, "x", "lo").AddAggregation(ss.MAX, "x", "hi").AddAggregation(ss.SUM, "v", "sv")
            .AddAggregation(ss.MIN, "f", "flo").AddAggregation(ss.MAX, "f", "fhi").AddAggregationWithDefinedOutputType(ss.MAX, "f", "fhd", ss.DOUBLE)
            .AddAggregation(ss.COUNT, "f", "cf"))
    ctx = ss.Context(0)
    ctx.set_option("group_partition", partition)
    group = ss.GroupAggregate(ss.ProjectNamedAttribute("g"), spec, None, ss.ScanView(view))
    got = run_both(group, ctx, ignore_order=True)
    if n == 9:
        lo = got.column(1).data[np.argsort(got.column(0).data)]
        assert np.isnan(lo[0]) and lo[1] == 5.0 and np.isnan(lo[2]) and lo[3] == 4.0     # leading NaN kept, later NaN skipped, only-NaN group, no NaN
    run_both(ss.ScalarAggregate(spec, ss.ScanView(view)), ctx)
    run_both(ss.ScalarAggregate(spec, ss.Filter(ss.Greater(NA("v"), ss.ConstInt64(49)), ss.ProjectAllAttributes(), ss.ScanView(view))), ctx)
    order = np.argsort(g, kind="stable")
    clustered = ss.View(schema, [g[order], x[order], ss.Column(f[order], fz[order]), view.column(3).data[order]])
    run_both(ss.AggregateClusters(ss.ProjectNamedAttribute("g"), spec, ss.ScanView(clustered)), ctx)
    # a plan keeps its exact form once it has needed it, and data without NaNs never pays for it
    plan = ss.Plan(group, ctx)
    plan.run(); plan.fetch()
    assert "NaN-exact" in plan.describe()
    clean = ss.View(schema, [g, np.nan_to_num(x), ss.Column(np.nan_to_num(f), fz), view.column(3).data])
    plan2 = ss.Plan(ss.GroupAggregate(ss.ProjectNamedAttribute("g"), spec, None, ss.ScanView(clean)), ctx)
    plan2.run(); plan2.fetch()
    assert "NaN-exact" not in plan2.describe()


@pytest.mark.parametrize("n", [1, 65, 1025, 100003])
def test_aggregates_into_other_result_types(gpu_ctx, n):
    # AddAggregationWithDefinedOutputType across type families (column_aggregator.cc:484-532): floating inputs into integer
    # results store the truncated value (MIN / MAX / FIRST / LAST; SUM is order-dependent there: next test), integers
    # into other integer types compare in their own type (aggregation_operators.h:187-228), FIRST / LAST cast the picked value
    rng = np.random.default_rng(n)
    schema = ss.TupleSchema([ss.Attribute("g", ss.INT32), ss.Attribute("x", ss.DOUBLE, ss.NULLABLE), ss.Attribute("f", ss.FLOAT),
                             ss.Attribute("i", ss.INT32), ss.Attribute("u", ss.UINT32), ss.Attribute("w", ss.INT64, ss.NULLABLE)])
    view = ss.View(schema, [rng.integers(0, 37, n).astype(np.int32), ss.Column(rng.normal(size=n) * 1000.0, rng.random(n) < 0.2),
                            (rng.normal(size=n) * 100.0).astype(np.float32), rng.integers(0, 1 << 30, n).astype(np.int32),
                            rng.integers(0, 1 << 31, n).astype(np.uint32), ss.Column(rng.integers(-(1 << 40), 1 << 40, n), rng.random(n) < 0.2)])
    spec = ss.AggregationSpecification()
    for agg, col, out, t in ((ss.MIN, "x", "mnx", ss.INT64), (ss.MAX, "x", "mxx", ss.INT32), (ss.MIN, "f", "mnf", ss.INT32), (ss.MAX, "f", "mxf", ss.INT64),
                             (ss.MAX, "i", "mxi", ss.UINT32), (ss.MIN, "i", "mni", ss.INT64), (ss.MIN, "u", "mnu", ss.INT32), (ss.MAX, "u", "mxu", ss.UINT64),
                             (ss.MAX, "w", "mxw", ss.DOUBLE), (ss.SUM, "i", "si", ss.INT64), (ss.SUM, "u", "su", ss.DOUBLE)):
        spec.AddAggregationWithDefinedOutputType(agg, col, out, t)
    run_both(ss.ScalarAggregate(spec, ss.ScanView(view)), gpu_ctx)
    run_both(ss.GroupAggregate(ss.ProjectNamedAttribute("g"), spec, None, ss.ScanView(view)), gpu_ctx, ignore_order=True)
    fl = ss.AggregationSpecification()
    for agg, col, out, t in ((ss.FIRST, "x", "fx", ss.INT64), (ss.LAST, "f", "lf", ss.INT64), (ss.FIRST, "i", "fi", ss.INT64), (ss.LAST, "w", "lw", ss.DOUBLE)):
        fl.AddAggregationWithDefinedOutputType(agg, col, out, t)
    run_both(ss.ScalarAggregate(fl, ss.ScanView(view)), gpu_ctx)
    run_both(ss.GroupAggregate(ss.ProjectNamedAttribute("g"), fl, None, ss.ScanView(view)), gpu_ctx, ignore_order=True)


@pytest.mark.parametrize("n", [0, 1, 2, 65, 1025, 30011])
def test_sum_of_floating_values_into_integer_results(gpu_ctx, n):
    # AggregationOperator<SUM> is `*result += val` (aggregation_operators.h:173-185): with an integer result and a floating
    # value C++ adds in the floating type and truncates back after EVERY row -- 0.6 + 0.6 + 0.6 is 0, not 1 -- so the result
    # depends on the row order and the device folds the rows one after the other in input order (the sorted shape for a
    # GroupAggregate, the clusters themselves, all rows for a ScalarAggregate).  Mixed signs, fractions, NULLs, FLOAT stays float.
    rng = np.random.default_rng(100 + n)
    schema = ss.TupleSchema([ss.Attribute("g", ss.INT32), ss.Attribute("x", ss.DOUBLE, ss.NULLABLE), ss.Attribute("f", ss.FLOAT),
                             ss.Attribute("p", ss.DOUBLE), ss.Attribute("i", ss.INT64), ss.Attribute("run", ss.INT32)])
    view = ss.View(schema, [rng.integers(0, 37, n).astype(np.int32), ss.Column(rng.normal(size=n) * 10.0, rng.random(n) < 0.2),
                            (rng.normal(size=n) * 100.0).astype(np.float32), rng.random(n) * 3.0, rng.integers(-50, 50, n),
                            (np.arange(n) // 7 % 5).astype(np.int32)])
    spec = ss.AggregationSpecification()
    for col, out, t in (("x", "sx64", ss.INT64), ("x", "sx32", ss.INT32), ("f", "sf64", ss.INT64), ("f", "sf32", ss.INT32), ("p", "spu64", ss.UINT64), ("p", "spu32", ss.UINT32)):
        spec.AddAggregationWithDefinedOutputType(ss.SUM, col, out, t)
    spec.AddAggregation(ss.SUM, "i", "si").AddAggregation(ss.COUNT, "x", "cx").AddAggregation(ss.MAX, "p", "mp").AddAggregation(ss.FIRST, "x", "fx")
    run_both(ss.ScalarAggregate(spec, ss.ScanView(view)), gpu_ctx)
    run_both(ss.GroupAggregate(ss.ProjectNamedAttribute("g"), spec, None, ss.ScanView(view)), gpu_ctx, ignore_order=True)
    run_both(ss.AggregateClusters(ss.ProjectNamedAttribute("run"), spec, ss.ScanView(view)), gpu_ctx)
    # below a Filter and a Compute: the folded column is a computed one, and the rows that pass keep their order
    e = ss.CompoundExpression().Add(NA("g")).AddAs("x", ss.Multiply(NA("x"), ss.ConstDouble(1.5))).Add(NA("f")).Add(NA("p")).Add(NA("i")).Add(NA("run"))
    child = ss.Compute(e, ss.Filter(ss.Less(NA("i"), ss.ConstInt64(25)), ss.ProjectAllAttributes(), ss.ScanView(view)))
    run_both(ss.ScalarAggregate(spec, child), gpu_ctx)
    run_both(ss.GroupAggregate(ss.ProjectNamedAttributes(["g", "run"]), spec, None, child), gpu_ctx, ignore_order=True)
    # under a key limit: the folded row's rows come from several keys and are folded in INPUT order (the rows sorted by (result row, row id))
    for limit in (0, 3, 36, 100):
        run_both(ss.GroupAggregate(ss.ProjectNamedAttribute("g"), spec, ss.GroupAggregateOptions().set_max_unique_keys_in_result_(limit), ss.ScanView(view)), gpu_ctx)
    run_both(ss.GroupAggregate(ss.ProjectNamedAttributes(["g", "run"]), spec, ss.GroupAggregateOptions().set_max_unique_keys_in_result_(5), child), gpu_ctx)
    # next to CONCAT (its shape keeps a group's rows adjacent and in input order), with and without a limit
    cspec = ss.AggregationSpecification().AddAggregation(ss.CONCAT, "i", "ci")
    for col, out, t in (("x", "sx64", ss.INT64), ("f", "sf32", ss.INT32), ("p", "spu64", ss.UINT64)):
        cspec.AddAggregationWithDefinedOutputType(ss.SUM, col, out, t)
    cspec.AddAggregation(ss.LAST, "x", "lx")
    if n <= 1025:
        run_both(ss.ScalarAggregate(cspec, ss.ScanView(view)), gpu_ctx)
        run_both(ss.GroupAggregate(ss.ProjectNamedAttribute("g"), cspec, None, child), gpu_ctx, ignore_order=True)
        run_both(ss.GroupAggregate(ss.ProjectNamedAttribute("g"), cspec, ss.GroupAggregateOptions().set_max_unique_keys_in_result_(4), ss.ScanView(view)), gpu_ctx)
        run_both(ss.AggregateClusters(ss.ProjectNamedAttribute("run"), cspec, ss.ScanView(view)), gpu_ctx)
    # next to DISTINCT aggregates: their shape sorts a group's rows by the values -- every DISTINCT column's flags are stored and a last
    # sort by (keys, row id) puts the rows back into input order before the fold
    dspec = ss.AggregationSpecification().AddDistinctAggregation(ss.COUNT, "i", "ci")
    for col, out, t in (("x", "sx64", ss.INT64), ("f", "sf32", ss.INT32), ("p", "spu64", ss.UINT64)):
        dspec.AddAggregationWithDefinedOutputType(ss.SUM, col, out, t)
    dspec.AddDistinctAggregation(ss.SUM, "i", "si").AddDistinctAggregation(ss.COUNT, "g", "cg").AddAggregation(ss.LAST, "x", "lx").AddAggregation(ss.COUNT, "", "n")
    run_both(ss.ScalarAggregate(dspec, ss.ScanView(view)), gpu_ctx)
    run_both(ss.GroupAggregate(ss.ProjectNamedAttribute("g"), dspec, None, ss.ScanView(view)), gpu_ctx, ignore_order=True)
    run_both(ss.GroupAggregate(ss.ProjectNamedAttributes(["g", "run"]), dspec, None, child), gpu_ctx, ignore_order=True)
    run_both(ss.GroupAggregate(ss.ProjectNamedAttribute("g"), dspec, ss.GroupAggregateOptions().set_max_unique_keys_in_result_(3), ss.ScanView(view)), gpu_ctx)
    run_both(ss.AggregateClusters(ss.ProjectNamedAttribute("run"), dspec, ss.ScanView(view)), gpu_ctx)


def test_sum_of_floating_values_into_integer_results_reference_arithmetic(gpu_ctx):
    # the C++ rule by hand: 0.6 three times is 0 (each step truncates); 2.5, -0.75, 0.5 -> 2, (2 - 0.75 = 1.25) 1, (1.5) 1;
    # FLOAT adds in float: 16777216 + 1.0f stays 16777216
    schema = ss.TupleSchema([ss.Attribute("a", ss.DOUBLE), ss.Attribute("b", ss.DOUBLE), ss.Attribute("c", ss.FLOAT)])
    view = ss.View(schema, [np.array([0.6, 0.6, 0.6]), np.array([2.5, -0.75, 0.5]), np.array([16777216.0, 1.0, 1.0], np.float32)])
    spec = (ss.AggregationSpecification().AddAggregationWithDefinedOutputType(ss.SUM, "a", "sa", ss.INT64)
            .AddAggregationWithDefinedOutputType(ss.SUM, "b", "sb", ss.INT32).AddAggregationWithDefinedOutputType(ss.SUM, "c", "sc", ss.INT64))
    got = run_both(ss.ScalarAggregate(spec, ss.ScanView(view)), gpu_ctx)
    assert [int(got.column(i).data[0]) for i in range(3)] == [0, 1, 16777216]


def test_sum_of_floating_values_into_an_integer_runs_in_pieces_and_can_be_interrupted():
    # ONE segment of 5 M rows: the fold runs in launches of 2^21 rows whose state stays on the device (same bits as one launch:
    # the oracle folds all rows in one loop) and looks at the plan's interrupt flag between them
    import threading
    import time
    n = 5_000_001
    rng = np.random.default_rng(77)
    schema = ss.TupleSchema([ss.Attribute("x", ss.DOUBLE, ss.NULLABLE), ss.Attribute("f", ss.FLOAT)])
    view = ss.View(schema, [ss.Column(rng.normal(size=n) * 10.0, rng.random(n) < 0.1), (rng.normal(size=n) * 3.0).astype(np.float32)])
    spec = (ss.AggregationSpecification().AddAggregationWithDefinedOutputType(ss.SUM, "x", "sx", ss.INT64)
            .AddAggregationWithDefinedOutputType(ss.SUM, "f", "sf", ss.INT32).AddAggregation(ss.COUNT, "x", "cx"))
    op = ss.ScalarAggregate(spec, ss.ScanView(view))
    ctx = ss.Context(0)
    run_both(op, ctx)
    plan = ss.Plan(op, ctx)
    plan.run()                                     # (buffers, upload)
    t0 = time.perf_counter()
    plan.run()
    ctx.synchronize()
    whole = time.perf_counter() - t0
    timer = threading.Timer(whole * 0.2, plan.interrupt)          # Cursor::Interrupt from another thread, a fifth of the way in
    timer.start()
    t0 = time.perf_counter()
    with pytest.raises(ss.SupersonicException) as err:
        plan.run()
    took = time.perf_counter() - t0
    timer.join()
    assert err.value.return_code == ss.INTERRUPTED
    assert took < whole * 0.9, (took, whole)       # it stopped at a piece boundary, not after the whole fold
    plan.run()                                     # and the plan is usable afterwards
    got = plan.fetch()
    _s, want = oracle_run(op)
    assert [int(got.column(i).data[0]) for i in range(3)] == [int(want[i][0][0]) for i in range(3)]


# ---- runtime specialisation (context option "specialize", csrc/rtc.cpp): the same handlers compiled per plan with the
# ---- opcode dispatch folded away must give bit-identical results ---------------------------------------------------------
@pytest.fixture(scope="module")
def specialized_ctx():
    c = ss.Context(0)
    c.set_option("specialize", 1)
    return c


def _run_specialized(op, ctx, expect_stages=1, **kw):
    got = run_both(op, ctx, **kw)
    plan = ss.Plan(op, ctx)
    plan.run()
    assert plan.specialized() >= expect_stages, plan.specialize_reason()
    return got


@pytest.mark.parametrize("n", [0, 1, 513, 2049, 100003])
def test_specialized_scalar_aggregates(specialized_ctx, n):
    _run_specialized(fpa_wide(make_view(n)), specialized_ctx)
    _run_specialized(fpa_narrow(make_view(n)), specialized_ctx)
    _run_specialized(fpa_wide(make_view(n, nullable=True)), specialized_ctx)


@pytest.mark.parametrize("n", [1, 1025, 100003])
def test_specialized_materialising_and_group_stages(specialized_ctx, n):
    _run_specialized(compute_exprs(make_view(n, nullable=True)), specialized_ctx)
    _run_specialized(ss.Filter(ss.Greater(NA("a"), ss.ConstInt64(499)), ss.ProjectAllAttributes(), ss.ScanView(make_view(n))), specialized_ctx)
    _run_specialized(group_query(make_view(n, nullable=True), True), specialized_ctx, ignore_order=True)


@pytest.mark.parametrize("specialize", [0, 1])
@pytest.mark.parametrize("groups", [100000, 900, 7])
def test_group_aggregate_with_records_of_more_than_16_words(groups, specialize):
    # 18 aggregates of NOT NULL columns = a 19-word partition record (round 4: ssgpu_part_agg_kernel<20>, plain scatter only) and an
    # LDS entry too wide for a table inside the pipeline kernel: the direct shape would send every row to the global table.  The
    # first run has nothing to go by (no table on chip, no feedback) and sizes partitions for its row count; every group count
    # has to come out right, whichever shape the later runs settle on.
    n = 300007
    ctx = ss.Context(0)
    ctx.set_option("specialize", specialize)
    view = make_view(n)
    keyed = ss.View(view.schema(), [view.column(i) if i != 2 else ss.Column(np.arange(n) * 7919 % groups, None) for i in range(view.column_count())])
    spec = ss.AggregationSpecification()
    for col in ("a", "b", "d"):
        spec.AddAggregation(ss.SUM, col, "s_" + col).AddAggregation(ss.MIN, col, "mn_" + col).AddAggregation(ss.MAX, col, "mx_" + col)
    for col in ("d1", "d2", "d3", "u"):
        spec.AddAggregation(ss.MIN, col, "mn_" + col).AddAggregation(ss.MAX, col, "mx_" + col)
    spec.AddAggregation(ss.COUNT, "", "n")
    op = ss.GroupAggregate(ss.ProjectNamedAttributes(["c"]), spec, None, ss.ScanView(keyed))
    _s, want = oracle_run(op)
    plan = ss.Plan(op, ctx)
    shapes = []
    for _ in range(4):
        plan.run(keyed)
        assert_cols_equal(sort_rows(to_cols(plan.fetch())), sort_rows(want), context="%d groups" % groups)
        shapes.append([st["group_shape"] for st in plan.stage_info() if st["kind"] == 3][-1])
    if groups > 7:                                   # (7 groups sit in the pipeline kernel's own LDS table: the direct shape is the right one)
        assert shapes[-1] in (1, 2, 3), shapes       # partitions, or one table for all groups: not the per-row global atomics again


def test_specialized_first_last_by_a_stored_row_id(specialized_ctx):
    # the round-4 forms of FIRST / LAST -- order taken from a stored row-id column next to DISTINCT aggregates, row-id twins
    # under a key limit -- through the per-plan compiled kernels
    view = make_view(30011, nullable=True)
    spec = (ss.AggregationSpecification().AddDistinctAggregation(ss.SUM, "a", "sd").AddAggregation(ss.FIRST, "d0", "fd").AddAggregation(ss.LAST, "d", "ld")
            .AddAggregation(ss.COUNT, "", "n"))
    _run_specialized(ss.GroupAggregate(ss.ProjectNamedAttributes(["k2"]), spec, None, ss.ScanView(view)), specialized_ctx, ignore_order=True)
    _run_specialized(ss.ScalarAggregate(spec, ss.ScanView(view)), specialized_ctx)
    plain = (ss.AggregationSpecification().AddAggregation(ss.SUM, "b", "sb").AddAggregation(ss.FIRST, "d0", "fd").AddAggregation(ss.LAST, "d", "ld"))
    _run_specialized(ss.GroupAggregate(ss.ProjectNamedAttributes(["k2"]), plain, ss.GroupAggregateOptions().set_max_unique_keys_in_result_(7), ss.ScanView(view)),
                     specialized_ctx)


@pytest.mark.parametrize("slab", [0, 2])
@pytest.mark.parametrize("n", [1025, 100003])
def test_specialized_partition_aggregation_kernel(n, slab):
    # the partitioned GroupAggregate's aggregation kernel compiled for the stage's aggregates (rtc.cpp:
    # ssgpu_rtc_specialize_part_agg; static LDS of 80 KiB for hash partitions, 159 KiB for the slab form)
    ctx = ss.Context(0)
    for k, v in (("specialize", 1), ("group_partition", 2), ("group_slab", slab), ("group_resident", 0)):   # (records through memory: the kernels named above)
        ctx.set_option(k, v)
    for nullable, keys in ((False, ("k1", "k2")), (True, ("k1",))):
        op = group_query(make_view(n, nullable=nullable), True, keys)
        run_both(op, ctx, ignore_order=True)
        plan = ss.Plan(op, ctx)
        plan.run()
        assert plan.specialized() >= 2, plan.specialize_reason()      # the scatter program and the aggregation kernel
    fl = ss.GroupAggregate(ss.ProjectNamedAttributes(["k2"]), first_last_spec(), None, ss.ScanView(make_view(n, nullable=True)))
    run_both(fl, ctx, ignore_order=True)


@pytest.mark.parametrize("n", [1025, 100003])
def test_specialized_resident_group_aggregation_kernel(n):
    # the resident form compiled for the stage: the row source's key packing, field list and predicates and the aggregates'
    # descriptors are all constants of the build (rtc.cpp: ssgpu_rtc_specialize_part_agg with a source)
    ctx = ss.Context(0)
    for k, v in (("specialize", 1), ("group_partition", 2), ("group_slab", 2)):
        ctx.set_option(k, v)
    for nullable, keys, with_filter in ((False, ("k1", "k2"), True), (True, ("k1",), False), (True, ("k1",), True)):
        op = group_query(make_view(n, nullable=nullable), with_filter, keys)
        run_both(op, ctx, ignore_order=True)
        plan = ss.Plan(op, ctx)
        plan.run()
        info = plan.stage_info()[-1]
        assert info["group_shape"] == 3 and info["specialized"] & 16, (info, plan.specialize_reason())


def test_specialized_group_stage_beyond_64k_of_lds(specialized_ctx):
    # a direct GroupAggregate whose LDS pre-aggregation table takes the launch past the 64 KiB of dynamic LDS a module-loaded
    # kernel may have: the specialised build declares its LDS statically, at exactly the launch's size (rtc.cpp static_lds)
    n = 300007
    rng = np.random.default_rng(3)
    schema = ss.TupleSchema([ss.Attribute("k", ss.INT32), ss.Attribute("v", ss.INT64), ss.Attribute("d", ss.DOUBLE, ss.NULLABLE)])
    view = ss.View(schema, [rng.integers(0, 3000, n).astype(np.int32), rng.integers(-1000, 1000, n), ss.Column(rng.integers(-4000, 4000, n) * 0.25, rng.random(n) < 0.1)])
    spec = (ss.AggregationSpecification().AddAggregation(ss.SUM, "v", "s").AddAggregation(ss.COUNT, "d", "c").AddAggregation(ss.MIN, "d", "mn")
            .AddAggregation(ss.SUM, "d", "sd").AddAggregation(ss.MAX, "v", "mx"))
    op = ss.GroupAggregate(ss.ProjectNamedAttributes(["k"]), spec, None, ss.ScanView(view))
    plan = ss.Plan(op, specialized_ctx)
    for _ in range(4):                       # the run feedback grows the LDS table (fewer workgroups per CU) over the first runs
        plan.run()
    assert plan.counters().lds_bytes > 64 * 1024, plan.counters().lds_bytes
    assert plan.specialized() >= 1, plan.specialize_reason()
    _schema, want = oracle_run(op)
    got = plan.fetch()
    assert_cols_equal(sort_rows(to_cols(got)), sort_rows(want))


def test_specialized_kernels_are_cached_and_report_errors(specialized_ctx):
    import time
    view = make_view(100003)
    t0 = time.time(); p1 = ss.Plan(fpa_wide(view), specialized_ctx); p1.run(); specialized_ctx.synchronize(); first = time.time() - t0
    t0 = time.time(); p2 = ss.Plan(fpa_wide(make_view(5000)), specialized_ctx); p2.run(); specialized_ctx.synchronize(); second = time.time() - t0
    assert p1.specialized() == 1 and p2.specialized() == 1
    assert second < max(first, 0.5)          # same program: no second compilation
    # evaluation errors surface the same way from a specialised kernel
    schema = ss.TupleSchema([ss.Attribute("b", ss.INT32)])
    bad = ss.View(schema, [np.array([4, 0, 1], np.int32)])
    spec = ss.AggregationSpecification().AddAggregation(ss.SUM, "q", "s")
    op = ss.ScalarAggregate(spec, ss.Compute(ss.CompoundExpression().AddAs("q", ss.DivideSignaling(ss.ConstInt32(8), NA("b"))), ss.ScanView(bad)))
    r = op.CreateCursor(specialized_ctx).Next()
    assert r.is_failure() and r.exception().return_code == ss.ERROR_EVALUATION_ERROR


# ---- slab mode of the partitioned GroupAggregate: few enough groups for ONE whole-LDS table per aggregation workgroup;
# ---- no hash partitions, the scatter writes records sequentially, tables are merged into the global one ------------------
# ---- plain stages (keys and aggregated values are input columns, predicates compare a column with a constant) take it
# ---- without any scatter: the aggregation workgroups read the input columns themselves (group_shape 3, "resident")
@pytest.mark.parametrize("resident", [1, 0])
@pytest.mark.parametrize("n", [0, 1, 65, 1025, 100003])
@pytest.mark.parametrize("with_filter", [False, True])
@pytest.mark.parametrize("nullable", [False, True])
def test_group_aggregate_slab_mode(n, with_filter, nullable, resident):
    ctx = ss.Context(0)
    ctx.set_option("group_partition", 2)
    ctx.set_option("group_slab", 2)
    ctx.set_option("group_resident", resident)
    keys = ("k1",) if nullable else ("k1", "k2")
    op = group_query(make_view(n, nullable=nullable), with_filter, keys)
    run_both(op, ctx, ignore_order=True)
    if 0 < n <= 1025:                    # (at 100003 rows the two-key case has as many groups as the table has entries: it may fall back)
        plan = ss.Plan(op, ctx)
        plan.run()
        assert plan.stage_info()[-1]["group_shape"] == (3 if resident else 2), plan.stage_info()
    run_both(ss.GroupAggregate(ss.ProjectNamedAttributes(["k2"]), first_last_spec(), None, ss.ScanView(make_view(n, nullable=True))), ctx, ignore_order=True)


def test_group_aggregate_slab_mode_falls_back_when_the_groups_do_not_fit():
    # forced slab mode with far more groups than one LDS table holds (and the EMPTY-valued key): the table overflow sends the
    # stage to the hash partitions
    n = 200000
    rng = np.random.default_rng(8)
    key = rng.integers(0, 50000, n).astype(np.int64)
    key[::777] = -1
    schema = ss.TupleSchema([ss.Attribute("k", ss.INT64), ss.Attribute("v", ss.INT64), ss.Attribute("d", ss.DOUBLE)])
    view = ss.View(schema, [key, rng.integers(-1000, 1000, n), rng.integers(-4000, 4000, n) * 0.25])
    spec = (ss.AggregationSpecification().AddAggregation(ss.SUM, "v", "s").AddAggregation(ss.COUNT, "", "c").AddAggregation(ss.MIN, "v", "mn")
            .AddAggregation(ss.SUM, "d", "sd").AddAggregation(ss.MAX, "d", "mx"))
    ctx = ss.Context(0)
    ctx.set_option("group_partition", 2)
    ctx.set_option("group_slab", 2)
    run_both(ss.GroupAggregate(ss.ProjectNamedAttributes(["k"]), spec, None, ss.ScanView(view)), ctx, ignore_order=True)
    small = ss.View(schema, [key % 700, view.column(1).data, view.column(2).data])   # 700 groups (+ the EMPTY key's image): fits
    run_both(ss.GroupAggregate(ss.ProjectNamedAttributes(["k"]), spec, None, ss.ScanView(small)), ctx, ignore_order=True)


# ---- GroupAggregateOptions::max_unique_keys_in_result (aggregate.h:160-205, row_hash_set.cc:500-511): the first limit + 1
# ---- keys in first-seen order keep a row, every other key's rows aggregate into the last kept row.  The device composes it
# ---- from a hash aggregate with a hidden first-seen row id, a sort by it and a fold of the tail: same rows, SAME ORDER ------
@pytest.mark.parametrize("limit", [0, 1, 7, 500, 999, 1000, 5000])
@pytest.mark.parametrize("n,partition", [(9, 1), (1025, 1), (100003, 1), (100003, 2)])
def test_group_aggregate_max_unique_keys_in_result(n, partition, limit):
    ctx = ss.Context(0)
    ctx.set_option("group_partition", partition)
    view = make_view(n, nullable=True)
    spec = (ss.AggregationSpecification().AddAggregation(ss.SUM, "b", "sb").AddAggregation(ss.COUNT, "d0", "c0").AddAggregation(ss.COUNT, "", "n")
            .AddAggregation(ss.MIN, "d0", "mn").AddAggregation(ss.MAX, "d", "mx").AddAggregation(ss.SUM, "d1", "sd").AddAggregation(ss.MIN, "u", "mu")
            .AddAggregation(ss.MAX, "f", "mf")
            # FIRST / LAST under the limit: the folded row answers with the value at the smallest / largest row id over every group
            # it absorbs (NULL inputs do not count: d0 / d / t are NULLABLE in the first two views)
            .AddAggregation(ss.FIRST, "d0", "fd").AddAggregation(ss.LAST, "d", "ld").AddAggregation(ss.LAST, "f", "lf").AddAggregation(ss.FIRST, "t", "ft"))
    opts = ss.GroupAggregateOptions().set_max_unique_keys_in_result_(limit)
    run_both(ss.GroupAggregate(ss.ProjectNamedAttributes(["k2"]), spec, opts,
                               ss.Filter(ss.Greater(NA("b"), ss.ConstInt64(499)), ss.ProjectAllAttributes(), ss.ScanView(view))), ctx)   # ordered: first-seen order
    run_both(ss.GroupAggregate(ss.ProjectNamedAttributes(["k1"]), spec, opts, ss.ScanView(view)), ctx)                                   # a NULL key group among them
    # NULLABLE k1 + k2 = 65 key bits: materialise (+ the input row id) -> sort by the keys -> clustered aggregation with MIN(row id)
    # as the first-seen order -> the same sort + fold; the FIRST / LAST twins order by that stored row id too
    run_both(ss.GroupAggregate(ss.ProjectNamedAttributes(["k1", "k2"]), spec, opts,
                               ss.Filter(ss.Greater(NA("b"), ss.ConstInt64(299)), ss.ProjectAllAttributes(), ss.ScanView(view))), ctx)
    # FIRST / LAST of a computed value take the sorted shape as well (the value is fetched from a stored column)
    e = ss.CompoundExpression().Add(NA("k2")).AddAs("x", ss.Plus(NA("a"), NA("b"))).Add(NA("d0"))
    spec_x = ss.AggregationSpecification().AddAggregation(ss.FIRST, "x", "fx").AddAggregation(ss.LAST, "x", "lx").AddAggregation(ss.SUM, "d0", "s")
    run_both(ss.GroupAggregate(ss.ProjectNamedAttributes(["k2"]), spec_x, opts, ss.Compute(e, ss.ScanView(view))), ctx)
    plain = make_view(n)                                # NOT NULL keys: two INT32 keys in one word
    run_both(ss.GroupAggregate(ss.ProjectNamedAttributes(["k1", "k2"]), spec, ss.GroupAggregateOptions().set_max_unique_keys_in_result_(limit),
                               ss.ScanView(plain)), ctx)


def test_group_aggregate_max_unique_keys_reference_vector_and_refusals(gpu_ctx):
    # aggregate_groups_test.cc:296-328 as written; what the composition cannot express is refused at bind, never ignored
    schema = ss.TupleSchema([ss.Attribute("col0", ss.INT32), ss.Attribute("col1", ss.INT32)])
    view = ss.View(schema, [np.array([1, 3, 1, 3, 4, 3, 5, 4, 1], np.int32), np.array([3, -3, 4, -5, 5, -1, 1, 3, -2], np.int32)])
    opts = ss.GroupAggregateOptions().set_max_unique_keys_in_result_(2)
    got = run_both(ss.GroupAggregate(ss.ProjectNamedAttribute("col0"), ss.AggregationSpecification().AddAggregation(ss.SUM, "col1", "sum"), opts, ss.ScanView(view)), gpu_ctx)
    assert got.column(0).data.tolist() == [1, 3, 4] and got.column(1).data.tolist() == [5, -9, 9]
    # what the composition cannot express: a CONCAT result below another operation (its strings exist on the host only)
    wide = make_view(100, nullable=True)
    for op in (ss.Sort(ss.SortOrder().add("k2", ss.ASCENDING), None, 0,
                       ss.GroupAggregate(ss.ProjectNamedAttributes(["k2"]), ss.AggregationSpecification().AddAggregation(ss.CONCAT, "b", "l").AddDistinctAggregation(ss.SUM, "b", "s"),
                                         opts, ss.ScanView(wide))),):
        with pytest.raises(ss.SupersonicException) as e:
            ss.Plan(op, gpu_ctx)
        assert e.value.return_code == ss.ERROR_NOT_IMPLEMENTED


@pytest.mark.parametrize("limit", [0, 1, 2, 7, 299, 300, 5000, 10 ** 12])
@pytest.mark.parametrize("n", [0, 1, 9, 1025, 100003])
def test_group_aggregate_distinct_under_max_unique_keys_in_result(gpu_ctx, n, limit):
    """DISTINCT aggregates under a key limit.  The reference's DISTINCT aggregator keeps one set of seen values per RESULT ROW
    (column_aggregator.cc:308-376), and beyond the limit every new key is answered with the last row (row_hash_set.cc:500-511): the
    folded row's COUNT(DISTINCT x) counts the distinct x over ALL its rows -- not a sum of per-key counts.  The device stores each
    input row's result row (first-seen rank of its key, clamped) and aggregates by it; same rows in the SAME (first-seen) order."""
    view = make_view(n, nullable=True)
    spec = (ss.AggregationSpecification().AddDistinctAggregation(ss.COUNT, "b", "cb").AddDistinctAggregation(ss.SUM, "b", "sb")
            .AddDistinctAggregation(ss.COUNT, "d0", "c0").AddAggregation(ss.COUNT, "", "n").AddAggregation(ss.SUM, "a", "sa")
            .AddDistinctAggregation(ss.SUM, "u", "su").AddAggregation(ss.MIN, "d0", "mn").AddAggregation(ss.MAX, "f", "mf")
            .AddAggregation(ss.FIRST, "d0", "fd").AddAggregation(ss.LAST, "t", "lt"))
    opts = ss.GroupAggregateOptions().set_max_unique_keys_in_result_(limit)
    run_both(ss.GroupAggregate(ss.ProjectNamedAttributes(["k2"]), spec, opts, ss.ScanView(view)), gpu_ctx)
    run_both(ss.GroupAggregate(ss.ProjectNamedAttributes(["k1"]), spec, opts,                                  # a NULL key group among them
                               ss.Filter(ss.Greater(NA("b"), ss.ConstInt64(299)), ss.ProjectAllAttributes(), ss.ScanView(view))), gpu_ctx)
    run_both(ss.GroupAggregate(ss.ProjectNamedAttributes(["k1", "k2"]), spec, opts, ss.ScanView(view)), gpu_ctx)   # 65 key bits
    plain = make_view(n)
    got = run_both(ss.GroupAggregate(ss.ProjectNamedAttributes(["k1", "k2"]), spec, opts, ss.ScanView(plain)), gpu_ctx)   # NOT NULL keys stay NOT NULL
    assert not got.schema().attribute(0).is_nullable() and not got.schema().attribute(1).is_nullable()
    # CONCAT under the limit: the folded row's string joins the values of all its keys in INPUT order
    cspec = (ss.AggregationSpecification().AddAggregation(ss.CONCAT, "d0", "cd").AddAggregation(ss.COUNT, "", "n").AddAggregation(ss.CONCAT, "k1", "ck")
             .AddAggregation(ss.SUM, "a", "sa").AddAggregation(ss.FIRST, "t", "ft").AddAggregation(ss.LAST, "d0", "ld"))
    if n <= 1025:
        run_both(ss.GroupAggregate(ss.ProjectNamedAttributes(["k2"]), cspec, opts, ss.ScanView(view)), gpu_ctx)
        run_both(ss.GroupAggregate(ss.ProjectNamedAttributes(["k1", "k2"]), cspec, opts,
                                   ss.Filter(ss.Greater(NA("b"), ss.ConstInt64(299)), ss.ProjectAllAttributes(), ss.ScanView(view))), gpu_ctx)


def test_distinct_under_key_limit_shares_one_set_beyond_the_limit(gpu_ctx):
    # keys 1, 2 keep their rows; 3, 4, 5 fold into the row of key 3: its distinct values of v are {7, 8, 9} -- 3, not 2 + 2 + 1
    schema = ss.TupleSchema([ss.Attribute("k", ss.INT32), ss.Attribute("v", ss.INT64)])
    view = ss.View(schema, [np.array([1, 2, 3, 4, 3, 5, 4, 1, 2], np.int32), np.array([5, 6, 7, 7, 8, 8, 9, 5, 1], np.int64)])
    spec = ss.AggregationSpecification().AddDistinctAggregation(ss.COUNT, "v", "c").AddDistinctAggregation(ss.SUM, "v", "s").AddAggregation(ss.COUNT, "", "n")
    got = run_both(ss.GroupAggregate(ss.ProjectNamedAttribute("k"), spec, ss.GroupAggregateOptions().set_max_unique_keys_in_result_(2), ss.ScanView(view)), gpu_ctx)
    assert got.column(0).data.tolist() == [1, 2, 3]
    assert got.column(1).data.tolist() == [1, 2, 3] and got.column(2).data.tolist() == [5, 7, 24] and got.column(3).data.tolist() == [2, 2, 5]


@pytest.mark.parametrize("specialize", [0, 1])
def test_merge_of_four_partial_tables_through_wide_partitions(specialize):
    """Four shards' partial tables (config #4's 12 aggregates + 4 residuals: a 17-word record) gathered on one GPU and merged the way a
    rank of a 4-GPU job merges them: the never-NULL partial columns declared NOT NULL (no contribution counts), the merge stage
    without a table on chip and therefore -- from its second run on -- through 20-word partition records, where every group now
    meets its four partial rows.  Every run's result is the oracle's GroupAggregate of the whole input; DOUBLE sums exact."""
    import torch
    from supersonic_amd.distributed import _shard_spec, _merge_spec, _merge_plan, _never_null, _declare_not_null
    ctx = ss.Context(0)
    ctx.set_option("specialize", specialize)
    n, world, groups = 480000, 4, 60000
    rng = np.random.default_rng(5)
    schema = ss.TupleSchema([ss.Attribute("k1", ss.INT32), ss.Attribute("k2", ss.INT32)] + [ss.Attribute("d%d" % i, ss.DOUBLE) for i in range(4)])
    g = rng.integers(0, groups, n)
    view = ss.View(schema, [(g // 300).astype(np.int32), (g % 300).astype(np.int32)] + [rng.integers(-4000, 4000, n) * 0.25 for _ in range(4)])
    spec = ss.AggregationSpecification()
    for i in range(4):
        spec.AddAggregation(ss.SUM, "d%d" % i, "s%d" % i).AddAggregation(ss.MIN, "d%d" % i, "mn%d" % i).AddAggregation(ss.MAX, "d%d" % i, "mx%d" % i)
    keys = ["k1", "k2"]
    shard_spec, with_residual = _shard_spec(spec, schema)
    merged_spec, counts = _merge_spec(spec, with_residual)
    never_null = _never_null(shard_spec, schema)
    assert len(never_null) == 16
    cap, dev = 65536, torch.device("cuda", 0)
    plans, images, image_bytes = [], [], None
    for s in range(world):
        lo, hi = n * s // world, n * (s + 1) // world
        sv = ss.View(schema, [ss.Column(view.column(i).data[lo:hi], None) for i in range(view.column_count())])
        plan = ss.Plan(ss.GroupAggregate(ss.ProjectNamedAttributes(keys), shard_spec, None, ss.ScanView(sv)), ctx)
        plan.run()
        image_bytes, _ub, _offs = plan.image_layout(cap, 1)
        out = torch.zeros(image_bytes, dtype=torch.uint8, device=dev)
        torch.cuda.synchronize()
        plan.pack_image(cap, out.data_ptr())
        ctx.synchronize()
        plans.append(plan)
        images.append(out)
    _ib, unpacked_bytes, _offs = plans[0].image_layout(cap, world)
    gathered = torch.cat(images)
    unpacked = torch.zeros(unpacked_bytes, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    everyone = _declare_not_null(plans[0].unpack_images(gathered.data_ptr(), world, cap, unpacked.data_ptr()), never_null)
    ctx.synchronize()
    trailer = unpacked[unpacked_bytes - 32:].view(torch.int64).tolist()
    assert trailer[2] == 0 and trailer[3] == 0, trailer
    merge = ss.Plan(_merge_plan(keys, merged_spec, counts, plans[0].result_schema, everyone, valid="__valid"), ctx)
    _s, want = oracle_run(ss.GroupAggregate(ss.ProjectNamedAttributes(keys), spec, None, ss.ScanView(view)))
    shapes = []
    for _ in range(4):
        merge.run(everyone)
        assert_cols_equal(sort_rows(to_cols(merge.fetch())), sort_rows(want), context="merged partial tables")
        shapes.append([st["group_shape"] for st in merge.stage_info() if st["kind"] == 3][-1])
    assert shapes[0] == 0 and shapes[-1] == 1, shapes          # direct once (nothing known), partitions from then on


# ---- lazy run feedback (runtime.cpp: settle_plan): in its steady state a GroupAggregate leaves its overflow words on the stream
# ---- instead of synchronising at the end of every run; a run that overflows after all is repeated when its result is touched ---
@pytest.mark.parametrize("partition", [1, 2])
def test_group_aggregate_lazy_feedback_repeats_an_overflowing_run(partition):
    rng = np.random.default_rng(11)
    schema = ss.TupleSchema([ss.Attribute("k", ss.INT64), ss.Attribute("v", ss.INT64), ss.Attribute("d", ss.DOUBLE)])

    def view_of(n, groups):
        return ss.View(schema, [rng.integers(0, groups, n), rng.integers(-1000, 1000, n), rng.integers(-4000, 4000, n) * 0.25])
    spec = (ss.AggregationSpecification().AddAggregation(ss.SUM, "v", "s").AddAggregation(ss.COUNT, "", "c").AddAggregation(ss.MIN, "v", "mn")
            .AddAggregation(ss.SUM, "d", "sd").AddAggregation(ss.MAX, "d", "mx"))
    few, many = view_of(300000, 3000), view_of(300000, 250000)
    ctx = ss.Context(0)
    ctx.set_option("lazy_feedback", 1)                # (opt-in since round 5: the default settles every run before it returns)
    ctx.set_option("group_partition", partition)
    ctx.set_option("group_capacity", 8192)            # the direct shape's global table: 3000 groups fit, 250000 do not
    op = lambda v: ss.GroupAggregate(ss.ProjectNamedAttributes(["k"]), spec, None, ss.ScanView(v))   # noqa: E731
    plan = ss.Plan(op(few), ctx)
    _s, want_few = oracle_run(op(few))
    for _ in range(6):                                # settles, then runs without a synchronise
        plan.run(few)
    assert_cols_equal(sort_rows(to_cols(plan.fetch())), sort_rows(want_few), context="steady state")
    plan.run(few)
    plan.run(many)                                    # overflows its tables: noticed when the result is touched, and repeated
    _s, want_many = oracle_run(op(many))
    assert_cols_equal(sort_rows(to_cols(plan.fetch())), sort_rows(want_many), context="overflow in the steady state")
    assert plan.stage_info()[0]["reruns"] >= 1
    plan.run(few)                                     # and back
    assert_cols_equal(sort_rows(to_cols(plan.fetch())), sort_rows(want_few), context="after the repeat")


# ---- key-range exchange of a sharded GroupAggregate (ssgpu_result_route_images, distributed.py exchange="key_range"):
# ---- a partial row goes only to the rank that owns its key; every rank merges 1 / world of the groups ----------------------
@pytest.mark.parametrize("n,world", [(100003, 3), (2000, 4), (0, 2)])
def test_key_range_exchange_routes_every_group_to_one_owner(gpu_ctx, n, world):
    """`world` ranks simulated on one GPU: every source shard routes its partial table into `world` images (one per owner),
    owner d unpacks image d of every source and merges.  The owners' results are disjoint in their keys and together are the
    oracle's GroupAggregate of the whole input -- DOUBLE sums as (SUM, SUM_RESIDUAL) pairs, COUNT kept NOT NULL, NULL keys."""
    import torch
    from supersonic_amd.distributed import _shard_spec, _merge_spec, _merge_plan
    view = make_view(n, nullable=True)
    spec = (ss.AggregationSpecification().AddAggregation(ss.SUM, "b", "sb").AddAggregation(ss.SUM, "d1", "sd").AddAggregation(ss.MIN, "d0", "mn")
            .AddAggregation(ss.MAX, "d", "mx").AddAggregation(ss.COUNT, "d0", "c0").AddAggregation(ss.COUNT, "", "n"))
    keys = ["k1", "t"]                                           # a NULLABLE INT32 and a NULLABLE BOOL key
    shard_spec, with_residual = _shard_spec(spec, view.schema())
    merged_spec, counts = _merge_spec(spec, with_residual)
    cuts = [n * i // world for i in range(world + 1)]
    sources, cap = [], max(1024, int(n / world * 1.3 / world) + 2048)
    dev = torch.device("cuda", 0)
    image_bytes = None
    for s in range(world):
        sv = ss.View(view.schema(), [ss.Column(view.column(i).data[cuts[s]:cuts[s + 1]], None if view.column(i).is_null is None else view.column(i).is_null[cuts[s]:cuts[s + 1]])
                                     for i in range(view.column_count())])
        plan = ss.Plan(ss.GroupAggregate(ss.ProjectNamedAttributes(keys), shard_spec, None, ss.ScanView(sv)), gpu_ctx)
        plan.run()
        image_bytes, _ub, _offs = plan.image_layout(cap, 1)
        out = torch.zeros(world * image_bytes, dtype=torch.uint8, device=dev)
        torch.cuda.synchronize()            # (torch fills on ITS stream; the library's kernels run on the context's)
        plan.route_images(len(keys), world, cap, out.data_ptr())
        gpu_ctx.synchronize()
        sources.append((plan, out))
    plan0 = sources[0][0]
    _ib, unpacked_bytes, _offs = plan0.image_layout(cap, world)
    owned, all_keys = [], []
    for d in range(world):
        arrived = torch.cat([out[d * image_bytes:(d + 1) * image_bytes] for (_p, out) in sources])      # what the all-to-all delivers to rank d
        unpacked = torch.zeros(unpacked_bytes, dtype=torch.uint8, device=dev)
        torch.cuda.synchronize()            # (the concatenation above has to be complete before another stream reads it)
        everyone = plan0.unpack_images(arrived.data_ptr(), world, cap, unpacked.data_ptr())
        gpu_ctx.synchronize()
        trailer = unpacked[unpacked_bytes - 32:].view(torch.int64).tolist()
        assert trailer[2] == 0 and trailer[3] == 0, trailer                                             # no image overflowed, no evaluation error
        got = ss.drain(_merge_plan(keys, merged_spec, counts, plan0.result_schema, everyone, valid="__valid").CreateCursor(gpu_ctx), 1 << 30)
        owned.append(to_cols(got))
        all_keys += list(zip(*[np.where(z, -7, dcol).tolist() if z is not None else dcol.tolist() for (dcol, z) in owned[-1][:2]]))
    assert len(all_keys) == len(set(all_keys))                                                          # every group has exactly one owner
    union = [(np.concatenate([o[i][0] for o in owned]), None if owned[0][i][1] is None else np.concatenate([o[i][1] for o in owned])) for i in range(len(owned[0]))]
    oschema, want = oracle_run(ss.GroupAggregate(ss.ProjectNamedAttributes(keys), spec, None, ss.ScanView(view)))
    assert_cols_equal(sort_rows(union), sort_rows(want), context="key-range exchange, %d owners" % world)
    if n >= 100000:
        assert min(len(o[0][0]) for o in owned) > 0                                                     # the hash spreads the groups


@pytest.mark.parametrize("exchange", ["key_range", "all_gather"])
def test_device_sharded_group_aggregate_exchange_forms_one_rank(exchange):
    import socket
    import torch
    import torch.distributed as dist
    from supersonic_amd.distributed import DeviceShardedGroupAggregate
    s = socket.socket(); s.bind(("127.0.0.1", 0)); port = s.getsockname()[1]; s.close()
    os.environ["MASTER_ADDR"] = "127.0.0.1"; os.environ["MASTER_PORT"] = str(port)
    torch.cuda.set_device(0)
    dist.init_process_group("nccl", rank=0, world_size=1)
    try:
        ctx = ss.Context(0)
        view = make_view(100003, nullable=True)
        spec = (ss.AggregationSpecification().AddAggregation(ss.SUM, "a", "sa").AddAggregation(ss.SUM, "d1", "sd").AddAggregation(ss.MIN, "d0", "mn")
                .AddAggregation(ss.COUNT, "d0", "c").AddAggregation(ss.COUNT, "", "n"))
        child = ss.Filter(ss.Greater(NA("b"), ss.ConstInt64(499)), ss.ProjectAllAttributes(), ss.ScanView(view))
        job = DeviceShardedGroupAggregate(ctx, ["k2", "t"], spec, child, exchange=exchange)
        for _ in range(3):
            job.step()
            while not job.check():
                job.step()
        assert job.collectives == 1
        got = job.gather_result()
        schema, want = oracle_run(ss.GroupAggregate(ss.ProjectNamedAttributes(["k2", "t"]), spec, None, child))
        assert_cols_equal(sort_rows(to_cols(got)), sort_rows(want), context="device sharded group aggregate, " + exchange)
    finally:
        dist.destroy_process_group()


# ---- CONCAT (column_aggregator.cc:496-505, aggregation_operators.h:236-283): the values of a group, printed (PrintTyped), joined
# ---- with ',' in input order; NULL inputs skipped, a group without a value is NULL.  The device orders the rows (materialise +
# ---- stable sort by the keys) and counts; the strings are printed on the host when the column is fetched ------------------------
@pytest.mark.parametrize("n", [1, 9, 2049])
def test_concat_of_dates_and_datetimes(gpu_ctx, n):
    # PrintTyped<DATE> / <DATETIME> (types_infrastructure.cc:92-114): gmtime + strftime "%Y/%m/%d[-%H:%M:%S]", microseconds dropped toward
    # zero; years before 1000 unpadded, before 0 with '-'.  DATEs inside +-24855 days (beyond that the reference's int32 product is undefined)
    rng = np.random.default_rng(n)
    schema = ss.TupleSchema([ss.Attribute("g", ss.INT32), ss.Attribute("day", ss.DATE, ss.NULLABLE), ss.Attribute("ts", ss.DATETIME, ss.NULLABLE)])
    days = rng.integers(-24855, 24856, n).astype(np.int32)
    ts = np.where(rng.random(n) < 0.5, rng.integers(-(1 << 62), 1 << 62, n), rng.integers(-4 * 10 ** 15, 4 * 10 ** 15, n))
    ts[:1] = -62135596800 * 1000000 - 1              # the last second of the year 0
    view = ss.View(schema, [rng.integers(0, 5, n).astype(np.int32), ss.Column(days, rng.random(n) < 0.2), ss.Column(ts, rng.random(n) < 0.2)])
    spec = (ss.AggregationSpecification().AddAggregation(ss.CONCAT, "day", "cd").AddAggregation(ss.CONCAT, "ts", "ct").AddDistinctAggregation(ss.CONCAT, "day", "dd")
            .AddAggregation(ss.MAX, "day", "md").AddAggregation(ss.MIN, "ts", "mt"))
    run_both(ss.ScalarAggregate(spec, ss.ScanView(view)), gpu_ctx)
    run_both(ss.GroupAggregate(ss.ProjectNamedAttribute("g"), spec, None, ss.ScanView(view)), gpu_ctx, ignore_order=True)
    run_both(ss.GroupAggregate(ss.ProjectNamedAttribute("g"), spec, ss.GroupAggregateOptions().set_max_unique_keys_in_result_(2), ss.ScanView(view)), gpu_ctx)


@pytest.mark.parametrize("n", [0, 1, 7, 1025, 30011])
def test_concat_aggregate(gpu_ctx, n):
    rng = np.random.default_rng(n + 1)
    words = np.empty(n, dtype=object)
    words[:] = [[b"baba", b"aba", b"", b"wada", b"x,y"][i] for i in rng.integers(0, 5, n)]
    schema = ss.TupleSchema([ss.Attribute("g", ss.INT32), ss.Attribute("h", ss.INT64, ss.NULLABLE), ss.Attribute("i", ss.INT32, ss.NULLABLE), ss.Attribute("u", ss.UINT64),
                             ss.Attribute("w", ss.STRING, ss.NULLABLE), ss.Attribute("d", ss.DOUBLE), ss.Attribute("f", ss.FLOAT), ss.Attribute("t", ss.BOOL, ss.NULLABLE),
                             ss.Attribute("a", ss.INT64)])
    dv = np.where(rng.random(n) < 0.2, rng.integers(-5, 5, n) * 0.5, rng.normal(size=n) * 10.0 ** rng.integers(-8, 12, n))
    if n > 6:
        dv[:6] = [float("nan"), float("inf"), float("-inf"), -0.0, 1.0 / 3.0, 1e22]
    view = ss.View(schema, [rng.integers(0, 23, n).astype(np.int32), ss.Column(rng.integers(0, 3, n), rng.random(n) < 0.2),
                            ss.Column(rng.integers(-(1 << 31), 1 << 31, n).astype(np.int32), rng.random(n) < 0.3),
                            rng.integers(0, 1 << 63, n).astype(np.uint64) * np.uint64(2), ss.Column(words, rng.random(n) < 0.2), dv, dv.astype(np.float32),
                            ss.Column(rng.integers(0, 2, n).astype(bool), rng.random(n) < 0.5), rng.integers(0, 1000, n)])
    spec = (ss.AggregationSpecification().AddAggregation(ss.CONCAT, "i", "ci").AddAggregation(ss.SUM, "a", "sa").AddAggregation(ss.CONCAT, "w", "cw")
            .AddAggregation(ss.CONCAT, "u", "cu").AddAggregation(ss.CONCAT, "d", "cd").AddAggregation(ss.CONCAT, "f", "cf").AddAggregation(ss.CONCAT, "t", "ct")
            .AddAggregation(ss.COUNT, "i", "n").AddAggregation(ss.MIN, "w", "mw"))
    flt = ss.Filter(ss.Greater(NA("a"), ss.ConstInt64(299)), ss.ProjectAllAttributes(), ss.ScanView(view))
    run_both(ss.GroupAggregate(ss.ProjectNamedAttributes(["g", "h"]), spec, None, flt), gpu_ctx, ignore_order=True)      # a NULLABLE INT64 key among them
    run_both(ss.GroupAggregate(ss.ProjectNamedAttributes(["g"]), spec, None, ss.ScanView(view)), gpu_ctx, ignore_order=True)
    run_both(ss.ScalarAggregate(spec, flt), gpu_ctx)
    order = np.argsort(view.column(0).data, kind="stable")
    clustered = ss.View(schema, [ss.Column(view.column(i).data[order], None if view.column(i).is_null is None else view.column(i).is_null[order]) for i in range(9)])
    run_both(ss.AggregateClusters(ss.ProjectNamedAttribute("g"), spec, ss.ScanView(clustered)), gpu_ctx)
    # DISTINCT CONCAT: a result row prints every value once, at its first occurrence (the DistinctAggregator in front of the CONCAT,
    # column_aggregator.cc:308-376); h has three values, t two, w five, d / f repeat their small halves and hold -0.0 next to 0.0
    dspec = (ss.AggregationSpecification().AddDistinctAggregation(ss.CONCAT, "h", "ch").AddAggregation(ss.CONCAT, "h", "ah").AddDistinctAggregation(ss.CONCAT, "w", "cw")
             .AddDistinctAggregation(ss.CONCAT, "t", "ct").AddDistinctAggregation(ss.CONCAT, "d", "cd").AddDistinctAggregation(ss.CONCAT, "f", "cf")
             .AddAggregation(ss.COUNT, "h", "n").AddDistinctAggregation(ss.CONCAT, "i", "ci"))
    run_both(ss.GroupAggregate(ss.ProjectNamedAttributes(["g"]), dspec, None, flt), gpu_ctx, ignore_order=True)
    run_both(ss.GroupAggregate(ss.ProjectNamedAttributes(["g", "h"]), dspec, None, ss.ScanView(view)), gpu_ctx, ignore_order=True)
    run_both(ss.GroupAggregate(ss.ProjectNamedAttributes(["g"]), dspec, ss.GroupAggregateOptions().set_max_unique_keys_in_result_(5), ss.ScanView(view)), gpu_ctx)
    run_both(ss.ScalarAggregate(dspec, flt), gpu_ctx)
    run_both(ss.AggregateClusters(ss.ProjectNamedAttribute("g"), dspec, ss.ScanView(clustered)), gpu_ctx)
    # CONCAT next to DISTINCT aggregates: the DISTINCT shape's rows are sorted back into input order (stored flags) before the host reads them
    mspec = (ss.AggregationSpecification().AddAggregation(ss.CONCAT, "i", "ci").AddDistinctAggregation(ss.COUNT, "h", "dh").AddDistinctAggregation(ss.CONCAT, "w", "cw")
             .AddDistinctAggregation(ss.SUM, "a", "da").AddAggregation(ss.FIRST, "i", "fi").AddAggregation(ss.COUNT, "", "n"))
    run_both(ss.GroupAggregate(ss.ProjectNamedAttributes(["g"]), mspec, None, flt), gpu_ctx, ignore_order=True)
    run_both(ss.GroupAggregate(ss.ProjectNamedAttributes(["g", "h"]), mspec, None, ss.ScanView(view)), gpu_ctx, ignore_order=True)
    run_both(ss.GroupAggregate(ss.ProjectNamedAttributes(["g"]), mspec, ss.GroupAggregateOptions().set_max_unique_keys_in_result_(5), ss.ScanView(view)), gpu_ctx)
    run_both(ss.ScalarAggregate(mspec, ss.ScanView(view)), gpu_ctx)
    run_both(ss.AggregateClusters(ss.ProjectNamedAttribute("g"), mspec, ss.ScanView(clustered)), gpu_ctx)
    # a computed CONCAT input, and the refusals: a consumer above the CONCAT, a non-STRING result type
    comp = ss.Compute(ss.CompoundExpression().Add(NA("g")).AddAs("s", ss.Plus(NA("a"), ss.ConstInt64(7))), ss.ScanView(view))
    run_both(ss.GroupAggregate(ss.ProjectNamedAttributes(["g"]), ss.AggregationSpecification().AddAggregation(ss.CONCAT, "s", "cs"), None, comp), gpu_ctx, ignore_order=True)
    for bad, code in ((ss.Sort(ss.SortOrder().add("g", ss.ASCENDING), None, 0, ss.GroupAggregate(ss.ProjectNamedAttributes(["g"]), ss.AggregationSpecification().AddAggregation(ss.CONCAT, "i", "c"), None, ss.ScanView(view))), ss.ERROR_NOT_IMPLEMENTED),
                      (ss.ScalarAggregate(ss.AggregationSpecification().AddAggregationWithDefinedOutputType(ss.CONCAT, "i", "c", ss.INT64), ss.ScanView(view)), ss.ERROR_INVALID_ARGUMENT_TYPE)):
        with pytest.raises(ss.SupersonicException) as e:
            ss.Plan(bad, gpu_ctx)
        assert e.value.return_code == code


# ---- wide schemas: every staged array (column or NULL mask) takes a slot of the kernel's argument block ---------------------------------
@pytest.mark.parametrize("n_in,dtype", [(24, "f8"), (26, "f8"), (32, "f8"), (40, "i4")])
def test_compute_over_many_nullable_columns(gpu_ctx, n_in, dtype):
    """26 NULLABLE DOUBLE columns are 52 staged arrays: until round 6 VmParams::staged held 48 and nothing checked -- the first and the last
    result columns came back wrong (found through the chunked GroupAggregate's merging plan, which reads 26 such columns)."""
    n = 5003
    rng = np.random.default_rng(n_in)
    schema = ss.TupleSchema([ss.Attribute("c%d" % i, ss.DOUBLE if dtype == "f8" else ss.INT32, ss.NULLABLE) for i in range(n_in)])
    view = ss.View(schema, [ss.Column(rng.integers(-1000, 1000, n).astype(dtype), rng.random(n) < 0.1) for _ in range(n_in)])
    e = ss.CompoundExpression()
    for i in range(0, n_in - 1, 2):
        e.AddAs("s%d" % i, ss.Plus(NA("c%d" % i), NA("c%d" % (i + 1))))
    run_both(ss.Compute(e, ss.ScanView(view)), gpu_ctx)
