"""PARSE_STRING (ParseStringQuiet / ParseStringNulling) on the device: the table kernel (string_parse_kernels.hip) entry by entry
through ssgpu_dict_parse for all seven targets -- both of its forms, one lane per value and a wave per long value, and for FLOAT /
DOUBLE the split between the device's exact fast path and the host's strtof / strtod --, then rows through plans wherever an
expression is legal.  The oracle does not know these operators: the expected values are tests/parse_string_model.py, which
tests/test_parse_string_cpu.py pins to the reference's own rows."""
import ctypes as C

import numpy as np
import pytest

import supersonic_amd as ss
import parse_string_model as model
import parse_string_pool as pool
from helpers import to_cols, assert_cols_equal

NA = ss.NamedAttribute
pytestmark = pytest.mark.gpu
TARGETS = [ss.INT32, ss.UINT32, ss.INT64, ss.UINT64, ss.FLOAT, ss.DOUBLE, ss.BOOL]
NAMES = {ss.INT32: "INT32", ss.UINT32: "UINT32", ss.INT64: "INT64", ss.UINT64: "UINT64", ss.FLOAT: "FLOAT", ss.DOUBLE: "DOUBLE", ss.BOOL: "BOOL"}
NP = {ss.INT32: np.int32, ss.UINT32: np.uint32, ss.INT64: np.int64, ss.UINT64: np.uint64, ss.FLOAT: np.float32, ss.DOUBLE: np.float64, ss.BOOL: np.bool_}
UINT = {1: np.uint8, 4: np.uint32, 8: np.uint64}
_CACHE = {}


def parsed(t, v):
    """model.parse, remembered per (type, value): the expected value and whether the parse fails"""
    key = (t, v)
    if key not in _CACHE:
        _CACHE[key] = model.parse(t, v)
    return _CACHE[key]


def hard_count(t, values):
    return sum(1 for v in values if model.fast_path(t, v) is False)


def check_tables(d, t, ctx, label):
    """every entry of both tables against the model, bit for bit; returns host_resolved"""
    values = d.values
    got, failed, resolved = d.parse(t, context=ctx)
    assert got.dtype == NP[t] and len(got) == len(failed) == len(values)
    width = np.dtype(NP[t]).itemsize
    have = np.ascontiguousarray(got).view(UINT[width])
    want = np.array([model.bits(t, parsed(t, v)[0]) for v in values], np.uint64).astype(UINT[width])
    want_failed = np.array([parsed(t, v)[1] for v in values], bool)
    bad = np.nonzero((have != want) | (failed != want_failed))[0]
    assert len(bad) == 0, "%s to %s: %d entries differ, first %s: value %r (%d bytes) got %s failed %s, want %s failed %s" % (
        label, NAMES[t], len(bad), bad[:3], values[bad[0]][:40], len(values[bad[0]]), got[bad[0]], failed[bad[0]], parsed(t, values[bad[0]])[0], want_failed[bad[0]])
    return resolved


@pytest.fixture(scope="module")
def specialized_ctx():
    c = ss.Context(0)
    c.set_option("specialize", 1)
    return c


@pytest.fixture(params=["interpreted", "specialized"])
def any_ctx(request, gpu_ctx, specialized_ctx):
    return (gpu_ctx, False) if request.param == "interpreted" else (specialized_ctx, True)


def run(plan, view=None):
    plan.run(view)
    return to_cols(plan.fetch())


def ran_compiled(plan):
    return all(st["specialized"] & 1 for st in plan.stage_info() if st["kind"] in (1, 2, 3))


# ---- the table kernel, entry by entry --------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def general():
    return ss.StringDictionary(pool.general_pool())


@pytest.mark.parametrize("t", TARGETS, ids=[NAMES[t] for t in TARGETS])
def test_table_kernel_entry_by_entry(gpu_ctx, general, t):
    resolved = check_tables(general, t, gpu_ctx, "general pool")
    assert resolved == (hard_count(t, general.values) if t in (ss.FLOAT, ss.DOUBLE) else 0)


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 257])
def test_table_sizes_around_a_wave_and_a_block(gpu_ctx, n):
    values = pool.general_pool()[:n]
    d = ss.StringDictionary(values)
    for t in (ss.INT64, ss.BOOL, ss.FLOAT):
        check_tables(d, t, gpu_ctx, "%d values" % n)


@pytest.mark.parametrize("t", TARGETS, ids=[NAMES[t] for t in TARGETS])
def test_lane_and_wave_forms_agree_at_the_threshold_lengths(gpu_ctx, t):
    # a dictionary of nothing but the threshold values: whole waves of long values, each at another offset in the heap.  Up to 128
    # bytes one lane parses a value, beyond that a wave in steps of 1024 bytes: the same number padded to 127 ... 5000 bytes is
    # the same number in both forms
    values = pool.threshold_values()
    assert {len(v) for v in values} >= set(pool.THRESHOLD_LENGTHS)
    d = ss.StringDictionary(values)
    check_tables(d, t, gpu_ctx, "threshold values")
    for n in pool.THRESHOLD_LENGTHS:
        if t in (ss.FLOAT, ss.DOUBLE, ss.BOOL):
            continue
        assert parsed(t, b" " * (n - 1) + b"7") == (7, False) and parsed(t, b"0" * (n - 1) + b"7") == (7, False)


def test_long_values_one_bad_byte_at_every_place(gpu_ctx):
    # 1100 digits, one of them replaced by a byte that ends the number -- in every lane's 16 bytes of the first step and on into the
    # second: the digits in front of it are far more than 20, so every integer type overflows, but a 0x00 cuts the value there
    size, values = 1100, []
    for p in list(range(0, 40)) + list(range(1000, 1100, 3)):
        for c in (b"x", b"\x00", b" "):
            values.append(b"0" * p + c + b"1" * (size - 1 - p))
            values.append(b"0" * (size - 30) + b"123" + b"4" * (p % 17) + c + b"5" * (26 - p % 17))
    d = ss.StringDictionary(values)
    for t in (ss.INT32, ss.UINT64, ss.DOUBLE):
        check_tables(d, t, gpu_ctx, "one bad byte")


@pytest.mark.parametrize("t", [ss.FLOAT, ss.DOUBLE], ids=["FLOAT", "DOUBLE"])
def test_floating_fast_path_is_exact_and_stays_on_the_device(gpu_ctx, t):
    d = ss.StringDictionary(pool.fast_decimals(t))
    assert len(d) == 2000
    resolved = check_tables(d, t, gpu_ctx, "fast decimals")            # bit-equal to libc
    assert resolved == 0                                               # a condition: these inputs lie inside the fast path by construction


@pytest.mark.parametrize("t", [ss.FLOAT, ss.DOUBLE], ids=["FLOAT", "DOUBLE"])
def test_floating_hard_road_goes_to_the_host(gpu_ctx, t):
    values = pool.hard_floats()
    d = ss.StringDictionary(values)
    resolved = check_tables(d, t, gpu_ctx, "hard values")
    assert resolved == hard_count(t, d.values) and resolved >= len(values) - 4
    # mixed with values the device keeps: only the hard ones travel
    mixed = ss.StringDictionary(values + pool.fast_decimals(t)[:500] + [b""])
    assert check_tables(mixed, t, gpu_ctx, "mixed") == resolved


# ---- rows through plans -----------------------------------------------------------------------------------------------------
def row_pool():
    rng = np.random.default_rng(437)
    vals = {b"", b" ", b"12", b" 12 ", b"-7", b"+7", b"12x", b"x12", b"2147483647", b"2147483648", b"-2147483649", b"1.5", b"-1.", b"1e3", b"1.OOPS", b"nan", b"inf",
            b"true", b" YES\t", b"no", b"False", b"1", b"12\x003", b"\x0012", b"\xa012", b"0x10", b"010", b"- 5", b"1e400", b"0.1", b" " * 200 + b"7", b"0" * 300 + b"12"}
    while len(vals) < 300:
        k = int(rng.integers(0, 6))
        n = int(rng.integers(-1000, 1000))
        vals.add([b"%d" % n, b" %d" % n, b"%d " % n, b"%d.%d" % (n, abs(n) % 7), b"%de%d" % (n, n % 5), b"%dq" % n][k])
    return np.array(sorted(vals), dtype=object)


def row_view(n, seed=0):
    rng = np.random.default_rng(seed + n)
    values = row_pool()
    s = values[rng.integers(0, len(values), n)]
    nulls = rng.random(n) < 0.2
    s[::5] = values[0]                  # rows that carry code 0 next to NULL rows, which carry it too: NULL in is NULL out, never a table's entry 0
    nulls[1::5] = True
    t = values[rng.integers(0, len(values), n)]
    schema = ss.TupleSchema([ss.Attribute("s", ss.STRING, ss.NULLABLE), ss.Attribute("t", ss.STRING), ss.Attribute("id", ss.INT32)])
    return ss.View(schema, [ss.Column(s, nulls), t, np.arange(n, dtype=np.int32)])


def want_parse(to, data, nulls, nulling, pre=lambda v: v):
    vals = np.array([parsed(to, pre(v))[0] for v in data], NP[to])
    failed = np.array([parsed(to, pre(v))[1] for v in data], bool)
    z = np.zeros(len(data), bool) if nulls is None else nulls
    return vals, (z | failed) if nulling else (z if nulls is not None else None)


def parity_expr():
    # every width under both functions: Quiet emits the gather alone, Nulling the failure byte too
    Q, N = ss.ParseStringQuiet, ss.ParseStringNulling
    return (ss.CompoundExpression().AddAs("q32", Q(ss.INT32, NA("s"))).AddAs("n32", N(ss.INT32, NA("s"))).AddAs("n64", N(ss.UINT64, NA("t")))
            .AddAs("qd", Q(ss.DOUBLE, NA("s"))).AddAs("nf", N(ss.FLOAT, NA("t"))).AddAs("qb", Q(ss.BOOL, NA("s"))).AddAs("nb", N(ss.BOOL, NA("t"))))


def parity_want(view):
    s, sz, t = view.column(0).data, view.column(0).is_null, view.column(1).data
    return [want_parse(ss.INT32, s, sz, False), want_parse(ss.INT32, s, sz, True), want_parse(ss.UINT64, t, None, True), want_parse(ss.DOUBLE, s, sz, False),
            want_parse(ss.FLOAT, t, None, True), want_parse(ss.BOOL, s, sz, False), want_parse(ss.BOOL, t, None, True)]


@pytest.mark.parametrize("n", [1, 70000])
def test_row_parity(any_ctx, n):
    ctx, compiled = any_ctx
    view = row_view(n)
    plan = ss.Plan(ss.Compute(parity_expr(), ss.ScanView(view)), ctx, extra_strings=list(row_pool()))      # (one dictionary for every n: one program)
    got = run(plan)
    assert ran_compiled(plan) == compiled, plan.specialize_reason()
    want = parity_want(view)
    assert_cols_equal(got, want, context="row parity, %d rows" % n)
    assert got[0][1] is not None and got[3][1] is not None
    if n > 1:
        sz = view.column(0).is_null
        assert np.array_equal(got[0][1], sz) and np.array_equal(got[5][1], sz)        # Quiet: NULL exactly where the argument is
        assert (got[1][1] & ~sz).any() and (~got[1][1]).any()                          # Nulling: failed parses too, and not everything
    # the plan's counter: what the host resolved for its floating tables (FLOAT and DOUBLE here)
    values = plan.strings.values
    line = [ln for ln in plan.describe().splitlines() if "PARSE_STRING to DOUBLE" in ln]
    assert len(line) == 1 and line[0].endswith(": %d" % (hard_count(ss.FLOAT, values) + hard_count(ss.DOUBLE, values))), line


@pytest.fixture(scope="module")
def small():
    return row_view(5000, seed=3)


def test_filter_on_a_parsed_value(gpu_ctx, small):
    s, sz, ids = small.column(0).data, small.column(0).is_null, small.column(2).data
    op = ss.Filter(ss.Greater(ss.ParseStringNulling(ss.INT32, NA("s")), ss.ConstInt32(100)), ss.ProjectNamedAttributes(["id"]), ss.ScanView(small))
    (got, _z), = run(ss.Plan(op, gpu_ctx))
    keep = [i for i in range(len(s)) if not sz[i] and not parsed(ss.INT32, s[i])[1] and parsed(ss.INT32, s[i])[0] > 100]
    assert len(keep) > 100 and got.tolist() == ids[keep].tolist()
    # Quiet keeps the failed rows with the parser's value: "2147483648" is INT32's max, "12x" is 12
    op = ss.Filter(ss.Greater(ss.ParseStringQuiet(ss.INT32, NA("t")), ss.ConstInt32(100)), ss.ProjectNamedAttributes(["id"]), ss.ScanView(small))
    (got, _z), = run(ss.Plan(op, gpu_ctx))
    t = small.column(1).data
    assert got.tolist() == [int(ids[i]) for i in range(len(t)) if parsed(ss.INT32, t[i])[0] > 100]


def test_group_by_a_parsed_value_with_sum_of_another(gpu_ctx, small):
    e = ss.CompoundExpression().AddAs("k", ss.ParseStringNulling(ss.INT32, NA("s"))).AddAs("v", ss.ParseStringQuiet(ss.INT64, NA("t")))
    spec = ss.AggregationSpecification().AddAggregation(ss.SUM, "v", "sum").AddAggregation(ss.COUNT, "", "n")
    got = run(ss.Plan(ss.GroupAggregate(ss.ProjectNamedAttributes(["k"]), spec, None, ss.Compute(e, ss.ScanView(small))), gpu_ctx))
    s, sz, t = small.column(0).data, small.column(0).is_null, small.column(1).data
    want = {}
    for i in range(len(s)):
        k = None if sz[i] or parsed(ss.INT32, s[i])[1] else parsed(ss.INT32, s[i])[0]
        a = want.setdefault(k, [0, 0])
        a[0] += parsed(ss.INT64, t[i])[0]
        a[1] += 1
    (kd, kz), (sd, _sz), (nd, _nz) = got
    have = {(None if kz[i] else int(kd[i])): [int(sd[i]), int(nd[i])] for i in range(len(kd))}
    assert have == want and len(have) == len(kd) and None in have and len(have) > 50


def test_sort_by_a_parsed_value(gpu_ctx, small):
    e = ss.CompoundExpression().AddAs("p", ss.ParseStringQuiet(ss.INT32, NA("t"))).AddAs("id", NA("id"))
    (pd, _pz), (idd, _iz) = run(ss.Plan(ss.Sort(ss.SortOrder().add("p", ss.DESCENDING), None, 0, ss.Compute(e, ss.ScanView(small))), gpu_ctx))
    t = small.column(1).data
    assert pd.tolist() == sorted((parsed(ss.INT32, v)[0] for v in t), reverse=True) and pd[0] == 2 ** 31 - 1 and pd[-1] == -2 ** 31
    assert [parsed(ss.INT32, t[i])[0] for i in idd] == pd.tolist() and sorted(idd.tolist()) == list(range(len(t)))


def test_parse_of_a_constant(gpu_ctx, small):
    n = small.row_count()
    e = (ss.CompoundExpression().AddAs("c", ss.ParseStringQuiet(ss.INT32, ss.ConstString(" 42 "))).AddAs("bad", ss.ParseStringNulling(ss.INT64, ss.ConstString("4x2")))
         .AddAs("null", ss.ParseStringQuiet(ss.DOUBLE, ss.Null(ss.STRING))).AddAs("same", ss.ParseStringNulling(ss.STRING, NA("t"))))
    got = run(ss.Plan(ss.Compute(e, ss.ScanView(small)), gpu_ctx))
    assert got[0][0].tolist() == [42] * n and (got[0][1] is None or not got[0][1].any())
    assert got[1][1].all() and got[2][1].all()
    assert got[3][0].tolist() == small.column(1).data.tolist()


def test_parse_of_trim_over_a_closed_dictionary(any_ctx, small):
    ctx, compiled = any_ctx
    e = (ss.CompoundExpression().AddAs("n", ss.ParseStringNulling(ss.INT32, ss.Trim(NA("s")))).AddAs("q", ss.ParseStringQuiet(ss.BOOL, ss.ToUpper(NA("t"))))
         .AddAs("plain", ss.ParseStringNulling(ss.INT32, NA("s"))))
    plan = ss.Plan(ss.Compute(e, ss.ScanView(small)), ctx)
    got = run(plan)
    assert ran_compiled(plan) == compiled, plan.specialize_reason()
    s, sz, t = small.column(0).data, small.column(0).is_null, small.column(1).data
    assert_cols_equal(got, [want_parse(ss.INT32, s, sz, True, lambda v: v.strip(b" ")), want_parse(ss.BOOL, t, None, False, lambda v: v.upper()),
                            want_parse(ss.INT32, s, sz, True)], context="parse over a closed dictionary")


def test_all_null_column_and_empty_dictionary(any_ctx):
    ctx, compiled = any_ctx
    n = 700
    schema = ss.TupleSchema([ss.Attribute("s", ss.STRING, ss.NULLABLE)])
    view = ss.View(schema, [ss.Column(np.array([b""] * n, dtype=object), np.ones(n, bool))])
    e = ss.CompoundExpression().AddAs("q", ss.ParseStringQuiet(ss.INT64, NA("s"))).AddAs("n", ss.ParseStringNulling(ss.BOOL, NA("s"))).AddAs("d", ss.ParseStringNulling(ss.DOUBLE, NA("s")))
    plan = ss.Plan(ss.Compute(e, ss.ScanView(view)), ctx)
    assert len(plan.strings) == 0                       # nothing but NULLs: every table is its one dummy entry
    got = run(plan)
    assert ran_compiled(plan) == compiled
    assert all(z.all() and len(z) == n for _d, z in got)


def test_hash_join_and_parse_table_in_one_pipeline(gpu_ctx, small):
    m = 40
    rview = ss.View(ss.TupleSchema([ss.Attribute("rid", ss.INT32), ss.Attribute("w", ss.INT64)]), [np.arange(m, dtype=np.int32), np.arange(m) * 1000])
    e = ss.CompoundExpression().AddAs("key", ss.Modulus(NA("id"), ss.ConstInt32(64))).AddAs("s", NA("s")).AddAs("t", NA("t"))
    proj = ss.CompoundMultiSourceProjector().add(0, ss.ProjectAllAttributes()).add(1, ss.ProjectNamedAttributes(["w"]))
    join = ss.HashJoin(ss.LEFT_OUTER, ss.ProjectNamedAttribute("key"), ss.ProjectNamedAttribute("rid"), proj, ss.UNIQUE, ss.Compute(e, ss.ScanView(small)), ss.ScanView(rview))
    out = (ss.CompoundExpression().AddAs("w", NA("w")).AddAs("p", ss.ParseStringNulling(ss.INT64, NA("s")))
           .AddAs("both", ss.Plus(NA("w"), ss.ParseStringQuiet(ss.INT64, NA("t")))))
    plan = ss.Plan(ss.Compute(out, join), gpu_ctx)
    assert len(plan.stage_info()) == 1                       # one pipeline: the probe, the rhs gather and the parse tables
    got = run(plan)
    s, sz, t, ids = small.column(0).data, small.column(0).is_null, small.column(1).data, small.column(2).data
    w, wz = (ids % 64).astype(np.int64) * 1000, (ids % 64) >= m
    tv, _z = want_parse(ss.INT64, t, None, False)
    with np.errstate(over="ignore"):
        both = w + tv
    assert_cols_equal(got, [(w, wz), want_parse(ss.INT64, s, sz, True), (both, wz)], context="join + parse tables")


def test_run_host_in_chunks(gpu_ctx, small):
    s, sz, t, ids = small.column(0).data, small.column(0).is_null, small.column(1).data, small.column(2).data
    plan = ss.Plan(ss.Filter(ss.Less(ss.ParseStringNulling(ss.DOUBLE, NA("t")), ss.ConstDouble(0.5)), ss.ProjectNamedAttributes(["id"]), ss.ScanView(small)), gpu_ctx)
    assert plan.chunked_form()[0] == 2
    plan.run_host(chunk_rows=1000)
    (got, _z), = to_cols(plan.fetch())
    assert got.tolist() == [int(ids[i]) for i in range(len(t)) if not parsed(ss.DOUBLE, t[i])[1] and parsed(ss.DOUBLE, t[i])[0] < 0.5]
    # GroupAggregate first: the per-chunk plan and the merging plan are derived inside the library and inherit the dictionary and its tables
    e = ss.CompoundExpression().AddAs("k", ss.ParseStringQuiet(ss.BOOL, NA("t"))).AddAs("v", ss.ParseStringNulling(ss.INT64, NA("s")))
    spec = ss.AggregationSpecification().AddAggregation(ss.SUM, "v", "sum").AddAggregation(ss.COUNT, "v", "n")
    plan = ss.Plan(ss.GroupAggregate(ss.ProjectNamedAttributes(["k"]), spec, None, ss.Compute(e, ss.ScanView(small))), gpu_ctx)
    assert plan.chunked_form()[0] == 3
    plan.run_host(chunk_rows=1000)
    (kd, _kz), (sd, sn), (nd, _nz) = to_cols(plan.fetch())
    want = {}
    for i in range(len(t)):
        a = want.setdefault(bool(parsed(ss.BOOL, t[i])[0]), [0, 0])
        if not sz[i] and not parsed(ss.INT64, s[i])[1]:
            a[0] += parsed(ss.INT64, s[i])[0]
            a[1] += 1
    have = {bool(kd[i]): [0 if (sn is not None and sn[i]) else int(sd[i]), int(nd[i])] for i in range(len(kd))}
    assert have == want and len(have) == 2


def test_bound_expression_evaluate(gpu_ctx, small):
    e = ss.CompoundExpression().AddAs("n", ss.ParseStringNulling(ss.INT32, NA("s"))).AddAs("q", ss.ParseStringQuiet(ss.FLOAT, NA("t")))
    tree = e.Bind(small.schema(), None, 0, gpu_ctx)
    r = tree.Evaluate(small)
    assert not r.is_failure(), r.exception()
    s, sz, t = small.column(0).data, small.column(0).is_null, small.column(1).data
    assert_cols_equal(to_cols(r.view()), [want_parse(ss.INT32, s, sz, True), want_parse(ss.FLOAT, t, None, False)], context="Evaluate")
    # DoEvaluate: skipped rows are NULL, the others as above
    skip = np.zeros(len(s), bool)
    skip[::3] = True
    r = tree.DoEvaluate(small, [skip.copy(), None])
    assert not r.is_failure(), r.exception()
    got = to_cols(r.view())
    assert_cols_equal([got[0]], [want_parse(ss.INT32, s, sz | skip, True)], context="DoEvaluate")


def test_tables_are_rebuilt_for_another_dictionary(gpu_ctx):
    schema = ss.TupleSchema([ss.Attribute("s", ss.STRING)])
    first = ss.View(schema, [np.array([b"12", b" 7", b"", b"x"], dtype=object)])
    e = ss.CompoundExpression().AddAs("n", ss.ParseStringNulling(ss.INT32, NA("s"))).AddAs("d", ss.ParseStringQuiet(ss.DOUBLE, NA("s")))

    def want(view):
        return [want_parse(ss.INT32, view.column(0).data, None, True), want_parse(ss.DOUBLE, view.column(0).data, None, False)]
    plan = ss.Plan(ss.Compute(e, ss.ScanView(first)), gpu_ctx)
    assert_cols_equal(run(plan), want(first))
    # an extension by values that sort behind every old one keeps the old codes and adds new ones
    old = plan.strings
    more = [b"z 1", b"y" + b" " * 300, b"\x7f77", b"~1e400"]
    more = [b"\xff" + v for v in more] + [b"\xfe"]
    wider, remap = old.extend(more)
    assert remap.tolist() == list(range(len(old))) and len(wider) == len(old) + 5
    plan.ctx.check(plan.lib.ssgpu_plan_set_dict(plan.handle, wider.handle))
    plan.strings = wider
    second = ss.View(schema, [np.array(more + [b"12", b""], dtype=object)])
    assert_cols_equal(run(plan, second), want(second), context="after a second ssgpu_plan_set_dict")
    plan.ctx.check(plan.lib.ssgpu_plan_set_dict(plan.handle, old.handle))     # and back: the tables follow the handle
    plan.strings = old
    assert_cols_equal(run(plan, first), want(first))


def test_run_without_a_dictionary_names_the_function(gpu_ctx):
    # straight through the C ABI: a plan nobody handed a dictionary
    lib, L = gpu_ctx.lib, ss._lib
    attrs = (L.Attr * 1)(L.Attr(b"s", ss.STRING, 0))
    exprs = (L.Expr * 2)(L.Expr(L.EXPR_ATTR_NAMED, 0, 0, 0, 0, 0, 0, 0.0, b"s"), L.Expr(L.EXPR_OP, 438, ss.INT32, 0, 1, 0, 0, 0.0, None))
    args = (C.c_int32 * 1)(0)
    h = C.c_void_p()
    gpu_ctx.check(lib.ssgpu_expr_bind(gpu_ctx.handle, attrs, 1, exprs, 2, args, 1, 1, 0, C.byref(h)))
    try:
        blk = ss.DeviceBlock(ss.TupleSchema([ss.Attribute("c", ss.INT32)]), 4, gpu_ctx)
        cols = (L.Column * 1)()
        cols[0].data = blk.column_ptr(0)
        res = C.c_void_p()
        rc = lib.ssgpu_plan_run(h, cols, 1, 0, C.byref(res))
        assert rc == ss.ERROR_INVALID_ARGUMENT_VALUE and "PARSE_STRING" in gpu_ctx.last_error() and "ssgpu_plan_set_dict" in gpu_ctx.last_error()
    finally:
        lib.ssgpu_plan_destroy(h)
