"""LENGTH, STRING_OFFSET, StringContains and StringContainsCI on the device: the table kernel (string_fn_kernels.hip) through
ssgpu_dict_eval entry by entry, the reference's own rows (tests/golden/string_expression_cases.json), row-level parity under the
interpreting and the specialised kernel, every place an expression is legal once, and a seeded fuzz of small plans.  The oracle
does not know these operators: the expected values are the Python restatement LENGTH = len(b), STRING_OFFSET = b.find(n) + 1,
StringContainsCI = b.lower().find(n.lower()) >= 0 (bytes.lower() folds ASCII only, like ascii_tolower)."""
import ctypes as C
import json
import os

import numpy as np
import pytest

import supersonic_amd as ss
from helpers import to_cols, assert_cols_equal

NA = ss.NamedAttribute
pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = json.load(open(os.path.join(ROOT, "tests", "golden", "string_expression_cases.json")))
LONG = 128          # string_fn_kernels.hip STRFN_LONG: up to this length one lane searches a string, beyond it a whole wave
LENGTH, OFFSET = ss.StringDictionary.LENGTH, ss.StringDictionary.STRING_OFFSET


# ---- the Python restatement ----------------------------------------------------------------------------------------------
def py_offset(b, n, fold=False):
    return (b.lower().find(n.lower()) if fold else b.find(n)) + 1


def want_length(data, nulls):
    return np.array([len(v) for v in data], np.uint32), nulls


def want_offset(data, nulls, needle, fold=False):
    if needle is None:
        return np.zeros(len(data), np.int32), np.ones(len(data), bool)
    return np.array([py_offset(v, needle, fold) for v in data], np.int32), nulls


def want_contains(data, nulls, needle, fold=False):
    d, z = want_offset(data, nulls, needle, fold)
    return d > 0, z


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
    """the last run's pipeline stages ran their runtime-compiled kernel (bit 0 of ssgpu_stage_info.specialized: the main program)"""
    return all(st["specialized"] & 1 for st in plan.stage_info() if st["kind"] in (1, 2, 3))


# ---- the table kernel, entry by entry -------------------------------------------------------------------------------------
def kernel_pool():
    """257 distinct values, the interesting ones first (a dictionary of the first n keeps them)."""
    rng = np.random.default_rng(20)
    abc = np.frombuffer(b"abAB", np.uint8)

    def rnd(n, alphabet=abc):
        return bytes(alphabet[rng.integers(0, len(alphabet), n)])
    long_one = rnd(1500) + b"QQ" + rnd(2500) + b"QQ" + rnd(997) + b"Z"          # 5002 bytes; "QQ" twice, far apart; 'Z' only at the end
    pool = [long_one, b"", b"a", rnd(LONG - 2) + b"Z", rnd(LONG - 1) + b"Z", rnd(LONG) + b"Z",      # lengths 127, 128, 129
            b"a\x00b\x00", b"\x00", b"\x80\xff\xc4bc", b"\xe4bc", b"\xc4BC", b"MiXeD CaSe Dog", b"aaab", b"xaaabaab", b"Two dogs", b"QQ..QQ",
            rnd(LONG + 40) + b"aab" + rnd(300), b"a" * 700 + b"b", b"A" * 127 + b"b", b"Z"]
    fill = np.frombuffer(b"abAB\x00\xc4\xe4Z", np.uint8)
    seen = set(pool)
    while len(pool) < 257:
        v = rnd(int(rng.integers(0, 41)), fill)
        if v not in seen:
            seen.add(v)
            pool.append(v)
    assert len(set(pool)) == 257
    return pool


def kernel_needles(pool):
    long_one, t127, t128, t129 = pool[0], pool[3], pool[4], pool[5]
    return [b"", long_one, long_one + b"x", t127, t128, t129, t128 + b"!", t127[1:], t129[:-1],      # empty, whole string, one byte longer
            b"Z", long_one[-5:],                                                                        # only at the last byte(s)
            b"QQ", b"aab", b"ab", b"AB", b"aaab", b"a" * 3 + b"b", b"a" * 130 + b"b",                  # twice / self-overlapping
            b"\x00", b"a\x00b", b"\x00\x00", b"\xc4", b"\xe4bc", b"\xe4BC", b"\x80\xff", b"dog", b"DOG", b"mixed case",
            long_one[1000:1040], long_one[1490:1510], t129[100:]]


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 257])
def test_table_kernel_entry_by_entry(gpu_ctx, n):
    pool = kernel_pool()
    d = ss.StringDictionary(pool[:n])
    values = d.values
    assert len(values) == n
    got = d.eval(LENGTH, context=gpu_ctx)
    assert got.tolist() == [len(v) for v in values]
    for needle in kernel_needles(pool):
        for fold in (False, True):
            got = d.eval(OFFSET, needle, fold, context=gpu_ctx)
            want = [py_offset(v, needle, fold) for v in values]
            bad = [i for i in range(n) if got[i] != want[i]]
            assert not bad, "needle %r fold %s: values %s got %s want %s" % (needle[:20], fold, [values[i][:20] for i in bad[:3]], got[bad[:3]], [want[i] for i in bad[:3]])


def test_wave_form_finds_a_match_across_every_chunk_boundary(gpu_ctx):
    # the wave form gives every lane 16 consecutive bytes of the heap per step (64 x 16 per step): a 4-byte needle at EVERY position of
    # a 1300-byte value starts in one lane's bytes and ends in the next lane's (or the next step's) at every boundary, whatever the
    # value's own alignment in the heap
    size = 1300
    values = [b"." * p + b"NEED" + b"." * (size - 4 - p) for p in range(size - 3)]
    # ... and twice, in different lanes and different steps: the earlier one is reported
    values += [b"-" * p + b"NEED" + b"-" * q + b"NEED" + b"-" * 7 for p, q in ((0, 1), (3, 9), (15, 16), (17, 1100), (1000, 30), (1023, 1), (1030, 2000))]
    values += [b"." * 2000 + b"NEE", b"NEE" + b"." * 2000 + b"EED", b"n" * 2000 + b"eEd!"]          # absent / only after folding
    d = ss.StringDictionary(values)
    ordered = d.values
    for needle, fold in ((b"NEED", False), (b"need", True), (b"need", False), (b"D", False), (b"EED-", False), (b"NEED.", False)):
        got = d.eval(OFFSET, needle, fold, context=gpu_ctx)
        want = np.array([py_offset(v, needle, fold) for v in ordered], np.int32)
        assert np.array_equal(got, want), (needle, fold, np.nonzero(got != want)[0][:5])


def test_table_kernel_threshold_lengths(gpu_ctx):
    # lengths on both sides of the lane / wave threshold, the needle at the start, in the middle, at the end, and absent
    values = []
    for n in (LONG - 1, LONG, LONG + 1, LONG + 15, LONG + 16, LONG + 17):
        for p in (0, 1, n // 2, n - 3, n - 2):
            values.append(b"x" * p + b"ab" + b"y" * (n - 2 - p))
        values.append(b"x" * (n - 1) + b"a")
    d = ss.StringDictionary(values)
    for needle in (b"ab", b"b", b"a", b"xab", b"aby", b"y" * 60 + b"a"):
        got = d.eval(OFFSET, needle, context=gpu_ctx)
        assert got.tolist() == [py_offset(v, needle) for v in d.values], needle


# ---- the reference's rows --------------------------------------------------------------------------------------------------
def string_view(rows_, nullable=True):
    data = np.array([(v.encode() if v is not None else b"") for v in rows_], dtype=object)
    nulls = np.array([v is None for v in rows_])
    schema = ss.TupleSchema([ss.Attribute("s", ss.STRING, ss.NULLABLE if nullable else ss.NOT_NULLABLE)])
    return ss.View(schema, [ss.Column(data, nulls) if nullable else data])


def test_golden_rows(any_ctx):
    ctx, compiled = any_ctx
    ev = GOLDEN["evaluation"]
    rows = ev["Length"]["rows"]
    plan = ss.Plan(ss.Compute(ss.Length(NA("s")), ss.ScanView(string_view([r[0] for r in rows]))), ctx)
    (data, nulls), = run(plan)
    assert data.dtype == np.uint32 and nulls.tolist() == [r[1] is None for r in rows]
    assert [int(x) for x, r in zip(data, rows) if r[1] is not None] == [r[1] for r in rows if r[1] is not None]
    assert ran_compiled(plan) == compiled
    # one plan per distinct needle over the rows that carry it; a NULL needle is Null(STRING)
    needles = []
    for r in ev["StringOffset"]["rows"]:
        if r[1] not in needles:
            needles.append(r[1])
    for needle in needles:
        idx = [i for i, r in enumerate(ev["StringOffset"]["rows"]) if r[1] == needle]
        hay = [ev["StringOffset"]["rows"][i][0] for i in idx]
        for name in ("StringOffset", "StringContains", "StringContainsCI"):
            assert [ev[name]["rows"][i][:2] for i in idx] == [[h, needle] for h in hay]       # the three vectors share their inputs

        def n_expr():
            return ss.Null(ss.STRING) if needle is None else ss.ConstString(needle)
        e = (ss.CompoundExpression().AddAs("off", ss.StringOffset(NA("s"), n_expr())).AddAs("has", ss.StringContains(NA("s"), n_expr()))
             .AddAs("has_ci", ss.StringContainsCI(NA("s"), n_expr())))
        plan = ss.Plan(ss.Compute(e, ss.ScanView(string_view(hay))), ctx)
        got = run(plan)
        assert ran_compiled(plan) == compiled
        for (data, nulls), name in zip(got, ("StringOffset", "StringContains", "StringContainsCI")):
            want = [ev[name]["rows"][i][2] for i in idx]
            assert nulls.tolist() == [w is None for w in want], (name, needle)
            assert [x.item() for x, w in zip(data, want) if w is not None] == [w for w in want if w is not None], (name, needle)


# ---- row-level parity --------------------------------------------------------------------------------------------------------
def parity_pool():
    rng = np.random.default_rng(5)
    abc = np.frombuffer(b"abcABC .", np.uint8)
    vals = {b"", b"a", b"abc", b"ABC", b"xabcabc", b"\xc4bc", b"\xe4BC", b"ab\x00c"}
    while len(vals) < 300:
        vals.add(bytes(abc[rng.integers(0, len(abc), int(rng.integers(0, 30)))]))
    vals.add(bytes(abc[rng.integers(0, len(abc), 400)]) + b"abc")
    return np.array(sorted(vals), dtype=object)


def parity_view(n, seed=0):
    rng = np.random.default_rng(seed + n)
    pool = parity_pool()
    s = pool[rng.integers(0, len(pool), n)]
    # NULL rows next to rows that carry code 0 (the pool's smallest value): NULL in gives NULL out, never T[0]
    nulls = rng.random(n) < 0.2
    s[::5] = pool[0]
    nulls[1::5] = True
    t = pool[rng.integers(0, len(pool), n)]
    schema = ss.TupleSchema([ss.Attribute("s", ss.STRING, ss.NULLABLE), ss.Attribute("t", ss.STRING), ss.Attribute("id", ss.INT32)])
    return ss.View(schema, [ss.Column(s, nulls), t, np.arange(n, dtype=np.int32)])


def parity_expr():
    # (five columns: the specialised build of this program is compiled once for all row counts, and its compile time grows with it)
    return (ss.CompoundExpression().AddAs("len_s", ss.Length(NA("s")))
            .AddAs("off", ss.StringOffset(NA("s"), ss.ConstString("abc")))
            .AddAs("has_ci", ss.StringContainsCI(NA("t"), ss.ConstString(b"\xe4bC")))
            .AddAs("const_hay", ss.StringOffset(ss.ConstString("xabcabc"), ss.ConstString("abc")))
            .AddAs("null_needle", ss.StringOffset(NA("t"), ss.Null(ss.STRING))))


def parity_want(view):
    n = view.row_count()
    s, sz, t = view.column(0).data, view.column(0).is_null, view.column(1).data
    const = np.array([b"xabcabc"] * n, dtype=object)
    return [want_length(s, sz), want_offset(s, sz, b"abc"), want_contains(t, None, b"\xe4bC", True), want_offset(const, None, b"abc"),
            want_offset(t, None, None)]


@pytest.mark.parametrize("n", [1, 511, 512, 513, 70001])
def test_row_parity(any_ctx, n):
    ctx, compiled = any_ctx
    view = parity_view(n)
    plan = ss.Plan(ss.Compute(parity_expr(), ss.ScanView(view)), ctx, extra_strings=list(parity_pool()))   # (one dictionary for every n: one program)
    got = run(plan)
    assert ran_compiled(plan) == compiled, plan.specialize_reason()
    assert_cols_equal(got, parity_want(view), context="row parity, %d rows" % n)


def test_all_null_column_and_empty_dictionary(any_ctx):
    ctx, compiled = any_ctx
    n = 700
    schema = ss.TupleSchema([ss.Attribute("s", ss.STRING, ss.NULLABLE)])
    view = ss.View(schema, [ss.Column(np.array([b""] * n, dtype=object), np.ones(n, bool))])
    e = ss.CompoundExpression().AddAs("len", ss.Length(NA("s"))).AddAs("off", ss.StringOffset(NA("s"), ss.Null(ss.STRING)))
    plan = ss.Plan(ss.Compute(e, ss.ScanView(view)), ctx)
    assert len(plan.strings) == 0                       # nothing but NULLs: the table is its one dummy entry
    got = run(plan)
    assert ran_compiled(plan) == compiled
    assert all(z.all() and len(z) == n for _d, z in got)
    # ... and with a needle, which is then the dictionary's only value
    plan = ss.Plan(ss.Compute(ss.StringContains(NA("s"), ss.ConstString("x")), ss.ScanView(view)), ctx)
    (_d, z), = run(plan)
    assert z.all() and len(plan.strings) == 1


# ---- everywhere an expression is legal, once ------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def small():
    return parity_view(5000, seed=3)


def test_filter_on_contains_and_contains_ci(gpu_ctx, small):
    s, sz, ids = small.column(0).data, small.column(0).is_null, small.column(2).data
    for make, fold in ((ss.StringContains, False), (ss.StringContainsCI, True)):
        op = ss.Filter(make(NA("s"), ss.ConstString("aB")), ss.ProjectNamedAttributes(["id"]), ss.ScanView(small))
        (got, _z), = run(ss.Plan(op, gpu_ctx))
        keep = [i for i in range(len(s)) if not sz[i] and py_offset(s[i], b"aB", fold) > 0]
        assert len(keep) > 0 and got.tolist() == ids[keep].tolist()


def test_group_by_length_with_sum_of_offsets(gpu_ctx, small):
    e = ss.CompoundExpression().AddAs("len", ss.Length(NA("s"))).AddAs("off", ss.StringOffset(NA("t"), ss.ConstString("b")))
    spec = ss.AggregationSpecification().AddAggregation(ss.SUM, "off", "sum").AddAggregation(ss.COUNT, "", "n")
    got = run(ss.Plan(ss.GroupAggregate(ss.ProjectNamedAttributes(["len"]), spec, None, ss.Compute(e, ss.ScanView(small))), gpu_ctx))
    s, sz, t = small.column(0).data, small.column(0).is_null, small.column(1).data
    want = {}
    for i in range(len(s)):
        k = None if sz[i] else len(s[i])
        a = want.setdefault(k, [0, 0])
        a[0] += py_offset(t[i], b"b")
        a[1] += 1
    (kd, kz), (sd, _sz), (nd, _nz) = got
    have = {(None if kz[i] else int(kd[i])): [int(sd[i]), int(nd[i])] for i in range(len(kd))}
    assert have == want and len(have) == len(kd)


def test_sort_by_length(gpu_ctx, small):
    e = ss.CompoundExpression().AddAs("len", ss.Length(NA("t"))).AddAs("id", NA("id"))
    (ld, _lz), (idd, _iz) = run(ss.Plan(ss.Sort(ss.SortOrder().add("len", ss.DESCENDING), None, 0, ss.Compute(e, ss.ScanView(small))), gpu_ctx))
    t = small.column(1).data
    assert ld.tolist() == sorted((len(v) for v in t), reverse=True)
    assert [len(t[i]) for i in idd] == ld.tolist() and sorted(idd.tolist()) == list(range(len(t)))


def test_hash_join_and_table_in_one_pipeline(gpu_ctx, small):
    m = 40
    rview = ss.View(ss.TupleSchema([ss.Attribute("rid", ss.INT32), ss.Attribute("w", ss.INT64)]), [np.arange(m, dtype=np.int32), np.arange(m) * 1000])
    e = ss.CompoundExpression().AddAs("key", ss.Modulus(NA("id"), ss.ConstInt32(64))).AddAs("s", NA("s")).AddAs("t", NA("t"))
    proj = ss.CompoundMultiSourceProjector().add(0, ss.ProjectAllAttributes()).add(1, ss.ProjectNamedAttributes(["w"]))
    join = ss.HashJoin(ss.LEFT_OUTER, ss.ProjectNamedAttribute("key"), ss.ProjectNamedAttribute("rid"), proj, ss.UNIQUE, ss.Compute(e, ss.ScanView(small)), ss.ScanView(rview))
    out = (ss.CompoundExpression().AddAs("w", NA("w")).AddAs("len", ss.Length(NA("s"))).AddAs("off", ss.StringOffset(NA("t"), ss.ConstString("c")))
           .AddAs("both", ss.Plus(NA("w"), ss.StringOffset(NA("t"), ss.ConstString("c")))))
    plan = ss.Plan(ss.Compute(out, join), gpu_ctx)
    assert len(plan.stage_info()) == 1                       # one pipeline: the probe, the rhs gather and both tables
    got = run(plan)
    s, sz, t, ids = small.column(0).data, small.column(0).is_null, small.column(1).data, small.column(2).data
    w, wz = (ids % 64).astype(np.int64) * 1000, (ids % 64) >= m
    off, _z = want_offset(t, None, b"c")
    assert_cols_equal(got, [(w, wz), want_length(s, sz), (off, None), (w + off, wz)], context="join + tables")


def test_slot_limit_refusal(gpu_ctx, small):
    e = ss.CompoundExpression()
    for i in range(25):
        e.AddAs("o%d" % i, ss.StringOffset(NA("t"), ss.ConstString("needle %d" % i)))
    with pytest.raises(ss.SupersonicException) as err:
        ss.Plan(ss.Compute(e, ss.ScanView(small)), gpu_ctx)
    assert err.value.return_code == ss.ERROR_NOT_IMPLEMENTED and "slots" in str(err.value)


def test_bound_expression_evaluate(gpu_ctx, small):
    e = ss.CompoundExpression().AddAs("len", ss.Length(NA("s"))).AddAs("has", ss.StringContainsCI(NA("t"), ss.ConstString("B C")))
    tree = e.Bind(small.schema(), None, 0, gpu_ctx)
    r = tree.Evaluate(small)
    assert not r.is_failure(), r.exception()
    s, sz, t = small.column(0).data, small.column(0).is_null, small.column(1).data
    assert_cols_equal(to_cols(r.view()), [want_length(s, sz), want_contains(t, None, b"B C", True)], context="Evaluate")
    # DoEvaluate: skipped rows are NULL, the others as above
    skip = np.zeros(len(s), bool)
    skip[::3] = True
    r = tree.DoEvaluate(small, [skip.copy(), None])
    assert not r.is_failure(), r.exception()
    got = to_cols(r.view())
    want_len, want_has = want_length(s, sz | skip), want_contains(t, None, b"B C", True)
    assert_cols_equal([got[0]], [want_len], context="DoEvaluate")
    assert np.array_equal(got[1][0], want_has[0]) and (got[1][1] is None or not got[1][1].any())


def test_run_host_in_chunks(gpu_ctx, small):
    s, sz, t, ids = small.column(0).data, small.column(0).is_null, small.column(1).data, small.column(2).data
    plan = ss.Plan(ss.Filter(ss.StringContains(NA("t"), ss.ConstString("ab")), ss.ProjectNamedAttributes(["id"]), ss.ScanView(small)), gpu_ctx)
    assert plan.chunked_form()[0] == 2
    plan.run_host(chunk_rows=1000)
    (got, _z), = to_cols(plan.fetch())
    assert got.tolist() == [int(ids[i]) for i in range(len(t)) if py_offset(t[i], b"ab") > 0]
    # GroupAggregate first: the per-chunk plan and the merging plan are derived inside the library and inherit the dictionary
    e = ss.CompoundExpression().AddAs("len", ss.Length(NA("t"))).AddAs("off", ss.StringOffset(NA("s"), ss.ConstString("a")))
    spec = ss.AggregationSpecification().AddAggregation(ss.SUM, "off", "sum").AddAggregation(ss.COUNT, "off", "n")
    plan = ss.Plan(ss.GroupAggregate(ss.ProjectNamedAttributes(["len"]), spec, None, ss.Compute(e, ss.ScanView(small))), gpu_ctx)
    assert plan.chunked_form()[0] == 3
    plan.run_host(chunk_rows=1000)
    (kd, _kz), (sd, sn), (nd, _nz) = to_cols(plan.fetch())
    want = {}
    for i in range(len(t)):
        a = want.setdefault(len(t[i]), [0, 0])
        if not sz[i]:
            a[0] += py_offset(s[i], b"a")
            a[1] += 1
    have = {int(kd[i]): [0 if (sn is not None and sn[i]) else int(sd[i]), int(nd[i])] for i in range(len(kd))}
    assert have == want


def test_block_with_device_encoded_strings(gpu_ctx, tmp_path, small):
    path = str(tmp_path / "strings.ssv")
    out = ss.FileOutput(path)
    out.Write(small)
    out.Finalize()
    dev = ss.FileInput(small.schema(), path, gpu_ctx, device_strings=True)
    needle = b"c A"
    assert needle not in dev.dictionary.values               # the plan extends the block's dictionary with it
    e = (ss.CompoundExpression().AddAs("id", NA("id")).AddAs("len", ss.Length(NA("s"))).AddAs("off", ss.StringOffset(NA("t"), ss.ConstString(needle))))
    plan = ss.Plan(ss.Filter(ss.StringContainsCI(NA("t"), ss.ConstString(needle)), ss.ProjectAllAttributes(), ss.Compute(
        ss.CompoundExpression().AddAs("id", NA("id")).AddAs("s", NA("s")).AddAs("t", NA("t")), ss.ScanView(dev))), gpu_ctx)
    assert len(plan.strings) == len(dev.dictionary) + 1
    got = run(plan)
    s, sz, t, ids = small.column(0).data, small.column(0).is_null, small.column(1).data, small.column(2).data
    keep = [i for i in range(len(t)) if py_offset(t[i], needle, True) > 0]
    assert len(keep) > 0 and got[0][0].tolist() == ids[keep].tolist()
    plan = ss.Plan(ss.Compute(e, ss.ScanView(dev)), gpu_ctx)
    got = run(plan)
    assert_cols_equal(got, [(ids, None), want_length(s, sz), want_offset(t, None, needle)], context="device-encoded block")


def test_tables_are_rebuilt_for_another_dictionary(gpu_ctx):
    schema = ss.TupleSchema([ss.Attribute("s", ss.STRING)])
    first = ss.View(schema, [np.array([b"ab", b"cab", b"", b"b"], dtype=object)])
    e = ss.CompoundExpression().AddAs("len", ss.Length(NA("s"))).AddAs("off", ss.StringOffset(NA("s"), ss.ConstString("ab")))
    plan = ss.Plan(ss.Compute(e, ss.ScanView(first)), gpu_ctx)
    assert_cols_equal(run(plan), [want_length(first.column(0).data, None), want_offset(first.column(0).data, None, b"ab")])
    # an extension by values that sort behind every old one keeps the old codes (the needle's among them) and adds new ones
    old = plan.strings
    more = [b"\xffzzab", b"\xff" + b"q" * 300 + b"ab", b"\xff"]
    wider, remap = old.extend(more)
    assert remap.tolist() == list(range(len(old))) and len(wider) == len(old) + 3
    plan.ctx.check(plan.lib.ssgpu_plan_set_dict(plan.handle, wider.handle))
    plan.strings = wider
    second = ss.View(schema, [np.array(more + [b"cab", b""], dtype=object)])
    assert_cols_equal(run(plan, second), [want_length(second.column(0).data, None), want_offset(second.column(0).data, None, b"ab")],
                      context="after a second ssgpu_plan_set_dict")
    plan.ctx.check(plan.lib.ssgpu_plan_set_dict(plan.handle, old.handle))     # and back: the tables follow the handle
    plan.strings = old
    assert_cols_equal(run(plan, first), [want_length(first.column(0).data, None), want_offset(first.column(0).data, None, b"ab")])


def test_run_without_a_dictionary_names_the_call(gpu_ctx):
    # straight through the C ABI: a plan nobody handed a dictionary
    lib, L = gpu_ctx.lib, ss._lib
    attrs = (L.Attr * 1)(L.Attr(b"s", ss.STRING, 0))
    exprs = (L.Expr * 2)(L.Expr(L.EXPR_ATTR_NAMED, 0, 0, 0, 0, 0, 0, 0.0, b"s"), L.Expr(L.EXPR_OP, 400, 0, 0, 1, 0, 0, 0.0, None))
    args = (C.c_int32 * 1)(0)
    h = C.c_void_p()
    gpu_ctx.check(lib.ssgpu_expr_bind(gpu_ctx.handle, attrs, 1, exprs, 2, args, 1, 1, 0, C.byref(h)))
    try:
        blk = ss.DeviceBlock(ss.TupleSchema([ss.Attribute("c", ss.INT32)]), 4, gpu_ctx)
        cols = (L.Column * 1)()
        cols[0].data = blk.column_ptr(0)
        res = C.c_void_p()
        rc = lib.ssgpu_plan_run(h, cols, 1, 0, C.byref(res))
        assert rc == ss.ERROR_INVALID_ARGUMENT_VALUE and "ssgpu_plan_set_dict" in gpu_ctx.last_error()
    finally:
        lib.ssgpu_plan_destroy(h)


# ---- fuzz ------------------------------------------------------------------------------------------------------------------------
class Gen(object):
    """Random small expressions over (s STRING NULLABLE, t STRING, id INT32) with their value under the Python restatement:
    every node is (expression factory, values, NULL mask)."""
    NEEDLES = [b"", b"a", b"ab", b"BC", b"c a", b"abcabc"]
    CONSTS = [b"", b"abc", b"xabcabc", b"A B C"]

    def __init__(self, rng, view):
        self.rng, self.n = rng, view.row_count()
        self.s, self.sz, self.t, self.ids = view.column(0).data, view.column(0).is_null, view.column(1).data, view.column(2).data
        self.tables = 0

    def pick(self, items):
        return items[int(self.rng.integers(0, len(items)))]

    def hay(self, depth):
        k = int(self.rng.integers(0, 6 if depth > 0 else 3))
        if k == 0:
            return (lambda: NA("s")), self.s, self.sz
        if k == 1:
            return (lambda: NA("t")), self.t, np.zeros(self.n, bool)
        if k == 2:
            c = self.pick(self.CONSTS)
            return (lambda: ss.ConstString(c)), np.array([c] * self.n, dtype=object), np.zeros(self.n, bool)
        if k == 3:
            a, b = self.hay(depth - 1), self.hay(depth - 1)
            return (lambda: ss.IfNull(a[0](), b[0]())), np.where(a[2], b[1], a[1]), a[2] & b[2]
        c, a, b = self.boolean(depth - 1), self.hay(depth - 1), self.hay(depth - 1)
        choose = c[1] & ~c[2]
        return (lambda: ss.If(c[0](), a[0](), b[0]())), np.where(choose, a[1], b[1]), np.where(choose, a[2], b[2])

    def integer(self, depth):
        k = int(self.rng.integers(0, 4 if depth > 0 else 3))
        if k == 0:
            h = self.hay(depth)
            self.tables += 1
            return (lambda: ss.Length(h[0]())), np.array([len(v) for v in h[1]], np.int64), h[2]
        if k in (1, 2):
            h, fold = self.hay(depth), bool(self.rng.integers(0, 2))
            needle = None if self.rng.random() < 0.1 else self.pick(self.NEEDLES)
            self.tables += 1
            d, z = want_offset(h[1], h[2], needle, fold)

            def make():
                n = ss.Null(ss.STRING) if needle is None else ss.ConstString(needle)
                return ss.StringOffset(ss.ToLower(h[0]()), ss.ToLower(n)) if fold else ss.StringOffset(h[0](), n)
            return make, d.astype(np.int64), z
        c, a, b = self.boolean(depth - 1), self.integer(depth - 1), self.integer(depth - 1)
        choose = c[1] & ~c[2]
        return (lambda: ss.If(c[0](), ss.CastTo(ss.INT64, a[0]()), ss.CastTo(ss.INT64, b[0]()))), np.where(choose, a[1], b[1]), np.where(choose, a[2], b[2])

    def boolean(self, depth):
        k = int(self.rng.integers(0, 7 if depth > 0 else 3))
        if k in (0, 1):
            h, fold, needle = self.hay(depth), k == 1, self.pick(self.NEEDLES)
            self.tables += 1
            d, z = want_contains(h[1], h[2], needle, fold)
            return (lambda: (ss.StringContainsCI if fold else ss.StringContains)(h[0](), ss.ConstString(needle))), d, z
        if k == 2:
            bound = int(self.rng.integers(0, self.n + 1))
            return (lambda: ss.Less(NA("id"), ss.ConstInt32(bound))), self.ids < bound, np.zeros(self.n, bool)
        if k == 3:
            a, b = self.integer(depth - 1), self.integer(depth - 1)
            op, fn = self.pick([(ss.Less, np.less), (ss.Equal, np.equal), (ss.LessOrEqual, np.less_equal)])
            return (lambda: op(a[0](), b[0]())), fn(a[1], b[1]), a[2] | b[2]
        if k == 4:
            a = self.boolean(depth - 1)
            return (lambda: ss.Not(a[0]())), ~a[1], a[2]
        if k == 5:
            a = self.integer(depth - 1)
            return (lambda: ss.IsNull(a[0]())), a[2].copy(), np.zeros(self.n, bool)
        a, b = self.boolean(depth - 1), self.boolean(depth - 1)
        if self.rng.integers(0, 2):      # AND: FALSE decides, else NULL if either is NULL
            false = (~a[1] & ~a[2]) | (~b[1] & ~b[2])
            return (lambda: ss.And(a[0](), b[0]())), a[1] & b[1] & ~false, (a[2] | b[2]) & ~false
        true = (a[1] & ~a[2]) | (b[1] & ~b[2])
        return (lambda: ss.Or(a[0](), b[0]())), true, (a[2] | b[2]) & ~true


def test_fuzz_small_plans(gpu_ctx):
    rng = np.random.default_rng(2024)
    views = [parity_view(n, seed=9) for n in (1, 37, 512, 700)]
    plans = with_tables = 0
    for it in range(300):
        view = views[it % len(views)]
        g = Gen(rng, view)
        shape = it % 3
        label = "fuzz plan %d (shape %d, %d rows)" % (it, shape, view.row_count())
        if shape == 0:       # Compute: every row of an integer and a BOOL expression
            a, b = g.integer(2), g.boolean(2)
            e = ss.CompoundExpression().AddAs("a", ss.CastTo(ss.INT64, a[0]())).AddAs("b", b[0]())
            got = run(ss.Plan(ss.Compute(e, ss.ScanView(view)), gpu_ctx))
            for (gd, gz), (wd, wz) in zip(got, ((a[1], a[2]), (b[1], b[2]))):
                gz = np.zeros(len(gd), bool) if gz is None else gz
                assert np.array_equal(gz, wz), label
                assert np.array_equal(gd[~wz], wd[~wz]), label
        elif shape == 1:     # Filter: the rows whose predicate is TRUE and not NULL
            b = g.boolean(2)
            (gd, _gz), = run(ss.Plan(ss.Filter(b[0](), ss.ProjectNamedAttributes(["id"]), ss.ScanView(view)), gpu_ctx))
            assert gd.tolist() == g.ids[b[1] & ~b[2]].tolist(), label
        else:                # ScalarAggregate: SUM and COUNT of an integer expression over the rows a predicate keeps
            a, b = g.integer(2), g.boolean(1)
            e = ss.CompoundExpression().AddAs("v", ss.CastTo(ss.INT64, a[0]()))
            spec = ss.AggregationSpecification().AddAggregation(ss.SUM, "v", "sum").AddAggregation(ss.COUNT, "v", "n")
            op = ss.ScalarAggregate(spec, ss.Compute(e, ss.Filter(b[0](), ss.ProjectAllAttributes(), ss.ScanView(view))))
            (sd, sz), (nd, _nz) = run(ss.Plan(op, gpu_ctx))
            live = b[1] & ~b[2] & ~a[2]
            assert int(nd[0]) == int(live.sum()), label
            if live.any():
                assert int(sd[0]) == int(a[1][live].sum()) and not (sz is not None and sz[0]), label
            else:
                assert sz is not None and sz[0], label
        plans += 1
        with_tables += 1 if g.tables else 0
    assert plans == 300 and with_tables >= 250
