"""STRING_REPLACE on the device: the two replace kernels (string_map_kernels.hip) through StringDictionary.close of ONE step and
step_table entry by entry over a pool built for them (string_replace_pool.py), nested steps, the reference's own rows
(tests/golden/string_replace_cases.json) under the interpreting and the specialised kernel, every place such an expression is legal
once, the guards, and a seeded fuzz.  The oracle does not know the operator: the expected values are the Python restatement
replace(h, n, s) = h if n == b"" else h.replace(n, s), pinned against the reference's loop in test_string_replace_cpu.py.

A needle and a substitute are constants of the plan, so values of the base dictionary: every base here holds them.  One consequence:
the image b"" only arises from a substitute b"" (or from the value b""), which the base then holds -- "an image b"" absent from the
base" cannot be stated for this operator; test_images_that_move_every_code uses an image that sorts before every base value instead."""
import json
import os

import numpy as np
import pytest

import supersonic_amd as ss
from helpers import to_cols, assert_cols_equal
from string_replace_pool import (LAST_A, LONG, NEEDLE17, NEEDLE130, PAIR_IDS, PAIRS, RUN100, STRING_REPLACE, SUB200, V1300, pool, replace)

NA = ss.NamedAttribute
CS = ss.ConstString
pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = json.load(open(os.path.join(ROOT, "tests", "golden", "string_replace_cases.json")))
LTRIM, RTRIM, TRIM, TO_UPPER = 404, 408, 412, 416
POOL = pool()


def py_fn(step):
    """step: (480, needle, substitute) with bytes, or (fn,) of the argument-less producers -> the function of one value"""
    if step[0] == STRING_REPLACE:
        return lambda b: replace(b, step[1], step[2])
    return {LTRIM: lambda b: b.lstrip(b" "), RTRIM: lambda b: b.rstrip(b" "), TRIM: lambda b: b.strip(b" "), TO_UPPER: lambda b: b.upper()}[step[0]]


def rep(needle, sub):
    return (STRING_REPLACE, needle, sub)


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


# ---- the kernels, entry by entry ----------------------------------------------------------------------------------------------
def check_close(ctx, base_values, steps):
    """Closes a dictionary of base_values (plus the steps' constants) under `steps` and checks EVERYTHING the closed dictionary
    promises; returns (closed, levels)."""
    consts = [c for st in steps if st[0] == STRING_REPLACE for c in st[1:]]
    d = ss.StringDictionary(list(base_values) + consts)
    levels = [d.values]                                      # D_0, D_1, ...: the restatement of the closure
    for st in steps:
        f = py_fn(st)
        levels.append(sorted(set(levels[-1]) | {f(v) for v in levels[-1]}))
    closed, remap = d.close(steps, ctx)
    values = closed.values
    assert values == levels[-1], ("closed values", [st[0] for st in steps], [v[:20] for v in set(values) ^ set(levels[-1])][:5])
    assert all(values[i] < values[i + 1] for i in range(len(values) - 1))                # sorted and distinct
    code = {v: i for i, v in enumerate(values)}
    assert remap.tolist() == [code[v] for v in levels[0]]
    for k, st in enumerate(steps):
        f = py_fn(st)
        T = closed.step_table(k)
        assert len(T) == len(values) and (len(T) == 0 or (T.min() >= 0 and T.max() < len(values))), k
        domain = set(levels[k])
        bad = [v for v in levels[k] if values[T[code[v]]] != f(v)]
        assert not bad, "step %d: %d values differ, first (%d bytes) %r -> got %r want %r" % (
            k, len(bad), len(bad[0]), bad[0][:40], values[T[code[bad[0]]]][:40], f(bad[0])[:40])
        assert all(T[code[v]] == 0 for v in values if v not in domain), k                # never -1, never garbage
    # a replace step is remembered in the CLOSED dictionary's codes
    assert closed.steps == [(STRING_REPLACE, 0, code[st[1]], code[st[2]]) if st[0] == STRING_REPLACE else (st[0], 0, 0, 0) for st in steps]
    return closed, levels


def test_the_pool_holds_what_the_kernels_can_get_wrong():
    lens = {len(v) for v in POOL}
    assert {0, 1, LONG - 1, LONG, LONG + 1} <= lens and len(POOL) == len(set(POOL)) and len(POOL) >= 300
    assert any(1020 <= n <= 1040 for n in lens) and 1300 in lens and 2100 in lens
    for v in [b"a" * k for k in range(21)] + [b"a" * 129, b"ab" * 600, b"aba" * 50, b"ababababa", V1300, LAST_A, b"b"]:
        assert v in POOL, v[:20]
    assert NEEDLE130 in V1300 and any(NEEDLE17 in v and len(v) > LONG for v in POOL) and all(len(v) < len(PAIRS[11][0]) for v in POOL)
    # a value that ends in 'a' right before one that starts with 'b', in the packed (sorted) dictionary of the "ab" case
    base = sorted(set(POOL) | {b"ab", b"ba"})
    i = base.index(LAST_A)
    assert base[i].endswith(b"a") and base[i + 1].startswith(b"b") and b"ab" not in base[i] and b"ab" not in base[i + 1]
    # the only match of "aba" at 24 consecutive offsets (one straddles an aligned 8-byte word and one an aligned 16-byte word wherever
    # the value starts), at the value's very end (lane and wave form), and at every offset around the sub-step and step boundaries
    only = [v for v in POOL if v.count(b"aba") == 1 and replace(v, b"aba", b"") == v.replace(b"aba", b"", 1)]
    assert {v.find(b"aba") for v in only if len(v) == 26} >= set(range(24))
    assert any(v.endswith(b"aba") and len(v) <= LONG for v in only) and any(v.endswith(b"aba") and len(v) > LONG for v in only)
    assert {v.find(b"aba") for v in only if len(v) == 203} >= set(range(44, 70))
    assert {v.find(b"aba") for v in only if len(v) == 1103} >= set(range(1003, 1029))
    # short values with long images, long values with short images
    assert any(len(v) <= LONG < len(replace(v, b"a", SUB200)) for v in POOL) and any(len(replace(v, RUN100, b"")) <= LONG < len(v) for v in POOL)


@pytest.mark.parametrize("pair", PAIRS, ids=PAIR_IDS)
@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, len(POOL)])
def test_close_one_replace_step_entry_by_entry(gpu_ctx, n, pair):
    check_close(gpu_ctx, POOL[:n], [rep(*pair)])


def test_images_that_move_every_code(gpu_ctx):
    # an image that sorts before every base value: every code moves
    base = [b"b", b"ab", b"b!"]
    closed, levels = check_close(gpu_ctx, base, [rep(b"b", b"ab")])
    assert closed.values[0] == b"aab" and min(levels[0]) == b"ab"
    # two values share one image, and an image is a base value
    closed, _levels = check_close(gpu_ctx, [b"a", b"b", b"ab", b"bb"], [rep(b"a", b"b")])
    T, code = closed.step_table(0), {v: i for i, v in enumerate(closed.values)}
    assert T[code[b"a"]] == T[code[b"b"]] == code[b"b"] and T[code[b"ab"]] == T[code[b"bb"]] == code[b"bb"] and closed.values == [b"a", b"ab", b"b", b"bb"]
    # leftmost, non-overlapping, left to right; the substitute is not searched again; an empty needle is the identity
    closed, _levels = check_close(gpu_ctx, [b"aaaaa"], [rep(b"aa", b"b")])
    assert closed.values[closed.step_table(0)[closed.code_of(b"aaaaa")]] == b"bba"
    check_close(gpu_ctx, [b"a", b"aaa", b"a" * 200], [rep(b"a", b"aa")])
    closed, _levels = check_close(gpu_ctx, [b"x", b"", b"y" * 300], [rep(b"", b"zzz")])
    assert closed.step_table(0).tolist() == list(range(len(closed.values)))


NESTED = {"replace(trim)": [(TRIM,), rep(b"a", b" b ")], "trim(replace)": [rep(b"a", b" "), (TRIM,)], "a-b then b-c": [rep(b"a", b"b"), rep(b"b", b"c")],
          "the same replace twice": [rep(b"aa", b"a"), rep(b"aa", b"a")]}


@pytest.mark.parametrize("name", sorted(NESTED))
def test_nested_steps(gpu_ctx, name):
    steps = NESTED[name]
    values = POOL[:150]
    closed, levels = check_close(gpu_ctx, values, steps)      # T_k is correct on all of D_(k-1), for every k; .steps are closed codes
    consts = [c for st in steps if st[0] == STRING_REPLACE for c in st[1:]]
    for st, kept in zip(steps, closed.steps):
        if st[0] == STRING_REPLACE:
            assert kept == (STRING_REPLACE, 0, closed.code_of(st[1]), closed.code_of(st[2]))
    # the same values in another input order (and repeated): identical values and identical tables
    rng = np.random.default_rng(1)
    other = consts + [values[i] for i in rng.permutation(len(values))] + values[:7]
    again, _remap = ss.StringDictionary(other).close(steps, gpu_ctx)
    assert again.values == closed.values and again.steps == closed.steps
    for k in range(len(steps)):
        assert np.array_equal(again.step_table(k), closed.step_table(k))


# ---- the reference's rows --------------------------------------------------------------------------------------------------
def test_golden_rows(any_ctx):
    ctx, compiled = any_ctx
    for h, n, s, want in GOLDEN["evaluation"]["StringReplace"]["rows"]:
        data = np.array([h.encode(), b"", h.encode()], dtype=object)
        schema = ss.TupleSchema([ss.Attribute("s", ss.STRING, ss.NULLABLE)])
        view = ss.View(schema, [ss.Column(data, np.array([False, True, False]))])
        plan = ss.Plan(ss.Compute(ss.StringReplace(NA("s"), CS(n), CS(s)), ss.ScanView(view)), ctx)
        (got, nulls), = run(plan)
        assert ran_compiled(plan) == compiled, plan.specialize_reason()
        assert nulls.tolist() == [False, True, False] and got[0] == got[2] == want.encode(), (h, n, s)


# ---- everywhere such an expression is legal, once -----------------------------------------------------------------------------
def make_view(n, seed):
    rng = np.random.default_rng(seed)
    short = [v for v in POOL if len(v) <= 40][:60] + [b"a" * 129, b"ababa" * 30, b"banana", b"bandana", b" a b a "]
    vals = np.array(short + [None], dtype=object)[:-1]
    s = vals[rng.integers(0, len(vals), n)]
    nulls = rng.random(n) < 0.2
    s[::5] = sorted(short)[0]             # NULL rows next to rows that carry code 0: NULL in gives NULL out, never T[0]
    nulls[1::5] = True
    u = vals[rng.integers(0, len(vals), n)]
    schema = ss.TupleSchema([ss.Attribute("t", ss.STRING, ss.NULLABLE), ss.Attribute("u", ss.STRING), ss.Attribute("id", ss.INT32)])
    return ss.View(schema, [ss.Column(s, nulls), u, np.arange(n, dtype=np.int32)])


@pytest.fixture(scope="module")
def rows300():
    return make_view(300, 480)


def cols_of(view):
    return view.column(0).data, view.column(0).is_null, view.column(1).data, view.column(2).data


def mapped(data, nulls, needle, sub):
    return np.array([replace(v, needle, sub) for v in data], dtype=object), nulls


def test_projection(any_ctx, rows300):
    ctx, compiled = any_ctx
    t, tz, u, _ids = cols_of(rows300)
    e = (ss.CompoundExpression().AddAs("a", ss.StringReplace(NA("t"), CS("a"), CS("bb"))).AddAs("b", ss.StringReplace(NA("u"), CS("ab"), CS("")))
         .AddAs("c", ss.StringReplace(CS("banana"), CS("an"), CS("AN"))).AddAs("d", ss.StringReplace(NA("u"), CS("a"), ss.Null(ss.STRING)))
         .AddAs("e", ss.StringReplace(NA("t"), CS(""), CS("never"))))
    plan = ss.Plan(ss.Compute(e, ss.ScanView(rows300)), ctx)
    got = run(plan)
    assert ran_compiled(plan) == compiled, plan.specialize_reason()
    const = np.array([b"bANANa"] * len(t), dtype=object)
    assert_cols_equal(got, [mapped(t, tz, b"a", b"bb"), mapped(u, None, b"ab", b""), (const, None), (u, np.ones(len(u), bool)), (t, tz)], context="projection")


def test_filter_on_replace_equals_constant(gpu_ctx, rows300):
    t, tz, _u, ids = cols_of(rows300)
    for sub, c in ((b"o", b"bonono"), (b"b", b"b" * 129), (b"b", b"nowhere")):           # constants that exist as images only, and one that is nowhere
        op = ss.Filter(ss.Equal(ss.StringReplace(NA("t"), CS("a"), CS(sub)), CS(c)), ss.ProjectNamedAttributes(["id"]), ss.ScanView(rows300))
        (got, _z), = run(ss.Plan(op, gpu_ctx))
        keep = [int(ids[i]) for i in range(len(t)) if not tz[i] and replace(t[i], b"a", sub) == c]
        assert got.tolist() == keep and (len(keep) > 0) == (c != b"nowhere")


def test_group_key_sort_key_and_min_max(gpu_ctx, rows300):
    t, tz, u, ids = cols_of(rows300)
    e = ss.CompoundExpression().AddAs("g", ss.StringReplace(NA("t"), CS("a"), CS(""))).AddAs("m", ss.StringReplace(NA("u"), CS("b"), CS("a"))).AddAs("id", NA("id"))
    spec = ss.AggregationSpecification().AddAggregation(ss.COUNT, "", "n")
    (kd, kz), (nd, _nz) = run(ss.Plan(ss.GroupAggregate(ss.ProjectNamedAttributes(["g"]), spec, None, ss.Compute(e, ss.ScanView(rows300))), gpu_ctx))
    want = {}
    for i in range(len(t)):
        k = None if tz[i] else replace(t[i], b"a", b"")
        want[k] = want.get(k, 0) + 1
    have = {(None if kz[i] else kd[i]): int(nd[i]) for i in range(len(kd))}
    assert have == want and len(have) == len(kd) and len(have) < len({v for i, v in enumerate(t) if not tz[i]}) + 1       # removing 'a' merged groups
    # scalar MIN / MAX of an image
    spec = ss.AggregationSpecification().AddAggregation(ss.MIN, "m", "lo").AddAggregation(ss.MAX, "m", "hi")
    (lo, _a), (hi, _b) = run(ss.Plan(ss.ScalarAggregate(spec, ss.Compute(e, ss.ScanView(rows300))), gpu_ctx))
    live = [replace(v, b"b", b"a") for v in u]
    assert (lo[0], hi[0]) == (min(live), max(live))
    # sort key: ORDER BY STRING_REPLACE(u, 'b', 'a'), id DESC
    order = ss.SortOrder().add("m", ss.ASCENDING).add("id", ss.DESCENDING)
    proj = ss.CompoundExpression().AddAs("m", ss.StringReplace(NA("u"), CS("b"), CS("a"))).AddAs("id", NA("id"))
    (md, _mz), (idd, _iz) = run(ss.Plan(ss.Sort(order, None, 0, ss.Compute(proj, ss.ScanView(rows300))), gpu_ctx))
    assert [(md[i], -int(idd[i])) for i in range(len(md))] == sorted((replace(u[i], b"b", b"a"), -int(ids[i])) for i in range(len(u)))


def test_under_and_over_other_string_expressions(gpu_ctx, rows300):
    t, tz, u, ids = cols_of(rows300)
    e = (ss.CompoundExpression().AddAs("a", ss.Length(ss.StringReplace(NA("t"), CS("a"), CS("xyz"))))
         .AddAs("b", ss.StringContains(ss.StringReplace(NA("u"), CS("a"), CS("b")), CS("bbb")))
         .AddAs("c", ss.StringReplace(ss.If(ss.Less(NA("id"), ss.ConstInt32(150)), NA("t"), NA("u")), CS("ab"), CS("ba")))
         .AddAs("d", ss.ToUpper(ss.StringReplace(NA("u"), CS("a"), CS("ab"))))
         .AddAs("e", ss.StringReplace(ss.Trim(NA("u")), CS(" "), CS("_"))))
    got = run(ss.Plan(ss.Compute(e, ss.ScanView(rows300)), gpu_ctx))
    n = len(t)
    a = np.array([len(replace(v, b"a", b"xyz")) for v in t], np.uint32)
    b = np.array([replace(v, b"a", b"b").find(b"bbb") >= 0 for v in u])
    c = np.array([replace(t[i] if i < 150 else u[i], b"ab", b"ba") for i in range(n)], dtype=object)
    cz = np.array([tz[i] if i < 150 else False for i in range(n)])
    d = np.array([replace(v, b"a", b"ab").upper() for v in u], dtype=object)
    ee = np.array([replace(v.strip(b" "), b" ", b"_") for v in u], dtype=object)
    assert b.any() and not b.all()
    assert_cols_equal(got, [(a, tz), (b, None), (c, cz), (d, None), (ee, None)], context="LENGTH / CONTAINS / IF / TO_UPPER / TRIM")


def test_hash_join_key(gpu_ctx, rows300):
    t, tz, _u, ids = cols_of(rows300)
    keys = sorted({replace(v, b"a", b"") for v in t})[::2]               # every other image has a partner
    rview = ss.View(ss.TupleSchema([ss.Attribute("rk", ss.STRING), ss.Attribute("w", ss.INT64)]), [np.array(keys, dtype=object), np.arange(len(keys)) * 10])
    e = ss.CompoundExpression().AddAs("key", ss.StringReplace(NA("t"), CS("a"), CS(""))).AddAs("id", NA("id"))
    proj = ss.CompoundMultiSourceProjector().add(0, ss.ProjectNamedAttributes(["id"])).add(1, ss.ProjectNamedAttributes(["w"]))
    join = ss.HashJoin(ss.INNER, ss.ProjectNamedAttribute("key"), ss.ProjectNamedAttribute("rk"), proj, ss.UNIQUE, ss.Compute(e, ss.ScanView(rows300)), ss.ScanView(rview))
    (idd, _iz), (wd, _wz) = run(ss.Plan(join, gpu_ctx))
    pos = {k: i * 10 for i, k in enumerate(keys)}
    want = [(int(ids[i]), pos[replace(t[i], b"a", b"")]) for i in range(len(t)) if not tz[i] and replace(t[i], b"a", b"") in pos]
    assert len(want) > 0 and list(zip(idd.tolist(), wd.tolist())) == want


def test_bound_expression_evaluate(gpu_ctx, rows300):
    t, tz, u, _ids = cols_of(rows300)
    e = ss.CompoundExpression().AddAs("a", ss.StringReplace(NA("t"), CS("ab"), CS("-"))).AddAs("b", ss.Length(ss.StringReplace(ss.StringReplace(NA("u"), CS("a"), CS("b")), CS("b"), CS("cc"))))
    tree = e.Bind(rows300.schema(), None, 0, gpu_ctx)
    r = tree.Evaluate(rows300)
    assert not r.is_failure(), r.exception()
    want_b = (np.array([len(replace(replace(v, b"a", b"b"), b"b", b"cc")) for v in u], np.uint32), None)
    assert_cols_equal(to_cols(r.view()), [mapped(t, tz, b"ab", b"-"), want_b], context="Evaluate")


def test_run_host_in_chunks(gpu_ctx, rows300):
    t, tz, u, ids = cols_of(rows300)
    e = (ss.CompoundExpression().AddAs("a", ss.StringReplace(NA("t"), CS("a"), CS("o"))).AddAs("b", ss.Trim(ss.StringReplace(NA("u"), CS("b"), CS(" "))))
         .AddAs("id", NA("id")))
    keep = ss.Filter(ss.Less(ss.Length(ss.StringReplace(NA("u"), CS("a"), CS(""))), ss.ConstUint32(8)), ss.ProjectAllAttributes(), ss.ScanView(rows300))
    plan = ss.Plan(ss.Compute(e, keep), gpu_ctx)
    plan.run_host(chunk_rows=64)             # 300 rows: four full chunks and a tail; the head / tail plans hold subsets of the steps
    got = to_cols(plan.fetch())
    rows = [i for i in range(len(t)) if len(replace(u[i], b"a", b"")) < 8]
    assert 0 < len(rows) < len(t)
    a, az = mapped(t[rows], tz[rows], b"a", b"o")
    b = np.array([replace(v, b"b", b" ").strip(b" ") for v in u[rows]], dtype=object)
    assert_cols_equal(got, [(a, az), (b, None), (ids[rows], None)], context="run_host, 64-row chunks")
    assert_cols_equal(run(plan), got, context="the same plan over the whole input")


# ---- the guards -------------------------------------------------------------------------------------------------------------------
def test_a_run_reads_only_its_own_tables(gpu_ctx):
    schema = ss.TupleSchema([ss.Attribute("s", ss.STRING)])
    data = np.array([b"banana", b"cab", b"", b"b"], dtype=object)
    view = ss.View(schema, [data])
    plan = ss.Plan(ss.Compute(ss.StringReplace(NA("s"), CS("a"), CS("o")), ss.ScanView(view)), gpu_ctx)
    want = [mapped(data, None, b"a", b"o")]
    assert_cols_equal(run(plan), want)
    closed = plan.strings
    assert closed.steps == [(STRING_REPLACE, 0, closed.code_of(b"a"), closed.code_of(b"o"))]
    # the same values -- so the same codes -- without steps, and closed under lists with OTHER constants (which add no value here)
    unclosed = ss.StringDictionary(closed.values)
    others, _r = ss.StringDictionary(closed.values).close([rep(b"o", b"o")], gpu_ctx)
    swapped, _r = ss.StringDictionary(closed.values).close([rep(b"a", b"a"), (TRIM,)], gpu_ctx)
    assert others.values == closed.values and swapped.values == closed.values
    for wrong in (unclosed, others, swapped):
        plan.ctx.check(plan.lib.ssgpu_plan_set_dict(plan.handle, wrong.handle))
        with pytest.raises(ss.SupersonicException) as err:
            plan.run()
        assert err.value.return_code == ss.ERROR_INVALID_ARGUMENT_VALUE and "ssgpu_dict_close" in str(err.value)
    # a list that holds the plan's step as a subsequence serves it
    wider, _r = ss.StringDictionary(closed.values).close([(TRIM,), rep(b"o", b"o"), rep(b"a", b"o"), rep(b"a", b"a")], gpu_ctx)
    assert wider.values == closed.values
    plan.ctx.check(plan.lib.ssgpu_plan_set_dict(plan.handle, wider.handle))
    plan.strings = wider
    assert_cols_equal(run(plan, ss.View(schema, [data.copy()])), want, context="a wider closure")


def test_codes_outside_the_base_are_refused(gpu_ctx):
    d = ss.StringDictionary([b"a", b"b", b"banana"])
    for step in ((STRING_REPLACE, 3, 0), (STRING_REPLACE, 0, 3), (STRING_REPLACE, -1, 0), (STRING_REPLACE, 0, 1 << 40)):
        with pytest.raises(ss.SupersonicException) as e:
            d.close([(TRIM,), step], gpu_ctx)
        assert e.value.return_code == ss.ERROR_INVALID_ARGUMENT_VALUE and "step 1" in str(e.value)
    with pytest.raises(ss.SupersonicException):
        d.close([rep(b"a", b"absent")], gpu_ctx)
    with pytest.raises(ss.SupersonicException):
        ss.StringDictionary([]).close([(STRING_REPLACE, 0, 0)], gpu_ctx)
    closed, _remap = d.close([(STRING_REPLACE, 0, 1)], gpu_ctx)           # codes as they are: a -> b
    assert closed.values == [b"a", b"b", b"banana", b"bbnbnb"]


# ---- fuzz ------------------------------------------------------------------------------------------------------------------------
def test_fuzz_small_plans(gpu_ctx):
    """150 plans: 1-3 nested producers of which at least one is a replace, needles of 0-4 and substitutes of 0-6 bytes over `a b space`,
    1-200 rows of 0-40 bytes and now and then 129-300, compared row by row with the restatement.  Every generated plan runs."""
    rng = np.random.default_rng(480)
    abc = np.frombuffer(b"ab ", np.uint8)

    def word(lo, hi):
        return bytes(abc[rng.integers(0, 3, int(rng.integers(lo, hi + 1)))])
    plans = 0
    for it in range(150):
        n = int(rng.integers(1, 201))
        data = np.array([word(129, 300) if rng.random() < 0.03 else word(0, 40) for _ in range(n)] + [None], dtype=object)[:-1]
        nulls = rng.random(n) < 0.15
        depth = int(rng.integers(1, 4))
        must = int(rng.integers(0, depth))                   # the level that is a replace whatever the dice say
        want, makers = list(data), []
        for level in range(depth):
            if level == must or rng.random() < 0.5:
                needle, sub = word(0, 4), word(0, 6)
                makers.append(lambda x, needle=needle, sub=sub: ss.StringReplace(x, CS(needle), CS(sub)))
                want = [replace(v, needle, sub) for v in want]
            else:
                make, f = [(ss.Trim, lambda b: b.strip(b" ")), (ss.Ltrim, lambda b: b.lstrip(b" ")), (ss.ToUpper, lambda b: b.upper())][int(rng.integers(0, 3))]
                makers.append(make)
                want = [f(v) for v in want]

        def expr():                                          # a fresh tree per use
            x = NA("s")
            for make in makers:
                x = make(x)
            return x
        view = ss.View(ss.TupleSchema([ss.Attribute("s", ss.STRING, ss.NULLABLE)]), [ss.Column(data, nulls)])
        e = ss.CompoundExpression().AddAs("r", expr()).AddAs("n", ss.Length(expr()))
        got = run(ss.Plan(ss.Compute(e, ss.ScanView(view)), gpu_ctx))
        assert_cols_equal(got, [(np.array(want + [None], dtype=object)[:-1], nulls), (np.array([len(v) for v in want], np.uint32), nulls)],
                          context="fuzz plan %d (%d rows, depth %d)" % (it, n, depth))
        plans += 1
    assert plans == 150
