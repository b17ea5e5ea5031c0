"""LTRIM / RTRIM / TRIM, TO_UPPER and SUBSTRING on the device: the closing kernels (string_map_kernels.hip + the encoder chain)
through StringDictionary.close of ONE step and step_table entry by entry, SUBSTRING's parameters at their edges, nested steps, the
reference's own rows (tests/golden/string_producing_cases.json) under the interpreting and the specialised kernel, every place such
an expression is legal once, the guards of a run, and a seeded fuzz of small plans.  The oracle does not know these operators: the
expected values are the Python restatement b.lstrip(b" ") / b.rstrip(b" ") / b.strip(b" "), b.upper() (folds ASCII only, like
ascii_toupper) and substring() below, transcribed from string_evaluators.h:41-67."""
import json
import os

import numpy as np
import pytest

import supersonic_amd as ss
from supersonic_amd import _lib as L
from helpers import to_cols, assert_cols_equal

NA = ss.NamedAttribute
pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = json.load(open(os.path.join(ROOT, "tests", "golden", "string_producing_cases.json")))
LONG = 128          # string_map_kernels.hip STRMAP_LONG: up to this length one lane maps a value, beyond it a whole wave
LTRIM, RTRIM, TRIM, TO_UPPER, TO_LOWER, SUBSTRING = 404, 408, 412, 416, 420, 427
I64_MAX, I64_MIN = 2 ** 63 - 1, -2 ** 63


# ---- the Python restatement ----------------------------------------------------------------------------------------------
def substring(b, pos, length=None):
    if length is not None:
        length = max(length, 0)
    if pos > 0:
        pos -= 1
    else:
        pos = max(pos + len(b), 0)
    return b[pos:] if length is None else b[pos:pos + length]


def py_fn(step):
    """step: (fn,), (SUBSTRING, pos) or (SUBSTRING, pos, len) -> the function of one value"""
    fn = step[0]
    if fn == SUBSTRING:
        return lambda b: substring(b, *step[1:])
    return {LTRIM: lambda b: b.lstrip(b" "), RTRIM: lambda b: b.rstrip(b" "), TRIM: lambda b: b.strip(b" "), TO_UPPER: lambda b: b.upper(),
            TO_LOWER: lambda b: b.lower()}[fn]


def mapped(data, nulls, step):
    f = py_fn(step)
    return np.array([f(v) for v in data], dtype=object), nulls


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
    """Closes a dictionary of base_values under `steps` and checks EVERYTHING the closed dictionary promises; returns it."""
    d = ss.StringDictionary(base_values)
    levels = [d.values]                                      # D_0, D_1, ...: the restatement of the closure
    for st in steps:
        f = py_fn(st)
        levels.append(sorted(set(levels[-1]) | {f(v) for v in levels[-1]}))
    closed, remap = d.close(steps, ctx)
    values = closed.values
    assert values == levels[-1], ("closed values", steps, [v[:20] for v in set(values) ^ set(levels[-1])][:5])
    assert all(values[i] < values[i + 1] for i in range(len(values) - 1))                # sorted and distinct
    code = {v: i for i, v in enumerate(values)}
    assert remap.tolist() == [code[v] for v in levels[0]]
    for k, st in enumerate(steps):
        f = py_fn(st)
        T = closed.step_table(k)
        assert len(T) == len(values) and (len(T) == 0 or (T.min() >= 0 and T.max() < len(values))), (steps, k)
        domain = set(levels[k])
        bad = [v for v in levels[k] if values[T[code[v]]] != f(v)]
        assert not bad, "step %d %s: %d values differ, first %r -> got %r want %r" % (k, st, len(bad), bad[0][:40], values[T[code[bad[0]]]][:40], f(bad[0])[:40])
        assert all(T[code[v]] == 0 for v in values if v not in domain), (steps, k)           # never -1, never garbage
    return closed


def kernel_pool():
    """257 distinct values, the interesting ones first (a dictionary of the first n keeps them)."""
    rng = np.random.default_rng(404)
    abc = np.frombuffer(b"abzAZ @[`{ ", np.uint8)

    def rnd(n, alphabet=abc):
        return bytes(alphabet[rng.integers(0, len(alphabet), n)])
    pool = [b"  " + rnd(1290) + b"x   ", b"", b" ", b"a", b"a ", b" a", b" a ",                  # ~1300 bytes; images that collide with "a" and with each other
            rnd(126) + b"x", b" " + rnd(126) + b" ", rnd(127) + b"x", b" " * 2 + rnd(126) + b"y", rnd(128) + b"x", b" " + rnd(127) + b"z ",      # 127, 128, 129
            b" " * 8, b" " * 16, b" " * 129, b" " * 1100,                                                  # all spaces
            b"\t x \t", b"\n", b" \n ", b" \x00 ", b"\x00", b"a\x00b", b"\x80\xff az \xe4\xc4", b" \xa0 ", b"@[`{az", b"`a{z@A[Z", b"Az" * 70 + b" ",
            b" " * 130 + b"q", b"q" + b" " * 130, b" " * 130 + b"q" + b" " * 130, b" " * 700 + b"mid dle" + b" " * 500, b"x" * 1023 + b" ", b" " + b"x" * 1040]
    # leading and trailing runs of every length up to 17 around a body: with the values packed end to end, the runs cross the
    # 8- and 16-byte words of the heap at every offset
    for k in range(18):
        pool.append(b" " * k + b"b%d" % k + b" " * (17 - k))
    for k in (1, 7, 8, 9, 15, 16, 17):
        pool.append(b" " * k + rnd(140).strip(b" ") + b"w" + b" " * k)
    seen = set(pool)
    assert len(seen) == len(pool)
    fill = np.frombuffer(b"abAB  \t\x00\xe4z", np.uint8)
    while len(pool) < 257:
        v = rnd(int(rng.integers(0, 41)), fill)
        if v not in seen:
            seen.add(v)
            pool.append(v)
    return pool


KERNEL_STEPS = [(LTRIM,), (RTRIM,), (TRIM,), (TO_UPPER,), (TO_LOWER,), (SUBSTRING, 2, 5), (SUBSTRING, -3), (SUBSTRING, 100, 60), (SUBSTRING, 0, 4)]


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 257])
def test_close_one_step_entry_by_entry(gpu_ctx, n):
    pool = kernel_pool()
    assert {0, 1, 127, 128, 129} <= {len(v) for v in pool} and any(1290 <= len(v) <= 1310 for v in pool)
    for step in KERNEL_STEPS:
        closed = check_close(gpu_ctx, pool[:n], [step])
        assert closed.steps == [(step[0], 1 if len(step) > 2 else 0, step[1] if len(step) > 1 else 0, step[2] if len(step) > 2 else 0)]


def test_images_that_move_every_code(gpu_ctx):
    # the image "" when "" is absent, from all-space values of lengths 1, 8, 16, 129 and 1100: it sorts before every base value
    base = [b" " * k for k in (1, 8, 16, 129, 1100)] + [b" x", b"y "]
    for step in ((TRIM,), (LTRIM,), (RTRIM,), (SUBSTRING, 1, 0), (SUBSTRING, 2000)):
        closed = check_close(gpu_ctx, base, [step])
        assert closed.values[0] == b"" and b"" not in base
    # an upper-cased image sorts before every (lower-case) base value; two values share one image; an image is a base value
    lower = [b"b", b"bb", b"c", b"c!", b"d"]
    closed = check_close(gpu_ctx, lower, [(TO_UPPER,)])
    assert closed.values == [v.upper() for v in lower] + lower and closed.step_table(0).tolist() == [0] * 5 + [0, 1, 2, 3, 4]
    check_close(gpu_ctx, [b"c", b"C", b"cC", b"Cc", b"CC"], [(TO_UPPER,)])
    check_close(gpu_ctx, [b"a ", b" a", b"a", b"  a  "], [(TRIM,)])
    # n == 0 steps: a copy of the base with an identity remap, and no tables
    d = ss.StringDictionary([b"z", b" y"])
    same, remap = d.close([], gpu_ctx)
    assert same.values == d.values and remap.tolist() == [0, 1]
    with pytest.raises(ss.SupersonicException):
        same.step_table(0)
    # extending a closed dictionary gives an ordinary one
    closed, _remap = d.close([(TRIM,)], gpu_ctx)
    ext, _r = closed.extend([b"w"])
    with pytest.raises(ss.SupersonicException):
        ext.step_table(0)
    with pytest.raises(ss.SupersonicException) as e:
        d.close([(400,)], gpu_ctx)                                  # LENGTH makes no strings
    assert e.value.return_code == ss.ERROR_INVALID_ARGUMENT_VALUE


def test_substring_parameters(gpu_ctx):
    # values on both sides of the lane / wave split; positions and lengths at every edge of two lengths L on either side of it
    rng = np.random.default_rng(427)
    abc = np.frombuffer(b"abcdefgh ", np.uint8)
    values = [bytes(abc[rng.integers(0, len(abc), n)]) for n in (0, 1, 5, LONG - 1, LONG - 1, LONG, LONG + 1, LONG + 1, 300, 1300)]
    d = ss.StringDictionary(values)
    base = d.values
    done = set()
    for Lv in (LONG - 1, LONG + 1):
        for pos in (1, 0, -1, Lv, Lv + 1, -Lv, -Lv - 1, I64_MAX, I64_MIN):
            for ln in (None, 0, -1, 1, Lv, I64_MAX):
                step = (SUBSTRING, pos) if ln is None else (SUBSTRING, pos, ln)
                if step in done:
                    continue
                done.add(step)
                closed, remap = d.close([step], gpu_ctx)
                vals, T = closed.values, closed.step_table(0)
                assert vals == sorted(set(base) | {substring(v, *step[1:]) for v in base}), step
                got = [vals[T[remap[c]]] for c in range(len(base))]
                assert got == [substring(v, *step[1:]) for v in base], (step, [(len(v), len(g)) for v, g in zip(base, got)])
    assert len(done) >= 80


@pytest.mark.parametrize("steps", [[(SUBSTRING, 2, 5), (TRIM,)], [(TRIM,), (SUBSTRING, 2)], [(TRIM,), (TO_UPPER,)],
                                   [(TRIM,), (SUBSTRING, 2), (TRIM,), (SUBSTRING, 2), (TO_UPPER,), (RTRIM,)]],
                         ids=["trim(substring)", "substring(trim)", "upper(trim)", "six-steps"])
def test_nested_steps(gpu_ctx, steps):
    pool = kernel_pool()[:120]
    closed = check_close(gpu_ctx, pool, steps)           # T_k is correct on all of D_(k-1), for every k
    # the same values in another input order (and repeated): identical values and identical tables
    rng = np.random.default_rng(1)
    other = [pool[i] for i in rng.permutation(len(pool))] + pool[:7]
    again, _remap = ss.StringDictionary(other).close(steps, gpu_ctx)
    assert again.values == closed.values
    for k in range(len(steps)):
        assert np.array_equal(again.step_table(k), closed.step_table(k))


# ---- the reference's rows --------------------------------------------------------------------------------------------------
def string_view(rows_, nullable=True):
    data = np.array([(v.encode() if v is not None else b"") for v in rows_], dtype=object)
    nulls = np.array([v is None for v in rows_])
    schema = ss.TupleSchema([ss.Attribute("s", ss.STRING, ss.NULLABLE if nullable else ss.NOT_NULLABLE)])
    return ss.View(schema, [ss.Column(data, nulls) if nullable else data])


def check_rows(plan, compiled, want, label):
    (data, nulls), = run(plan)
    assert ran_compiled(plan) == compiled, plan.specialize_reason()
    assert data.dtype == object and nulls.tolist() == [w is None for w in want], label
    assert [v for v, w in zip(data, want) if w is not None] == [w.encode() for w in want if w is not None], label


def test_golden_rows(any_ctx):
    ctx, compiled = any_ctx
    ev = GOLDEN["evaluation"]
    for name, make in (("Ltrim", ss.Ltrim), ("Rtrim", ss.Rtrim), ("Trim", ss.Trim), ("ToUpper", ss.ToUpper)):
        rows = ev[name]["rows"]
        plan = ss.Plan(ss.Compute(make(NA("s")), ss.ScanView(string_view([r[0] for r in rows]))), ctx)
        check_rows(plan, compiled, [r[1] for r in rows], name)

    # one plan per distinct (position, length) over the rows that carry it; a NULL one is Null(INT64)
    def num(v):
        return ss.Null(ss.INT64) if v is None else ss.ConstInt64(v)
    rows = ev["Substring"]["rows"]
    for key in sorted({(r[1], r[2]) for r in rows}, key=str):
        mine = [r for r in rows if (r[1], r[2]) == key]
        plan = ss.Plan(ss.Compute(ss.Substring(NA("s"), num(key[0]), num(key[1])), ss.ScanView(string_view([r[0] for r in mine]))), ctx)
        check_rows(plan, compiled, [r[3] for r in mine], ("Substring", key))
    rows = ev["TrailingSubstring"]["rows"]
    for key in sorted({r[1] for r in rows}, key=str):
        mine = [r for r in rows if r[1] == key]
        plan = ss.Plan(ss.Compute(ss.TrailingSubstring(NA("s"), num(key)), ss.ScanView(string_view([r[0] for r in mine]))), ctx)
        check_rows(plan, compiled, [r[2] for r in mine], ("TrailingSubstring", key))


# ---- everywhere such an expression is legal, once -----------------------------------------------------------------------------
def small_pool():
    rng = np.random.default_rng(7)
    abc = np.frombuffer(b"abAB  ", np.uint8)
    vals = {b"", b" ", b"abc", b" abc", b"abc ", b"  ABC  ", b"Abc", b"ab\x00c ", b" \xe4b", b"x" * 140 + b" ", b"  " + b"y" * 150}
    while len(vals) < 40:
        vals.add(bytes(abc[rng.integers(0, len(abc), int(rng.integers(0, 9)))]))
    return np.array(sorted(vals), dtype=object)


def small_view(n, seed=0):
    rng = np.random.default_rng(seed + n)
    pool = small_pool()
    s = pool[rng.integers(0, len(pool), n)]
    nulls = rng.random(n) < 0.2
    s[::5] = pool[0]              # NULL rows next to rows that carry code 0: NULL in gives NULL out, never T[0]
    nulls[1::5] = True
    t = pool[rng.integers(0, len(pool), n)]
    schema = ss.TupleSchema([ss.Attribute("s", ss.STRING, ss.NULLABLE), ss.Attribute("t", ss.STRING), ss.Attribute("id", ss.INT32)])
    return ss.View(schema, [ss.Column(s, nulls), t, np.arange(n, dtype=np.int32)])


@pytest.fixture(scope="module")
def small():
    return small_view(1500, seed=3)


def cols_of(view):
    return view.column(0).data, view.column(0).is_null, view.column(1).data, view.column(2).data


def test_projection(any_ctx, small):
    ctx, compiled = any_ctx
    s, sz, t, _ids = cols_of(small)
    e = (ss.CompoundExpression().AddAs("a", ss.Trim(NA("s"))).AddAs("b", ss.ToUpper(NA("t"))).AddAs("c", ss.Substring(NA("s"), ss.ConstInt32(2), ss.ConstUint32(3)))
         .AddAs("d", ss.Ltrim(ss.Rtrim(NA("t")))).AddAs("e", ss.TrailingSubstring(ss.ConstString("  const  "), ss.ConstInt64(-4)))
         .AddAs("f", ss.Substring(NA("t"), ss.Null(ss.INT64), ss.ConstInt64(1))))
    plan = ss.Plan(ss.Compute(e, ss.ScanView(small)), ctx)
    got = run(plan)
    assert ran_compiled(plan) == compiled, plan.specialize_reason()
    const = np.array([b"  const  "] * len(t), dtype=object)
    want = [mapped(s, sz, (TRIM,)), mapped(t, None, (TO_UPPER,)), mapped(s, sz, (SUBSTRING, 2, 3)), mapped(t, None, (TRIM,)),
            mapped(const, None, (SUBSTRING, -4)), (t, np.ones(len(t), bool))]
    assert_cols_equal(got, want, context="projection")


def test_filter_on_trim_equals_constant(gpu_ctx, small):
    s, sz, _t, ids = cols_of(small)
    op = ss.Filter(ss.Equal(ss.Trim(NA("s")), ss.ConstString("abc")), ss.ProjectNamedAttributes(["id"]), ss.ScanView(small))
    (got, _z), = run(ss.Plan(op, gpu_ctx))
    keep = [i for i in range(len(s)) if not sz[i] and s[i].strip(b" ") == b"abc"]
    assert len(keep) > 0 and got.tolist() == ids[keep].tolist()
    # a constant that only exists as an image, and one that is nowhere
    for c in (b"ABC", b"nowhere"):
        op = ss.Filter(ss.Equal(ss.ToUpper(ss.Trim(NA("s"))), ss.ConstString(c)), ss.ProjectNamedAttributes(["id"]), ss.ScanView(small))
        (got, _z), = run(ss.Plan(op, gpu_ctx))
        assert got.tolist() == [int(ids[i]) for i in range(len(s)) if not sz[i] and s[i].strip(b" ").upper() == c]


def test_comparison_of_two_images(gpu_ctx, small):
    s, sz, t, _ids = cols_of(small)
    e = ss.CompoundExpression().AddAs("lt", ss.Less(ss.ToUpper(NA("s")), ss.ToUpper(NA("t")))).AddAs("eq", ss.Equal(ss.Trim(NA("s")), ss.Trim(NA("t"))))
    got = run(ss.Plan(ss.Compute(e, ss.ScanView(small)), gpu_ctx))
    lt = np.array([a.upper() < b.upper() for a, b in zip(s, t)])
    eq = np.array([a.strip(b" ") == b.strip(b" ") for a, b in zip(s, t)])
    assert lt[~sz].any() and eq[~sz].any()
    assert_cols_equal(got, [(lt, sz), (eq, sz)], context="images compared")


def test_group_key_sort_key_and_min_max(gpu_ctx, small):
    s, sz, t, ids = cols_of(small)
    e = ss.CompoundExpression().AddAs("g", ss.Trim(NA("s"))).AddAs("u", ss.ToUpper(NA("t"))).AddAs("id", NA("id"))
    spec = (ss.AggregationSpecification().AddAggregation(ss.COUNT, "", "n").AddAggregation(ss.MIN, "u", "lo").AddAggregation(ss.MAX, "u", "hi"))
    got = run(ss.Plan(ss.GroupAggregate(ss.ProjectNamedAttributes(["g"]), spec, None, ss.Compute(e, ss.ScanView(small))), gpu_ctx))
    want = {}
    for i in range(len(s)):
        k = None if sz[i] else s[i].strip(b" ")
        a = want.setdefault(k, [0, None, None])
        u = t[i].upper()
        a[0], a[1], a[2] = a[0] + 1, u if a[1] is None else min(a[1], u), u if a[2] is None else max(a[2], u)
    (kd, kz), (nd, _nz), (lo, _lz), (hi, _hz) = got
    have = {(None if kz[i] else kd[i]): [int(nd[i]), lo[i], hi[i]] for i in range(len(kd))}
    assert have == want and len(have) == len(kd) and len(have) < len({v for v in s})          # trimming merged groups
    # scalar MIN / MAX of an image
    spec = ss.AggregationSpecification().AddAggregation(ss.MIN, "g", "lo").AddAggregation(ss.MAX, "g", "hi")
    (lo, _a), (hi, _b) = run(ss.Plan(ss.ScalarAggregate(spec, ss.Compute(e, ss.ScanView(small))), gpu_ctx))
    live = [s[i].strip(b" ") for i in range(len(s)) if not sz[i]]
    assert (lo[0], hi[0]) == (min(live), max(live))
    # sort key: ORDER BY SUBSTRING(t, 1, 3), id
    e = ss.CompoundExpression().AddAs("k", ss.Substring(NA("t"), ss.ConstInt64(1), ss.ConstInt64(3))).AddAs("id", NA("id"))
    order = ss.SortOrder().add("k", ss.ASCENDING).add("id", ss.DESCENDING)
    (kd, _kz), (idd, _iz) = run(ss.Plan(ss.Sort(order, None, 0, ss.Compute(e, ss.ScanView(small))), gpu_ctx))
    want = sorted(((t[i][:3], -int(ids[i])) for i in range(len(t))))
    assert [(kd[i], -int(idd[i])) for i in range(len(kd))] == want


def test_hash_join_key(gpu_ctx, small):
    s, sz, _t, ids = cols_of(small)
    keys = sorted({v.strip(b" ") for v in small_pool()})[::2]               # every other trimmed value has a partner
    rview = ss.View(ss.TupleSchema([ss.Attribute("rk", ss.STRING), ss.Attribute("w", ss.INT64)]), [np.array(keys, dtype=object), np.arange(len(keys)) * 10])
    e = ss.CompoundExpression().AddAs("key", ss.Trim(NA("s"))).AddAs("id", NA("id"))
    proj = ss.CompoundMultiSourceProjector().add(0, ss.ProjectNamedAttributes(["id"])).add(1, ss.ProjectNamedAttributes(["w"]))
    join = ss.HashJoin(ss.INNER, ss.ProjectNamedAttribute("key"), ss.ProjectNamedAttribute("rk"), proj, ss.UNIQUE, ss.Compute(e, ss.ScanView(small)), ss.ScanView(rview))
    (idd, _iz), (wd, _wz) = run(ss.Plan(join, gpu_ctx))
    pos = {k: i * 10 for i, k in enumerate(keys)}
    want = [(int(ids[i]), pos[s[i].strip(b" ")]) for i in range(len(s)) if not sz[i] and s[i].strip(b" ") in pos]
    assert len(want) > 0 and list(zip(idd.tolist(), wd.tolist())) == want


def test_under_if_case_ifnull_and_as_haystack(gpu_ctx, small):
    s, sz, t, _ids = cols_of(small)
    case = ss.Case(ss.ExpressionList(ss.Trim(NA("t")), ss.ConstString("other"), ss.ConstString("abc"), ss.ToUpper(NA("t")), ss.ConstString(""), ss.ConstString("empty")))
    e = (ss.CompoundExpression().AddAs("a", ss.If(ss.IsNull(NA("s")), ss.Trim(NA("t")), ss.ToUpper(NA("s"))))
         .AddAs("b", ss.IfNull(ss.Trim(NA("s")), ss.ConstString("was null")))
         .AddAs("c", case)
         .AddAs("d", ss.Length(ss.Trim(NA("s")))).AddAs("e", ss.StringContains(ss.ToUpper(NA("t")), ss.ConstString("AB")))
         .AddAs("f", ss.StringOffset(ss.Substring(NA("t"), ss.ConstInt64(2), ss.ConstInt64(4)), ss.ConstString("b")))
         .AddAs("g", ss.Trim(ss.If(ss.Less(NA("id"), ss.ConstInt32(700)), NA("t"), ss.ConstString("  big  ")))))
    got = run(ss.Plan(ss.Compute(e, ss.ScanView(small)), gpu_ctx))
    n = len(s)
    a = np.array([t[i].strip(b" ") if sz[i] else s[i].upper() for i in range(n)], dtype=object)
    b = np.array([b"was null" if sz[i] else s[i].strip(b" ") for i in range(n)], dtype=object)
    c = np.array([t[i].upper() if t[i].strip(b" ") == b"abc" else b"empty" if t[i].strip(b" ") == b"" else b"other" for i in range(n)], dtype=object)
    d = np.array([len(v.strip(b" ")) for v in s], np.uint32)
    ee = np.array([v.upper().find(b"AB") >= 0 for v in t])
    f = np.array([substring(v, 2, 4).find(b"b") + 1 for v in t], np.int32)
    g = np.array([(t[i] if i < 700 else b"  big  ").strip(b" ") for i in range(n)], dtype=object)
    assert_cols_equal(got, [(a, None), (b, None), (c, None), (d, sz), (ee, None), (f, None), (g, None)], context="IF / CASE / IFNULL / haystack")


def test_concat_aggregate_of_an_image(gpu_ctx):
    view = small_view(60, seed=11)
    _s, _sz, t, ids = cols_of(view)
    e = ss.CompoundExpression().AddAs("k", ss.Modulus(NA("id"), ss.ConstInt32(4))).AddAs("v", ss.Trim(NA("t")))
    spec = ss.AggregationSpecification().AddAggregation(ss.CONCAT, "v", "all")
    (kd, _kz), (cd, _cz) = run(ss.Plan(ss.GroupAggregate(ss.ProjectNamedAttributes(["k"]), spec, None, ss.Compute(e, ss.ScanView(view))), gpu_ctx))
    want = {k: b",".join(t[i].strip(b" ") for i in range(len(t)) if ids[i] % 4 == k) for k in range(4)}
    assert {int(kd[i]): cd[i] for i in range(len(kd))} == want


def test_bound_expression_evaluate_and_skip(gpu_ctx, small):
    s, sz, t, _ids = cols_of(small)
    e = ss.CompoundExpression().AddAs("a", ss.Trim(NA("s"))).AddAs("b", ss.Length(ss.ToUpper(ss.TrailingSubstring(NA("t"), ss.ConstInt64(2)))))
    tree = e.Bind(small.schema(), None, 0, gpu_ctx)
    r = tree.Evaluate(small)
    assert not r.is_failure(), r.exception()
    want_b = (np.array([len(v[1:]) for v in t], np.uint32), None)
    assert_cols_equal(to_cols(r.view()), [mapped(s, sz, (TRIM,)), want_b], context="Evaluate")
    skip = np.zeros(len(s), bool)
    skip[::3] = True
    r = tree.DoEvaluate(small, [skip.copy(), None])
    assert not r.is_failure(), r.exception()
    got = to_cols(r.view())
    assert_cols_equal([got[0]], [mapped(s, sz | skip, (TRIM,))], context="DoEvaluate")
    assert np.array_equal(got[1][0], want_b[0])


def test_device_encoded_block_whose_codes_the_closure_moves(gpu_ctx, tmp_path, small):
    path = str(tmp_path / "strings.ssv")
    out = ss.FileOutput(path)
    out.Write(small)
    out.Finalize()
    dev = ss.FileInput(small.schema(), path, gpu_ctx, device_strings=True)
    s, sz, t, ids = cols_of(small)
    e = ss.CompoundExpression().AddAs("id", NA("id")).AddAs("s", NA("s")).AddAs("u", ss.ToUpper(NA("t"))).AddAs("x", ss.Equal(ss.Trim(NA("s")), ss.ConstString("A new one")))
    plan = ss.Plan(ss.Compute(e, ss.ScanView(dev)), gpu_ctx)
    base = dev.dictionary.values
    assert len(plan.strings) > len(base) + 1                                    # the constant and the images joined
    assert plan.strings.values.index(base[-1]) != len(base) - 1                 # ... and moved the block's codes
    got = run(plan)
    x = np.zeros(len(s), bool)
    assert_cols_equal(got, [(ids, None), (s, sz), mapped(t, None, (TO_UPPER,)), (x, sz)], context="device-encoded block")
    # a block whose dictionary needs no extension at all: the closure's remap alone recodes it
    plan = ss.Plan(ss.Compute(ss.CompoundExpression().AddAs("s", NA("s")).AddAs("u", ss.ToUpper(NA("t"))), ss.ScanView(dev)), gpu_ctx)
    assert_cols_equal(run(plan), [(s, sz), mapped(t, None, (TO_UPPER,))], context="device-encoded block, closure only")


def test_null_rows_with_an_empty_dictionary(any_ctx):
    ctx, compiled = any_ctx
    n = 700
    schema = ss.TupleSchema([ss.Attribute("s", ss.STRING, ss.NULLABLE)])
    view = ss.View(schema, [ss.Column(np.array([b""] * n, dtype=object), np.ones(n, bool))])
    e = ss.CompoundExpression().AddAs("a", ss.Trim(NA("s"))).AddAs("b", ss.Length(ss.ToUpper(ss.Substring(NA("s"), ss.ConstInt64(2), ss.ConstInt64(2)))))
    plan = ss.Plan(ss.Compute(e, ss.ScanView(view)), ctx)
    assert len(plan.strings) == 0
    got = run(plan)
    assert ran_compiled(plan) == compiled
    assert all(z.all() and len(z) == n for _d, z in got)


# ---- the guards -------------------------------------------------------------------------------------------------------------------
def test_a_run_reads_only_its_own_tables(gpu_ctx):
    schema = ss.TupleSchema([ss.Attribute("s", ss.STRING)])
    view = ss.View(schema, [np.array([b" ab ", b"cab", b"", b" b"], dtype=object)])
    e = ss.CompoundExpression().AddAs("a", ss.Trim(NA("s"))).AddAs("b", ss.ToUpper(ss.Trim(NA("s"))))
    plan = ss.Plan(ss.Compute(e, ss.ScanView(view)), gpu_ctx)
    data = view.column(0).data
    want = [mapped(data, None, (TRIM,)), (np.array([v.strip(b" ").upper() for v in data], dtype=object), None)]
    assert_cols_equal(run(plan), want)
    closed = plan.strings
    assert [st[0] for st in closed.steps] == [TRIM, TO_UPPER]
    unclosed = ss.StringDictionary(closed.values)                                # the same values, no steps
    other, _r = ss.StringDictionary(closed.values).close([(TO_UPPER,), (TRIM,)], gpu_ctx)       # closed under another list
    shorter, _r = ss.StringDictionary(closed.values).close([(TRIM,)], gpu_ctx)
    for wrong in (unclosed, other, shorter):
        plan.ctx.check(plan.lib.ssgpu_plan_set_dict(plan.handle, wrong.handle))
        with pytest.raises(ss.SupersonicException) as err:
            plan.run()
        assert err.value.return_code == ss.ERROR_INVALID_ARGUMENT_VALUE and "ssgpu_dict_close" in str(err.value)
    # a list that holds the plan's as a subsequence serves it
    wider, _r = ss.StringDictionary(closed.values).close([(LTRIM,), (TRIM,), (SUBSTRING, 1, 1), (TO_UPPER,), (TRIM,)], gpu_ctx)
    plan.ctx.check(plan.lib.ssgpu_plan_set_dict(plan.handle, wider.handle))
    plan.strings = wider                                       # (a host View is staged in codes of plan.strings, once per View object)
    assert_cols_equal(run(plan, ss.View(schema, [data.copy()])), want, context="a wider closure")
    plan.ctx.check(plan.lib.ssgpu_plan_set_dict(plan.handle, closed.handle))
    plan.strings = closed
    assert_cols_equal(run(plan, ss.View(schema, [data.copy()])), want, context="back to the plan's own")


class CountingLib(object):
    def __init__(self, lib):
        self._lib, self.closes = lib, 0

    def __getattr__(self, name):
        fn = getattr(self._lib, name)
        if name != "ssgpu_dict_close":
            return fn

        def counted(*args):
            self.closes += 1
            return fn(*args)
        return counted


def test_a_plan_without_producers_closes_nothing(gpu_ctx, small, monkeypatch):
    counting = CountingLib(L.load())
    monkeypatch.setattr(L, "_lib", counting)                   # what every StringDictionary made from here on calls through
    monkeypatch.setattr(gpu_ctx, "lib", counting)
    e = ss.CompoundExpression().AddAs("len", ss.Length(NA("s"))).AddAs("has", ss.StringContainsCI(NA("t"), ss.ConstString("ab"))).AddAs("t", NA("t"))
    plan = ss.Plan(ss.Filter(ss.Equal(NA("t"), ss.ConstString("abc")), ss.ProjectAllAttributes(), ss.Compute(e, ss.ScanView(small))), gpu_ctx)
    run(plan)
    tree = e.Bind(small.schema(), None, 0, gpu_ctx)
    assert not tree.Evaluate(small).is_failure()
    assert counting.closes == 0
    run(ss.Plan(ss.Compute(ss.Trim(NA("t")), ss.ScanView(small)), gpu_ctx))
    assert counting.closes == 1                                # the counter does see a plan with producers


# ---- fuzz ------------------------------------------------------------------------------------------------------------------------
class Gen(object):
    """Random small expressions over (s STRING NULLABLE, t STRING, id INT32) with their value under the Python restatement:
    every node is (expression factory, values, NULL mask)."""
    CONSTS = [b"", b"abc", b"  AB ", b"b a", b"A"]
    STEPS = [(LTRIM,), (RTRIM,), (TRIM,), (TO_UPPER,), (SUBSTRING, 2), (SUBSTRING, -2), (SUBSTRING, 1, 2), (SUBSTRING, 2, 3), (SUBSTRING, 0, 1), (SUBSTRING, -3, 2)]

    def __init__(self, rng, view):
        self.rng, self.n = rng, view.row_count()
        self.s, self.sz, self.t, self.ids = view.column(0).data, view.column(0).is_null, view.column(1).data, view.column(2).data
        self.producers = 0

    def pick(self, items):
        return items[int(self.rng.integers(0, len(items)))]

    @staticmethod
    def make(step, arg):
        fn = step[0]
        if fn == SUBSTRING:
            return ss.TrailingSubstring(arg, ss.ConstInt64(step[1])) if len(step) == 2 else ss.Substring(arg, ss.ConstInt32(step[1]), ss.ConstInt64(step[2]))
        return {LTRIM: ss.Ltrim, RTRIM: ss.Rtrim, TRIM: ss.Trim, TO_UPPER: ss.ToUpper}[fn](arg)

    def string(self, depth):
        """depth: how many producers may still be nested on this path"""
        k = int(self.rng.integers(0, 10 if depth > 0 else 3))
        if k == 0:
            return (lambda: NA("s")), self.s, self.sz
        if k == 1:
            return (lambda: NA("t")), self.t, np.zeros(self.n, bool)
        if k == 2:
            c = self.pick(self.CONSTS)
            return (lambda: ss.ConstString(c)), np.array([c] * self.n, dtype=object), np.zeros(self.n, bool)
        if k == 3:
            a, b = self.string(depth - 1), self.string(depth - 1)
            return (lambda: ss.IfNull(a[0](), b[0]())), np.where(a[2], b[1], a[1]), a[2] & b[2]
        if k == 4:
            bound = int(self.rng.integers(0, self.n + 1))
            a, b = self.string(depth - 1), self.string(depth - 1)
            choose = self.ids < bound
            return (lambda: ss.If(ss.Less(NA("id"), ss.ConstInt32(bound)), a[0](), b[0]())), np.where(choose, a[1], b[1]), np.where(choose, a[2], b[2])
        step, a = self.pick(self.STEPS), self.string(depth - 1)
        self.producers += 1
        d, z = mapped(a[1], a[2], step)
        return (lambda: self.make(step, a[0]())), d, z


def test_fuzz_small_plans(gpu_ctx):
    rng = np.random.default_rng(2025)
    views = [small_view(n, seed=9) for n in (1, 37, 128, 200)]
    plans = with_producers = deep = 0
    for it in range(300):
        view = views[it % len(views)]
        g = Gen(rng, view)
        shape = it % 4
        label = "fuzz plan %d (shape %d, %d rows)" % (it, shape, view.row_count())
        if shape == 0:       # Compute: every row of a STRING expression, and the length of another
            a, b = g.string(3), g.string(2)
            e = ss.CompoundExpression().AddAs("a", a[0]()).AddAs("b", ss.Length(b[0]()))
            got = run(ss.Plan(ss.Compute(e, ss.ScanView(view)), gpu_ctx))
            assert_cols_equal(got, [(a[1], a[2]), (np.array([len(v) for v in b[1]], np.uint32), b[2])], context=label)
        elif shape == 1:     # Filter: the rows where one STRING expression is less than / equal to another
            a, b = g.string(3), g.string(1)
            op, fn = g.pick([(ss.Less, lambda x, y: x < y), (ss.Equal, lambda x, y: x == y), (ss.LessOrEqual, lambda x, y: x <= y)])
            (gd, _gz), = run(ss.Plan(ss.Filter(op(a[0](), b[0]()), ss.ProjectNamedAttributes(["id"]), ss.ScanView(view)), gpu_ctx))
            keep = [i for i in range(g.n) if not a[2][i] and not b[2][i] and fn(a[1][i], b[1][i])]
            assert gd.tolist() == g.ids[keep].tolist(), label
        elif shape == 2:     # GroupAggregate: the STRING expression as the key
            a = g.string(3)
            e = ss.CompoundExpression().AddAs("k", a[0]())
            spec = ss.AggregationSpecification().AddAggregation(ss.COUNT, "", "n")
            (kd, kz), (nd, _nz) = run(ss.Plan(ss.GroupAggregate(ss.ProjectNamedAttributes(["k"]), spec, None, ss.Compute(e, ss.ScanView(view))), gpu_ctx))
            want = {}
            for i in range(g.n):
                k = None if a[2][i] else a[1][i]
                want[k] = want.get(k, 0) + 1
            kz = np.zeros(len(kd), bool) if kz is None else kz
            assert {(None if kz[i] else kd[i]): int(nd[i]) for i in range(len(kd))} == want and len(kd) == len(want), label
        else:                # ScalarAggregate over a Filter: MIN and MAX of one expression over the rows another keeps
            a, b = g.string(3), g.string(1)
            e = ss.CompoundExpression().AddAs("v", a[0]())
            spec = ss.AggregationSpecification().AddAggregation(ss.MIN, "v", "lo").AddAggregation(ss.MAX, "v", "hi").AddAggregation(ss.COUNT, "v", "n")
            pred = ss.Less(ss.Length(b[0]()), ss.ConstUint32(3))
            op = ss.ScalarAggregate(spec, ss.Compute(e, ss.Filter(pred, ss.ProjectAllAttributes(), ss.ScanView(view))))
            (lo, lz), (hi, _hz), (nd, _nz) = run(ss.Plan(op, gpu_ctx))
            live = [a[1][i] for i in range(g.n) if not b[2][i] and len(b[1][i]) < 3 and not a[2][i]]
            assert int(nd[0]) == len(live), label
            if live:
                assert (lo[0], hi[0]) == (min(live), max(live)) and not (lz is not None and lz[0]), label
            else:
                assert lz is not None and lz[0], label
        plans += 1
        with_producers += 1 if g.producers else 0
        deep += 1 if g.producers >= 3 else 0
    assert plans == 300 and with_producers >= 200 and deep >= 30
