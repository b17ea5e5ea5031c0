"""One plan that gathers from every kind of table over the STRING dictionary at once -- computed (LENGTH, STRING_OFFSET with and
without case folding), brought along by the closed dictionary (TRIM, SUBSTRING, STRING_REPLACE) and parsed (PARSE_STRING) -- from
both programs of its stage: Filter(StringContainsCI) -> Compute, so the count pass and the main program gather.  It runs at 0, 1 and
65 rows, again after ssgpu_plan_set_dict with a second closed dictionary of other values (the tables are rebuilt for it), and over
an all-NULL column.  Expected values: the Python models of the string suites (py_offset, substring, replace, parse_string_model).

The plan bakes its STRING constants as codes, so the second dictionary holds the same three constants at the same codes; the test
checks that before it relies on it.  A dictionary closed under a STRING_REPLACE step holds the step's two constants, so it is never
empty: the all-NULL case runs the whole plan over the smallest dictionary there is (the constants and their images) and the functions
that have no constant over a dictionary that is really empty."""
import numpy as np
import pytest

import supersonic_amd as ss
import parse_string_model as model
from helpers import to_cols, assert_cols_equal
from string_replace_pool import replace
from test_string_functions_gpu import py_offset
from test_string_producers_gpu import substring

NA = ss.NamedAttribute
CS = ss.ConstString
pytestmark = pytest.mark.gpu
LENGTH, TRIM, SUBSTRING, STRING_OFFSET, STRING_REPLACE = 400, 412, 427, 476, 480
SCHEMA = ss.TupleSchema([ss.Attribute("s", ss.STRING, ss.NULLABLE)])
HARD = b"1e400"           # tests/test_parse_string_gpu.py row_pool: outside the device's exact floating path, finished by the host
# eight values each: the empty string, a value with leading and trailing spaces, a value the host parses, a number the device
# parses, and the plan's three constants
FIRST = [b"", b"  banana bread  ", HARD, b"2.5e3", b"E", b"Eagle a", b"a", b"bb"]
SECOND = [b"", b" bay  sale ", b"1e-400", b" -7E1 ", b"E", b"Eprl a e", b"a", b"bb"]
CONSTS = [b"E", b"a", b"bb"]
STEPS = [(TRIM,), (SUBSTRING, 2, 3), (STRING_REPLACE, b"a", b"bb")]


def closure(values):
    """the values of the dictionary closed under STEPS (the restatement test_string_replace_gpu.check_close pins)"""
    level = set(values)
    for f in (lambda v: v.strip(b" "), lambda v: substring(v, 2, 3), lambda v: replace(v, b"a", b"bb")):
        level |= {f(v) for v in level}
    return sorted(level)


def operation(view):
    keep = ss.Filter(ss.StringContainsCI(NA("s"), CS("E")), ss.ProjectAllAttributes(), ss.ScanView(view))
    e = (ss.CompoundExpression().AddAs("len", ss.Length(NA("s"))).AddAs("off", ss.StringOffset(NA("s"), CS("a")))
         .AddAs("sub", ss.Substring(ss.Trim(NA("s")), ss.ConstInt64(2), ss.ConstInt64(3))).AddAs("rep", ss.StringReplace(NA("s"), CS("a"), CS("bb")))
         .AddAs("num", ss.ParseStringNulling(ss.DOUBLE, NA("s"))))
    return ss.Compute(e, keep)


def make_view(values, n, seed):
    rng = np.random.default_rng(seed)
    vals = np.array(list(values) + [None], dtype=object)[:-1]
    s = vals[np.arange(n) % len(vals)]            # every value occurs from 8 rows on
    nulls = rng.random(n) < 0.2
    if n > 1:
        nulls[1::5] = True
        s[1::5] = vals[0]                         # NULL rows carry code 0, like the rows of the empty string next to them
    return ss.View(SCHEMA, [ss.Column(s, nulls)])


def want(view):
    s, z = view.column(0).data, view.column(0).is_null
    rows = [v for v, null in zip(s, z) if not null and py_offset(v, b"E", True) > 0]
    parsed = [model.parse(ss.DOUBLE, v) for v in rows]
    strings = lambda f: np.array([f(v) for v in rows] + [None], dtype=object)[:-1]
    return [(np.array([len(v) for v in rows], np.uint32), None), (np.array([py_offset(v, b"a") for v in rows], np.int32), None),
            (strings(lambda v: substring(v.strip(b" "), 2, 3)), None), (strings(lambda v: replace(v, b"a", b"bb")), None),
            (np.array([p[0] for p in parsed], np.float64), np.array([p[1] for p in parsed], bool))]


def run(plan, view):
    plan.run(view)
    return to_cols(plan.fetch())


def table_lines(plan):
    return sorted(ln for ln in plan.describe().splitlines() if ln.startswith("dictionary table: "))


def want_lines(d, hard):
    a, bb = d.code_of(b"a"), d.code_of(b"bb")
    return sorted(["dictionary table: LENGTH", "dictionary table: STRING_OFFSET needle code %d length 1 fold 0" % a,
                   "dictionary table: STRING_OFFSET needle code %d length 1 fold 1" % d.code_of(b"E"), "dictionary table: TRIM (codes of the closed dictionary)",
                   "dictionary table: SUBSTRING position 2 length 3 (codes of the closed dictionary)",
                   "dictionary table: STRING_REPLACE needle code %d substitute code %d (codes of the closed dictionary)" % (a, bb),
                   "dictionary table: PARSE_STRING to DOUBLE (values and failure bytes) host-resolved entries of the plan's floating tables: %d" % hard])


def hard_count(values):
    return sum(1 for v in values if model.fast_path(ss.DOUBLE, v) is False)


def test_every_kind_of_table_in_both_programs_and_their_rebuild(gpu_ctx):
    assert len(set(FIRST)) == len(set(SECOND)) == 8 and set(FIRST) & set(SECOND) == set(CONSTS) | {b""}
    assert model.fast_path(ss.DOUBLE, HARD) is False and model.fast_path(ss.DOUBLE, b"2.5e3") is True
    plan = ss.Plan(operation(make_view(FIRST, 65, 1)), gpu_ctx, extra_strings=FIRST)
    first = plan.strings
    assert first.values == closure(FIRST)
    assert [st[0] for st in first.steps] == [st[0] for st in STEPS]
    stage, = plan.stage_info()
    for n in (0, 1, 65):
        view = make_view(FIRST, n, n)
        got = run(plan, view)
        assert_cols_equal(got, want(view), context="%d rows" % n)
        assert len(got[0][0]) == {0: 0, 1: 0}.get(n, len(got[0][0])) and (n < 65 or (0 < len(got[0][0]) < 65 and got[4][1].any() and not got[4][1].all()))
        assert table_lines(plan) == want_lines(first, hard_count(first.values)), plan.describe()
    # another closed dictionary, other values: the plan's constants keep their codes (they are baked into its programs and steps)
    second, _remap = ss.StringDictionary(SECOND).close(STEPS, gpu_ctx)
    assert second.values == closure(SECOND) and second.values != first.values
    assert [second.code_of(c) for c in CONSTS] == [first.code_of(c) for c in CONSTS] and second.steps == first.steps
    plan.ctx.check(plan.lib.ssgpu_plan_set_dict(plan.handle, second.handle))
    plan.strings = second
    view = make_view(SECOND, 65, 2)
    got = run(plan, view)
    assert_cols_equal(got, want(view), context="65 rows after a second ssgpu_plan_set_dict")
    assert 0 < len(got[0][0]) < 65 and table_lines(plan) == want_lines(second, hard_count(second.values)), plan.describe()


def test_all_null_column_over_the_smallest_and_the_empty_dictionary(gpu_ctx):
    n = 65
    view = ss.View(SCHEMA, [ss.Column(np.array([b""] * n, dtype=object), np.ones(n, bool))])
    plan = ss.Plan(operation(view), gpu_ctx)
    assert plan.strings.values == closure(CONSTS)            # the constants and their images, nothing else
    got = run(plan, view)
    assert len(got) == 5 and all(len(d) == 0 for d, _z in got)
    # no constants: the dictionary is empty and every table its one dummy entry
    e = (ss.CompoundExpression().AddAs("len", ss.Length(NA("s"))).AddAs("sub", ss.Substring(ss.Trim(NA("s")), ss.ConstInt64(2), ss.ConstInt64(3)))
         .AddAs("num", ss.ParseStringNulling(ss.DOUBLE, NA("s"))))
    plan = ss.Plan(ss.Compute(e, ss.ScanView(view)), gpu_ctx)
    assert len(plan.strings) == 0
    got = run(plan, view)
    assert len(got) == 3 and all(len(z) == n and z.all() for _d, z in got)
