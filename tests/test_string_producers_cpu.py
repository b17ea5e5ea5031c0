"""LTRIM / RTRIM / TRIM, TO_UPPER and SUBSTRING at bind time (bind-only context, no device): result names, types and nullability
as the reference states them (tests/golden/string_producing_cases.json), every refusal with its code -- TO_LOWER as a value
included, which stays refused --, the plan's step list (ssgpu_plan_string_steps), what needs a device and what does not, and the
C++ mirror's declarations."""
import ctypes as C
import json
import os
import subprocess
import tempfile

import pytest

import supersonic_amd as ss
from supersonic_amd import _lib as L

NA = ss.NamedAttribute
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = json.load(open(os.path.join(ROOT, "tests", "golden", "string_producing_cases.json")))
TYPES = {"STRING": ss.STRING, "INT32": ss.INT32, "UINT32": ss.UINT32, "INT64": ss.INT64, "UINT64": ss.UINT64, "BOOL": ss.BOOL,
         "DATETIME": ss.DATETIME, "DOUBLE": ss.DOUBLE, "FLOAT": ss.FLOAT}
FUNCTIONS = {"Ltrim": ss.Ltrim, "Rtrim": ss.Rtrim, "Trim": ss.Trim, "ToUpper": ss.ToUpper, "Substring": ss.Substring,
             "TrailingSubstring": ss.TrailingSubstring}
CONSTS = {"INT32": ss.ConstInt32, "UINT32": ss.ConstUint32, "INT64": ss.ConstInt64, "UINT64": ss.ConstUint64, "DOUBLE": ss.ConstDouble,
          "FLOAT": ss.ConstFloat}
LTRIM, RTRIM, TRIM, TO_UPPER, SUBSTRING = 404, 408, 412, 416, 427


@pytest.fixture(scope="module")
def ctx():
    return ss.Context(-1)


def scan(*attrs):
    """A schema-only input: nothing is read at bind time."""
    schema = ss.TupleSchema([ss.Attribute(n, t, z) for n, t, z in attrs])
    return ss.ScanView(ss.DeviceView(schema, [(0, 0)] * len(attrs), 0))


def bound(ctx, expr, *attrs):
    plan = ss.Plan(ss.Compute(expr, scan(*attrs)), ctx)
    a = plan.result_schema.attribute(0)
    return plan, (a.name(), a.type(), a.is_nullable())


def refusal(ctx, expr, *attrs):
    with pytest.raises(ss.SupersonicException) as e:
        ss.Plan(ss.Compute(expr, scan(*attrs)), ctx)
    return e.value.return_code, str(e.value)


def steps_of(plan):
    n = plan.lib.ssgpu_plan_string_steps(plan.handle, None, 0)
    recs = (L.StringStep * max(n, 1))()
    assert plan.lib.ssgpu_plan_string_steps(plan.handle, recs, n) == n
    return [(r.fn, r.has_len, r.pos, r.len) for r in recs[:n]]


@pytest.mark.parametrize("fact", GOLDEN["binding"], ids=[f["line"] for f in GOLDEN["binding"]])
def test_reference_binding_facts(ctx, fact):
    # the reference binds attributes; here the position and the length are constants, so their placeholders read CONST_<type> --
    # a promoted constant is folded, as everywhere in this binder, and reads CONST_INT64
    args = [NA("$0")] + [CONSTS[t](2) for t in fact["arg_types"][1:]]
    _plan, (name, dtype, nullable) = bound(ctx, FUNCTIONS[fact["function"]](*args), ("$0", ss.STRING, ss.NOT_NULLABLE))
    assert (dtype, nullable) == (TYPES[fact["type"]], fact["nullable"])
    want = fact["description"]
    for i, _t in enumerate(fact["arg_types"][1:], 1):
        want = want.replace("CAST_INT32_TO_INT64($%d)" % i, "CONST_INT64").replace("CAST_UINT32_TO_INT64($%d)" % i, "CONST_INT64").replace("$%d" % i, "CONST_INT64")
    assert name == want


@pytest.mark.parametrize("fact", GOLDEN["binding_failures"], ids=[f["line"] for f in GOLDEN["binding_failures"]])
def test_reference_binding_failures(ctx, fact):
    args = [NA("$0")] + [CONSTS[t](2) for t in fact["arg_types"][1:]]
    code, _msg = refusal(ctx, FUNCTIONS[fact["function"]](*args), ("$0", TYPES[fact["arg_types"][0]], ss.NOT_NULLABLE))
    assert code == ss.ERROR_ATTRIBUTE_TYPE_MISMATCH


def test_names_types_and_nullability(ctx):
    s, t = ("s", ss.STRING, ss.NULLABLE), ("t", ss.STRING, ss.NOT_NULLABLE)
    for make, name in ((ss.Ltrim, "LTRIM"), (ss.Rtrim, "RTRIM"), (ss.Trim, "TRIM"), (ss.ToUpper, "TO_UPPER")):
        assert bound(ctx, make(NA("s")), s)[1] == (name + "(s)", ss.STRING, True)
        assert bound(ctx, make(NA("t")), t)[1] == (name + "(t)", ss.STRING, False)
        assert bound(ctx, make(ss.ConstString(" x ")), t)[1] == (name + "(CONST_STRING)", ss.STRING, False)
    assert bound(ctx, ss.Substring(NA("t"), ss.ConstInt64(2), ss.ConstInt64(3)), t)[1] == ("SUBSTRING(t, CONST_INT64, CONST_INT64)", ss.STRING, False)
    assert bound(ctx, ss.Substring(NA("s"), ss.ConstInt64(2), ss.ConstInt64(3)), s)[1] == ("SUBSTRING(s, CONST_INT64, CONST_INT64)", ss.STRING, True)
    assert bound(ctx, ss.TrailingSubstring(NA("t"), ss.ConstInt64(-2)), t)[1] == ("SUBSTRING(t, CONST_INT64)", ss.STRING, False)
    # any integer type is taken as INT64 (promoted constants fold, as elsewhere in this binder)
    for make in (ss.ConstInt32, ss.ConstUint32, ss.ConstInt64, ss.ConstUint64):
        assert bound(ctx, ss.Substring(NA("t"), make(1), make(2)), t)[1] == ("SUBSTRING(t, CONST_INT64, CONST_INT64)", ss.STRING, False)
    # nullability follows the arguments: a NULL position or length makes the result NULLABLE (and all NULL: no table)
    plan, fact = bound(ctx, ss.Substring(NA("t"), ss.Null(ss.INT64), ss.ConstInt64(1)), t)
    assert fact == ("SUBSTRING(t, NULL, CONST_INT64)", ss.STRING, True) and "dictionary table" not in plan.describe() and steps_of(plan) == []
    plan, fact = bound(ctx, ss.Substring(NA("t"), ss.ConstInt64(1), ss.Null(ss.INT32)), t)
    assert fact == ("SUBSTRING(t, CONST_INT64, NULL)", ss.STRING, True) and steps_of(plan) == []
    plan, fact = bound(ctx, ss.TrailingSubstring(NA("t"), ss.Null(ss.INT64)), t)
    assert fact == ("SUBSTRING(t, NULL)", ss.STRING, True) and steps_of(plan) == []
    # nested, and under / over the existing functions
    assert bound(ctx, ss.Trim(ss.Substring(NA("s"), ss.ConstInt64(2), ss.ConstInt64(5))), s)[1] == ("TRIM(SUBSTRING(s, CONST_INT64, CONST_INT64))", ss.STRING, True)
    assert bound(ctx, ss.Length(ss.Trim(NA("t"))), t)[1] == ("LENGTH(TRIM(t))", ss.UINT32, False)
    assert bound(ctx, ss.StringContainsCI(ss.Trim(NA("t")), ss.ConstString("x")), t)[1] == (
        "(CONST_UINT32 < STRING_OFFSET(TO_LOWER(TRIM(t)), TO_LOWER(CONST_STRING)))", ss.BOOL, False)
    assert bound(ctx, ss.Equal(ss.ToUpper(NA("s")), ss.ConstString("X")), s)[1] == ("(TO_UPPER(s) == CONST_STRING)", ss.BOOL, True)
    assert bound(ctx, ss.Trim(ss.IfNull(NA("s"), NA("t"))), s, t)[1] == ("TRIM(IFNULL(s, t))", ss.STRING, False)


def test_refusals(ctx):
    s, t = ("s", ss.STRING, ss.NULLABLE), ("t", ss.STRING, ss.NOT_NULLABLE)
    x, b, f = ("x", ss.INT32, ss.NOT_NULLABLE), ("b", ss.BINARY, ss.NOT_NULLABLE), ("f", ss.DOUBLE, ss.NOT_NULLABLE)
    one = ss.ConstInt64(1)
    # a non-STRING first argument, BINARY included: a type mismatch, no promotion
    for expr in (ss.Ltrim(NA("x")), ss.Rtrim(NA("b")), ss.Trim(NA("f")), ss.ToUpper(NA("x")), ss.Trim(ss.ConstInt32(1)), ss.ToUpper(ss.Length(NA("t"))),
                 ss.Substring(NA("x"), one, one), ss.Substring(NA("b"), one, one), ss.TrailingSubstring(NA("f"), one)):
        assert refusal(ctx, expr, t, x, b, f)[0] == ss.ERROR_ATTRIBUTE_TYPE_MISMATCH
    # a FLOAT / DOUBLE (or any non-integer) position or length, constant or not
    for expr in (ss.Substring(NA("t"), ss.ConstDouble(1.0), one), ss.Substring(NA("t"), one, ss.ConstFloat(1.0)), ss.TrailingSubstring(NA("t"), ss.ConstDouble(2.0)),
                 ss.Substring(NA("t"), NA("f"), one), ss.Substring(NA("t"), one, ss.ConstString("1")), ss.Substring(NA("t"), ss.ConstBool(True), one),
                 ss.TrailingSubstring(NA("t"), NA("t")), ss.Substring(NA("t"), ss.Null(ss.DOUBLE), one)):
        assert refusal(ctx, expr, t, x, b, f)[0] == ss.ERROR_ATTRIBUTE_TYPE_MISMATCH
    # a position or a length that varies per row
    for expr, word in ((ss.Substring(NA("t"), NA("x"), one), "position"), (ss.Substring(NA("t"), one, NA("x")), "length"),
                       (ss.TrailingSubstring(NA("t"), NA("x")), "position"), (ss.Substring(NA("t"), ss.Plus(NA("x"), ss.ConstInt32(1)), one), "position"),
                       (ss.Substring(NA("t"), one, ss.Length(NA("t"))), "length")):
        code, msg = refusal(ctx, expr, t, x)
        assert code == ss.ERROR_NOT_IMPLEMENTED and word in msg and "varies per row" in msg
    # wrong arity
    assert refusal(ctx, ss.api._op(TRIM, NA("t"), NA("t")), t)[0] == ss.ERROR_ATTRIBUTE_COUNT_MISMATCH
    assert refusal(ctx, ss.api._op(SUBSTRING, NA("t")), t)[0] == ss.ERROR_ATTRIBUTE_COUNT_MISMATCH
    assert refusal(ctx, ss.api._op(SUBSTRING, NA("t"), one, one, one), t)[0] == ss.ERROR_ATTRIBUTE_COUNT_MISMATCH
    # TO_LOWER as a value: still refused, in every form, next to the new functions too
    for expr in (ss.ToLower(NA("t")), ss.Length(ss.ToLower(NA("t"))), ss.Equal(ss.ToLower(NA("t")), ss.ConstString("a")),
                 ss.StringOffset(ss.ToLower(NA("t")), ss.ConstString("a")), ss.StringOffset(NA("t"), ss.ToLower(ss.ConstString("a"))),
                 ss.Alias("low", ss.ToLower(NA("t"))), ss.StringOffset(ss.ToLower(ss.ToLower(NA("t"))), ss.ToLower(ss.ConstString("a"))),
                 ss.Trim(ss.ToLower(NA("t"))), ss.ToUpper(ss.ToLower(NA("t"))), ss.ToLower(ss.Trim(NA("t"))), ss.Substring(ss.ToLower(NA("t")), one, one),
                 ss.If(ss.IsNull(NA("t")), ss.ToLower(NA("t")), ss.Trim(NA("t")))):
        code, msg = refusal(ctx, expr, t)
        assert code == ss.ERROR_NOT_IMPLEMENTED and "TO_LOWER" in msg


def test_slot_limit_counts_producer_tables(ctx):
    t = ("t", ss.STRING, ss.NOT_NULLABLE)

    def many(n):
        e = ss.CompoundExpression()
        for i in range(n):
            e.AddAs("o%d" % i, ss.TrailingSubstring(NA("t"), ss.ConstInt64(i + 1)))
        return e
    assert ss.Plan(ss.Compute(many(24), scan(t)), ctx).describe().count("dictionary table: SUBSTRING") == 24
    code, msg = refusal(ctx, many(25), t)
    assert code == ss.ERROR_NOT_IMPLEMENTED and "slots" in msg
    # nodes with an equal (function, position, length) key share one slot
    e = ss.CompoundExpression()
    for i in range(30):
        e.AddAs("o%d" % i, ss.Substring(ss.IfNull(NA("t"), ss.ConstString("c%d" % i)), ss.ConstInt64(i % 3), ss.ConstInt64(2)))
    assert ss.Plan(ss.Compute(e, scan(t)), ctx).describe().count("dictionary table") == 3


def test_step_list_is_post_order(ctx):
    s, k = ("s", ss.STRING, ss.NULLABLE), ("k", ss.INT32, ss.NOT_NULLABLE)
    two, five = ss.ConstInt64(2), ss.ConstInt32(5)
    # arguments before the node that uses them; columns left to right
    e = (ss.CompoundExpression().AddAs("a", ss.Trim(ss.Substring(NA("s"), two, five))).AddAs("b", ss.TrailingSubstring(ss.Trim(NA("s")), two))
         .AddAs("c", ss.ToUpper(ss.Ltrim(ss.Rtrim(NA("s"))))))
    plan = ss.Plan(ss.Compute(e, scan(s)), ctx)
    assert steps_of(plan) == [(SUBSTRING, 1, 2, 5), (TRIM, 0, 0, 0), (TRIM, 0, 0, 0), (SUBSTRING, 0, 2, 0), (RTRIM, 0, 0, 0), (LTRIM, 0, 0, 0), (TO_UPPER, 0, 0, 0)]
    # a key that occurs twice is listed twice -- depth needs it: TRIM(SUBSTRING(TRIM(s), 2)) is three steps
    plan = ss.Plan(ss.Compute(ss.Trim(ss.TrailingSubstring(ss.Trim(NA("s")), two)), scan(s)), ctx)
    assert steps_of(plan) == [(TRIM, 0, 0, 0), (SUBSTRING, 0, 2, 0), (TRIM, 0, 0, 0)]
    # every program of every stage counts: a Filter's predicate is evaluated by the counting pass and by the main program,
    # and a second stage adds its own nodes behind the first one's
    spec = ss.AggregationSpecification().AddAggregation(ss.COUNT, "", "n")
    op = ss.Compute(ss.CompoundExpression().AddAs("u", ss.ToUpper(NA("g"))).AddAs("n", NA("n")),
                    ss.GroupAggregate(ss.ProjectNamedAttributes(["g"]), spec, None,
                                      ss.Compute(ss.CompoundExpression().AddAs("g", ss.Trim(NA("s"))), scan(s, k))))
    got = steps_of(ss.Plan(op, ctx))          # (the GroupAggregate stage has a partition-scatter program next to its main one)
    assert got[-1] == (TO_UPPER, 0, 0, 0) and len(got) >= 2 and set(got[:-1]) == {(TRIM, 0, 0, 0)}
    filt = ss.Filter(ss.Equal(ss.Rtrim(NA("s")), ss.ConstString("x")), ss.ProjectAllAttributes(), scan(s, k))
    got = steps_of(ss.Plan(filt, ctx))
    assert len(got) >= 1 and set(got) == {(RTRIM, 0, 0, 0)}
    # no producers: 0, and nothing is written
    plan = ss.Plan(ss.Compute(ss.Length(NA("s")), scan(s)), ctx)
    assert plan.lib.ssgpu_plan_string_steps(plan.handle, None, 0) == 0 and steps_of(plan) == []
    # a short buffer gets the first `cap` records and the full count
    plan = ss.Plan(ss.Compute(e, scan(s)), ctx)
    recs = (L.StringStep * 2)()
    assert plan.lib.ssgpu_plan_string_steps(plan.handle, recs, 2) == 7 and [r.fn for r in recs] == [SUBSTRING, TRIM]


def test_describe_names_producer_tables(ctx):
    s = ("s", ss.STRING, ss.NULLABLE)
    e = (ss.CompoundExpression().AddAs("a", ss.Trim(NA("s"))).AddAs("b", ss.Substring(NA("s"), ss.ConstInt64(-3), ss.ConstInt64(2)))
         .AddAs("c", ss.TrailingSubstring(NA("s"), ss.ConstInt64(4))).AddAs("d", ss.Length(ss.ToUpper(NA("s")))))
    lines = [ln for ln in ss.Plan(ss.Compute(e, scan(s)), ctx).describe().splitlines() if ln.startswith("dictionary table")]
    assert lines == ["dictionary table: TRIM (codes of the closed dictionary)",
                     "dictionary table: SUBSTRING position -3 length 2 (codes of the closed dictionary)",
                     "dictionary table: SUBSTRING position 4 to the end (codes of the closed dictionary)",
                     "dictionary table: TO_UPPER (codes of the closed dictionary)",
                     "dictionary table: LENGTH"]


def test_closing_needs_a_device_and_binding_does_not(ctx):
    d = ss.StringDictionary([b" a", b"bb "])
    for steps in ([(TRIM,)], []):
        with pytest.raises(ss.SupersonicException) as e:
            d.close(steps, ctx)
        assert e.value.return_code == ss.ERROR_NO_DEVICE
    with pytest.raises(ss.SupersonicException):
        d.step_table(0)                                        # not a closed dictionary
    # a plan with producers over host strings still binds on a bind-only context: it keeps the first plan and its unclosed dictionary
    import numpy as np
    view = ss.View(ss.TupleSchema([ss.Attribute("s", ss.STRING)]), [np.array([b" abc ", b"x"], dtype=object)])
    op = ss.Compute(ss.CompoundExpression().AddAs("t", ss.Trim(NA("s"))).AddAs("c", ss.Equal(ss.Trim(NA("s")), ss.ConstString("abc"))), ss.ScanView(view))
    plan = ss.Plan(op, ctx)
    assert plan.result_schema.attribute(0).name() == "t" and plan.result_schema.attribute(0).type() == ss.STRING
    assert "dictionary table: TRIM" in plan.describe() and sorted(plan.strings.values) == [b" abc ", b"abc", b"x"]
    tree = ss.Trim(NA("s")).Bind(view.schema(), None, 0, ctx)
    assert tree.result_schema.attribute(0).name() == "TRIM(s)"
    # ... and running it fails loudly
    r = op.CreateCursor(ctx).Next(1024)
    assert r.is_failure() and r.exception().return_code == ss.ERROR_NO_DEVICE


def test_abi_version_is_unchanged_and_the_symbols_are_bound():
    lib = L.load()
    assert lib.ssgpu_abi_version() == 10
    bound_names = {n for n, _r, _a in L.SYMBOLS}
    assert {"ssgpu_plan_string_steps", "ssgpu_dict_close", "ssgpu_dict_step_table"} <= bound_names
    assert C.sizeof(L.StringStep) == 24


def test_cpp_mirror_compiles():
    src = """
#include "supersonic/supersonic.h"
#include "supersonic/expression/core/string_expressions.h"
using namespace supersonic;
int main() {
  const Expression* a = Ltrim(NamedAttribute("s"));
  const Expression* b = Rtrim(NamedAttribute("s"));
  const Expression* c = Trim(Substring(NamedAttribute("s"), ConstInt64(2), ConstInt32(5)));
  const Expression* d = ToUpper(TrailingSubstring(NamedAttribute("s"), ConstInt64(-3)));
  const Expression* e = Equal(Trim(NamedAttribute("s")), ConstString("x"));
  delete a; delete b; delete c; delete d; delete e;
  return 0;
}
"""
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "string_producer_mirror.cc")
        open(path, "w").write(src)
        subprocess.check_call(["g++", "-std=c++14", "-fsyntax-only", "-D__HIP_PLATFORM_AMD__", "-I" + os.path.join(ROOT, "include"), path])
