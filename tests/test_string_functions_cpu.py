"""LENGTH, STRING_OFFSET, StringContains(CI) and TO_LOWER at bind time (bind-only context, no device): result names, types and
nullability as the reference states them (tests/golden/string_expression_cases.json), every refusal with its code, the
describe() line of a dictionary table, and the chunked forms the operators leave as they are."""
import json
import os
import subprocess
import tempfile

import pytest

import supersonic_amd as ss

NA = ss.NamedAttribute
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = json.load(open(os.path.join(ROOT, "tests", "golden", "string_expression_cases.json")))
TYPES = {"STRING": ss.STRING, "INT32": ss.INT32, "UINT32": ss.UINT32, "BOOL": ss.BOOL, "BINARY": ss.BINARY, "FLOAT": ss.FLOAT}
FUNCTIONS = {"Length": ss.Length, "StringOffset": ss.StringOffset, "StringContains": ss.StringContains, "StringContainsCI": ss.StringContainsCI}


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


def const_of(type_name):
    return {"STRING": ss.ConstString("needle"), "INT32": ss.ConstInt32(1)}[type_name]


@pytest.mark.parametrize("fact", GOLDEN["binding"], ids=[f["line"] for f in GOLDEN["binding"]])
def test_reference_binding_facts(ctx, fact):
    # the reference binds two attributes; here the needle is a constant, so its placeholder reads CONST_STRING
    args = [NA("$0")] + [const_of(t) for t in fact["arg_types"][1:]]
    _plan, (name, dtype, nullable) = bound(ctx, FUNCTIONS[fact["function"]](*args), ("$0", TYPES[fact["arg_types"][0]], ss.NOT_NULLABLE))
    assert (dtype, nullable) == (TYPES[fact["type"]], fact["nullable"])
    if "(9)" not in fact["description"]:      # (that description is the reference test's own rendering; the bound fact next to it names both arguments)
        assert name == fact["description"].replace("$1", "CONST_STRING")


@pytest.mark.parametrize("fact", GOLDEN["binding_failures"], ids=[f["line"] for f in GOLDEN["binding_failures"]])
def test_reference_binding_failures(ctx, fact):
    args = [NA("$0")] + [const_of(t) for t in fact["arg_types"][1:]]
    code, _msg = refusal(ctx, FUNCTIONS[fact["function"]](*args), ("$0", TYPES[fact["arg_types"][0]], ss.NOT_NULLABLE))
    assert code == ss.ERROR_ATTRIBUTE_TYPE_MISMATCH


def test_names_types_and_nullability(ctx):
    s, t = ("s", ss.STRING, ss.NULLABLE), ("t", ss.STRING, ss.NOT_NULLABLE)
    assert bound(ctx, ss.Length(NA("s")), s)[1] == ("LENGTH(s)", ss.UINT32, True)
    assert bound(ctx, ss.Length(NA("t")), t)[1] == ("LENGTH(t)", ss.UINT32, False)
    assert bound(ctx, ss.StringOffset(NA("s"), ss.ConstString("x")), s)[1] == ("STRING_OFFSET(s, CONST_STRING)", ss.INT32, True)
    assert bound(ctx, ss.StringOffset(NA("t"), ss.ConstString("x")), t)[1] == ("STRING_OFFSET(t, CONST_STRING)", ss.INT32, False)
    assert bound(ctx, ss.StringOffset(NA("t"), ss.Null(ss.STRING)), t)[1] == ("STRING_OFFSET(t, NULL)", ss.INT32, True)      # nullable iff either argument is
    assert bound(ctx, ss.StringOffset(ss.ConstString("hay"), ss.ConstString("a")), t)[1] == ("STRING_OFFSET(CONST_STRING, CONST_STRING)", ss.INT32, False)
    hay = ss.If(ss.IsNull(NA("s")), NA("t"), NA("s"))
    assert bound(ctx, ss.StringOffset(hay, ss.ConstString("x")), s, t)[1] == ("STRING_OFFSET(IF ISNULL(s) THEN t ELSE s, CONST_STRING)", ss.INT32, True)
    assert bound(ctx, ss.Length(ss.IfNull(NA("s"), ss.ConstString(""))), s)[1] == ("LENGTH(IFNULL(s, CONST_STRING))", ss.UINT32, False)


def test_predicates_are_the_references_compositions(ctx):
    s, t = ("s", ss.STRING, ss.NULLABLE), ("t", ss.STRING, ss.NOT_NULLABLE)
    assert bound(ctx, ss.StringContains(NA("t"), ss.ConstString("x")), t)[1] == ("(CONST_UINT32 < STRING_OFFSET(t, CONST_STRING))", ss.BOOL, False)
    assert bound(ctx, ss.StringContains(NA("s"), ss.ConstString("x")), s)[1] == ("(CONST_UINT32 < STRING_OFFSET(s, CONST_STRING))", ss.BOOL, True)
    assert bound(ctx, ss.StringContainsCI(NA("s"), ss.ConstString("x")), s)[1] == (
        "(CONST_UINT32 < STRING_OFFSET(TO_LOWER(s), TO_LOWER(CONST_STRING)))", ss.BOOL, True)
    # the explicit form of StringContainsCI binds to the same thing
    explicit = ss.Less(ss.ConstUint32(0), ss.StringOffset(ss.ToLower(NA("t")), ss.ToLower(ss.ConstString("x"))))
    assert bound(ctx, explicit, t)[1] == ("(CONST_UINT32 < STRING_OFFSET(TO_LOWER(t), TO_LOWER(CONST_STRING)))", ss.BOOL, False)


def test_refusals(ctx):
    s, t = ("s", ss.STRING, ss.NULLABLE), ("t", ss.STRING, ss.NOT_NULLABLE)
    x, b = ("x", ss.INT32, ss.NOT_NULLABLE), ("b", ss.BINARY, ss.NOT_NULLABLE)
    # a needle that varies per row
    code, msg = refusal(ctx, ss.StringOffset(NA("t"), NA("s")), s, t)
    assert code == ss.ERROR_NOT_IMPLEMENTED and "needle" in msg
    assert refusal(ctx, ss.StringContains(NA("t"), ss.IfNull(NA("s"), ss.ConstString("x"))), s, t)[0] == ss.ERROR_NOT_IMPLEMENTED
    # a non-STRING argument on either side, BINARY included: a type mismatch, no promotion
    for expr in (ss.Length(NA("x")), ss.Length(NA("b")), ss.StringOffset(NA("x"), ss.ConstString("a")), ss.StringOffset(NA("b"), ss.ConstString("a")),
                 ss.StringOffset(NA("t"), ss.ConstInt32(1)), ss.StringOffset(NA("t"), NA("b")), ss.StringOffset(NA("t"), NA("x")),
                 ss.StringContains(NA("x"), ss.ConstString("a")), ss.StringContainsCI(NA("t"), ss.ConstInt32(1)), ss.StringContainsCI(NA("b"), ss.ConstString("a"))):
        assert refusal(ctx, expr, t, x, b)[0] == ss.ERROR_ATTRIBUTE_TYPE_MISMATCH
    # TO_LOWER anywhere but under both arguments of a STRING_OFFSET
    for expr in (ss.ToLower(NA("t")), ss.Length(ss.ToLower(NA("t"))), ss.Equal(ss.ToLower(NA("t")), ss.ConstString("a")),
                 ss.StringOffset(ss.ToLower(NA("t")), ss.ConstString("a")), ss.StringOffset(NA("t"), ss.ToLower(ss.ConstString("a"))),
                 ss.Alias("low", ss.ToLower(NA("t"))), ss.StringOffset(ss.ToLower(ss.ToLower(NA("t"))), ss.ToLower(ss.ConstString("a")))):
        code, msg = refusal(ctx, expr, t)
        assert code == ss.ERROR_NOT_IMPLEMENTED and "TO_LOWER" in msg
    # wrong arity
    assert refusal(ctx, ss.api._op(476, NA("t")), t)[0] == ss.ERROR_ATTRIBUTE_COUNT_MISMATCH


def test_slot_limit_is_a_bind_error(ctx):
    t = ("t", ss.STRING, ss.NOT_NULLABLE)

    def many(n):
        e = ss.CompoundExpression()
        for i in range(n):
            e.AddAs("o%d" % i, ss.StringOffset(NA("t"), ss.ConstString("needle %d" % i)))
        return e
    plan = ss.Plan(ss.Compute(many(24), scan(t)), ctx)               # the 24 gather slots of a pipeline
    assert plan.describe().count("dictionary table: STRING_OFFSET") == 24
    code, msg = refusal(ctx, many(25), t)
    assert code == ss.ERROR_NOT_IMPLEMENTED and "slots" in msg
    # equal (function, needle, fold) nodes share one table: 30 columns over 3 tables bind
    e = ss.CompoundExpression()
    for i in range(30):
        e.AddAs("o%d" % i, ss.Plus(ss.StringOffset(NA("t"), ss.ConstString("n%d" % (i % 3))), ss.ConstInt32(i)))
    assert ss.Plan(ss.Compute(e, scan(t)), ctx).describe().count("dictionary table") == 3


def test_describe_names_every_table(ctx):
    s = ("s", ss.STRING, ss.NULLABLE)
    e = (ss.CompoundExpression().AddAs("l", ss.Length(NA("s"))).AddAs("a", ss.StringOffset(NA("s"), ss.ConstString("abc")))
         .AddAs("b", ss.StringContainsCI(NA("s"), ss.ConstString("abcde"))).AddAs("c", ss.StringContains(NA("s"), ss.ConstString("abc"))))
    lines = [ln for ln in ss.Plan(ss.Compute(e, scan(s)), ctx).describe().splitlines() if ln.startswith("dictionary table")]
    assert lines == ["dictionary table: LENGTH",
                     "dictionary table: STRING_OFFSET needle code 0 length 3 fold 0",
                     "dictionary table: STRING_OFFSET needle code 1 length 5 fold 1"]
    # a NULL needle needs no table; a plan without the operators gains no line
    assert "dictionary table" not in ss.Plan(ss.Compute(ss.StringOffset(NA("s"), ss.Null(ss.STRING)), scan(s)), ctx).describe()
    assert "dictionary table" not in ss.Plan(ss.Compute(ss.Equal(NA("s"), ss.ConstString("abc")), scan(s)), ctx).describe()


def test_chunked_form_is_unchanged(ctx):
    s, k = ("s", ss.STRING, ss.NULLABLE), ("k", ss.INT32, ss.NOT_NULLABLE)
    plain = ss.Plan(ss.Filter(ss.Equal(NA("s"), ss.ConstString("abc")), ss.ProjectAllAttributes(), scan(s, k)), ctx).chunked_form()
    with_fn = ss.Plan(ss.Filter(ss.StringContains(NA("s"), ss.ConstString("abc")), ss.ProjectAllAttributes(), scan(s, k)), ctx).chunked_form()
    assert plain[0] == with_fn[0] == 2
    spec = ss.AggregationSpecification().AddAggregation(ss.SUM, "v", "sum")

    def grouped(key, value):
        e = ss.CompoundExpression().AddAs("g", key).AddAs("v", value)
        return ss.Plan(ss.GroupAggregate(ss.ProjectNamedAttributes(["g"]), spec, None, ss.Compute(e, scan(s, k))), ctx).chunked_form()
    plain = grouped(NA("k"), NA("k"))
    with_fn = grouped(ss.Length(NA("s")), ss.StringOffset(NA("s"), ss.ConstString("abc")))
    assert plain[0] == with_fn[0] == 3
    assert with_fn[1].count("GATHER_32") >= 2 and "GATHER_32" not in plain[1]    # the per-chunk plan gathers from both tables ...
    assert "GATHER_32" not in with_fn[2]                                            # ... the merging plan only sums


def test_dict_eval_needs_a_device(ctx):
    d = ss.StringDictionary([b"a", b"bb"])
    with pytest.raises(ss.SupersonicException) as e:
        d.eval(ss.StringDictionary.LENGTH, context=ctx)
    assert e.value.return_code == ss.ERROR_NO_DEVICE


def test_a_run_without_a_device_fails_loudly(ctx):
    import numpy as np
    view = ss.View(ss.TupleSchema([ss.Attribute("s", ss.STRING)]), [np.array([b"abc"], dtype=object)])
    cur = ss.Compute(ss.Length(NA("s")), ss.ScanView(view)).CreateCursor(ctx)
    r = cur.Next(1024)
    assert r.is_failure() and r.exception().return_code == ss.ERROR_NO_DEVICE


def test_cpp_mirror_compiles():
    src = """
#include "supersonic/supersonic.h"
#include "supersonic/expression/core/string_expressions.h"
using namespace supersonic;
int main() {
  const Expression* e = StringContainsCI(NamedAttribute("s"), ConstString("x"));
  const Expression* f = StringContains(NamedAttribute("s"), ConstString("x"));
  const Expression* g = StringOffset(ToLower(NamedAttribute("s")), ToLower(ConstString("x")));
  const Expression* h = Length(NamedAttribute("s"));
  delete e; delete f; delete g; delete h;
  return 0;
}
"""
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "string_mirror.cc")
        open(path, "w").write(src)
        subprocess.check_call(["g++", "-std=c++14", "-fsyntax-only", "-D__HIP_PLATFORM_AMD__", "-I" + os.path.join(ROOT, "include"), path])
