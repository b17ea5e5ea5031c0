"""PARSE_STRING (ParseStringQuiet 437 / ParseStringNulling 438) without a device: the model the GPU tests compare against
(tests/parse_string_model.py) reproduces every row of the reference's own tests (tests/golden/parse_string_cases.json) and sorts
the fast-path inputs the way the device has to; at bind time -- a bind-only context -- names, types, nullability, every refusal
with its code, the slots the tables take, the C++ mirror, and the plan-free call's answer without a device."""
import math
import os
import subprocess
import tempfile

import numpy as np
import pytest

import supersonic_amd as ss
import parse_string_model as model
import parse_string_pool as pool

NA = ss.NamedAttribute
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = pool.GOLDEN
TYPES = {"INT32": ss.INT32, "UINT32": ss.UINT32, "INT64": ss.INT64, "UINT64": ss.UINT64, "FLOAT": ss.FLOAT, "DOUBLE": ss.DOUBLE, "BOOL": ss.BOOL,
         "STRING": ss.STRING, "DATE": ss.DATE, "DATETIME": ss.DATETIME, "BINARY": ss.BINARY}
TARGETS = [ss.INT32, ss.UINT32, ss.INT64, ss.UINT64, ss.FLOAT, ss.DOUBLE, ss.BOOL]
FUNCTIONS = {"ParseStringQuiet": ss.ParseStringQuiet, "ParseStringNulling": ss.ParseStringNulling}


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


# ---- the model ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("row", [r for r in GOLDEN["evaluation"] if r["input"] is not None], ids=lambda r: "line%d" % r["line"])
def test_model_reproduces_the_reference_rows(row):
    t = TYPES[row["type"]]
    value, failed = model.parse(t, row["input"].encode())
    if row["expected"] is None:
        assert row["function"] == "ParseStringNulling" and failed          # the Quiet tests hold no failing row: "the behaviour is undefined"
    elif row["expected"] == "NaN":
        assert not failed and math.isnan(value)
    else:
        want = np.float32(row["expected"]) if t == ss.FLOAT else row["expected"]
        assert not failed and value == want and type(value) is type(row["expected"])


def test_golden_file_is_the_whole_of_the_reference_tests():
    rows = GOLDEN["evaluation"]
    assert len(rows) == 47 and sum(1 for r in rows if r["input"] is None) == 2
    assert sorted({r["type"] for r in rows}) == ["BOOL", "DOUBLE", "FLOAT", "INT32", "INT64", "UINT32", "UINT64"]
    assert [b["line"] for b in GOLDEN["binding"]] == [71, 73, 74, 77, 79, 80]


def test_model_states_the_rules():
    i32, u32, i64, u64 = ss.INT32, ss.UINT32, ss.INT64, ss.UINT64
    assert model.parse(u64, b"125 OOPS") == (125, True) and model.parse(u64, b"OOPS 125") == (0, True) and model.parse(i32, b"12 3") == (12, True)
    assert model.parse(i32, b"-2147483648") == (-2 ** 31, False) and model.parse(i32, b"-2147483649") == (-2 ** 31, True)
    assert model.parse(i32, b"2147483648") == (2 ** 31 - 1, True) and model.parse(u64, b"18446744073709551615") == (2 ** 64 - 1, False)
    assert model.parse(u64, b"18446744073709551616") == (2 ** 64 - 1, True) and model.parse(i64, b"-9223372036854775809") == (-2 ** 63, True)
    assert model.parse(u32, b"-0") == (0, True) and model.parse(i32, b"-0") == (0, False) and model.parse(i32, b"+") == (0, True)
    assert model.parse(i32, b"- 5") == (0, True) and model.parse(i32, b"010") == (10, False) and model.parse(i32, b"0x10") == (0, True)
    assert model.parse(i32, b"\v\f 7\r\n") == (7, False) and model.parse(i32, b"\xa07") == (0, True)
    assert model.parse(i32, b"12\x003") == (12, False) and model.parse(i32, b"\x0012") == (0, True) and model.parse(i32, b"12\x00") == (12, False)
    assert model.parse(ss.BOOL, b" \tyEs\r") == (True, False) and model.parse(ss.BOOL, b"\ntrue") == (False, True) and model.parse(ss.BOOL, b"1") == (False, True)
    assert model.parse(ss.DOUBLE, b"1.OOPS") == (1.0, True) and model.parse(ss.DOUBLE, b"--12") == (0.0, True) and model.parse(ss.DOUBLE, b"") == (0.0, True)
    assert model.parse(ss.DOUBLE, b" 0x1p3 ") == (8.0, False) and model.parse(ss.DOUBLE, b"1e400") == (math.inf, False) and model.parse(ss.DOUBLE, b" ") == (0.0, True)
    assert model.bits(ss.DOUBLE, model.parse(ss.DOUBLE, b"-0")[0]) == 1 << 63 and model.parse(ss.FLOAT, b"0.1")[0] == float(np.float32(0.1))


@pytest.mark.parametrize("t", [ss.FLOAT, ss.DOUBLE], ids=["FLOAT", "DOUBLE"])
def test_model_classifies_the_floating_inputs(t):
    # the GPU test demands host_resolved == 0 for these and == the model's count for those: the inputs are what they claim to be
    fast = pool.fast_decimals(t)
    assert len(fast) == 2000 and all(model.fast_path(t, v) is True for v in fast)
    assert all(not model.parse(t, v)[1] for v in fast)
    forms = [any(b"." in v for v in fast), any(b"." not in v for v in fast), any(b"e" in v.lower() for v in fast), any(b"e" not in v.lower() for v in fast),
             any(v.strip()[:1] == b"-" for v in fast), any(v.strip()[:1] == b"+" for v in fast), any(v != v.strip() for v in fast), any(v == v.strip() for v in fast)]
    assert all(forms)
    hard = pool.hard_floats()
    always = [b"1234567890123456789", b"9007199254740993", b"1e23", b"1e-23", b"1e400", b"1e-400", b"inf", b"-Infinity", b"NaN", b"0x1p3", b"1.OOPS", b"1.1.", b"--12", b".", b"e5"]
    assert all(v in hard and model.fast_path(t, v) is False for v in always)
    assert model.fast_path(t, b"") is None and model.fast_path(t, b"\x001") is None
    assert model.fast_path(ss.DOUBLE, b"9007199254740992") is True and model.fast_path(ss.FLOAT, b"16777216") is True and model.fast_path(ss.FLOAT, b"16777217") is False
    assert model.fast_path(ss.DOUBLE, b"1e22") is True and model.fast_path(ss.FLOAT, b"1e10") is True and model.fast_path(ss.FLOAT, b"1e11") is False


def test_pool_covers_what_it_promises():
    values = pool.general_pool()
    assert 3500 <= len(values) <= 4500 and len(set(values)) == len(values)
    lengths = {len(v) for v in values}
    assert set(pool.THRESHOLD_LENGTHS) <= lengths
    for probe in (b"+", b"-", b"", b" ", b"- 5", b"5 -", b"0x10", b"010", b"12\x003", b"\x0012", b"12\x00", b"2147483648", b"\v-2147483649\v", b"18446744073709551616\f"):
        assert probe in values, probe
    assert any(v and max(v) >= 0x80 for v in values)


# ---- binding ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fact", GOLDEN["binding"], ids=lambda f: "line%d" % f["line"])
def test_reference_binding_facts(ctx, fact):
    expr = FUNCTIONS[fact["function"]](TYPES[fact["type"]], NA("$0"))
    if fact["type"] == "DATE":         # the reference binds it; here it is the refusal the header states
        code, msg = refusal(ctx, expr, ("$0", ss.STRING, ss.NOT_NULLABLE))
        assert code == ss.ERROR_NOT_IMPLEMENTED and "DATE" in msg
        return
    _plan, (name, dtype, _nullable) = bound(ctx, expr, ("$0", ss.STRING, ss.NOT_NULLABLE))
    assert (name, dtype) == (fact["description"], TYPES[fact["type"]])


def test_names_types_and_nullability(ctx):
    s, t = ("s", ss.STRING, ss.NULLABLE), ("t", ss.STRING, ss.NOT_NULLABLE)
    for to in TARGETS:
        assert bound(ctx, ss.ParseStringQuiet(to, NA("s")), s)[1] == ("PARSE_STRING(s)", to, True)
        assert bound(ctx, ss.ParseStringQuiet(to, NA("t")), t)[1] == ("PARSE_STRING(t)", to, False)        # Quiet: nullable iff the argument is
        assert bound(ctx, ss.ParseStringNulling(to, NA("s")), s)[1] == ("PARSE_STRING(s)", to, True)
        assert bound(ctx, ss.ParseStringNulling(to, NA("t")), t)[1] == ("PARSE_STRING(t)", to, True)       # Nulling: always
    # a constant is a code like any other value; a NULL constant needs no table
    plan, fact = bound(ctx, ss.ParseStringQuiet(ss.INT64, ss.ConstString("12")), t)
    assert fact == ("PARSE_STRING(CONST_STRING)", ss.INT64, False) and plan.describe().count("dictionary table: PARSE_STRING") == 1
    plan, fact = bound(ctx, ss.ParseStringNulling(ss.INT64, ss.Null(ss.STRING)), t)
    assert fact == ("PARSE_STRING(NULL)", ss.INT64, True) and "dictionary table" not in plan.describe()
    # over another STRING expression
    plan, fact = bound(ctx, ss.ParseStringNulling(ss.INT32, ss.Trim(NA("t"))), t)
    assert fact == ("PARSE_STRING(TRIM(t))", ss.INT32, True)
    assert bound(ctx, ss.ParseStringQuiet(ss.DOUBLE, ss.IfNull(NA("s"), ss.ConstString("0"))), s)[1] == ("PARSE_STRING(IFNULL(s, CONST_STRING))", ss.DOUBLE, False)
    # the result is a number: arithmetic and comparisons bind on top
    assert bound(ctx, ss.Greater(ss.ParseStringNulling(ss.INT32, NA("t")), ss.ConstInt32(5)), t)[1][1:] == (ss.BOOL, True)


def test_string_target_returns_the_child(ctx):
    s, t = ("s", ss.STRING, ss.NULLABLE), ("t", ss.STRING, ss.NOT_NULLABLE)
    for make in (ss.ParseStringQuiet, ss.ParseStringNulling):
        plan, fact = bound(ctx, make(ss.STRING, NA("s")), s)
        assert fact == ("s", ss.STRING, True) and "GATHER" not in plan.describe()
        assert bound(ctx, make(ss.STRING, NA("t")), t)[1] == ("t", ss.STRING, False)


def test_refusals(ctx):
    t, x, b, f = ("t", ss.STRING, ss.NOT_NULLABLE), ("x", ss.INT32, ss.NOT_NULLABLE), ("b", ss.BINARY, ss.NOT_NULLABLE), ("f", ss.DOUBLE, ss.NOT_NULLABLE)
    for make in (ss.ParseStringQuiet, ss.ParseStringNulling):
        for to, name in ((ss.DATE, "DATE"), (ss.DATETIME, "DATETIME"), (ss.BINARY, "BINARY")):
            code, msg = refusal(ctx, make(to, NA("t")), t)
            assert code == ss.ERROR_NOT_IMPLEMENTED and name in msg and "PARSE_STRING" in msg
        for arg in ("x", "b", "f"):
            code, msg = refusal(ctx, make(ss.INT32, NA(arg)), t, x, b, f)
            assert code == ss.ERROR_ATTRIBUTE_TYPE_MISMATCH and "PARSE_STRING" in msg
        assert refusal(ctx, make(ss.STRING, NA("x")), t, x)[0] == ss.ERROR_ATTRIBUTE_TYPE_MISMATCH       # the STRING target takes a STRING too
        assert refusal(ctx, make(ss.INT32, ss.ConstInt32(1)), t)[0] == ss.ERROR_ATTRIBUTE_TYPE_MISMATCH
    # wrong arity
    assert refusal(ctx, ss.Expression(ss._lib.EXPR_OP, op=437, dtype=ss.INT32, args=[NA("t"), NA("t")]), t)[0] == ss.ERROR_ATTRIBUTE_COUNT_MISMATCH


def test_one_slot_per_target_type(ctx):
    s = ("s", ss.STRING, ss.NULLABLE)
    e = (ss.CompoundExpression().AddAs("q", ss.ParseStringQuiet(ss.INT32, NA("s"))).AddAs("n", ss.ParseStringNulling(ss.INT32, NA("s")))
         .AddAs("n2", ss.Plus(ss.ParseStringNulling(ss.INT32, ss.IfNull(NA("s"), ss.ConstString("1"))), ss.ConstInt32(1))))
    text = ss.Plan(ss.Compute(e, scan(s)), ctx).describe()
    assert text.count("dictionary table") == 1 and "dictionary table: PARSE_STRING to INT32" in text       # 437 and 438 of one type: one slot
    assert text.count("GATHER_NULL") == 2 and text.count("GATHER_32") == 3                               # Quiet reads no failure byte
    e = ss.CompoundExpression().AddAs("a", ss.ParseStringNulling(ss.INT32, NA("s"))).AddAs("b", ss.ParseStringNulling(ss.UINT32, NA("s")))
    text = ss.Plan(ss.Compute(e, scan(s)), ctx).describe()
    assert text.count("dictionary table") == 2 and "PARSE_STRING to UINT32" in text                       # two types, equal width: two slots
    e = ss.CompoundExpression()
    for i, to in enumerate(TARGETS):
        e.AddAs("o%d" % i, ss.ParseStringQuiet(to, NA("s")))
    text = ss.Plan(ss.Compute(e, scan(s)), ctx).describe()
    assert text.count("dictionary table: PARSE_STRING") == 7
    assert text.count("GATHER_8 ") == 1 and text.count("GATHER_32") == 3 and text.count("GATHER_64") == 3 and "GATHER_NULL" not in text


def test_slot_limit_is_a_bind_error(ctx):
    s = ("s", ss.STRING, ss.NOT_NULLABLE)

    def many(offsets):
        e = ss.CompoundExpression()
        for i, to in enumerate(TARGETS):
            e.AddAs("p%d" % i, ss.ParseStringNulling(to, NA("s")))
        for i in range(offsets):
            e.AddAs("o%d" % i, ss.StringOffset(NA("s"), ss.ConstString("needle %d" % i)))
        return e
    plan = ss.Plan(ss.Compute(many(17), scan(s)), ctx)              # 7 parse slots + 17 others: the pipeline's 24
    assert plan.describe().count("dictionary table") == 24
    code, msg = refusal(ctx, many(18), s)                            # the 25th
    assert code == ss.ERROR_NOT_IMPLEMENTED and "slots" in msg


def test_chunked_forms_keep_the_tables(ctx):
    s, k = ("s", ss.STRING, ss.NULLABLE), ("k", ss.INT32, ss.NOT_NULLABLE)
    form = ss.Plan(ss.Filter(ss.Greater(ss.ParseStringNulling(ss.INT32, NA("s")), ss.ConstInt32(3)), ss.ProjectAllAttributes(), scan(s, k)), ctx).chunked_form()
    assert form[0] == 2
    e = ss.CompoundExpression().AddAs("g", ss.ParseStringNulling(ss.INT32, NA("s"))).AddAs("v", ss.ParseStringQuiet(ss.INT64, NA("s")))
    spec = ss.AggregationSpecification().AddAggregation(ss.SUM, "v", "sum")
    form = ss.Plan(ss.GroupAggregate(ss.ProjectNamedAttributes(["g"]), spec, None, ss.Compute(e, scan(s, k))), ctx).chunked_form()
    assert form[0] == 3 and "GATHER_NULL" in form[1] and "GATHER_64" in form[1] and "GATHER" not in form[2]     # the per-chunk plan parses, the merging plan sums


def test_cpp_mirror_compiles_and_binds():
    src = """
#include "supersonic/supersonic.h"
#include "supersonic/expression/core/elementary_expressions.h"
#include <stdio.h>
using namespace supersonic;
int main() {
  TupleSchema schema;
  schema.add_attribute(Attribute("s", STRING, NULLABLE));
  const Expression* q = ParseStringQuiet(INT32, NamedAttribute("s"));
  const Expression* n = ParseStringNulling(DOUBLE, NamedAttribute("s"));
  const Expression* same = ParseStringNulling(STRING, NamedAttribute("s"));
  const Expression* date = ParseStringQuiet(DATE, NamedAttribute("s"));
  const Expression* list[3] = {q, n, same};
  for (int i = 0; i < 3; ++i) {
    FailureOrOwned<BoundExpressionTree> b = list[i]->Bind(schema, HeapBufferAllocator::Get(), 16);
    if (b.is_failure()) { printf("bind failed: %s\\n", b.exception().message().c_str()); return 1; }
    const Attribute& a = b->result_schema().attribute(0);
    printf("%s %d %d\\n", a.name().c_str(), static_cast<int>(a.type()), a.is_nullable() ? 1 : 0);
  }
  FailureOrOwned<BoundExpressionTree> d = date->Bind(schema, HeapBufferAllocator::Get(), 16);
  printf("date %d\\n", d.is_failure() ? static_cast<int>(d.exception().return_code()) : 0);
  delete q; delete n; delete same; delete date;
  return 0;
}
"""
    with tempfile.TemporaryDirectory() as tmp:
        path, exe = os.path.join(tmp, "parse_mirror.cc"), os.path.join(tmp, "parse_mirror")
        open(path, "w").write(src)
        lib_dir = os.path.join(ROOT, "supersonic_amd", "lib")
        subprocess.check_call(["g++", "-std=c++14", "-D__HIP_PLATFORM_AMD__", "-I" + os.path.join(ROOT, "include"), path, "-o", exe,
                               "-L" + lib_dir, "-lssgpu", "-Wl,-rpath," + lib_dir])
        out = subprocess.check_output([exe]).decode().splitlines()
    assert out == ["PARSE_STRING(s) %d 1" % ss.INT32, "PARSE_STRING(s) %d 1" % ss.DOUBLE, "s %d 1" % ss.STRING, "date %d" % ss.ERROR_NOT_IMPLEMENTED]


def test_dict_parse_needs_a_device(ctx):
    d = ss.StringDictionary([b"1", b"22"])
    for to in TARGETS:
        with pytest.raises(ss.SupersonicException) as e:
            d.parse(to, context=ctx)
        assert e.value.return_code == ss.ERROR_NO_DEVICE
    with pytest.raises(ss.SupersonicException) as e:
        d.parse(ss.DATE, context=ctx)
    assert e.value.return_code == ss.ERROR_INVALID_ARGUMENT_VALUE


def test_a_run_without_a_device_fails_loudly(ctx):
    view = ss.View(ss.TupleSchema([ss.Attribute("s", ss.STRING)]), [np.array([b"12"], dtype=object)])
    cur = ss.Compute(ss.ParseStringNulling(ss.INT32, NA("s")), ss.ScanView(view)).CreateCursor(ctx)
    r = cur.Next(1024)
    assert r.is_failure() and r.exception().return_code == ss.ERROR_NO_DEVICE
