"""STRING_REPLACE at bind time (bind-only context, no device): the Python restatement pinned against the reference's own rows
(tests/golden/string_replace_cases.json) and against a literal transcription of its loop, the bound name, type and nullability, every
refusal with its code, the plan's step list with the constants' codes, what needs a device, and the C++ mirror's declaration."""
import ctypes as C
import json
import os
import subprocess
import tempfile

import numpy as np
import pytest

import supersonic_amd as ss
from supersonic_amd import _lib as L
from string_replace_pool import PAIRS, STRING_REPLACE, pool, reference_loop, replace

NA = ss.NamedAttribute
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = json.load(open(os.path.join(ROOT, "tests", "golden", "string_replace_cases.json")))
TYPES = {"STRING": ss.STRING, "INT32": ss.INT32}
TRIM = 412


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


# ---- the restatement ---------------------------------------------------------------------------------------------------------
def test_restatement_gives_the_reference_rows():
    rows = GOLDEN["evaluation"]["StringReplace"]["rows"]
    assert len(rows) == 4
    for h, n, s, want in rows:
        assert replace(h.encode(), n.encode(), s.encode()) == want.encode(), (h, n, s)
        assert reference_loop(h.encode(), n.encode(), s.encode()) == want.encode(), (h, n, s)
    assert replace(b"aaaaa", b"aa", b"b") == b"bba" and replace(b"a", b"a", b"aa") == b"aa" and replace(b"xyz", b"", b"q") == b"xyz"


def test_restatement_is_the_reference_loop_on_the_whole_pool():
    values = pool()
    pairs = 0
    for needle, sub in PAIRS:
        for v in values + [needle, sub]:
            assert replace(v, needle, sub) == reference_loop(v, needle, sub), (v[:40], needle[:20], sub[:20])
            pairs += 1
    assert pairs == len(PAIRS) * (len(values) + 2)


# ---- binding -----------------------------------------------------------------------------------------------------------------
def test_reference_binding_fact(ctx):
    fact, = GOLDEN["binding"]
    assert ss.StringDictionary.STRING_REPLACE == STRING_REPLACE
    for z in (ss.NOT_NULLABLE, ss.NULLABLE):
        attrs = [("$%d" % i, TYPES[t], z) for i, t in enumerate(fact["arg_types"])]
        # the reference binds three attributes; the needle and the substitute must be constants here, so they read CONST_STRING
        _plan, got = bound(ctx, ss.StringReplace(NA("$0"), ss.ConstString("x"), ss.ConstString("y")), *attrs)
        want = fact["description"].replace("$1", "CONST_STRING").replace("$2", "CONST_STRING")
        assert got == (want, TYPES[fact["type"]], fact["nullable"] or z == ss.NULLABLE), "STRING_REPLACE (480) binding"


def test_constants_in_the_name_and_nesting(ctx):
    s, t = ("s", ss.STRING, ss.NULLABLE), ("t", ss.STRING, ss.NOT_NULLABLE)
    x, y = ss.ConstString("x"), ss.ConstString("yy")
    assert bound(ctx, ss.StringReplace(ss.ConstString("c"), x, y), t)[1] == ("STRING_REPLACE(CONST_STRING, CONST_STRING, CONST_STRING)", ss.STRING, False)
    assert bound(ctx, ss.StringReplace(ss.Trim(NA("s")), x, y), s)[1] == ("STRING_REPLACE(TRIM(s), CONST_STRING, CONST_STRING)", ss.STRING, True)
    assert bound(ctx, ss.Length(ss.StringReplace(NA("t"), x, y)), t)[1] == ("LENGTH(STRING_REPLACE(t, CONST_STRING, CONST_STRING))", ss.UINT32, False)
    assert bound(ctx, ss.StringReplace(ss.IfNull(NA("s"), NA("t")), x, y), s, t)[1] == ("STRING_REPLACE(IFNULL(s, t), CONST_STRING, CONST_STRING)", ss.STRING, False)
    # an empty needle folds nothing: still one step, and a table
    plan, _fact = bound(ctx, ss.StringReplace(NA("t"), ss.ConstString(""), y), t)
    assert len(steps_of(plan)) == 1 and "dictionary table: STRING_REPLACE" in plan.describe()


def test_non_string_arguments_are_a_type_mismatch(ctx):
    fact, = GOLDEN["binding_failures"]
    attrs = [("$%d" % i, TYPES[t], ss.NOT_NULLABLE) for i, t in enumerate(fact["arg_types"])]
    code, msg = refusal(ctx, ss.StringReplace(NA("$0"), NA("$1"), NA("$2")), *attrs)
    assert code == ss.ERROR_ATTRIBUTE_TYPE_MISMATCH and "STRING_REPLACE" in msg, "STRING_REPLACE (480): (INT32, INT32, INT32)"
    t, k = ("t", ss.STRING, ss.NOT_NULLABLE), ("k", ss.INT32, ss.NOT_NULLABLE)
    x = ss.ConstString("x")
    for expr in (ss.StringReplace(NA("k"), x, x), ss.StringReplace(NA("t"), ss.ConstInt32(1), x), ss.StringReplace(NA("t"), x, ss.ConstInt64(1)),
                 ss.StringReplace(NA("t"), x, NA("k")), ss.StringReplace(NA("t"), ss.Null(ss.INT32), x), ss.StringReplace(ss.Length(NA("t")), x, x)):
        code, msg = refusal(ctx, expr, t, k)
        assert code == ss.ERROR_ATTRIBUTE_TYPE_MISMATCH and "STRING_REPLACE" in msg


def test_a_needle_or_substitute_that_varies_per_row_is_not_implemented(ctx):
    t, u = ("t", ss.STRING, ss.NOT_NULLABLE), ("u", ss.STRING, ss.NOT_NULLABLE)
    x = ss.ConstString("x")
    for expr, word in ((ss.StringReplace(NA("t"), NA("u"), x), "needle"), (ss.StringReplace(NA("t"), x, NA("u")), "substitute"),
                       (ss.StringReplace(NA("t"), ss.Trim(NA("u")), x), "needle"), (ss.StringReplace(NA("t"), x, ss.IfNull(NA("u"), x)), "substitute")):
        code, msg = refusal(ctx, expr, t, u)
        assert code == ss.ERROR_NOT_IMPLEMENTED and "STRING_REPLACE" in msg and word in msg and "varies per row" in msg, "STRING_REPLACE (480): per-row " + word


def test_a_null_needle_or_substitute_is_all_null_and_no_step(ctx):
    t = ("t", ss.STRING, ss.NOT_NULLABLE)
    x = ss.ConstString("x")
    plan, fact = bound(ctx, ss.StringReplace(NA("t"), ss.Null(ss.STRING), x), t)
    assert fact == ("STRING_REPLACE(t, NULL, CONST_STRING)", ss.STRING, True) and steps_of(plan) == [] and "dictionary table" not in plan.describe()
    plan, fact = bound(ctx, ss.StringReplace(NA("t"), x, ss.Null(ss.STRING)), t)
    assert fact == ("STRING_REPLACE(t, CONST_STRING, NULL)", ss.STRING, True) and steps_of(plan) == [] and "dictionary table" not in plan.describe()
    # ... and so is everything on top of it, while a producer below it still is a step
    plan, fact = bound(ctx, ss.Trim(ss.StringReplace(ss.Rtrim(NA("t")), x, ss.Null(ss.STRING))), t)
    assert fact[1:] == (ss.STRING, True) and [st[0] for st in steps_of(plan)] == [408, TRIM]


def test_wrong_arity(ctx):
    t = ("t", ss.STRING, ss.NOT_NULLABLE)
    x = ss.ConstString("x")
    for args in ((NA("t"),), (NA("t"), x), (NA("t"), x, x, x)):
        code, _msg = refusal(ctx, ss.api._op(STRING_REPLACE, *args), t)
        assert code == ss.ERROR_ATTRIBUTE_COUNT_MISMATCH, "STRING_REPLACE (480) with %d arguments" % len(args)


# ---- the step list -----------------------------------------------------------------------------------------------------------
def test_step_list_carries_the_constants_codes(ctx):
    view = ss.View(ss.TupleSchema([ss.Attribute("t", ss.STRING)]), [np.array([b" banana ", b"x"], dtype=object)])
    e = ss.Trim(ss.StringReplace(ss.StringReplace(NA("t"), ss.ConstString("a"), ss.ConstString("b")), ss.ConstString("b"), ss.ConstString("c")))
    plan = ss.Plan(ss.Compute(e, ss.ScanView(view)), ctx)
    code = plan.strings.code_of
    assert steps_of(plan) == [(STRING_REPLACE, 0, code(b"a"), code(b"b")), (STRING_REPLACE, 0, code(b"b"), code(b"c")), (TRIM, 0, 0, 0)]
    assert len({code(b"a"), code(b"b"), code(b"c")}) == 3
    lines = [ln for ln in plan.describe().splitlines() if ln.startswith("dictionary table")]
    assert lines == ["dictionary table: STRING_REPLACE needle code %d substitute code %d (codes of the closed dictionary)" % (code(b"a"), code(b"b")),
                     "dictionary table: STRING_REPLACE needle code %d substitute code %d (codes of the closed dictionary)" % (code(b"b"), code(b"c")),
                     "dictionary table: TRIM (codes of the closed dictionary)"]
    # equal constants share one table slot, different ones do not
    e = ss.CompoundExpression()
    for i in range(30):
        e.AddAs("o%d" % i, ss.StringReplace(ss.IfNull(NA("t"), ss.ConstString("c%d" % i)), ss.ConstString("a"), ss.ConstString("s%d" % (i % 3))))
    assert ss.Plan(ss.Compute(e, ss.ScanView(view)), ctx).describe().count("dictionary table") == 3


def test_closing_needs_a_device(ctx):
    """ssgpu_dict_close answers ERROR_NO_DEVICE on a bind-only context BEFORE it looks at the steps: a 480-step whose codes lie outside
    the base gets ERROR_NO_DEVICE here too, and ERROR_INVALID_ARGUMENT_VALUE only where there is a device (test_string_replace_gpu.py)."""
    d = ss.StringDictionary([b"a", b"b", b"banana"])
    for steps in ([(STRING_REPLACE, b"a", b"b")], [(STRING_REPLACE, 0, 1)], [(STRING_REPLACE, 0, 99)], [(STRING_REPLACE, -1, 0)]):
        with pytest.raises(ss.SupersonicException) as e:
            d.close(steps, ctx)
        assert e.value.return_code == ss.ERROR_NO_DEVICE
    # the Python mirror resolves bytes with code_of on the dictionary itself: an absent value raises before anything is called
    with pytest.raises(ss.SupersonicException):
        d.close([(STRING_REPLACE, b"a", b"absent")], ctx)
    with pytest.raises(ss.SupersonicException):
        d.close([(STRING_REPLACE, b"a")], ctx)
    # a plan with a replace node over host strings still binds without a device; running it fails loudly
    view = ss.View(ss.TupleSchema([ss.Attribute("s", ss.STRING)]), [np.array([b"banana", b"x"], dtype=object)])
    op = ss.Compute(ss.StringReplace(NA("s"), ss.ConstString("an"), ss.ConstString("AN")), ss.ScanView(view))
    plan = ss.Plan(op, ctx)
    assert plan.result_schema.attribute(0).type() == ss.STRING and sorted(plan.strings.values) == [b"AN", b"an", b"banana", b"x"]
    r = op.CreateCursor(ctx).Next(1024)
    assert r.is_failure() and r.exception().return_code == ss.ERROR_NO_DEVICE


def test_abi_version_and_record_are_unchanged():
    lib = L.load()
    assert lib.ssgpu_abi_version() == 10 and C.sizeof(L.StringStep) == 24


def test_cpp_mirror_compiles_and_binds():
    src = """
#include "supersonic/supersonic.h"
#include "supersonic/expression/core/string_expressions.h"
#include <cstdio>
using namespace supersonic;
int main() {
  const Expression* r = StringReplace(NamedAttribute("s"), ConstString("x"), ConstString("yy"));
  TupleSchema schema;
  schema.add_attribute(Attribute("s", STRING, NULLABLE));
  FailureOrOwned<BoundExpressionTree> bound = r->Bind(schema, HeapBufferAllocator::Get(), 16);
  if (bound.is_failure()) { std::printf("bind failed: %s\\n", bound.exception().message().c_str()); return 1; }
  const Attribute& a = bound->result_schema().attribute(0);
  std::printf("%s %d %d\\n", a.name().c_str(), static_cast<int>(a.type() == STRING), static_cast<int>(a.is_nullable()));
  delete r;
  return 0;
}
"""
    with tempfile.TemporaryDirectory() as tmp:
        path, exe = os.path.join(tmp, "string_replace_mirror.cc"), os.path.join(tmp, "string_replace_mirror")
        open(path, "w").write(src)
        libdir = os.path.join(ROOT, "supersonic_amd", "lib")
        subprocess.check_call(["g++", "-std=c++14", "-D__HIP_PLATFORM_AMD__", "-I" + os.path.join(ROOT, "include"), path, "-o", exe,
                               "-L" + libdir, "-lssgpu", "-Wl,-rpath," + libdir])
        out = subprocess.check_output([exe]).decode()
        assert out.strip() == "STRING_REPLACE(s, CONST_STRING, CONST_STRING) 1 1", out
