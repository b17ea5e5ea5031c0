"""tests/expression_reference.py checked without a GPU: against hand-computed literals rule by rule (so that it does not merely agree
with the oracle), its pools against what they claim, and every case tests/test_values_expression_edges_gpu.py runs against the oracle (x86 C)
under the NaN rule.  Nothing is masked: a case either agrees or fails.  Where the two disagreed while this file was written, the
reference's source settled it, and it was the Python side that was wrong both times: AndNot is three-valued like And / Or
(elementary_bound_expressions.cc:388-404), and SUM folds in the input's type unless the specification names another
(aggregator.cc:63-78, aggregation_operators.h:173-186) -- a FLOAT sum is folded in FLOAT, an INT32 sum wraps in INT32."""
import math
from fractions import Fraction

import numpy as np
import pytest

import expression_reference as er
import supersonic_amd as ss
from oracle import oracle

I32, I64, U32, U64, F32, F64, B8 = er.INT32, er.INT64, er.UINT32, er.UINT64, er.FLOAT, er.DOUBLE, er.BOOL


def bits(v):
    return int(np.array([v]).view("u%d" % np.array([v]).dtype.itemsize)[0])


# ---- the rules against literals ---------------------------------------------------------------------------------------------------------------
def test_integer_wrap_rules():
    assert er.arith("+", I32, 2 ** 31 - 1, 1) == -2 ** 31
    assert er.arith("-", I32, -2 ** 31, 1) == 2 ** 31 - 1
    assert er.arith("*", I32, 46341, 46341) == -2147479015           # 2147488281 - 2^32
    assert er.arith("*", I32, 65536, 65536) == 0
    assert er.arith("+", U32, 2 ** 32 - 1, 2) == 1
    assert er.arith("-", U32, 0, 1) == 2 ** 32 - 1
    assert er.arith("+", I64, 2 ** 63 - 1, 1) == -2 ** 63
    assert er.arith("*", I64, 3037000500, 3037000500) == -9223372036709301616    # 9223372037000250000 - 2^64
    assert er.arith("*", I64, 2 ** 32, 2 ** 32) == 0
    assert er.arith("*", U64, 2 ** 63 + 1, 2) == 2
    assert er.arith("-", U64, 0, 1) == 2 ** 64 - 1
    assert er.wrap(I32, 2 ** 31) == -2 ** 31 and er.wrap(U32, -1) == 2 ** 32 - 1 and er.wrap(I64, 2 ** 64 - 1) == -1
    assert er.bitwise(I64, "~&", -1, 5) == 0 and er.bitwise(I32, "~&", 0, -2 ** 31) == -2 ** 31 and er.bitwise(U64, "^", 2 ** 64 - 1, 1) == 2 ** 64 - 2


def test_division_and_modulus_rules():
    # x / -1 wraps, x % -1 = 0 (vm_body.inc CDIV_I32 / MOD_I32 ..., bind.cpp fold_binary)
    assert er.cpp_divide(I32, -2 ** 31, -1) == -2 ** 31 and er.cpp_divide(I64, -2 ** 63, -1) == -2 ** 63
    assert er.modulus(I32, -2 ** 31, -1) == 0 and er.modulus(I64, -2 ** 63, -1) == 0
    assert er.cpp_divide(I32, 7, -1) == -7 and er.modulus(I64, 7, -1) == 0
    # truncation toward zero, the remainder has the dividend's sign
    assert er.cpp_divide(I32, -7, 2) == -3 and er.modulus(I32, -7, 2) == -1
    assert er.cpp_divide(I64, 7, -2) == -3 and er.modulus(I64, 7, -2) == 1
    assert er.cpp_divide(I64, -2 ** 63, 2) == -2 ** 62 and er.modulus(I64, -2 ** 63 + 1, 2) == -1
    assert er.cpp_divide(I64, 2 ** 63 - 1, -2 ** 63) == 0 and er.modulus(I64, 2 ** 63 - 1, -2 ** 63) == 2 ** 63 - 1
    assert er.cpp_divide(I64, -2 ** 63, -2 ** 63) == 1 and er.cpp_divide(I64, -2 ** 63, 2 ** 63 - 1) == -1 and er.modulus(I64, -2 ** 63, 2 ** 63 - 1) == -1
    assert er.cpp_divide(U64, 2 ** 64 - 1, 2 ** 63) == 1 and er.modulus(U64, 2 ** 64 - 1, 2 ** 63) == 2 ** 63 - 1
    assert er.cpp_divide(U32, 2 ** 32 - 1, 2 ** 32 - 1) == 1 and er.modulus(U32, 2 ** 31, 2 ** 32 - 1) == 2 ** 31
    # a zero divisor is NULL
    for t in er.INTS:
        assert er.cpp_divide(t, 5, 0) is None and er.modulus(t, 5, 0) is None
    assert er.divide(np.float64(1.0), np.float64(0.0)) == math.inf and er.divide(np.float64(-1.0), np.float64(0.0)) == -math.inf
    assert math.isnan(er.divide(np.float64(0.0), np.float64(0.0))) and er.divide(np.float64(1.0), np.float64(-0.0)) == -math.inf
    assert bits(er.divide(np.float64(4.9e-324), np.float64(2.0))) == 0                  # half the smallest subnormal: ties to even, +0.0
    assert bits(er.divide(np.float64(2.2250738585072014e-308), np.float64(2.0))) == 0x0008000000000000     # a subnormal result


def test_shift_rules():
    assert er.shift(I32, False, -2 ** 31, 31) == -1 and er.shift(U32, False, 2 ** 31, 31) == 1
    assert er.shift(I64, False, -2 ** 63, 63) == -1 and er.shift(U64, False, 2 ** 63, 63) == 1
    assert er.shift(I64, False, -7, 1) == -4 and er.shift(I32, False, -1, 31) == -1
    assert er.shift(I32, True, 1, 31) == -2 ** 31 and er.shift(I64, True, 3, 63) == -2 ** 63 and er.shift(U64, True, 3, 63) == 2 ** 63
    assert er.shift(I32, True, 2 ** 30, 1) == -2 ** 31 and er.shift(U32, True, 2 ** 31 + 1, 1) == 2


def test_mixed_sign_compares_are_value_correct():
    assert er.compare("<", I64, -1, U64, 2 ** 64 - 1) and not er.compare("==", I64, -1, U64, 2 ** 64 - 1)
    assert er.compare("<", I64, 2 ** 63 - 1, U64, 2 ** 63) and er.compare(">", U64, 2 ** 63, I64, -2 ** 63)
    assert er.compare("!=", I64, -2 ** 63, U64, 2 ** 63) and er.compare("==", I64, 2 ** 63 - 1, U64, 2 ** 63 - 1)
    assert er.compare("<", I32, -1, U32, 2 ** 32 - 1) and er.compare(">=", U32, 2 ** 31, I32, 2 ** 31 - 1)
    # through a float: both sides converted first (bind_compare), so 2^53 + 1 equals 2^53 as a DOUBLE, 2^24 + 1 equals 2^24 as a FLOAT
    assert er.compare("==", I64, 2 ** 53 + 1, F64, np.float64(2.0 ** 53)) and er.compare("==", I64, 2 ** 24 + 1, F32, np.float32(2.0 ** 24))
    assert er.compare("==", I64, 2 ** 63 - 1, F64, np.float64(2.0 ** 63)) and not er.compare("<", I64, 2 ** 63 - 1, F64, np.float64(2.0 ** 63))
    nan = np.float64(math.nan)
    for sym in ("<", "<=", "==", ">", ">="):
        assert not er.compare(sym, F64, nan, F64, nan) and not er.compare(sym, F64, nan, I64, 0)
    assert er.compare("!=", F64, nan, F64, nan) and er.compare("==", F64, np.float64(0.0), F64, np.float64(-0.0))


def test_integer_to_float_rounds_once():
    f = er.int_to_float
    assert bits(f(F32, 2 ** 24 + 1)) == 0x4B800000                    # tie: to even, 2^24
    assert bits(f(F32, 2 ** 24 + 3)) == 0x4B800002                    # tie: to even, 2^24 + 4
    assert bits(f(F64, 2 ** 53 + 1)) == 0x4340000000000000            # tie: 2^53
    assert bits(f(F64, 2 ** 63 + 2 ** 10)) == 0x43E0000000000000      # tie: 2^63
    assert bits(f(F64, 2 ** 63 + 2 ** 10 + 1)) == 0x43E0000000000001
    assert bits(f(F32, 2 ** 64 - 2 ** 39)) == 0x5F800000              # tie: up to 2^64
    assert bits(f(F32, 2 ** 64 - 2 ** 39 - 1)) == 0x5F7FFFFF
    assert bits(f(F64, 2 ** 64 - 1)) == 0x43F0000000000000 and bits(f(F32, -2 ** 63)) == 0xDF000000
    # where a detour through DOUBLE rounds twice: 2^53 + 2^29 + 1 -> (double) 2^53 + 2^29 (a FLOAT tie, to even: 2^53) but the exact value lies above the tie
    v = 2 ** 53 + 2 ** 29 + 1
    assert bits(f(F32, v)) == 0x5A000001 and bits(np.float32(float(v))) == 0x5A000000
    assert bits(f(F32, 2 ** 31 - 1)) == 0x4F000000 and bits(f(F64, -2 ** 31)) == 0xC1E0000000000000
    assert bits(er.convert(F32, F64, np.float64(1.0 + 2.0 ** -24))) == 0x3F800000 and bits(er.convert(F32, F64, np.float64(1.0 + 3 * 2.0 ** -24))) == 0x3F800002
    assert bits(er.convert(F32, F64, np.float64(1.0 + 2.0 ** -24 + 2.0 ** -52))) == 0x3F800001
    assert bits(er.convert(F32, F64, np.float64(3.4028235677973366e38))) == 0x7F800000 and bits(er.convert(F32, F64, np.float64(7.006492321624085e-46))) == 0
    assert bits(er.convert(F32, F64, np.float64(1.401298464324817e-45))) == 1
    assert er.convert(I32, I64, 2 ** 31) == -2 ** 31 and er.convert(U32, I64, -1) == 2 ** 32 - 1 and er.convert(U64, I32, -1) == 2 ** 64 - 1
    assert er.convert(I64, U64, 2 ** 63) == -2 ** 63 and er.convert(I32, U64, 2 ** 64 - 2 ** 39) == 0


def test_exact_math_rules():
    d, f = np.float64, np.float32
    assert bits(er.f_abs(F64, d(-0.0))) == 0x8000000000000000 and er.f_abs(F64, d(-1.5)) == 1.5           # math_evaluators.h:127-132
    assert er.c_round(F64, d(0.5)) == 1.0 and er.c_round(F64, d(-0.5)) == -1.0 and er.c_round(F64, d(2.5)) == 3.0 and er.c_round(F64, d(-2.5)) == -3.0
    assert bits(er.c_round(F64, d(0.49999999999999994))) == 0 and bits(er.c_round(F32, f(0.49999997))) == 0
    assert bits(er.c_round(F64, d(-0.0))) == 0x8000000000000000 and er.c_round(F64, d(2.0 ** 52)) == 2.0 ** 52
    assert er.c_round(F32, f(2.0 ** 23 + 1)) == 2.0 ** 23 + 1 and bits(er.c_round(F64, d(-4.9e-324))) == 0x8000000000000000
    # CVT_I64_X86: NaN and everything outside [-2^63, 2^63) is INT64_MIN
    m = er.INT64_MIN
    assert er.to_int64(d(math.nan)) == m and er.to_int64(d(2.0 ** 63)) == m and er.to_int64(d(math.inf)) == m and er.to_int64(d(-math.inf)) == m
    assert er.to_int64(d(9223372036854774784.0)) == 9223372036854774784 and er.to_int64(d(-2.0 ** 63)) == m and er.to_int64(d(-2.0 ** 63 - 2048)) == m
    assert er.to_int64(d(1e19)) == m and er.to_int64(f(2.0 ** 63)) == m and er.to_int64(d(-1.0)) == -1
    assert er.is_normal(d(2.2250738585072014e-308)) and not er.is_normal(d(2.225073858507201e-308)) and not er.is_normal(d(0.0))
    assert er.is_normal(d(f(1.401298464324817e-45)))                 # a FLOAT subnormal is a normal DOUBLE: IsNormal works on the promoted value


def test_sum_rules():
    inf = math.inf
    assert er.fold_sum(I64, [2 ** 63 - 1, 1]) == -2 ** 63 and er.fold_sum(I32, [2 ** 31 - 1, 2 ** 31 - 1]) == -2 and er.fold_sum(I32, [2 ** 31 - 1, 2 ** 31 - 1], I64) == 2 ** 32 - 2
    assert er.fold_sum(U64, [2 ** 64 - 1, 2]) == 1 and er.fold_sum(U32, [2 ** 32 - 1, 2 ** 32 - 1]) == 2 ** 32 - 2
    assert er.fold_sum(F64, [np.float64(1.0), np.float64(inf), np.float64(-2.0)]) == inf and er.fold_sum(F64, [np.float64(-inf), np.float64(5.0)]) == -inf
    assert math.isnan(er.fold_sum(F64, [np.float64(inf), np.float64(1.0), np.float64(-inf)])) and math.isnan(er.fold_sum(F64, [np.float64(1.0), er.NAN64]))
    assert er.fold_sum(F64, [er.DBL_MAX, er.DBL_MAX]) == inf and er.fold_sum(F64, [-er.DBL_MAX, None, -er.DBL_MAX]) == -inf
    assert er.fold_sum(F64, [None, None]) is None and er.fold_sum(F64, [np.float64(0.1)] * 10) == 1.0


# ---- the pools hit what they claim --------------------------------------------------------------------------------------------------------------
def test_pools_hold_the_named_edges():
    p = er.POOL
    assert {0, 1, -1, 46341, 2 ** 31 - 1, -2 ** 31, -2 ** 31 + 1} <= set(p[I32]) and {2 ** 31, 2 ** 32 - 1, 65537} <= set(p[U32])
    assert {2 ** 24 + 1, 3037000500, 2 ** 53 + 1, 2 ** 63 - 1, -2 ** 63, -2 ** 31 - 1, 2 ** 32} <= set(p[I64])
    assert {2 ** 63, 2 ** 63 + 2 ** 10, 2 ** 64 - 2 ** 39, 2 ** 64 - 1, 2 ** 53 + 1} <= set(p[U64])
    # the named products overflow, their neighbours do not
    assert 46341 ** 2 > 2 ** 31 - 1 >= 46340 ** 2 and 3037000500 ** 2 > 2 ** 63 - 1 >= 3037000499 ** 2
    # the named ties are ties: exactly half way between two neighbours of the target format
    for t, v, nbits in ((F32, 2 ** 24 + 1, 24), (F64, 2 ** 53 + 1, 53), (F64, 2 ** 63 + 2 ** 10, 53), (F32, 2 ** 64 - 2 ** 39, 24)):
        e = v.bit_length() - nbits
        assert v & ((1 << e) - 1) == 1 << (e - 1), v
    tie = Fraction(float(np.float64(1.0 + 2.0 ** -24)))
    assert tie - 1 == Fraction(1, 2 ** 24)                                               # half an ULP of FLOAT at 1.0
    assert Fraction(3.4028235677973366e38) - Fraction(float(er.FLT_MAX)) == Fraction(2) ** 103      # FLT_MAX plus half its ULP (2^104)
    assert Fraction(7.006492321624085e-46) * 2 == Fraction(1.401298464324817e-45) == Fraction(1, 2 ** 149)
    # the values that tell one rounding from two: above a FLOAT tie by less than half an ULP of DOUBLE
    for v in (2 ** 53 + 2 ** 29 + 1, 2 ** 63 + 2 ** 39 + 1):
        assert v in p[U64] and bits(er.int_to_float(F32, v)) == bits(np.float32(float(v))) + 1
    assert 2 ** 53 + 2 ** 29 + 1 in p[I64] and bits(er.int_to_float(F32, 2 ** 63 + 2 ** 39 + 1)) == 0x5F000001
    d = [bits(v) for v in p[F64]]
    for want in (0, 1 << 63, 1, (1 << 63) | 1, 0x000FFFFFFFFFFFFF, 0x0010000000000000, 0x7FEFFFFFFFFFFFFF, 0xFFEFFFFFFFFFFFFF, 0x7FF0000000000000,
                 0xFFF0000000000000, 0x7FF8000000000000, 0x43E0000000000000, 0x43DFFFFFFFFFFFFF, 0xC3E0000000000000, 0xC3E0000000000001, 0x3FDFFFFFFFFFFFFF):
        assert want in d, hex(want)
    f = [bits(v) for v in p[F32]]
    for want in (0, 1 << 31, 0x3EFFFFFF, 0x4B000001, 0x4B800000, 0x4F000000, 0x5F000000, 0x7F7FFFFF, 0x00800000, 0x007FFFFF, 1, 0x7F800000, 0xFF800000, 0x7FC00000):
        assert want in f, hex(want)
    assert len(set(d)) == len(d) and len(set(f)) == len(f)
    for t in er.NUMERIC:
        assert len(p[t]) * len(er.RHS[t]) <= 1024 and set(map(bits, [er.NP[t](v) for v in er.RHS[t]])) <= set(map(bits, [er.NP[t](v) for v in p[t]] + [er.NP[t](3)]))


@pytest.mark.parametrize("t", er.NUMERIC, ids=er.type_id)
def test_every_pool_value_survives_the_null_masks(t):
    cols = er.cross(t, er.POOL[t], t, er.RHS[t], True)
    for (c, vals, z), pool in zip(cols, (er.POOL[t], er.RHS[t])):
        alive = {bits(er.NP[t](v)) for v, dead in zip(vals, z) if not dead}
        assert alive == {bits(er.NP[t](v)) for v in pool} and z.any(), c.name
    (c, vals, z), = er.single(t, er.POOL[t], True)
    assert {bits(er.NP[t](v)) for v, dead in zip(vals, z) if not dead} == {bits(er.NP[t](v)) for v in er.POOL[t]} and z.any()
    # the shift family's second column has three values: the masks of a 3-wide cross product
    zx, zy = er.null_masks(len(er.POOL[t]), 3)
    grid = np.arange(len(er.POOL[t]) * 3)
    assert set(grid[~zx] // 3) == set(range(len(er.POOL[t]))) and set(grid[~zy] % 3) == {0, 1, 2}


# ---- every case against the oracle ----------------------------------------------------------------------------------------------------------------
def against_oracle(case):
    if case.error is not None:
        with pytest.raises(oracle.OracleError) as e:
            oracle.run(case.op())
        assert e.value.return_code == case.error, (case.name, e.value)
        return
    schema, want, moved = case.expected()
    oschema, got = oracle.run(case.op())
    assert oschema == schema, (case.name, oschema, schema)
    er.same(got, want, moved, case.name)


def test_compiled_cases_against_the_oracle():
    for case in er.compiled_cases().values():
        against_oracle(case)
    for shape in ("scalar", "partitions"):
        (case,) = er.agg_cases(shape, 1025, er.COMPILED_AGGS)
        assert len(case.columns) == len(er.COMPILED_AGGS) > 8


def test_dense_cases_keep_the_plain_scatter():
    # dense slots exist for stages whose partition scatter has the plain form (dense_eligible, runtime.cpp): at most 24 record fields
    for n in er.AGG_ROWS:
        for case in er.agg_cases("dense", n):
            assert ("plain partition scatter" in ss.Plan(case.op(), ss.Context(-1)).describe()) == case.plain(), case.name


PARAMS = [(family, t) for family, types in er.FAMILIES.items() for t in types]


@pytest.mark.parametrize("family,t", PARAMS, ids=["%s-%s" % (f, er.type_id(t)) for f, t in PARAMS])
def test_reference_agrees_with_the_oracle(family, t):
    forms = er.family_forms(family, t)
    n = 0
    for form in sorted(forms):
        for case in forms[form]:
            against_oracle(case)
            n += 1
    assert n > 0


@pytest.mark.parametrize("t", er.NUMERIC, ids=er.type_id)
def test_signaling_forms_against_the_oracle(t):
    for failing, filtered in er.signaling_cases(t):
        against_oracle(failing)
        against_oracle(filtered)
    if t not in (U32, U64):            # (an unsigned pool holds nothing negative)
        against_oracle(er.sqrt_signaling_failure(t))


def test_logic_against_the_oracle():
    for case in er.logic_cases():
        against_oracle(case)


@pytest.mark.parametrize("t", sorted(er.MOVE_POOL), ids=er.type_id)
def test_selection_against_the_oracle(t):
    for case in er.selection_cases(t):
        against_oracle(case)


def test_bool_casts_are_not_part_of_the_api():
    # make_cast (bind.cpp): "Only numeric casts are supported" -- BOOL <-> number never reaches a CAST_B8_* / CAST_*_B8 handler through CastTo
    schema = ss.TupleSchema([ss.Attribute("b", ss.BOOL), ss.Attribute("x", ss.DOUBLE)])
    view = ss.View(schema, [np.array([True]), np.array([math.nan])])
    for e in (ss.CastTo(ss.INT32, ss.NamedAttribute("b")), ss.CastTo(ss.BOOL, ss.NamedAttribute("x"))):
        with pytest.raises(ss.SupersonicException) as err:
            ss.Plan(ss.Compute(ss.CompoundExpression().AddAs("r", e), ss.ScanView(view)), ss.Context(-1))
        assert err.value.return_code == ss.ERROR_ATTRIBUTE_TYPE_MISMATCH
        with pytest.raises(oracle.OracleError):
            oracle.run(ss.Compute(ss.CompoundExpression().AddAs("r", e), ss.ScanView(view)))


@pytest.mark.parametrize("shape", er.AGG_SHAPES)
@pytest.mark.parametrize("n", er.AGG_ROWS)
def test_aggregate_cases_against_the_oracle(n, shape):
    for case in er.agg_cases(shape, n):
        schema, want, moved, inexact = case.expected()
        oschema, got = oracle.run(case.op())
        assert oschema == schema, (case.name, oschema, schema)
        if shape != "scalar":
            order = np.argsort(got[0][0], kind="stable")
            got = [(d[order], None if z is None else z[order]) for d, z in got]
        # the oracle folds row after row: its finite DOUBLE sum is held to the bound of recursive summation, (n - 1) u sum|x|, around the
        # exactly rounded sum the device is held to 1 ULP of
        exact = [i for i in range(len(want)) if not inexact[i]]
        er.same([got[i] for i in exact], [want[i] for i in exact], [moved[i] for i in exact], case.name)
        first = len(want) - len(case.columns)
        for i in (i for i in range(len(want)) if inexact[i]):
            for k, vals in enumerate(case.columns[i - first].per_group):
                bound = len(vals) * 2.0 ** -53 * math.fsum(abs(float(v)) for v in vals if v is not None)
                assert abs(float(got[i][0][k]) - float(want[i][0][k])) <= bound and not got[i][1][k], (case.name, i, k, got[i][0][k], want[i][0][k], bound)
