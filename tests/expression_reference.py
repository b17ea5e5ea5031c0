"""An exact reference for the element-wise operators and the aggregate sinks at integer and IEEE edge values.

It shares no text with the device (supersonic_amd/csrc/vm_body.inc), the host fold (bind.cpp) or the oracle (oracle/ss_oracle.c):
  * integers are Python integers, reduced mod 2^32 / 2^64 and reinterpreted in the result type (`wrap`);
  * IEEE + - * / sqrt and float <-> float are NumPy scalars of the operand type: correctly rounded here, subnormals kept;
  * integer -> FLOAT rounds ONCE from the exact integer (`int_to_float`: round-half-even on the 24-bit significand; never via a double);
  * the project's rules, as its code comments state them:
      x / -1 wraps, x % -1 = 0                          vm_body.inc "CDIV_*" / "MOD_*", bind.cpp fold_binary
      a zero divisor is NULL (nulling) / fails (signaling) vm_body.inc "NULL_DIVZERO" / "FAIL_DIVZERO"
      *_TO_INT of a NaN or outside int64 = INT64_MIN     vm_body.inc CVT_I64_X86 (x86-64 cvttsd2si, "integer indefinite")
      RoundToInt = CEIL_TO_INT(ROUND(x))                 bind.cpp "RoundToInt binds as CEIL_TO_INT(ROUND(x))" (math_bound_expressions.cc:327-339)
      Abs = (x < 0 ? -x : x), so Abs(-0.0) = -0.0        math_evaluators.h:127-132
      integer Abs returns the unsigned type             bind.cpp OP_ABS
      Negate of an unsigned value is of the signed type  bind.cpp OP_NEGATE (CreateUnarySignedNumericExpression)
      mixed-sign 64-bit compares are value-correct       vm_body.inc LT_I64_U64 ..., bind_compare "value-correct functors"
  * NaN rule: where an ARITHMETIC result is NaN the device may give any NaN; a value that is only MOVED (If, IfNull, Case, NullingIf,
    projection, FIRST, LAST, store pass) keeps its bits (`same`);
  * nothing is skipped or masked: what the reference leaves undefined (variable shift counts outside [0, width), MIN / MAX over +0.0
    and -0.0, sums whose intermediate overflows while the exact sum does not) is not in the pools.  NULL rows compare by mask only.

A Case is one plan over one input with the expected result; tests/test_expression_reference_cpu.py checks every case against the
oracle and the rules against hand-computed literals, tests/test_values_expression_edges_gpu.py runs every case on the device."""
import math
from fractions import Fraction

import numpy as np

import supersonic_amd as ss

INT32, INT64, UINT32, UINT64, FLOAT, DOUBLE, BOOL = ss.INT32, ss.INT64, ss.UINT32, ss.UINT64, ss.FLOAT, ss.DOUBLE, ss.BOOL
NP = {INT32: np.int32, INT64: np.int64, UINT32: np.uint32, UINT64: np.uint64, FLOAT: np.float32, DOUBLE: np.float64, BOOL: np.bool_}
NAME = {INT32: "i32", INT64: "i64", UINT32: "u32", UINT64: "u64", FLOAT: "f32", DOUBLE: "f64", BOOL: "b8"}
WIDTH = {INT32: 32, UINT32: 32, INT64: 64, UINT64: 64}
INTS = (INT32, UINT32, INT64, UINT64)
FLOATS = (FLOAT, DOUBLE)
NUMERIC = INTS + FLOATS
SIGNED = (INT32, INT64)
CONST = {INT32: ss.ConstInt32, INT64: ss.ConstInt64, UINT32: ss.ConstUint32, UINT64: ss.ConstUint64, FLOAT: ss.ConstFloat,
         DOUBLE: ss.ConstDouble, BOOL: ss.ConstBool}
INT64_MIN = -2 ** 63
MAX_OUTPUTS = 16          # expressions of one Compute over columns
MAX_FOLDED = 32           # ... of one Compute of folded constants (NOT NULL columns: no NULL masks among the pipeline's outputs)


def f64_of_bits(u):
    return np.array([u], np.uint64).view(np.float64)[0]


def f32_of_bits(u):
    return np.array([u], np.uint32).view(np.float32)[0]


F64, F32 = np.float64, np.float32
NAN64, NAN64_PAYLOAD = f64_of_bits(0x7FF8000000000000), f64_of_bits(0xFFF8000000000001)
NAN32 = f32_of_bits(0x7FC00000)
DBL_MAX, FLT_MAX = F64(1.7976931348623157e308), F32(3.4028234663852886e38)

# ---- edge pools (the issue's lists; a few more values, none removed) ---------------------------------------------------------------------
POOL = {
    INT32: [0, 1, -1, 2, -2, 3, 7, -7, 46341, 65536, -65536, 2 ** 30, 2 ** 31 - 1, -2 ** 31, -2 ** 31 + 1],
    UINT32: [0, 1, 2, 3, 65535, 65536, 65537, 2 ** 31 - 1, 2 ** 31, 2 ** 31 + 1, 2 ** 32 - 1],
    # 2^53 + 2^29 + 1 and 2^63 + 2^39 + 1 lie just above a FLOAT tie and round to that tie as a DOUBLE: a cast through DOUBLE rounds twice
    INT64: [0, 1, -1, 2, -2, 3, 7, -7, 2 ** 24 + 1, 2 ** 31 - 1, 2 ** 31, -2 ** 31 - 1, 2 ** 32 - 1, 2 ** 32, 3037000500, 2 ** 53 - 1, 2 ** 53,
            2 ** 53 + 1, 2 ** 53 + 2 ** 29 + 1, 2 ** 62, 2 ** 63 - 1, -2 ** 63, -2 ** 63 + 1],
    UINT64: [0, 1, 2, 3, 2 ** 24 + 1, 2 ** 53 + 1, 2 ** 53 + 2 ** 29 + 1, 2 ** 63 - 1, 2 ** 63, 2 ** 63 + 1, 2 ** 63 + 2 ** 10, 2 ** 63 + 2 ** 39 + 1,
             2 ** 64 - 2 ** 39, 2 ** 64 - 1],
    DOUBLE: [F64(v) for v in (0.0, -0.0, 0.5, -0.5, 1.5, -1.5, 2.5, -2.5, 0.49999999999999994, 2.0 ** 52, -2.0 ** 52, 2.0 ** 53,
                              4.9e-324, -4.9e-324, 2.225073858507201e-308, 2.2250738585072014e-308, 1.7976931348623157e308, -1.7976931348623157e308,
                              math.inf, -math.inf, 2.0 ** 63, 9223372036854774784.0, -2.0 ** 63, -2.0 ** 63 - 2048.0, 1e19,
                              3.4028234663852886e38, 3.4028235677973366e38, 1.401298464324817e-45, 7.006492321624085e-46,
                              1.0 + 2.0 ** -24, 1.0 + 2.0 ** -24 + 2.0 ** -52, 1.0 + 3 * 2.0 ** -24)] + [NAN64],
    FLOAT: [F32(v) for v in (0.0, -0.0, 0.5, -0.5, 1.5, -1.5, 2.5, -2.5, 0.49999997, 2.0 ** 23 + 1, 2.0 ** 24, 2.0 ** 31, 2.0 ** 63,
                             3.4028234663852886e38, -3.4028234663852886e38, 1.1754943508222875e-38, 1.1754942106924411e-38, 1.401298464324817e-45,
                             math.inf, -math.inf)] + [NAN32],
    BOOL: [False, True],
}
# the second operand of a binary family over DOUBLE: a cross product stays within one 1024-row tile
RHS = dict(POOL)
RHS[DOUBLE] = [F64(v) for v in (0.0, -0.0, 0.5, -1.5, 2.5, 2.0 ** 53, 4.9e-324, -4.9e-324, 2.225073858507201e-308, 2.2250738585072014e-308,
                                1.7976931348623157e308, -1.7976931348623157e308, math.inf, -math.inf, 2.0 ** 63, 9223372036854774784.0,
                                -2.0 ** 63, 1e19, 3.4028234663852886e38, 1.401298464324817e-45, 1.0 + 2.0 ** -24, 3.0)] + [NAN64]


# ---- scalar rules ------------------------------------------------------------------------------------------------------------------------
def wrap(t, v):
    w = WIDTH[t]
    v &= (1 << w) - 1
    return v - (1 << w) if (t in SIGNED and v >> (w - 1)) else v


def int_to_float(t, i):
    """The integer i as FLOAT / DOUBLE, rounded once (half to even) from the exact value."""
    bits = 24 if t == FLOAT else 53
    m, e = abs(i), 0
    if m.bit_length() > bits:
        e = m.bit_length() - bits
        q, r, half = m >> e, m & ((1 << e) - 1), 1 << (e - 1)
        if r > half or (r == half and (q & 1)):
            q += 1
        m = q << e
    v = NP[t](float(m))               # m has at most `bits` significant bits: float() and the narrowing are exact
    assert Fraction(float(v)) == m
    return -v if i < 0 else v


def convert(to, frm, v):
    """CastTo(to, v) / an implicit promotion: what make_cast (bind.cpp) allows."""
    if to == frm:
        return v
    if to in INTS:
        assert frm in INTS
        return wrap(to, v)
    if frm in INTS:
        return int_to_float(to, v)
    with np.errstate(all="ignore"):
        return NP[to](v)


def fop(t, op, a, b):
    with np.errstate(all="ignore"):
        a, b = NP[t](a), NP[t](b)
        return a + b if op == "+" else a - b if op == "-" else a * b if op == "*" else a / b


def arith(op, t, a, b):
    if t in INTS:
        return wrap(t, a + b if op == "+" else a - b if op == "-" else a * b)
    return fop(t, op, a, b)


def cpp_divide(t, a, b):
    """Integer division, truncating; NULL (None) for a zero divisor; x / -1 wraps."""
    if b == 0:
        return None
    q = abs(a) // abs(b)
    return wrap(t, q if (a < 0) == (b < 0) else -q)


def modulus(t, a, b):
    """a - b * trunc(a / b); x % -1 = 0; NULL (None) for a zero divisor."""
    if b == 0:
        return None
    if t in SIGNED and b == -1:
        return 0
    q = abs(a) // abs(b)
    return wrap(t, a - b * (q if (a < 0) == (b < 0) else -q))


def divide(a, b):
    return fop(DOUBLE, "/", a, b)


def shift(t, left, a, n):
    assert 0 <= n < WIDTH[t]
    return wrap(t, a << n) if left else wrap(t, a >> n)       # Python's >> of a negative integer is arithmetic; unsigned values are >= 0


def bitwise(t, op, a, b):
    m = (1 << WIDTH[t]) - 1
    a, b = a & m, b & m
    return wrap(t, a & b if op == "&" else a | b if op == "|" else a ^ b if op == "^" else (~a) & b)


def compare_type(ta, tb):
    """bind_compare: DOUBLE if either side is, else FLOAT if either side is, else the values themselves (None)."""
    if ta == tb:
        return ta
    if DOUBLE in (ta, tb):
        return DOUBLE
    if FLOAT in (ta, tb):
        return FLOAT
    return None


def compare(op, ta, a, tb, b):
    t = compare_type(ta, tb)
    if t in FLOATS:
        a, b = convert(t, ta, a), convert(t, tb, b)
    return bool({"<": a < b, "<=": a <= b, "==": a == b, "!=": a != b, ">": a > b, ">=": a >= b}[op])


def c_round(t, x):
    """round(): half away from zero, the sign of a zero result kept."""
    if not np.isfinite(x):
        return x
    r = np.trunc(x)
    if abs(x - r) >= 0.5:             # x - trunc(x) is exact
        r = r + NP[t](math.copysign(1.0, x))
    return NP[t](r)


def to_int64(x):
    """static_cast<int64> on x86-64 (cvttsd2si): INT64_MIN for a NaN and outside [-2^63, 2^63)."""
    if np.isnan(x) or not (-2.0 ** 63 <= float(x) < 2.0 ** 63):
        return INT64_MIN
    return int(x)


def f_abs(t, x):
    return -x if x < 0 else x


def f_sqrt(x):
    with np.errstate(all="ignore"):
        return np.sqrt(np.float64(x))


def is_normal(x):
    x = float(x)
    return math.isfinite(x) and abs(x) >= 2.2250738585072014e-308


# ---- comparing under the NaN rule ----------------------------------------------------------------------------------------------------------
def column_of(t, values):
    """(data, is_null) of typed values; None is NULL."""
    z = np.array([v is None for v in values], bool)
    if t in INTS:
        d = np.array([0 if v is None else v & ((1 << WIDTH[t]) - 1) for v in values], np.uint64).astype(NP[UINT32] if WIDTH[t] == 32 else np.uint64).view(NP[t])
    elif t == BOOL:
        d = np.array([bool(v) for v in values], np.bool_)
    else:
        d = np.array([NP[t](0) if v is None else v for v in values], NP[t])
    return d, z


def same(got, want, moved, where=""):
    """got / want: [(data, is_null or None)]; moved[i]: column i is a move (bits kept) -- else a NaN may be any NaN."""
    assert len(got) == len(want), (where, len(got), len(want))
    for i, ((gd, gz), (wd, wz)) in enumerate(zip(got, want)):
        assert len(gd) == len(wd), "%s column %d: %d rows, expected %d" % (where, i, len(gd), len(wd))
        gz = np.zeros(len(gd), bool) if gz is None else np.asarray(gz, bool)
        wz = np.zeros(len(wd), bool) if wz is None else np.asarray(wz, bool)
        assert np.array_equal(gz, wz), "%s column %d: NULL masks differ at rows %s" % (where, i, np.nonzero(gz != wz)[0][:10])
        assert gd.dtype == wd.dtype, (where, i, gd.dtype, wd.dtype)
        ok = gd.view("u%d" % gd.dtype.itemsize) == wd.view("u%d" % wd.dtype.itemsize) if gd.dtype != np.bool_ else gd == wd
        if gd.dtype.kind == "f" and not moved[i]:
            ok = ok | (np.isnan(gd) & np.isnan(wd))
        bad = np.nonzero(~(ok | wz))[0]
        assert len(bad) == 0, "%s column %d: %d rows differ, first rows %s: got %r, expected %r" % (where, i, len(bad), bad[:6], gd[bad[:6]], wd[bad[:6]])


# ---- cases ------------------------------------------------------------------------------------------------------------------------------------
class Col(object):
    def __init__(self, name, t, nullable):
        self.name, self.t, self.nullable, self.const = name, t, nullable, False

    def expr(self):
        return ss.NamedAttribute(self.name)

    def value(self, row):
        return row[self.name]


class Const(object):
    def __init__(self, t, v):
        self.t, self.v, self.nullable, self.const = t, v, False, True

    def expr(self):
        return CONST[self.t](float(self.v) if self.t in FLOATS else self.v)

    def value(self, row):
        return self.v


class Out(object):
    """One result column: its alias, expression, type, nullability and the reference's value of a row (None = NULL)."""

    def __init__(self, alias, expr, t, nullable, fn, moved=False):
        self.alias, self.expr, self.t, self.nullable, self.fn, self.moved = alias, expr, t, nullable, fn, moved


def make(alias, builder, args, t, fn, nulling=False, moved=False):
    """builder(*expressions) over Col / Const operands; fn(*values) -> value, called where no operand is NULL (strict operators).  A
    nulling operator may return None.  With constants only the binder folds: the column is NULLABLE iff the folded value is NULL."""
    def value(row):
        vals = [a.value(row) for a in args]
        return None if any(v is None for v in vals) else fn(*vals)
    if all(a.const for a in args):
        nullable = value({}) is None
    else:
        nullable = nulling or any(a.nullable for a in args)
    return Out(alias, builder(*[a.expr() for a in args]), t, nullable, value, moved)


class Case(object):
    """One plan: Compute(outs) over [Filter(keep) over] the input; `error`: the run must fail with this code instead."""

    def __init__(self, name, cols, outs, keep=None, error=None, predicate=None):
        self.name, self.cols, self.outs, self.keep, self.error, self.predicate = name, cols, outs, keep, error, predicate
        assert outs is None or 0 < len(outs) <= MAX_FOLDED, (name, len(outs))
        self.rows = len(cols[0][1])
        assert 0 < self.rows <= 1024, (name, self.rows)

    def schema(self):
        return ss.TupleSchema([ss.Attribute(c.name, c.t, ss.NULLABLE if c.nullable else ss.NOT_NULLABLE) for c, _d, _z in self.cols])

    def view(self):
        cols = []
        for c, vals in self.expand():
            d, z = column_of(c.t, vals)
            cols.append(ss.Column(d, z if c.nullable else None))
        return ss.View(self.schema(), cols)

    def expand(self):
        """[(column, its values with None at the NULL rows)]"""
        return [(c, [None if (z is not None and z[i]) else v for i, v in enumerate(vals)]) for c, vals, z in self.cols]

    def op(self, view=None):
        view = view if view is not None else self.view()
        child = ss.ScanView(view)
        if self.keep is not None:
            child = ss.Filter(self.keep[0], ss.ProjectAllAttributes(), child)
        if self.outs is None:         # a Filter alone: the predicate through SEL_FROM_PRED, every input column moved
            return ss.Filter(self.predicate[0], ss.ProjectAllAttributes(), child)
        e = ss.CompoundExpression()
        for o in self.outs:
            e.AddAs(o.alias, o.expr)
        return ss.Compute(e, child)

    def input_rows(self):
        cols = self.expand()
        rows = [{c.name: vals[i] for c, vals in cols} for i in range(self.rows)]
        if self.keep is not None:
            rows = [r for r in rows if self.keep[1](r) is True]
        return rows

    def expected(self):
        """-> (schema [(name, type, nullable)], [(data, is_null or None)], moved [bool])"""
        rows = self.input_rows()
        if self.outs is None:
            rows = [r for r in rows if self.predicate[1](r) is True]
            schema = [(c.name, c.t, 1 if c.nullable else 0) for c, _d, _z in self.cols]
            cols = [column_of(c.t, [r[c.name] for r in rows]) for c, _d, _z in self.cols]
            return schema, [(d, z if s[2] else None) for (d, z), s in zip(cols, schema)], [True] * len(schema)
        schema = [(o.alias, o.t, 1 if o.nullable else 0) for o in self.outs]
        cols = []
        for o in self.outs:
            vals = [o.fn(r) for r in rows]
            assert o.nullable or all(v is not None for v in vals), (self.name, o.alias)
            d, z = column_of(o.t, vals)
            cols.append((d, z if o.nullable else None))
        return schema, cols, [o.moved for o in self.outs]


def null_masks(nx, ny):
    """Masks over the cross product (row = i * ny + j) that leave every value of either pool non-NULL at least once."""
    i, j = np.divmod(np.arange(nx * ny), ny)
    return (i + j) % 3 == 0, (i + 2 * j) % 5 == 1


def cross(tx, px, ty, py, nullable, names=("x", "y")):
    """The two columns of the cross product of two pools."""
    xs = [a for a in px for _b in py]
    ys = [b for _a in px for b in py]
    zx, zy = null_masks(len(px), len(py)) if nullable else (None, None)
    if nullable and len(py) == 1:
        zx = np.arange(len(px)) % 3 == 1
    return [(Col(names[0], tx, nullable), xs, zx), (Col(names[1], ty, nullable), ys, zy)]


def single(t, pool, nullable, name="x"):
    """One column holding the pool (twice when NULLABLE, so that every value is there non-NULL)."""
    vals = list(pool) * (2 if nullable else 1)
    k = np.arange(len(vals))
    z = ((k % len(pool)) % 2 == (k >= len(pool))) if nullable else None        # NULL at the even places of the first copy, the odd ones of the second
    return [(Col(name, t, nullable), vals, z)]


def three_rows():
    return [(Col("x", INT32, False), [1, 2, 3], None)]


def chunks(outs, n=MAX_OUTPUTS):
    return [outs[i:i + n] for i in range(0, len(outs), n)]


def packed(name, cols, outs, n=MAX_OUTPUTS, **kw):
    return [Case("%s/%d" % (name, i), cols, part, **kw) for i, part in enumerate(chunks(outs, n))]


# ---- the binary families ------------------------------------------------------------------------------------------------------------------------
def _b(name, builder, rtype, fn, nulling=False):
    return (name, builder, rtype, fn, nulling)


def arithmetic_ops(t):
    return [_b("plus", ss.Plus, t, lambda a, b: arith("+", t, a, b)), _b("minus", ss.Minus, t, lambda a, b: arith("-", t, a, b)),
            _b("times", ss.Multiply, t, lambda a, b: arith("*", t, a, b))]


def negate(t, operand, alias="neg"):
    st = {UINT32: INT32, UINT64: INT64}.get(t, t)
    return make(alias, ss.Negate, [operand], st, (lambda a: wrap(st, -a)) if t in INTS else (lambda a: -a))


def division_ops(t, signaling=False):
    """Nulling forms (and the signaling ones, for inputs without a zero divisor)."""
    if t in FLOATS:
        ops = [_b("divq", ss.DivideQuiet, DOUBLE, lambda a, b: divide(convert(DOUBLE, t, a), convert(DOUBLE, t, b))),
               _b("divn", ss.DivideNulling, DOUBLE, lambda a, b: None if b == 0 else divide(convert(DOUBLE, t, a), convert(DOUBLE, t, b)), True)]
        if signaling:
            ops.append(_b("divs", ss.DivideSignaling, DOUBLE, lambda a, b: divide(convert(DOUBLE, t, a), convert(DOUBLE, t, b))))
        return ops
    ops = [_b("cdivn", ss.CppDivideNulling, t, lambda a, b: cpp_divide(t, a, b), True), _b("modn", ss.ModulusNulling, t, lambda a, b: modulus(t, a, b), True)]
    if signaling:
        ops += [_b("cdivs", ss.CppDivideSignaling, t, lambda a, b: cpp_divide(t, a, b)), _b("mods", ss.ModulusSignaling, t, lambda a, b: modulus(t, a, b))]
    return ops


def bitwise_ops(t):
    return [_b("band", ss.BitwiseAnd, t, lambda a, b: bitwise(t, "&", a, b)), _b("bor", ss.BitwiseOr, t, lambda a, b: bitwise(t, "|", a, b)),
            _b("bxor", ss.BitwiseXor, t, lambda a, b: bitwise(t, "^", a, b)), _b("bandnot", ss.BitwiseAndNot, t, lambda a, b: bitwise(t, "~&", a, b))]


def shift_ops(t):
    return [_b("shl", ss.ShiftLeft, t, lambda a, n: shift(t, True, a, n)), _b("shr", ss.ShiftRight, t, lambda a, n: shift(t, False, a, n))]


COMPARISONS = (("lt", ss.Less, "<"), ("le", ss.LessOrEqual, "<="), ("eq", ss.Equal, "=="), ("ne", ss.NotEqual, "!="), ("gt", ss.Greater, ">"),
               ("ge", ss.GreaterOrEqual, ">="))


def comparison_ops(ta, tb, swapped=False):
    """swapped: the operands arrive as (tb value, ta value)."""
    def one(sym):
        return (lambda b, a: compare(sym, tb, b, ta, a)) if swapped else (lambda a, b: compare(sym, ta, a, tb, b))
    return [_b(nm, builder, BOOL, one(sym)) for nm, builder, sym in COMPARISONS]


def binary_forms(name, tx, px, ty, py, ops, unary=None, fold_both_ways=True, const_both_ways=True):
    """The forms of one binary family over pools px (type tx) x py (type ty):
       cc   column o column, NOT NULL and NULLABLE (+ `unary(operand)` outputs on x)
       ck   column o constant and constant o column: one plan per constant of py (x o c), and of px (c o y) where const_both_ways
       kk   constant o constant, folded on the host, over a 3-row view
    `ops(ta, tb)` -> [(name, builder, result type, fn, nulling)] for operands of these types in this order.  -> {"cc": [...], "ck": [...], "kk": [...]}"""
    forms = {"cc": [], "ck": [], "kk": []}
    for nullable in (False, True):
        cols = cross(tx, px, ty, py, nullable)
        x, y = cols[0][0], cols[1][0]
        outs = [make(nm, b, [x, y], rt, fn, nulling) for nm, b, rt, fn, nulling in ops(tx, ty)]
        if unary:
            outs += unary(x)
        forms["cc"] += packed("%s-cc-%s" % (name, "nullable" if nullable else "notnull"), cols, outs)
    cols = single(tx, px, False)
    x = cols[0][0]
    for k, c in enumerate(py):
        outs = [make("%s_xc" % nm, b, [x, Const(ty, c)], rt, fn, nulling) for nm, b, rt, fn, nulling in ops(tx, ty)]
        forms["ck"] += packed("%s-xc-%d" % (name, k), cols, outs)
    if const_both_ways:
        cols = single(ty, py, True, "y")
        y = cols[0][0]
        for k, c in enumerate(px):
            outs = [make("%s_cy" % nm, b, [Const(tx, c), y], rt, fn, nulling) for nm, b, rt, fn, nulling in ops(tx, ty)]
            forms["ck"] += packed("%s-cy-%d" % (name, k), cols, outs)
    outs = []
    for i, a in enumerate(px):
        for j, c in enumerate(py):
            for nm, b, rt, fn, nulling in ops(tx, ty):
                outs.append(make("%s_%d_%d" % (nm, i, j), b, [Const(tx, a), Const(ty, c)], rt, fn, nulling))
    if unary:
        for i, a in enumerate(px):
            outs += [Out("%s_%d" % (o.alias, i), o.expr, o.t, o.nullable, o.fn, o.moved) for o in unary(Const(tx, a))]
    forms["kk"] = packed("%s-kk" % name, three_rows(), outs, MAX_FOLDED)
    return forms


def arithmetic_family(t):
    return binary_forms("arith-" + NAME[t], t, POOL[t], t, RHS[t], lambda ta, tb: arithmetic_ops(t), unary=lambda x: [negate(t, x)])


def nonzero(pool):
    return [v for v in pool if v != 0]


def division_family(t):
    """Nulling (and for the floats quiet) forms over the whole pools; the signaling forms over non-zero divisors (`signaling_cases` holds the
    failing runs)."""
    forms = binary_forms("div-" + NAME[t], t, POOL[t], t, RHS[t], lambda ta, tb: division_ops(t))
    sig = binary_forms("divs-" + NAME[t], t, POOL[t], t, nonzero(RHS[t]), lambda ta, tb: [o for o in division_ops(t, True) if o[0] in ("divs", "cdivs", "mods")])
    # a signaling division by a constant zero is not folded: it fails when it is evaluated (bind.cpp fold_binary)
    return {k: forms[k] + sig[k] for k in forms}


def signaling_cases(t):
    """[(failing case, the same case behind a Filter that drops the zero divisors)] for column and constant zero divisors."""
    out = []
    builders = [ss.DivideSignaling] if t in FLOATS else [ss.CppDivideSignaling, ss.ModulusSignaling]
    rt = DOUBLE if t in FLOATS else t
    zero = NP[t](0.0) if t in FLOATS else 0
    for nullable in (False, True):
        cols = cross(t, POOL[t], t, RHS[t], nullable)
        x, y = cols[0][0], cols[1][0]
        ops = [o for o in division_ops(t, True) if o[0] in ("divs", "cdivs", "mods")]
        outs = [make(nm, b, [x, y], r, fn) for nm, b, r, fn, _n in ops]
        keep = (ss.NotEqual(y.expr(), Const(t, zero).expr()), lambda r: None if r["y"] is None else bool(r["y"] != 0))
        tag = "%s-%s" % (NAME[t], "nullable" if nullable else "notnull")
        out.append((Case("sig-fails-" + tag, cols, outs, error=ss.ERROR_EVALUATION_ERROR), Case("sig-filtered-" + tag, cols, outs, keep=keep)))
    cols = single(t, POOL[t], False)
    x = cols[0][0]
    outs = [make("q%d" % i, b, [x, Const(t, zero)], rt, lambda a, b: None) for i, b in enumerate(builders)]
    never = (ss.Less(x.expr(), x.expr()), lambda r: False)
    out.append((Case("sig-fails-const-" + NAME[t], cols, outs, error=ss.ERROR_EVALUATION_ERROR), Case("sig-filtered-const-" + NAME[t], cols, outs, keep=never)))
    return out


def bitwise_family(t):
    return binary_forms("bits-" + NAME[t], t, POOL[t], t, POOL[t], lambda ta, tb: bitwise_ops(t),
                        unary=lambda x: [make("bnot", ss.BitwiseNot, [x], t, lambda a: wrap(t, ~a))])


def shift_counts(t):
    return [0, 1, WIDTH[t] - 1]


def shift_family(t):
    return binary_forms("shift-" + NAME[t], t, POOL[t], t, shift_counts(t), lambda ta, tb: shift_ops(t), const_both_ways=False)


COMPARE_PAIRS = [(a, b) for a in NUMERIC for b in NUMERIC] + [(BOOL, BOOL)]
# the pairs whose constant and Filter forms run too: every type against itself, the mixed-sign and mixed-width integers, an integer against either float
DEEP_PAIRS = [(t, t) for t in NUMERIC + (BOOL,)] + [(INT64, UINT64), (UINT64, INT64), (INT32, UINT32), (UINT32, INT32), (INT64, DOUBLE), (UINT64, FLOAT)]


def comparison_family(ta, tb):
    deep = (ta, tb) in DEEP_PAIRS
    forms = binary_forms("cmp-%s-%s" % (NAME[ta], NAME[tb]), ta, POOL[ta], tb, RHS[tb], comparison_ops)
    if not deep:
        forms["ck"], forms["kk"] = [], []
    if compare_type(ta, tb) is None:
        forms["kk"] = []              # mixed integer constants are not folded: they run on the device, as the ck forms do
    forms["filter"] = []
    if deep:
        for nullable in (False, True):
            cols = cross(ta, POOL[ta], tb, RHS[tb], nullable)
            x, y = cols[0][0], cols[1][0]
            for nm, builder, sym in COMPARISONS:
                def pred(r, sym=sym):
                    return None if (r["x"] is None or r["y"] is None) else compare(sym, ta, r["x"], tb, r["y"])
                forms["filter"].append(Case("cmp-%s-%s-filter-%s-%s" % (NAME[ta], NAME[tb], nm, "nullable" if nullable else "notnull"), cols, None,
                                            predicate=(builder(x.expr(), y.expr()), pred)))
    return forms


# ---- casts ------------------------------------------------------------------------------------------------------------------------------------
def cast_targets(frm):
    return [to for to in NUMERIC if to != frm and not (frm in FLOATS and to in INTS)]


def cast_outs(frm, operand, tag=""):
    return [make("to_%s%s" % (NAME[to], tag), lambda e, to=to: ss.CastTo(to, e), [operand], to, lambda a, to=to: convert(to, frm, a)) for to in cast_targets(frm)]


def cast_family(frm):
    forms = {"cc": [], "ck": [], "kk": []}
    for nullable in (False, True):
        cols = single(frm, POOL[frm], nullable)
        forms["cc"] += packed("cast-%s-%s" % (NAME[frm], "nullable" if nullable else "notnull"), cols, cast_outs(frm, cols[0][0]))
    outs = []
    for i, v in enumerate(POOL[frm]):
        outs += cast_outs(frm, Const(frm, v), "_%d" % i)
    forms["kk"] = packed("cast-%s-kk" % NAME[frm], three_rows(), outs, MAX_FOLDED)
    return forms


# ---- exact math family ----------------------------------------------------------------------------------------------------------------------------
def math_outs(t, x, tag=""):
    """Every operator of the exact family the binder accepts for type t, over operand x."""
    def m(nm, builder, rt, fn, nulling=False, moved=False):
        return make(nm + tag, builder, [x], rt, fn, nulling, moved)

    def dbl(a):
        return convert(DOUBLE, t, a)
    outs = []
    if t in FLOATS:
        outs += [m("abs", ss.Abs, t, lambda a: f_abs(t, a)), m("round", ss.Round, t, lambda a: c_round(t, a)), m("ceil", ss.Ceil, t, lambda a: NP[t](np.ceil(a))),
                 m("floor", ss.Floor, t, lambda a: NP[t](np.floor(a))), m("trunc", ss.Trunc, t, lambda a: NP[t](np.trunc(a))),
                 m("round2i", ss.RoundToInt, INT64, lambda a: to_int64(np.ceil(c_round(t, a)))), m("ceil2i", ss.CeilToInt, INT64, lambda a: to_int64(np.ceil(a))),
                 m("floor2i", ss.FloorToInt, INT64, lambda a: to_int64(np.floor(a)))]
    else:
        ut = {INT32: UINT32, INT64: UINT64}.get(t, t)
        # integers are already rounded: the rounding family is the argument itself (bind.cpp "integers are already rounded"), moved
        outs += [m("abs", ss.Abs, ut, lambda a: abs(a), moved=t == ut)]
        outs += [m(nm, b, t, lambda a: a, moved=True) for nm, b in (("round", ss.Round), ("ceil", ss.Ceil), ("floor", ss.Floor), ("trunc", ss.Trunc),
                                                                      ("round2i", ss.RoundToInt), ("ceil2i", ss.CeilToInt), ("floor2i", ss.FloorToInt))]
        outs += [m("odd", ss.IsOdd, BOOL, lambda a: a % 2 != 0), m("even", ss.IsEven, BOOL, lambda a: a % 2 == 0)]
    outs += [m("sqrtq", ss.SqrtQuiet, DOUBLE, lambda a: f_sqrt(dbl(a))), m("sqrtn", ss.SqrtNulling, DOUBLE, lambda a: None if dbl(a) < 0 else f_sqrt(dbl(a)), True)]
    outs += [m("fin", ss.IsFinite, BOOL, lambda a: bool(np.isfinite(dbl(a)))), m("inf", ss.IsInf, BOOL, lambda a: bool(np.isinf(dbl(a)))),
             m("nan", ss.IsNaN, BOOL, lambda a: bool(np.isnan(dbl(a)))), m("nrm", ss.IsNormal, BOOL, lambda a: is_normal(dbl(a)))]
    return outs


def math_family(t):
    forms = {"cc": [], "ck": [], "kk": []}
    for nullable in (False, True):
        cols = single(t, POOL[t], nullable)
        x = cols[0][0]
        outs = math_outs(t, x)
        # SqrtSignaling where the Filter keeps x >= 0 (NaN and the negative values dropped; -0.0 stays and gives -0.0)
        forms["cc"] += packed("math-%s-%s" % (NAME[t], "nullable" if nullable else "notnull"), cols, outs)
        zero = Const(t, NP[t](0) if t in FLOATS else 0)
        keep = (ss.GreaterOrEqual(x.expr(), zero.expr()), lambda r: None if r["x"] is None else bool(r["x"] >= 0))
        sig = [make("sqrts", ss.SqrtSignaling, [x], DOUBLE, lambda a: f_sqrt(convert(DOUBLE, t, a)))]
        forms["cc"].append(Case("math-%s-sqrts-%s" % (NAME[t], "nullable" if nullable else "notnull"), cols, sig, keep=keep))
    outs = []
    for i, v in enumerate(POOL[t]):
        outs += math_outs(t, Const(t, v), "_%d" % i)
    forms["kk"] = packed("math-%s-kk" % NAME[t], three_rows(), outs, MAX_FOLDED)
    return forms


def sqrt_signaling_failure(t):
    cols = single(t, POOL[t], False)
    return Case("math-%s-sqrts-fails" % NAME[t], cols, [make("sqrts", ss.SqrtSignaling, [cols[0][0]], DOUBLE, lambda a: None)], error=ss.ERROR_EVALUATION_ERROR)


# ---- selection and logic ------------------------------------------------------------------------------------------------------------------------
def logic_cases():
    """And / Or / AndNot (three-valued: a decided side wins over a NULL, elementary_bound_expressions.cc:343-404 MakeResultSkipVector), Xor /
    Not (strict) over all nine (value, NULL) pairs -- both hidden values under a NULL."""
    states = [(False, False), (True, False), (False, True), (True, True)]        # (value, is NULL)
    xs, zx, ys, zy = [], [], [], []
    for a, na in states:
        for b, nb in states:
            xs.append(a); zx.append(na); ys.append(b); zy.append(nb)
    x, y = Col("x", BOOL, True), Col("y", BOOL, True)
    cols = [(x, xs, np.array(zx)), (y, ys, np.array(zy))]

    def and3(r):
        a, b = r["x"], r["y"]
        return False if (a is False or b is False) else (None if (a is None or b is None) else True)

    def or3(r):
        a, b = r["x"], r["y"]
        return True if (a is True or b is True) else (None if (a is None or b is None) else False)

    def andnot3(r):                   # NOT x AND y
        a, b = r["x"], r["y"]
        return False if (a is True or b is False) else (None if (a is None or b is None) else True)
    outs = [Out("and", ss.And(x.expr(), y.expr()), BOOL, True, and3), Out("or", ss.Or(x.expr(), y.expr()), BOOL, True, or3),
            make("xor", ss.Xor, [x, y], BOOL, lambda a, b: a != b), Out("andnot", ss.AndNot(x.expr(), y.expr()), BOOL, True, andnot3),
            make("not", ss.Not, [x], BOOL, lambda a: not a)]
    cases = [Case("logic-nullable", cols, outs)]
    x2, y2 = Col("x", BOOL, False), Col("y", BOOL, False)
    cols2 = [(x2, [False, False, True, True], None), (y2, [False, True, False, True], None)]
    outs2 = [make(nm, b, [x2, y2], BOOL, fn) for nm, b, fn in (("and", ss.And, lambda a, b: a and b), ("or", ss.Or, lambda a, b: a or b), ("xor", ss.Xor, lambda a, b: a != b),
                                                                 ("andnot", ss.AndNot, lambda a, b: (not a) and b))] + [make("not", ss.Not, [x2], BOOL, lambda a: not a)]
    for k, (a, b) in enumerate([(False, False), (False, True), (True, False), (True, True)]):
        outs2 += [make("%s_k%d" % (nm, k), bld, [Const(BOOL, a), Const(BOOL, b)], BOOL, fn) for nm, bld, fn in
                  (("and", ss.And, lambda a, b: a and b), ("or", ss.Or, lambda a, b: a or b), ("xor", ss.Xor, lambda a, b: a != b), ("andnot", ss.AndNot, lambda a, b: (not a) and b))]
    cases += packed("logic-notnull", cols2, outs2)
    # a constant on one side: the immediate operand of AND3 / OR3 and of the strict forms
    outs3 = []
    for k, c in enumerate((False, True)):
        kc = Const(BOOL, c)
        outs3 += [Out("and_xc%d" % k, ss.And(x.expr(), kc.expr()), BOOL, True, lambda r, c=c: False if (r["x"] is False or not c) else r["x"]),
                  Out("or_cx%d" % k, ss.Or(kc.expr(), x.expr()), BOOL, True, lambda r, c=c: True if (r["x"] is True or c) else r["x"]),
                  make("xor_xc%d" % k, ss.Xor, [x, kc], BOOL, lambda a, b: a != b),
                  Out("andnot_cx%d" % k, ss.AndNot(kc.expr(), x.expr()), BOOL, True, lambda r, c=c: False if (c or r["x"] is False) else r["x"])]
    cases += packed("logic-const", cols, outs3)
    return cases


MOVE_POOL = {DOUBLE: POOL[DOUBLE] + [NAN64_PAYLOAD], INT64: POOL[INT64], FLOAT: POOL[FLOAT] + [f32_of_bits(0xFFC00001)], UINT64: POOL[UINT64],
             INT32: POOL[INT32], UINT32: POOL[UINT32]}


def selection_cases(t):
    """If / NullingIf / IfNull / Case / In with the pool of t as data: a NULLABLE condition c over (c, x) crossed, y the pool reversed."""
    pool = MOVE_POOL[t]
    conds = [(False, False), (True, False), (True, True)]
    cs, zc, xs, ys = [], [], [], []
    for i, v in enumerate(pool):
        for c, nc in conds:
            cs.append(c); zc.append(nc); xs.append(v); ys.append(pool[len(pool) - 1 - i])
    n = len(xs)
    c, x, y = Col("c", BOOL, True), Col("x", t, True), Col("y", t, False)
    zx = np.arange(n) % 7 == 3
    cols = [(c, cs, np.array(zc)), (x, xs, zx), (y, ys, None)]
    k = Const(t, pool[4])

    def pick(r, nulling):
        if r["c"] is None:
            return None if nulling else r["y"]
        return r["x"] if r["c"] else r["y"]
    eqv = lambda a, b: compare("==", t, a, t, b)       # noqa: E731
    w1, w2 = pool[1], pool[-1]                          # WHEN constants: an ordinary value and the last one (a NaN for the floats: never matches)

    def case_of(r):
        if r["x"] is not None and eqv(r["x"], w1):
            return r["y"]
        if r["x"] is not None and eqv(r["x"], w2):
            return k.v
        return r["x"]

    def in_of(r, lst):
        if r["x"] is None:
            return None
        return any(eqv(r["x"], v) for v in lst)
    lst = [pool[0], pool[3], pool[-1]]
    outs = [Out("if", ss.If(c.expr(), x.expr(), y.expr()), t, True, lambda r: pick(r, False), True),
            Out("nif", ss.NullingIf(c.expr(), x.expr(), y.expr()), t, True, lambda r: pick(r, True), True),
            Out("if_k", ss.If(c.expr(), k.expr(), x.expr()), t, True, lambda r: k.v if r["c"] else r["x"], True),
            Out("if_yk", ss.If(c.expr(), y.expr(), k.expr()), t, False, lambda r: r["y"] if r["c"] else k.v, True),
            Out("ifnull", ss.IfNull(x.expr(), y.expr()), t, False, lambda r: r["y"] if r["x"] is None else r["x"], True),
            Out("ifnull_k", ss.IfNull(x.expr(), k.expr()), t, False, lambda r: k.v if r["x"] is None else r["x"], True),
            Out("case", ss.Case([x.expr(), x.expr(), Const(t, w1).expr(), y.expr(), Const(t, w2).expr(), k.expr()]), t, True, case_of, True),
            Out("in", ss.In(x.expr(), [Const(t, v).expr() for v in lst]), BOOL, True, lambda r: in_of(r, lst)),
            Out("in_y", ss.In(y.expr(), [x.expr(), Const(t, pool[2]).expr()]), BOOL, True,
                lambda r: True if ((r["x"] is not None and eqv(r["y"], r["x"])) or eqv(r["y"], pool[2])) else (None if r["x"] is None else False)),
            Out("copy", x.expr(), t, True, lambda r: r["x"], True)]
    return [Case("select-" + NAME[t], cols, outs)]


# ---- aggregate sinks ------------------------------------------------------------------------------------------------------------------------------
AGG_ROWS = (1, 64, 1025)
MINMAX_IDENTITIES = {UINT64: (2 ** 64 - 1, 0), INT64: (2 ** 63 - 1, -2 ** 63), UINT32: (2 ** 32 - 1, 0), INT32: (2 ** 31 - 1, -2 ** 31),
                     FLOAT: (F32(math.inf), F32(-math.inf)), DOUBLE: (F64(math.inf), F64(-math.inf)), BOOL: (True, False)}
def fold_sum(t, values, out=None):
    """SUM as the reference folds it, row after row, in the result type (aggregation_operators.h:173-186 `*result += val`; the result
    type is the input's unless the specification names one, aggregator.cc:63-78): integers wrap, floats add in the result type.  Finite
    DOUBLE data: the exactly rounded sum (math.fsum) -- the device is held to 1 ULP of it.  Finite FLOAT data must
    have exact partial sums (asserted), so that the FLOAT fold and the device's DOUBLE accumulators rounded once agree."""
    out = t if out is None else out
    vals = [v for v in values if v is not None]
    if not vals:
        return None
    if t in INTS:
        return wrap(out, sum(vals))
    if all(math.isfinite(float(v)) for v in vals):
        exact = sum(Fraction(float(v)) for v in vals)
        if out == DOUBLE:
            if abs(exact) < Fraction(float(DBL_MAX)) + Fraction(2) ** 970:
                return F64(math.fsum(float(v) for v in vals))
            return F64(math.inf if exact > 0 else -math.inf)
        if abs(exact) < Fraction(float(FLT_MAX)):
            s = F32(0.0)
            for v in vals:
                s = s + F32(v)
            assert Fraction(float(s)) == exact, "a finite FLOAT sum of the pools must be exact"
            return s
    s = NP[out](0.0)
    with np.errstate(all="ignore"):
        for v in vals:
            s = s + NP[out](v)
    return s


class AggColumn(object):
    """One aggregated input column: `base` everywhere, `special` planted at `where` (0 or -1), everything else NULL when base is None."""

    def __init__(self, name, t, kind, values, want, want_type, exact=True, moved=False, otype=None):
        self.name, self.t, self.kind, self.values, self.want, self.want_type, self.exact, self.moved = name, t, kind, values, want, want_type, exact, moved
        self.otype = otype            # AddAggregationWithDefinedOutputType

    def widens(self):
        """Not a field of the plain scatter's record (lower.cpp, Stage::PlainScatter): a SUM converted to a wider result type before the
        sink, and FIRST / LAST, whose field is the row id the VM makes."""
        return self.otype is not None or self.kind in (ss.FIRST, ss.LAST)


def _planted(n, base, specials):
    """n values: `base` (None = NULL) with specials[(row index)] planted; row indices 0 and -1 meet at n = 1 (the last one wins)."""
    vals = [base] * n
    for where, v in specials:
        vals[where] = v
    return vals


def agg_columns(n):
    """The aggregated columns of one input of n rows -> [AggColumn].  Every column is NULLABLE."""
    cols = []

    def add(name, t, kind, vals, want, wt=None, exact=True, moved=False, otype=None):
        cols.append(AggColumn(name, t, kind, vals, want, wt if wt is not None else t, exact, moved, otype))
    for t, (top, bottom) in MINMAX_IDENTITIES.items():
        for where, tag in ((0, "first"), (-1, "last")):
            # the only non-NULL value equals the accumulator's identity
            add("min_%s_%s" % (NAME[t], tag), t, ss.MIN, _planted(n, None, [(where, top)]), top)
            add("max_%s_%s" % (NAME[t], tag), t, ss.MAX, _planted(n, None, [(where, bottom)]), bottom)
        add("min_%s_null" % NAME[t], t, ss.MIN, [None] * n, None)
        add("max_%s_null" % NAME[t], t, ss.MAX, [None] * n, None)
    # integer sums that wrap: two rows carry the values (one row: the last alone)
    for t, a, b in ((INT64, 2 ** 63 - 1, 2 ** 63 - 1), (INT32, 2 ** 31 - 1, 2 ** 31 - 1), (UINT32, 2 ** 32 - 1, 2 ** 32 - 1), (UINT64, 2 ** 64 - 1, 2)):
        vals = _planted(n, 1 if n > 2 else None, [(0, a), (-1, b)])
        add("sum_%s_wrap" % NAME[t], t, ss.SUM, vals, fold_sum(t, vals))
        if t == INT32:                # past 2^31 into an INT64 result
            add("sum_i32_into_i64", t, ss.SUM, vals, fold_sum(t, vals, INT64), INT64, otype=INT64)
    add("sum_i64_null", INT64, ss.SUM, [None] * n, None, INT64)
    for t in FLOATS:
        big = DBL_MAX if t == DOUBLE else FLT_MAX
        inf, nan = NP[t](math.inf), (NAN64 if t == DOUBLE else NAN32)
        fin = [NP[t](v) for v in (0.25, -3.5, 1024.0, 0.1 if t == DOUBLE else 0.125)]
        base = [fin[i % 4] for i in range(n)]
        for tag, specials in (("pinf_first", [(0, inf)]), ("pinf_last", [(-1, inf)]), ("ninf_first", [(0, -inf)]), ("ninf_last", [(-1, -inf)]),
                              ("both_inf", [(0, inf), (-1, -inf)]), ("nan_first", [(0, nan)]), ("nan_last", [(-1, nan)])):
            if tag == "both_inf" and n == 1:
                continue
            vals = list(base)
            for where, v in specials:
                vals[where] = v
            add("sum_%s_%s" % (NAME[t], tag), t, ss.SUM, vals, fold_sum(t, vals))
        if n > 1:
            vals = _planted(n, None, [(0, big), (-1, big)])
            add("sum_%s_overflow" % NAME[t], t, ss.SUM, vals, fold_sum(t, vals))
        add("sum_%s_finite" % NAME[t], t, ss.SUM, base, fold_sum(t, base), exact=t != DOUBLE)
        add("sum_%s_null" % NAME[t], t, ss.SUM, [None] * n, None)
        payload = NAN64_PAYLOAD if t == DOUBLE else f32_of_bits(0xFFC00001)
        add("first_%s_nan" % NAME[t], t, ss.FIRST, _planted(n, NP[t](1.5), [(0, payload)]), payload, moved=True)
        add("last_%s_nan" % NAME[t], t, ss.LAST, _planted(n, NP[t](1.5), [(-1, payload)]), payload, moved=True)
    return cols


AGG_SHAPES = ("scalar", "direct", "partitions", "dense")
GROUPS = 3            # group keys 0, 1, 2 dealt round-robin: every group holds the same column pattern over its own rows


class AggCase(object):
    """`per_plan` aggregations over one input.  scalar: ScalarAggregate, the first aggregation on slot 0 (registers) -- with `lds` the
    aggregations are preceded by 8 COUNTs, so they sit on slots 8.. (LDS).  Group shapes: the key `g` has GROUPS values; group k's rows
    are k, k + GROUPS, ... and hold the column pattern of agg_columns(rows of the group), so every group expects the same row."""

    def __init__(self, shape, n, columns, lds=False):
        self.shape, self.n, self.columns, self.lds = shape, n, columns, lds
        self.name = "agg-%s-%d-%s%s" % (shape, n, columns[0].name, "-lds" if lds else "")

    def groups(self):
        return 1 if self.shape == "scalar" else min(GROUPS, self.n)

    def plain(self):
        """Every aggregation is a field of the plain scatter's record: the stage may take dense slots."""
        return not any(c.widens() for c in self.columns)

    def view(self):
        g = self.groups()
        attrs, data = [], []
        if self.shape != "scalar":
            attrs.append(ss.Attribute("g", INT32, ss.NOT_NULLABLE))
            data.append(ss.Column(np.arange(self.n, dtype=np.int32) % g, None))
        attrs.append(ss.Attribute("one", INT32, ss.NOT_NULLABLE))
        data.append(ss.Column(np.ones(self.n, np.int32), None))
        for c in self.columns:
            vals = [None] * self.n
            for k in range(g):
                rows = list(range(k, self.n, g))
                for r, v in zip(rows, c.per_group[k]):
                    vals[r] = v
            d, z = column_of(c.t, vals)
            attrs.append(ss.Attribute(c.name, c.t, ss.NULLABLE))
            data.append(ss.Column(d, z))
        return ss.View(ss.TupleSchema(attrs), data)

    def op(self, view=None):
        view = view if view is not None else self.view()
        spec = ss.AggregationSpecification()
        if self.lds:
            for i in range(8):
                spec.AddAggregation(ss.COUNT, "one", "cnt%d" % i)
        for c in self.columns:
            if c.otype is not None:
                spec.AddAggregationWithDefinedOutputType(c.kind, c.name, "r_" + c.name, c.otype)
            else:
                spec.AddAggregation(c.kind, c.name, "r_" + c.name)
        if self.shape == "scalar":
            return ss.ScalarAggregate(spec, ss.ScanView(view))
        return ss.GroupAggregate(ss.ProjectNamedAttributes(["g"]), spec, None, ss.ScanView(view))

    def expected(self):
        """-> (schema, cols sorted by key, moved, inexact [bool])"""
        g = self.groups()
        schema, cols, moved, inexact = [], [], [], []
        if self.shape != "scalar":
            schema.append(("g", INT32, 0)); cols.append((np.arange(g, dtype=np.int32), None)); moved.append(True); inexact.append(False)
        if self.lds:
            for i in range(8):
                counts = [len(range(k, self.n, g)) for k in range(g)]
                schema.append(("cnt%d" % i, UINT64, 0)); cols.append((np.array(counts, np.uint64), None)); moved.append(True); inexact.append(False)
        for c in self.columns:
            schema.append(("r_" + c.name, c.want_type, 1))
            cols.append(column_of(c.want_type, [c.want_per_group[k] for k in range(g)]))
            moved.append(c.moved); inexact.append(not c.exact)
        return schema, cols, moved, inexact


AGG_OPTIONS = {
    "scalar": {"grid_limit": 2},
    "direct": {"grid_limit": 2, "group_partition": 0, "group_capacity": 64, "group_local": 1, "group_dense": 0},
    "partitions": {"grid_limit": 2, "group_partition": 2, "part_n": 16, "group_slab": 0, "group_dense": 0},
    "dense": {"grid_limit": 2, "group_dense": 1, "dense_min_rows": 1},
}
AGGS_PER_PLAN = 10        # key + 10 values + 10 NULL masks: within the 24 record fields of the plain scatter, which dense slots need (lower.cpp)


COMPILED_AGGS = ("min_u64_first", "max_i64_last", "min_f64_last", "sum_i64_wrap", "sum_f64_pinf_first", "sum_f64_ninf_last", "sum_f64_both_inf",
                 "sum_f64_overflow", "sum_f64_finite", "last_f64_nan")


def agg_cases(shape, n, only=None):
    """Every column of agg_columns (or those named in `only`) in plans of AGGS_PER_PLAN aggregations; in a group shape each group gets
    the pattern for ITS row count."""
    g = 1 if shape == "scalar" else min(GROUPS, n)
    sizes = [len(range(k, n, g)) for k in range(g)]
    per_size = {s: agg_columns(s) for s in set(sizes)}
    names = [c.name for c in per_size[min(sizes)]]         # (a 1-row group has no two-value columns: keep what every group has)
    cols = []
    for name in names:
        c0 = next(c for c in per_size[sizes[0]] if c.name == name)
        c = AggColumn(c0.name, c0.t, c0.kind, None, None, c0.want_type, c0.exact, c0.moved, c0.otype)
        c.per_group = [next(x for x in per_size[s] if x.name == name).values for s in sizes]
        c.want_per_group = [next(x for x in per_size[s] if x.name == name).want for s in sizes]
        cols.append(c)
    if only is not None:
        cols = [c for c in cols if c.name in only]
        return [AggCase(shape, n, cols)]
    # a stage with a SUM into a wider type or a FIRST / LAST has no plain scatter and cannot take dense slots -- plans of their own
    wide = [c for c in cols if c.widens()]
    cols = [c for c in cols if not c.widens()]
    cases = [AggCase(shape, n, part[i:i + AGGS_PER_PLAN]) for part in (cols, wide) for i in range(0, len(part), AGGS_PER_PLAN)]
    if shape == "scalar":
        cases += [AggCase(shape, n, cols[i:i + AGGS_PER_PLAN], lds=True) for i in range(0, len(cols), AGGS_PER_PLAN)]
    return cases


def ulp_of(got, want):
    """Distance in ULPs between two finite doubles."""
    def key(v):
        b = int(np.array([v], np.float64).view(np.int64)[0])
        return -(2 ** 63) - b if b < 0 else b
    return abs(key(got) - key(want))


def same_aggregates(got, want, moved, inexact, where=""):
    """`same`, with the inexact (finite float SUM) columns held to 1 ULP of the exactly rounded sum."""
    exact = [i for i in range(len(want)) if not inexact[i]]
    same([got[i] for i in exact], [want[i] for i in exact], [moved[i] for i in exact], where)
    for i in (i for i in range(len(want)) if inexact[i]):
        (gd, gz), (wd, wz) = got[i], want[i]
        assert np.array_equal(np.zeros(len(gd), bool) if gz is None else gz, wz), (where, i)
        for r in range(len(wd)):
            if not wz[r]:
                assert ulp_of(gd[r], wd[r]) <= 1, "%s column %d row %d: got %r, math.fsum %r" % (where, i, r, gd[r], wd[r])


# ---- every case, by family --------------------------------------------------------------------------------------------------------------------
def family_forms(family, t):
    if family == "arithmetic":
        return arithmetic_family(t)
    if family == "division":
        return division_family(t)
    if family == "bitwise":
        return bitwise_family(t)
    if family == "shift":
        return shift_family(t)
    if family == "comparison":
        return comparison_family(*t)
    if family == "cast":
        return cast_family(t)
    if family == "math":
        return math_family(t)
    raise KeyError(family)


FAMILIES = {"arithmetic": NUMERIC, "division": NUMERIC, "bitwise": INTS, "shift": INTS, "comparison": tuple(COMPARE_PAIRS), "cast": NUMERIC, "math": NUMERIC}


def type_id(t):
    return "-".join(NAME[x] for x in t) if isinstance(t, tuple) else NAME[t]


# ---- the compiled legs: column o constant forms packed into one plan per family (the constants hiprtc folds) ----------------------------------
def constant_forms(name, t, consts, ops_of, extra=None):
    """One plan over the NULLABLE pool column of type t: op(x, c) for every (constant type, constant) of `consts` and every operator."""
    cols = single(t, POOL[t], True)
    x = cols[0][0]
    outs = []
    for k, (tc, c) in enumerate(consts):
        outs += [make("%s_%d" % (nm, k), b, [x, Const(tc, c)], rt, fn, nulling) for nm, b, rt, fn, nulling in ops_of(tc)]
    if extra:
        outs += extra(x)
    return Case(name + "-compiled", cols, outs)


def compiled_cases():
    """{name: case} -- one specialised kernel each, about one per family; a compilation costs a second or so per output, so each plan
    holds the few forms whose folding can go wrong."""
    i64 = lambda *vs: [(INT64, v) for v in vs]      # noqa: E731

    def some(case, names):
        return Case(case.name, case.cols, [o for o in case.outs if o.alias in names])
    x64 = Col("x", DOUBLE, True)
    cases = [
        constant_forms("arith-i64", INT64, i64(-1, 3037000500), lambda tc: arithmetic_ops(INT64)),
        constant_forms("arith-f64", DOUBLE, [(DOUBLE, F64(math.inf)), (DOUBLE, F64(4.9e-324))], lambda tc: arithmetic_ops(DOUBLE)),
        constant_forms("div-i64", INT64, i64(-1, 0), lambda tc: division_ops(INT64)),
        constant_forms("divs-i32", INT32, [(INT32, -1)], lambda tc: division_ops(INT32, True)),
        constant_forms("div-f64", DOUBLE, [(DOUBLE, F64(-0.0)), (DOUBLE, F64(3.0))], lambda tc: division_ops(DOUBLE)),
        constant_forms("bits-i64", INT64, i64(-2 ** 63), lambda tc: bitwise_ops(INT64), lambda x: [make("bnot", ss.BitwiseNot, [x], INT64, lambda a: wrap(INT64, ~a))]),
        constant_forms("shift-i64", INT64, i64(0, 1, 63), lambda tc: shift_ops(INT64)),
        constant_forms("cmp-i64-u64", INT64, [(UINT64, 2 ** 63)], lambda tc: comparison_ops(INT64, tc)),
        constant_forms("cmp-f64", DOUBLE, [(DOUBLE, NAN64)], lambda tc: comparison_ops(DOUBLE, tc)),
        Case("cast-u64-compiled", single(UINT64, POOL[UINT64], True), cast_outs(UINT64, Col("x", UINT64, True))),
        Case("cast-f64-compiled", single(DOUBLE, POOL[DOUBLE], True), cast_outs(DOUBLE, x64)),
        some(Case("math-f64-compiled", single(DOUBLE, POOL[DOUBLE], True), math_outs(DOUBLE, x64)), ("abs", "round", "round2i", "ceil2i", "floor2i", "nrm")),
        some(selection_cases(DOUBLE)[0], ("if", "nif", "ifnull_k", "case", "in")),
        logic_cases()[0],
    ]
    return {c.name: c for c in cases}
