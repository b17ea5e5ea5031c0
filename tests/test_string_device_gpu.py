"""STRING columns of View files encoded on the device (FileInput(..., device_strings=True), BlockFromColumns): the block's own
order-preserving dictionary, its codes, plans over such blocks (dictionary extended by the plan's constants and recoded on the
device), the write back to the file format.  The expected answer always comes from the host reader (read_view_file) of the
same file."""
import ctypes as C
import struct

import numpy as np
import pytest

import supersonic_amd as ss
from oracle import oracle
from helpers import to_cols, assert_cols_equal, sort_rows

NA = ss.NamedAttribute
pytestmark = pytest.mark.gpu


def schema3():
    return ss.TupleSchema([ss.Attribute("s", ss.STRING, ss.NULLABLE), ss.Attribute("k", ss.INT32), ss.Attribute("t", ss.STRING)])


def pool(rng, n, maxlen=14):
    out = set()
    while len(out) < n:
        out.add(bytes(rng.integers(0, 256, rng.integers(0, maxlen + 1), dtype=np.uint8)))
    return np.array(sorted(out), dtype=object)


def write(path, schema, cols):
    out = ss.FileOutput(path)
    out.Write(ss.View(schema, cols))
    out.Finalize()


def make_file(tmp_path, n, seed=1, distinct=500, name="in.ssv", values=None):
    rng = np.random.default_rng(seed)
    vals = values if values is not None else pool(rng, distinct)
    s = vals[rng.integers(0, len(vals), n)] if n else np.zeros(0, dtype=object)
    t = vals[rng.integers(0, len(vals), n)] if n else np.zeros(0, dtype=object)
    cols = [ss.Column(s, rng.random(n) < 0.1), rng.integers(-50, 50, n).astype(np.int32), t]
    path = str(tmp_path / name)
    write(path, schema3(), cols)
    return path


def raw_codes(ctx, view):
    """The block's cells as they are on the device (codes and NULL masks), through a plan that copies them."""
    plan = ss.Plan(ss.Project(ss.ProjectAllAttributes(), ss.ScanView(view)), ctx)
    res = plan.run()
    rows = plan.lib.ssgpu_result_row_count(res)
    out = []
    for i in range(view.schema().attribute_count()):
        a = view.schema().attribute(i)
        dp, npn = C.c_void_p(), C.c_void_p()
        ctx.check(plan.lib.ssgpu_result_column(res, i, C.byref(dp), C.byref(npn)))
        dt = np.int32 if a.type() == ss.STRING else ss.api._NP[a.type()]
        data = np.frombuffer(C.string_at(dp, rows * np.dtype(dt).itemsize), dt).copy() if rows else np.zeros(0, dt)
        nulls = None
        if a.is_nullable():
            nulls = (np.frombuffer(C.string_at(npn, rows), np.uint8) != 0) if rows else np.zeros(0, bool)
        out.append((data, nulls))
    assert plan.strings.handle.value == view.dictionary.handle.value     # no constants: the plan scans the block's own codes
    return out


def check_block(ctx, dev, host):
    """dictionary == sorted distinct non-NULL values of every STRING column; decoded codes == the host reader's values."""
    d = dev.dictionary
    assert d is not None
    schema = host.schema()
    want = set()
    for i in range(schema.attribute_count()):
        if schema.attribute(i).type() == ss.STRING:
            c = host.column(i)
            want.update(v for j, v in enumerate(c.data) if c.is_null is None or not c.is_null[j])
    values = d.values
    assert values == sorted(want)
    got = raw_codes(ctx, dev)
    for i in range(schema.attribute_count()):
        c = host.column(i)
        data, nulls = got[i]
        if c.is_null is not None:
            assert np.array_equal(nulls, c.is_null)
        if schema.attribute(i).type() != ss.STRING:
            assert np.array_equal(data, c.data)
            continue
        if c.is_null is not None:
            assert not data[c.is_null].any(), "a NULL row's code is 0"
        live = np.ones(len(data), bool) if c.is_null is None else ~c.is_null
        assert [values[x] for x in data[live]] == list(c.data[live])
    return got


@pytest.mark.parametrize("n", [0, 1, 8192, 8193, 1000003])
def test_file_to_device_block(gpu_ctx, tmp_path, n):
    src = make_file(tmp_path, n, distinct=50000 if n > 100000 else 300)
    dev = ss.FileInput(schema3(), src, gpu_ctx, device_strings=True)
    assert isinstance(dev, ss.BlockView) and dev.row_count() == n
    check_block(gpu_ctx, dev, ss.read_view_file(schema3(), src))
    copy = str(tmp_path / "copy.ssv")
    dev.write_file(copy)                                   # file -> block -> file: the same bytes
    assert open(copy, "rb").read() == open(src, "rb").read()


def adversarial(kind, rng):
    if kind == "edge":
        vals = [b"", b"a", b"a\x00", b"a\x00\x00", b"\x00", b"\x7f", b"\x80", b"\xff", b"\xff\xff", b"b"]
        for plen in (8, 16, 40):
            stem = bytes(rng.integers(0, 256, plen, dtype=np.uint8))
            vals += [stem, stem + b"\x00", stem + b"\x01", stem + b"\xfe", stem + b"\xff", stem[:-1] + b"\xff"]
        vals.append(bytes(rng.integers(0, 256, 200 * 1024, dtype=np.uint8)))     # one 200 KiB value
        vals.append(b"http://www.example.com/index/" + b"x" * 11)
        vals.append(b"http://www.example.com/index/" + b"x" * 10 + b"y")
        return np.array(vals, dtype=object), 20000
    if kind == "distinct":
        return np.array([b"v%07d" % i + bytes([i % 251]) for i in range(1000000)], dtype=object), 1000000
    return np.array([b"hot", b"", b"hot\x00"], dtype=object), 1000000


@pytest.mark.parametrize("kind", ["edge", "distinct", "hot"])
def test_adversarial_values(gpu_ctx, tmp_path, kind):
    rng = np.random.default_rng(7)
    vals, n = adversarial(kind, rng)
    if kind == "distinct":
        s, t = vals[rng.permutation(n)], vals.copy()          # every row distinct within a column
    else:
        s, t = vals[rng.integers(0, len(vals), n)], vals[rng.integers(0, len(vals), n)]
        t[:len(vals)] = vals                                  # every value present at least once
    src = str(tmp_path / "adv.ssv")
    write(src, schema3(), [ss.Column(s, rng.random(n) < 0.05), np.arange(n, dtype=np.int32), t])
    dev = ss.FileInput(schema3(), src, gpu_ctx, device_strings=True)
    check_block(gpu_ctx, dev, ss.read_view_file(schema3(), src))


@pytest.fixture(scope="module")
def big(tmp_path_factory):
    src = make_file(tmp_path_factory.mktemp("big"), 1 << 20, seed=3, distinct=20000)
    return src, ss.read_view_file(schema3(), src)


def run_both(ctx, big, query, max_rows=1 << 21):
    src, host = big
    dev = ss.FileInput(schema3(), src, ctx, device_strings=True)
    plan = ss.Plan(query(dev), ctx)
    plan.run()
    got = to_cols(plan.fetch())
    _schema, want = oracle.run(query(host), max_rows)
    return got, want


def test_group_aggregate_on_string_key(gpu_ctx, big):
    spec = ss.AggregationSpecification().AddAggregation(ss.MIN, "s", "mn").AddAggregation(ss.MAX, "s", "mx").AddAggregation(ss.COUNT, "s", "c")
    got, want = run_both(gpu_ctx, big, lambda v: ss.GroupAggregate(ss.ProjectNamedAttributes(["t"]), spec, None, ss.ScanView(v)))
    assert_cols_equal(sort_rows(got), sort_rows(want), context="GroupAggregate over device-encoded STRING")


@pytest.mark.parametrize("present", [True, False])
@pytest.mark.parametrize("op", ["less", "equal"])
def test_filter_with_constants(gpu_ctx, big, op, present):
    values = sorted(set(big[1].column(2).data))
    const = values[len(values) // 2] if present else values[len(values) // 2] + b"\x00"   # not in the file: forces a recode
    assert present == (const in set(values))
    pred = (lambda: ss.Less(NA("t"), ss.ConstString(const))) if op == "less" else (lambda: ss.Equal(NA("s"), ss.ConstString(const)))
    got, want = run_both(gpu_ctx, big, lambda v: ss.Filter(pred(), ss.ProjectAllAttributes(), ss.ScanView(v)))
    assert len(want[0][0]) > 0 or op == "equal"
    assert_cols_equal(got, want, context="Filter %s %s" % (op, present))


@pytest.mark.parametrize("order", [ss.ASCENDING, ss.DESCENDING])
def test_sort_on_string_key(gpu_ctx, big, order):
    got, want = run_both(gpu_ctx, big, lambda v: ss.Sort(ss.SortOrder().add("s", order), None, 0, ss.ScanView(v)))
    assert np.array_equal(got[0][1], want[0][1]) and list(got[0][0]) == list(want[0][0])    # keys (NULLs included) in order
    assert_cols_equal(sort_rows(got), sort_rows(want), context="Sort")


def test_determinism_and_permutation(gpu_ctx, tmp_path):
    src = make_file(tmp_path, 300000, seed=5, distinct=40000)
    a = ss.FileInput(schema3(), src, gpu_ctx, device_strings=True)
    b = ss.FileInput(schema3(), src, gpu_ctx, device_strings=True)
    ca, cb = raw_codes(gpu_ctx, a), raw_codes(gpu_ctx, b)
    assert all(np.array_equal(x[0], y[0]) for x, y in zip(ca, cb))
    host = ss.read_view_file(schema3(), src)
    perm = np.random.default_rng(1).permutation(host.row_count())
    cols = [ss.Column(host.column(0).data[perm], host.column(0).is_null[perm]), host.column(1).data[perm], host.column(2).data[perm]]
    psrc = str(tmp_path / "perm.ssv")
    write(psrc, schema3(), cols)
    p = ss.FileInput(schema3(), psrc, gpu_ctx, device_strings=True)
    assert p.dictionary.values == a.dictionary.values
    assert np.array_equal(raw_codes(gpu_ctx, p)[2][0], ca[2][0][perm])


def arrow(col, nulls=None):
    vals = [b"" if (nulls is not None and nulls[j]) else v for j, v in enumerate(col)]
    offs = np.zeros(len(vals) + 1, np.int64)
    offs[1:] = np.cumsum([len(v) for v in vals])
    return offs, np.frombuffer(b"".join(vals), np.uint8), nulls


def test_host_columns_entry_point(gpu_ctx, tmp_path):
    src = make_file(tmp_path, 50000, seed=8, distinct=3000)
    host = ss.read_view_file(schema3(), src)
    blk = ss.BlockFromColumns(schema3(), [arrow(host.column(0).data, host.column(0).is_null), host.column(1).data,
                                          arrow(host.column(2).data)], gpu_ctx)
    dev = ss.FileInput(schema3(), src, gpu_ctx, device_strings=True)
    assert blk.dictionary.values == dev.dictionary.values
    a, b = raw_codes(gpu_ctx, blk), raw_codes(gpu_ctx, dev)
    for x, y in zip(a, b):
        assert np.array_equal(x[0], y[0])
    check_block(gpu_ctx, blk, host)


def test_corrupt_string_file_is_an_io_error(gpu_ctx, tmp_path):
    schema = ss.TupleSchema([ss.Attribute("s", ss.STRING)])
    for lens, payload in (([3, 1 << 40], b"abc"), ([5, 5], b"abcdefgh"), ([2], b"")):
        path = str(tmp_path / "bad.ssv")
        with open(path, "wb") as f:
            f.write(struct.pack("<Q", len(lens)) + np.array(lens, np.uint64).tobytes() + payload)
        with pytest.raises(ss.SupersonicException) as e:
            ss.FileInput(schema, path, gpu_ctx, device_strings=True)
        assert e.value.return_code == ss.ERROR_GENERAL_IO_ERROR
    good = str(tmp_path / "good.ssv")
    write(good, schema, [np.array([b"x", b"yy"], dtype=object)])
    assert ss.FileInput(schema, good, gpu_ctx, device_strings=True).dictionary.values == [b"x", b"yy"]


def test_plan_over_another_blocks_dictionary(gpu_ctx, tmp_path):
    rng = np.random.default_rng(11)
    vals = pool(rng, 400)
    a_src = make_file(tmp_path, 30000, seed=12, name="a.ssv", values=vals)
    sub_src = make_file(tmp_path, 20000, seed=13, name="sub.ssv", values=vals[::3])
    new_src = make_file(tmp_path, 20000, seed=14, name="new.ssv", values=np.array(list(vals[:50]) + [b"\xffnot in a"], dtype=object))

    def query(v):
        return ss.Filter(ss.Less(NA("t"), ss.ConstString(vals[200] + b"\x00")), ss.ProjectAllAttributes(), ss.ScanView(v))
    a = ss.FileInput(schema3(), a_src, gpu_ctx, device_strings=True)
    plan = ss.Plan(query(a), gpu_ctx)
    sub = ss.FileInput(schema3(), sub_src, gpu_ctx, device_strings=True)
    assert sub.dictionary.values != a.dictionary.values
    plan.run(sub)                                            # its values are all in the plan's dictionary: recoded, then run
    _s, want = oracle.run(query(ss.read_view_file(schema3(), sub_src)), 1 << 20)
    assert_cols_equal(to_cols(plan.fetch()), want, context="run over another block's dictionary")
    with pytest.raises(ss.SupersonicException) as e:         # a value the plan's dictionary lacks: refused, never run
        plan.run(ss.FileInput(schema3(), new_src, gpu_ctx, device_strings=True))
    assert e.value.return_code == ss.ERROR_INVALID_ARGUMENT_VALUE
    plan.run(a)
    _s, want = oracle.run(query(ss.read_view_file(schema3(), a_src)), 1 << 20)
    assert_cols_equal(to_cols(plan.fetch()), want, context="the plan's own block after another")
