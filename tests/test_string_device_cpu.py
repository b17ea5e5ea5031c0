"""STRING dictionaries without a GPU: ssgpu_dict_extend (base U strings, with the order-preserving remap of the base's codes),
and the device-block entry points of STRING columns refusing a bind-only context."""
import ctypes as C

import numpy as np
import pytest

import supersonic_amd as ss
from supersonic_amd import _lib as L


def test_extend_is_sorted_unique_and_remap_preserves_order():
    base = ss.StringDictionary([b"m", b"a", b"zz", b"a\x00", b"\xff", b""])
    ext, remap = base.extend([b"b", b"a", b"a\x00\x00", b"\x80", b"b", b"zz", b"aa"])
    vals = ext.values
    assert vals == sorted({b"m", b"a", b"zz", b"a\x00", b"\xff", b"", b"b", b"a\x00\x00", b"\x80", b"aa"})
    old = base.values
    assert len(remap) == len(old)
    assert [vals[remap[c]] for c in range(len(old))] == old
    assert all(remap[i] < remap[i + 1] for i in range(len(remap) - 1))


@pytest.mark.parametrize("extra", [[], [b"a", b"m", b""], [b"m", b"m"]])
def test_extend_by_nothing_new_is_the_identity(extra):
    base = ss.StringDictionary([b"m", b"a", b"", b"a\x00"])
    ext, remap = base.extend(extra)
    assert ext.values == base.values
    assert list(remap) == list(range(len(base)))


def test_extend_of_an_empty_dictionary():
    ext, remap = ss.StringDictionary([]).extend([b"q", b"p", b"q"])
    assert ext.values == [b"p", b"q"] and len(remap) == 0


def test_block_entry_points_need_a_device(tmp_path):
    lib = L.load()
    ctx = ss.Context(-1)
    schema = ss.TupleSchema([ss.Attribute("s", ss.STRING, ss.NULLABLE), ss.Attribute("k", ss.INT32)])
    path = str(tmp_path / "s.ssv")
    out = ss.FileOutput(path)
    out.Write(ss.View(schema, [ss.Column(np.array([b"a", b"b"], dtype=object), np.array([False, True])), np.array([1, 2], np.int32)]))
    out.Finalize()
    with pytest.raises(ss.SupersonicException) as e:
        ss.FileInput(schema, path, ctx, device_strings=True)
    assert e.value.return_code == ss.ERROR_NO_DEVICE
    with pytest.raises(ss.SupersonicException) as e:
        ss.BlockFromColumns(schema, [(np.array([0, 1, 1], np.int64), np.frombuffer(b"a", np.uint8), np.array([False, True])),
                                     np.array([1, 2], np.int32)], ctx)
    assert e.value.return_code == ss.ERROR_NO_DEVICE
    codes = np.zeros(2, np.int32)
    remap = (C.c_int32 * 1)(0)
    assert lib.ssgpu_codes_recode(ctx.handle, codes.ctypes.data, None, 2, remap, 1, codes.ctypes.data) == ss.ERROR_NO_DEVICE
    assert not lib.ssgpu_block_dict(None)


def test_file_input_default_stays_on_the_host(tmp_path):
    schema = ss.TupleSchema([ss.Attribute("s", ss.STRING), ss.Attribute("k", ss.INT32)])
    path = str(tmp_path / "h.ssv")
    out = ss.FileOutput(path)
    out.Write(ss.View(schema, [np.array([b"x", b""], dtype=object), np.array([3, 4], np.int32)]))
    out.Finalize()
    v = ss.FileInput(schema, path, ss.Context(-1))
    assert isinstance(v, ss.View) and list(v.column(0).data) == [b"x", b""]
