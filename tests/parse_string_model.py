"""A small model of the reference's ParseString (expression_evaluators.h:73-78 over types_infrastructure.cc:154-205 and
utils/strings/numbers.cc:565-829), the expected values of tests/test_parse_string_*.py.

parse(to_type, value) -> (result, failed): `value` is the STRING's bytes; what is parsed is the value cut at its first 0x00 byte.
Integers and BOOL are written out from the rules; DOUBLE / FLOAT ask libc's strtod / strtof -- the reference's own parser -- through
ctypes and apply the consumed-everything rule.  A failed parse has a value too (what ParseStringQuiet yields): the conversion of
the digits in front of the first bad byte, max / min after an overflow, false for BOOL (the reference leaves that one
uninitialised; the library says false), whatever strtod returned.

fast_path(to_type, value) -> True when a FLOAT / DOUBLE value lies on the device's exact fast path (include/ssgpu.h "PARSE_STRING"),
False when the host has to resolve it, None for the empty value (a failure nobody parses).  The tests count with it."""
import ctypes
import ctypes.util
import struct

import supersonic_amd as ss

ISSPACE = b" \t\n\v\f\r"
LIMITS = {ss.INT32: (-2 ** 31, 2 ** 31 - 1), ss.UINT32: (0, 2 ** 32 - 1), ss.INT64: (-2 ** 63, 2 ** 63 - 1), ss.UINT64: (0, 2 ** 64 - 1)}
WINDOW = 64

_libc = ctypes.CDLL(ctypes.util.find_library("c") or "libc.so.6")
_libc.strtod.restype = ctypes.c_double
_libc.strtod.argtypes = [ctypes.c_void_p, ctypes.POINTER(ctypes.c_void_p)]
_libc.strtof.restype = ctypes.c_float
_libc.strtof.argtypes = [ctypes.c_void_p, ctypes.POINTER(ctypes.c_void_p)]


def cut(value):
    value = bytes(value)
    k = value.find(b"\0")
    return value if k < 0 else value[:k]


def parse_int(to_type, value):
    lo, hi = LIMITS[to_type]
    s = cut(value).strip(ISSPACE)
    if not s:
        return 0, True
    negative = s[:1] == b"-"
    if s[:1] in (b"-", b"+"):
        s = s[1:]
        if not s:
            return 0, True
    if negative and lo == 0:
        return 0, True
    v = 0
    for c in s:
        if not 48 <= c <= 57:
            return v, True
        d = c - 48
        if negative:
            if v < -((-lo) // 10):       # vmin / 10, truncated towards zero
                return lo, True
            v *= 10
            if v < lo + d:
                return lo, True
            v -= d
        else:
            if v > hi // 10:
                return hi, True
            v *= 10
            if v > hi - d:
                return hi, True
            v += d
    return v, False


def parse_bool(value):
    s = cut(value).strip(b" \t\r")
    word = bytes(c | 0x20 if 65 <= c <= 90 else c for c in s)
    if word in (b"true", b"yes"):
        return True, False
    if word in (b"false", b"no"):
        return False, False
    return False, True


def parse_float(to_type, value):
    s = cut(value)
    buf = ctypes.create_string_buffer(s)            # NUL-terminated copy
    end = ctypes.c_void_p()
    base = ctypes.addressof(buf)
    v = (_libc.strtof if to_type == ss.FLOAT else _libc.strtod)(base, ctypes.byref(end))
    k = (end.value or base) - base
    if k != 0:
        while k < len(s) and s[k] in ISSPACE:
            k += 1
    return v, not (len(s) > 0 and k == len(s))


def parse(to_type, value):
    if to_type == ss.BOOL:
        return parse_bool(value)
    if to_type in (ss.FLOAT, ss.DOUBLE):
        return parse_float(to_type, value)
    return parse_int(to_type, value)


def bits(to_type, v):
    """The value's device representation, for bit-exact comparisons (NaN == NaN, -0.0 != 0.0)."""
    if to_type == ss.FLOAT:
        return struct.unpack("<I", struct.pack("<f", v))[0]
    if to_type == ss.DOUBLE:
        return struct.unpack("<Q", struct.pack("<d", v))[0]
    if to_type == ss.BOOL:
        return int(bool(v))
    return int(v) & (0xFFFFFFFF if to_type in (ss.INT32, ss.UINT32) else 0xFFFFFFFFFFFFFFFF)


def fast_path(to_type, value):
    s = cut(value)
    if not s:
        return None
    s = s.strip(ISSPACE)
    if s[:1] in (b"-", b"+"):
        s = s[1:]
    if not s:
        return False
    rest = s.lstrip(b"0")
    if len(rest) > WINDOW:
        return False
    digits = len(rest) < len(s)
    i, w, nsig, frac = 0, 0, 0, 0
    while i < len(rest) and 48 <= rest[i] <= 57:
        w, nsig, digits, i = w * 10 + rest[i] - 48, nsig + 1, True, i + 1
    if i < len(rest) and rest[i:i + 1] == b".":
        i += 1
        while i < len(rest) and 48 <= rest[i] <= 57:
            if nsig or rest[i] != 48:
                w, nsig = w * 10 + rest[i] - 48, nsig + 1
            frac, digits, i = frac + 1, True, i + 1
    if not digits or nsig > 19:
        return False
    ex = 0
    if i < len(rest) and rest[i:i + 1] in (b"e", b"E"):
        i += 1
        eneg = rest[i:i + 1] == b"-"
        if rest[i:i + 1] in (b"-", b"+"):
            i += 1
        j = i
        while i < len(rest) and 48 <= rest[i] <= 57:
            i += 1
        if not 1 <= i - j <= 4:
            return False
        ex = -int(rest[j:i]) if eneg else int(rest[j:i])
    if i != len(rest):
        return False
    e10 = ex - frac
    if to_type == ss.FLOAT:
        return w <= 2 ** 24 and -10 <= e10 <= 10
    return w <= 2 ** 53 and -22 <= e10 <= 22
