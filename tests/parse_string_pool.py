"""The values the PARSE_STRING tests parse (tests/test_parse_string_cpu.py, tests/test_parse_string_gpu.py): built once, deterministic.

general_pool()      about 4000 distinct byte strings for every target type: the reference's own rows, every integer limit and its
                    neighbours, signs and spaces in every place, 0x00 and bytes >= 0x80, the BOOL words, random digit strings, and
                    the THRESHOLD values: one number padded to the lengths at which the table kernel changes form (one lane per value
                    up to 128 bytes, a wave per longer value in steps of 64 x 16 = 1024 bytes).
fast_decimals(t)    2000 plain decimals that lie on the device's exact fast path for FLOAT / DOUBLE by construction.
hard_floats()       values that leave it, each for a stated reason."""
import json
import os
import random

import supersonic_amd as ss

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = json.load(open(os.path.join(ROOT, "tests", "golden", "parse_string_cases.json")))
SPACES = [b" ", b"\t", b"\n", b"\v", b"\f", b"\r"]
THRESHOLD_LENGTHS = [127, 128, 129, 1023, 1024, 1025, 5000]


def threshold_values():
    out = []
    for n in THRESHOLD_LENGTHS:
        for core in (b"7", b"-12", b"+2147483647", b"18446744073709551616", b"true", b"1.5e3", b"12x"):
            k = n - len(core)
            out += [b" " * k + core, core + b" " * k, b" " * (k // 2) + core + b"\t" * (k - k // 2)]
            if core[:1] in b"-+":
                out.append(core[:1] + b"0" * k + core[1:])
            elif core[:1].isdigit():
                out.append(b"0" * k + core)
        out.append(b"9" * n)                                   # digits only: an overflow in every integer type
        out.append(b"0" * (n - 1) + b".")                      # a floating zero that is no integer
    out.append(b"1" + b"0" * 1500 + b"x" + b"0" * 3)         # the only non-digit sits in the value's last 16-byte word
    out.append(b"0" * 2000 + b"5" + b"\x00" + b"9" * 100)      # a 0x00 in the second wave step: what follows does not count
    out.append(b" " * 1030 + b"42" + b"\x00" + b"x" * 50)
    out.append(b" " * 200 + b"7")
    out.append(b"0" * 300 + b"12")
    out.append(b"0." + b"0" * 200 + b"1")                      # a legal decimal whose digits lie past the window one lane walks
    out.append(b"1" + b"0" * 200 + b"e-200")
    return out


def general_pool():
    rng = random.Random(437)
    pool = [r["input"].encode() for r in GOLDEN["evaluation"] if r["input"] is not None]
    for lo, hi in ((-2 ** 31, 2 ** 31 - 1), (0, 2 ** 32 - 1), (-2 ** 63, 2 ** 63 - 1), (0, 2 ** 64 - 1)):
        for v in (lo - 1, lo, lo + 1, hi - 1, hi, hi + 1):
            text = str(abs(v)).encode()
            for form in (text, b"+" + text, b"-" + text):
                pool.append(form)
                for sp in SPACES:
                    pool += [sp + form, form + sp, sp + form + sp]
    pool += [b"+", b"-", b"", b" ", b"- 5", b"5 -", b"0x10", b"010", b"-0", b"+0", b"00", b"12 3", b"1_000", b"\xd9\xa1\xd9\xa2", b"--1", b"+-1", b" \t\n\v\f\r"]
    pool += [b"\x0012", b"12\x003", b"12\x00", b"\x00", b" 12\x00 ", b"true\x00x", b"\x00true", b"1.5\x00e3", b"-\x001"]
    pool += [b"12\x80", b"\x8012", b"\xa012", b"12\xa0", b"\xff", b"tru\xc5", b"1\xe9"]
    for word in (b"true", b"yes", b"false", b"no", b"True", b"YES", b"fAlSe", b"nO", b"TRUE", b"tRuE", b"truee", b"ye", b"falsee", b"n", b"on", b"1", b"0", b"t", b"y"):
        pool.append(word)
        for sp in (b" ", b"\t", b"\r", b"\n"):
            pool += [sp + word, word + sp, sp + word + sp, sp + sp + word + sp]
    for _ in range(2600):
        n = rng.randint(1, 25)
        digits = "".join(rng.choice("0123456789") for _ in range(n)).encode()
        pool.append(rng.choice([b"", b"", b"-", b"+"]) + digits)
    pool += threshold_values()
    seen, out = set(), []
    for v in pool:
        if v not in seen:
            seen.add(v)
            out.append(v)
    return out


def fast_decimals(to_type):
    """At most 15 (FLOAT: 7) significant digits and exponent - fraction digits in [-22, 22] (FLOAT: [-10, 10]), in every form:
    with and without '.', exponent, sign and padding."""
    rng = random.Random(438 + to_type)
    max_digits, max_e = (7, 10) if to_type == ss.FLOAT else (15, 22)
    out, seen = [], set()
    while len(out) < 2000:
        n = rng.randint(1, max_digits)
        digits = "".join(rng.choice("0123456789") for _ in range(n))
        frac = rng.randint(0, n)                       # digits behind the point
        e10 = rng.randint(-max_e, max_e)               # the decimal exponent of the integer mantissa
        ex = e10 + frac
        if not -9999 <= ex <= 9999:
            continue
        text = digits[:n - frac]
        if frac or rng.random() < 0.2:
            text += "." + digits[n - frac:]
        if not digits[:n - frac] and rng.random() < 0.5:
            text = "0" + text
        if ex or rng.random() < 0.3:
            text += rng.choice("eE") + (rng.choice(["", "+"]) if ex >= 0 else "-") + ("%0*d" % (rng.randint(1, 4), abs(ex)))[-4:]
        text = rng.choice(["", "", "-", "+"]) + rng.choice(["", "0", "000"]) * (text[:1] != ".") + text
        text = rng.choice(["", " ", "\t ", "\n"]) + text + rng.choice(["", " ", " \r\n", "\f"])
        if text not in seen:
            seen.add(text)
            out.append(text.encode())
    return out


def hard_floats():
    return [b"12345678901234567", b"123456789012345678", b"1234567890123456789", b"0.1234567890123456789", b"9007199254740993",
            b"1e23", b"1e-23", b"1.5e-22", b"16777217", b"1e400", b"1e-400", b"inf", b"-Infinity", b"NaN", b"nan(0x1)", b"0x1p3", b"1.OOPS", b"1.1.", b"--12", b".", b"e5",
            b"+", b"-", b" ", b"1e", b"1e+", b"1e12345", b"12345678901234567890", b"1 2", b"0x", b"1d5", b"4e-324", b"1.7976931348623157e308", b"1e11", b"1e-11",
            b"0." + b"0" * 200 + b"1", b"1" + b"0" * 200 + b"e-200", b"1.5" + b"0" * 70]
