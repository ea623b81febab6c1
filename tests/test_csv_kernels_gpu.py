"""The three CSV kernels (ops/csrc/hip/csv_kernels.hip) one by one against plain-Python oracles, on files of a few KB
whose interesting bytes sit where the kernels can go wrong:

* ``csv_fields_kernel`` against a per-row state machine -- separators, quotes and ``""`` escapes on the edges of its
  64-byte ballot windows, rows at unaligned offsets, one to five rows (a workgroup holds four);
* ``csv_parse_num_kernel`` against ``float()`` / ``int()`` of ASCII decimals (correctly rounded, so exact bits are
  the assertion) at the limits of its fast path: 19 digits, a mantissa below 2**53, an exponent within +-22;
* ``csv_hash_text_kernel`` against FNV-1a-64 of the decoded cell.

The oracle itself is checked without a device against ``csv.reader``."""
import csv
import random
import re
import struct

import pytest
import torch

gpu = pytest.mark.gpu

NA = ["#N/A", "#N/A N/A", "#NA", "-1.#IND", "-1.#QNAN", "-NaN", "-nan", "1.#IND", "1.#QNAN", "<NA>", "N/A", "NA",
      "NULL", "NaN", "None", "n/a", "nan", "null"]
M64 = (1 << 64) - 1


# ---- oracles ---------------------------------------------------------------------------------------------------

def rows_of(data: bytes):
    """``(start, end)`` of every non-blank row: rows end at ``\\n`` or the buffer's end; an empty row or a lone
    ``\\r`` is skipped (as the reader does)."""
    out, s = [], 0
    while s < len(data):
        e = data.find(b"\n", s)
        e = len(data) if e < 0 else e
        if e > s and data[s:e] != b"\r":
            out.append((s, e))
        s = e + 1
    return out


def split_row(data: bytes, s: int, e: int, sep: int):
    """The oracle: ``(nfields, field starts, end)`` of row ``data[s:e]``. Every ``"`` toggles the quote state, a
    separator outside quotes starts a field, a trailing ``\\r`` is dropped; a row that ends inside quotes has
    nfields -1."""
    if e > s and data[e - 1] == 13:
        e -= 1
    starts, inq = [s], False
    for p in range(s, e):
        c = data[p]
        if c == 34:
            inq = not inq
        elif c == sep and not inq:
            starts.append(p + 1)
    return (-1 if inq else len(starts)), starts, e


def expected_fstart(starts, e, ncols):
    """The slots the kernel writes: field starts 0 .. min(nf, ncols) - 1, then end + 1."""
    nf = len(starts)
    return starts[:min(nf, ncols)] + [e + 1]


def decode(raw: bytes) -> bytes:
    """A cell's value: quoted when its first and last bytes are quotes (they go, ``""`` is one quote), else literal."""
    if len(raw) >= 2 and raw[:1] == b'"' and raw[-1:] == b'"':
        return raw[1:-1].replace(b'""', b'"')
    return raw


def fnv1a(b: bytes) -> int:
    h = 14695981039346656037
    for c in b:
        h = ((h ^ c) * 1099511628211) & M64
    return h or 1


def check_hash(b: bytes) -> int:
    g = 0x9E3779B97F4A7C15
    for c in b:
        g = ((g ^ c) * 0xFF51AFD7ED558CCD) & M64
        g ^= g >> 32
    return g ^ len(b)


# ---- the kernels, called the way readers/gpu_csv.py _parse_chunk does --------------------------------------------

def run_kernels(data: bytes, ncols: int, sep: str = ",", num=(), kinds=(), txt=()):
    from transmogrifai_amd.ops import _native as N
    lib = N.hip()
    dev = torch.device("cuda")
    rows = rows_of(data)
    nrows = len(rows)
    buf = torch.frombuffer(bytearray(data), dtype=torch.uint8).to(dev)
    starts = torch.tensor([r[0] for r in rows], dtype=torch.int64, device=dev)
    ends = torch.tensor([r[1] for r in rows], dtype=torch.int64, device=dev)
    fstart = torch.full((nrows, ncols + 1), -7, dtype=torch.int64, device=dev)
    nf = torch.full((nrows,), -7, dtype=torch.int32, device=dev)
    st = N.stream(dev)
    N.check(lib.tmog_hip_csv_fields(N.ptr(buf), N.ptr(starts), N.ptr(ends), nrows, ncols, ord(sep), N.ptr(fstart),
                                    N.ptr(nf), st), "csv_fields")
    out = {"rows": rows, "fstart": fstart.cpu().tolist(), "nf": nf.cpu().tolist()}
    if num:
        nn = len(num)
        cols = torch.tensor(num, dtype=torch.int32, device=dev)
        kind = torch.tensor(kinds, dtype=torch.int32, device=dev)
        vals = torch.full((nrows, nn), -7, dtype=torch.int64, device=dev)
        ok = torch.full((nrows, nn), 7, dtype=torch.uint8, device=dev)
        slow = torch.full((nrows, nn), 7, dtype=torch.uint8, device=dev)
        N.check(lib.tmog_hip_csv_parse_num(N.ptr(buf), N.ptr(fstart), N.ptr(nf), nrows, ncols, N.ptr(cols),
                                           N.ptr(kind), nn, N.ptr(vals), N.ptr(ok), N.ptr(slow), st), "csv_parse_num")
        out.update(vals=vals.cpu().tolist(), ok=ok.cpu().tolist(), slow=slow.cpu().tolist())
    if txt:
        nt = len(txt)
        cols = torch.tensor(txt, dtype=torch.int32, device=dev)
        th = torch.full((nrows, nt), -7, dtype=torch.int64, device=dev)
        sp = torch.full((nrows, nt, 2), -7, dtype=torch.int64, device=dev)
        ck = torch.full((nrows, nt), -7, dtype=torch.int64, device=dev)
        N.check(lib.tmog_hip_csv_hash_text(N.ptr(buf), N.ptr(fstart), N.ptr(nf), nrows, ncols, N.ptr(cols), nt,
                                           N.ptr(th), N.ptr(sp), N.ptr(ck), st), "csv_hash_text")
        out.update(hash=[[v & M64 for v in r] for r in th.cpu().tolist()], span=sp.cpu().tolist(),
                   check=[[v & M64 for v in r] for r in ck.cpu().tolist()])
    return out


# ---- csv_fields_kernel -----------------------------------------------------------------------------------------

def _filled(n, seps=()):
    """A row of ``n`` bytes: letters, with a separator at every offset of ``seps``."""
    b = bytearray(b"abcdefghijklmnopqrstuvwxyz" * (n // 26 + 1))[:n]
    for p in seps:
        b[p] = ord(",")
    return bytes(b)


# well-formed rows (every quoted field is closed, quotes only around whole fields): name -> row
WELL_FORMED = {
    **{f"len{n}": _filled(n) for n in (1, 63, 64, 65, 127, 128, 129, 200)},
    **{f"len{n}_seps": _filled(n, [p for p in (0, 31, 62, 63, 64, 65, 126, 127, 128, 199) if p < n])
       for n in (1, 63, 64, 65, 127, 128, 129, 200)},
    **{f"sep_at_{p}": _filled(p) + b"," + b"tail" for p in (62, 63, 64, 65)},
    **{f"sep_last_{p}": _filled(p) + b"," for p in (62, 63, 64, 65)},
    "quote_63_64": _filled(62) + b',"",x,y',                    # opening quote at 63, closing at 64, separator at 65
    "escape_63_64": _filled(50) + b',"' + b"b" * 11 + b'""c,d",e',      # "" on 63/64, then a quoted separator
    "quoted_sep_64": _filled(60) + b',"bb,c",z',                # the separator at 64 is inside quotes
    "quoted_sep_63": _filled(59) + b',"bb,c",z',
    "three_windows": b'"' + b"x," * 80 + b'",end',              # one quoted field over windows 0, 1 and 2
    "quote_closes_at_127_128": _filled(3) + b',"' + b"q," * 61 + b'",r,s',
    "empty70": b"," * 69,                                       # 70 empty fields: window 0 holds 64 separators
    "empty129": b"," * 128,
    "all_quoted": b'"a","b,b","c""c",""',
}
ODD = {"odd_open": _filled(62) + b',"x,y', "odd_at_64": _filled(64) + b'",z', "odd_escape": b'a,"b""",c"'}


def _file(rows, eols):
    """The rows joined with the given line ends (cycled); the last row keeps its line end unless it is None."""
    out = b""
    for k, r in enumerate(rows):
        eol = eols[k % len(eols)]
        out += r + (eol or b"")
    return out


def _fields_cases():
    names = list(WELL_FORMED)
    pre = [b"a", b"ab", b"abc"]                                 # rows of 1, 2 and 3 bytes: unaligned offsets behind
    for k, nm in enumerate(names):
        # one row alone; behind 1 + 2 + 3-byte rows (4 rows); 5 rows; 3 rows -- rotating through the names
        yield f"{nm}-1row", _file([WELL_FORMED[nm]], [b"\n"]), 70 if "empty" in nm else 4, ","
        yield f"{nm}-4rows", _file(pre + [WELL_FORMED[nm]], [b"\n"]), 4, ","
        yield f"{nm}-5rows", _file(pre[:2] + [WELL_FORMED[nm], WELL_FORMED[names[(k + 1) % len(names)]], b"z,z"],
                                   [b"\n"]), 3, ","
        yield f"{nm}-3rows-nonl", _file([pre[k % 3], WELL_FORMED[nm], WELL_FORMED[names[(k + 7) % len(names)]]],
                                        [b"\n", b"\n", None]), 5, ","
    every = [WELL_FORMED[nm] for nm in names]
    yield "all-ncols1", _file(pre + every, [b"\n"]), 1, ","
    yield "all-ncols2", _file(pre + every, [b"\n"]), 2, ","
    yield "all-ncols130", _file(pre + every, [b"\n"]), 130, ","
    yield "all-crlf-lf-mixed", _file(pre + every, [b"\r\n", b"\n", b"\r\n", b"\r\n", b"\n"]), 4, ","
    yield "all-crlf-blank-lines", _file(pre + every, [b"\r\n\r\n", b"\n\n", b"\r\n"]), 4, ","
    yield "all-semicolon", _file(pre + [r.replace(b",", b";") for r in every] + [b'a,b;"c;d";e,f'], [b"\n"]), 4, ";"
    yield "commas-under-semicolon", _file(pre + every, [b"\n"]), 4, ";"
    yield "odd-parity", _file(pre + [ODD["odd_open"], b"p,q", ODD["odd_at_64"], ODD["odd_escape"], b"r"],
                              [b"\n", b"\r\n"]), 3, ","


FIELDS_CASES = list(_fields_cases())


@gpu
@pytest.mark.parametrize("data,ncols,sep", [pytest.param(d, n, s, id=i) for i, d, n, s in FIELDS_CASES])
def test_fields_match_state_machine(data, ncols, sep):
    got = run_kernels(data, ncols, sep)
    assert len(got["rows"]) > 0
    for r, (s, e) in enumerate(got["rows"]):
        nf, starts, end = split_row(data, s, e, ord(sep))
        assert got["nf"][r] == nf, (r, data[s:e])
        want = expected_fstart(starts, end, ncols)
        assert got["fstart"][r][:len(want)] == want, (r, data[s:e])


def test_row_counts_and_lengths_are_covered():
    """The cases hold what they are meant to: row counts 1, 3, 4 and 5, every row length on a window edge, and a
    window in which all 64 lanes hold a separator."""
    counts = {len(rows_of(d)) for _, d, _, _ in FIELDS_CASES}
    assert {1, 3, 4, 5} <= counts
    lengths = {e - s for _, d, _, _ in FIELDS_CASES for s, e in rows_of(d)}
    assert {1, 2, 3, 63, 64, 65, 127, 128, 129, 200} <= lengths
    assert WELL_FORMED["empty70"][:64] == b"," * 64 and len(WELL_FORMED["empty70"]) == 69
    assert {s % 4 for _, d, _, _ in FIELDS_CASES for s, _ in rows_of(d)} == {0, 1, 2, 3}


@pytest.mark.parametrize("name", list(WELL_FORMED))
@pytest.mark.parametrize("sep", [",", ";"])
def test_oracle_matches_csv_reader(name, sep):
    """On well-formed rows the state machine's fields, unquoted, are the fields of Python's ``csv.reader``."""
    row = WELL_FORMED[name].replace(b",", sep.encode())
    for eol in (b"", b"\r"):
        data = row + eol
        nf, starts, e = split_row(data, 0, len(data), ord(sep))
        bounds = starts + [e + 1]
        fields = [decode(data[bounds[k]:bounds[k + 1] - 1]).decode() for k in range(nf)]
        assert e == len(row)
        assert fields == next(csv.reader([row.decode()], delimiter=sep))
    # the odd rows are what the oracle says they are: open at the row's end
    assert all(split_row(r, 0, len(r), 44)[0] == -1 for r in ODD.values())


# ---- csv_parse_num_kernel --------------------------------------------------------------------------------------

_DEC = re.compile(r"([+-]?)([0-9]*)\.?([0-9]*)(?:[eE]([+-]?[0-9]+))?")


def eligible(s: str) -> bool:
    """The documented fast path of a plain decimal: after the sign and the leading zeros at most 19 significant
    digits as written, their integer m < 2**53, and the exponent left after the fraction digits in [-22, 22]."""
    _, ip, fp, ex = _DEC.fullmatch(s).groups()
    sig = (ip + fp).lstrip("0")
    e10 = (int(ex) if ex else 0) - len(fp)
    return len(sig) <= 19 and int(sig or "0") < 2 ** 53 and -22 <= e10 <= 22


def bits(x: float) -> int:
    return struct.unpack("<q", struct.pack("<d", x))[0]


def generated_cells(n=3000, seed=20240607):
    rng = random.Random(seed)
    out = []
    for _ in range(n):
        nd = rng.choice([1, 2, 3, 5, 8, 12, 15, 16, 17, 18, 19, 20, 21])
        d = str(rng.randint(1, 9)) + "".join(rng.choice("0123456789") for _ in range(nd - 1))
        if rng.random() < 0.25:                       # mantissas on both sides of 2**53
            d = str(2 ** 53 + rng.randint(-3, 3) * rng.choice([1, 10 ** 3, 10 ** 9]))
        full = "0" * rng.choice([0, 0, 0, 1, 3]) + d + "0" * rng.choice([0, 0, 0, 1, 2, 4])
        if rng.random() < 0.7:
            p = rng.randint(0, len(full))
            full = full[:p] + "." + full[p:]
        if rng.random() < 0.5:
            full += rng.choice("eE") + rng.choice(["", "+", "-"]) + "0" * rng.choice([0, 0, 2]) + \
                str(rng.randint(0, 30))
        out.append(rng.choice(["", "", "-", "+"]) + full)
    return out


EDGE_CELLS = [
    str(2 ** 53 - 1), str(2 ** 53), str(2 ** 53 + 1), "-" + str(2 ** 53 - 1), str(2 ** 53 - 1) + "e22",
    str(2 ** 53 - 1) + "e-22", str(2 ** 53) + "e-22", "0.%d" % (2 ** 53 - 1), "0.%d" % (2 ** 53),
    "1e22", "1e-22", "1e23", "1e-23", "12.5e23", "12.5e24", "125e-22", "125e-23", "1.5e-21", "1.5e-22", "0.001e25",
    "0.001e26", "1000e19", "1000e20", "1.0000000000000000000000e22", "9e22", "9e23",
    "1234567890123456789", "12345678901234567890", "1234567.890123456789", "1234567.8901234567891",
    "1000000000000000000", "10000000000000000000", "100000000000000000000", "1.000000000000000000",
    "1.0000000000000000000", "1.0000000000000000001", "1234567890123456780", "1234567890123456789.0",
    "1234567890123456789.5", "123456789012345678.90", "123456789012345678.91", "9007199254740.991", "12345678901234567800",
    "12345678901234567810", "9007199254740991.000", "9007199254740991.0000", "9007199254740991.0001",
    "0", "-0", "+0", "-0.0", "0e5", "0.000", "0.0e-30", "000", "0e400", "-0e-400", "0." + "0" * 40,
    ".5", "5.", "-.5", "+5.", "00012", "-00012.50", "5e-0005", "5E+0005", "5e0", "5e-0", "5e+0", "1E22", "1E-22",
    "0." + "0" * 30 + "5", "0." + "0" * 22 + "5", "0." + "0" * 21 + "5", "0." + "0" * 20 + "12",
    "1e400", "-1e400", "1e-400", "4.9e-324", "2.2250738585072011e-308", "2.2250738585072014e-308",
    "1.7976931348623157e308", "9007199254740993", "9007199254740992", "0.1", "0.3", "123456789.123456789",
    "3.14159265358979323846", "179769313486231570000000000000000000000", "1" + "0" * 22, "1" + "0" * 23,
    "8.5", "7", "-2.5E+3", "1e-30", "1e0000000000000000000000001", "1e-0000000000000000000000001",
]


@pytest.fixture(scope="module")
def num_run():
    """Every numeric test cell as ``x,<cell>`` rows, parsed once as float64 (output 0) and as int64 (output 1)."""
    cells = generated_cells() + EDGE_CELLS + [repr(0.7351 * 10.0 ** k) for k in range(-9, 10, 3)]
    n_gen = 3000
    rng = random.Random(11)
    reprs = [repr(rng.gauss(0.0, 100.0)) for _ in range(500)]
    ints = ["7", "-42", "007", "-007", "0", "-0", "000", "999999999999999999", "-999999999999999999",
            "000000000000000000000999999999999999999", "100000000000000000", "1" + "0" * 17, "123456789012345678",
            "9223372036854775807", "-9223372036854775808", "9223372036854775808", "-9223372036854775809",
            "1000000000000000000", "1234567890123456789", "-1234567890123456789", "9999999999999999999",
            "99999999999999999999", "+5", "1e3", "5.0", "5.", "1E0", "-1e2", "+007", "12e0"]
    ints += [str(random.Random(3).randint(-10 ** k, 10 ** k)) for k in range(1, 19)]
    special = NA + ["", '""'] + ['"%s"' % s for s in NA] + [" NA", "NA ", "\tnan", " ", "  \t", '" "', ' "5"',
                                                            '"5"', '" 5"', " 5 ", "\t5", '"5" ', "x", "1_000",
                                                            "٣", "0x10", "1e", "1e+", ".", "-", "+", "e5", "--5", "5f",
                                                            "inf", "-inf", "Infinity", "1.2.3", "1 2", '"1""2"']
    allc = cells + reprs + ints + special
    data = "".join("x," + c + ("\r\n" if k % 7 == 3 else "\n") for k, c in enumerate(allc)).encode()
    got = run_kernels(data, 2, ",", num=[1, 1], kinds=[0, 1])
    assert len(got["rows"]) == len(allc) and all(v == 2 for v in got["nf"])
    idx = {}
    pos = 0
    for name, part in (("cells", cells), ("reprs", reprs), ("ints", ints), ("special", special)):
        idx[name] = [(c, pos + k) for k, c in enumerate(part)]
        pos += len(part)
    return got, idx, n_gen


def _float_checks(got, c, r):
    """The three conditions on one plain decimal read as float64; returns whether the cell went to the host."""
    v, ok, slow = got["vals"][r][0], got["ok"][r][0], got["slow"][r][0]
    assert ok in (0, 1) and slow in (0, 1), c
    want = bits(float(c))
    if ok:
        assert v == want and not slow, (c, v, want)                 # never valid with other bits
    if eligible(c):
        assert (slow, ok, v) == (0, 1, want), (c, slow, ok, v, want)
    assert slow or ok, c                                            # a number is never read as missing
    return bool(slow)


@gpu
def test_parse_float_exact_or_slow(num_run):
    got, idx, n_gen = num_run
    nslow = sum(_float_checks(got, c, r) for c, r in idx["cells"][:n_gen])
    nslow_rest = sum(_float_checks(got, c, r) for c, r in idx["cells"][n_gen:])
    nelig = sum(eligible(c) for c, _ in idx["cells"])
    assert nelig > 500 and nslow + nslow_rest > 500                 # both classes are exercised
    rslow = sum(_float_checks(got, c, r) for c, r in idx["reprs"])
    print(f"\nslow share: generated cells {nslow}/{n_gen} = {nslow / n_gen:.3f}; "
          f"repr() doubles {rslow}/{len(idx['reprs'])} = {rslow / len(idx['reprs']):.3f}")
    # the integer cells are plain decimals too
    for c, r in idx["ints"]:
        _float_checks(got, c, r)


FAST_EDGES = [str(2 ** 53 - 1), "-" + str(2 ** 53 - 1), str(2 ** 53 - 1) + "e22", str(2 ** 53 - 1) + "e-22", "1e22",
              "1e-22", "12.5e23", "0.001e25", "1000e19", "1000e20", "125e-22", "1.5e-21", "9007199254740.991",
              "0", "-0", "+0", "-0.0", "0e5", "0.000", ".5", "5.", "00012", "5e-0005", "0." + "0" * 21 + "5"]
HOST_EDGES = [str(2 ** 53), str(2 ** 53 + 1), str(2 ** 53) + "e-22", "1e23", "1e-23", "12.5e24", "0.001e26", "125e-23",
              "1.5e-22", "12345678901234567890", "1234567.8901234567891", "0." + "0" * 30 + "5",
              "0." + "0" * 22 + "5", "1e400", "1e-400", "4.9e-324", "2.2250738585072011e-308", "9007199254740993"]


def test_eligibility_rule_on_the_edges():
    """The rule the conditions rest on, on hand-written cells on both sides of every limit (a wrong rule would make
    the condition test vacuous)."""
    assert all(c in EDGE_CELLS for c in FAST_EDGES + HOST_EDGES)
    assert all(eligible(c) for c in FAST_EDGES)
    assert not any(eligible(c) for c in HOST_EDGES)


@gpu
def test_parse_float_edges_take_the_documented_path(num_run):
    got, idx, _ = num_run
    where = dict(idx["cells"])
    for c in FAST_EDGES:
        assert (got["slow"][where[c]][0], got["ok"][where[c]][0], got["vals"][where[c]][0]) == \
            (0, 1, bits(float(c))), c
    for c in HOST_EDGES:                                            # past a limit by one: the host's float()
        assert (got["slow"][where[c]][0], got["ok"][where[c]][0]) == (1, 0), c
    for c in ("0e400", "-0e-400", "0." + "0" * 40):                 # a zero mantissa is zero whatever the exponent
        assert (got["slow"][where[c]][0], got["ok"][where[c]][0], got["vals"][where[c]][0]) == \
            (0, 1, bits(float(c))), c


_PLAIN_INT = re.compile(r"-?[0-9]+")


@gpu
def test_parse_int_exact_or_slow(num_run):
    got, idx, _ = num_run
    must_be_slow = {"9223372036854775807", "-9223372036854775808", "9223372036854775808", "-9223372036854775809",
                    "1000000000000000000", "1234567890123456789", "-1234567890123456789", "9999999999999999999",
                    "99999999999999999999", "+5", "1e3", "5.0", "5.", "1E0", "-1e2", "+007", "12e0"}
    seen = set()
    for c, r in idx["ints"] + idx["cells"] + idx["reprs"]:
        v, ok, slow = got["vals"][r][1], got["ok"][r][1], got["slow"][r][1]
        assert ok in (0, 1) and slow in (0, 1), c
        plain = _PLAIN_INT.fullmatch(c) is not None
        if ok:                                                      # never valid and wrong
            assert plain and v == int(c) and not slow, (c, v)
        if plain and len(c.lstrip("-").lstrip("0")) <= 18:          # at most 18 digits: fast and exact
            assert (slow, ok, v) == (0, 1, int(c)), (c, slow, ok, v)
        if c in must_be_slow or not plain:
            assert (slow, ok) == (1, 0), (c, slow, ok)
            seen.add(c)
        assert slow or ok, c
    assert must_be_slow <= seen


@gpu
def test_parse_num_missing_and_rejected(num_run):
    got, idx, _ = num_run
    missing = set(NA) | {"", '""'} | {'"%s"' % s for s in NA}
    fast5 = {'"5"', '" 5"', " 5 ", "\t5"}
    for c, r in idx["special"]:
        for j in (0, 1):
            v, ok, slow = got["vals"][r][j], got["ok"][r][j], got["slow"][r][j]
            if c in missing:
                assert (ok, slow) == (0, 0), (c, j)
            elif c in fast5:
                assert (slow, ok, v) == (0, 1, bits(5.0) if j == 0 else 5), (c, j)
            else:                       # padded NA, padding alone, quotes behind padding, other grammars: the host
                assert (ok, slow) == (0, 1), (c, j)


# ---- csv_hash_text_kernel --------------------------------------------------------------------------------------

TEXT_CELLS = ["alpha", "b", " b", "b ", "\tb", '" b "', ' "q" ', '"q"', "q", 'e""f', '"e""""f"', '"e""f"',
              '"c,d"', '"c,d,,e"', '""', "", '""""', '" "', " ", "gamma delta", "née", '"née"', "日本語", '"日本,語"',
              "ß" * 40, '"' + "x" * 70 + '"', "y" * 64, "y" * 63, '"' + 'z""' * 30 + '"', " NA", "NA ", '" NA"',
              "9", "nul", "nulls", "#N/A N/A", "#N/A N/A ", "123456789"] + NA + ['"%s"' % s for s in NA]
MALFORMED = ['"a"b', '"a" ', '"a"b"c"']        # even quote parity, but no well-formed quoted field


@gpu
def test_hash_text_matches_fnv1a():
    cells = TEXT_CELLS + MALFORMED
    data = "".join(f"k{k}," + c + ",z" + ("\r\n" if k % 5 == 2 else "\n") for k, c in enumerate(cells)).encode()
    got = run_kernels(data, 3, ",", txt=[1, 0, 2])
    assert len(got["rows"]) == len(cells)
    missing = set(NA) | {"", '""'} | {'"%s"' % s for s in NA}
    for r, ((s, e), c) in enumerate(zip(got["rows"], cells)):
        nf, starts, end = split_row(data, s, e, 44)
        assert got["nf"][r] == nf == 3, c
        bounds = starts + [end + 1]
        for j, col in enumerate((1, 0, 2)):
            raw = data[bounds[col]:bounds[col + 1] - 1]
            if col == 1:
                assert raw == c.encode()
            val = decode(raw)
            if col == 1 and c in MALFORMED:
                assert (got["hash"][r][j], got["check"][r][j], got["span"][r][j]) == (0, 0, [-1, -1]), c
            elif col == 1 and c in missing:
                assert (got["hash"][r][j], got["check"][r][j]) == (0, 0), c
            else:
                assert got["hash"][r][j] == fnv1a(val), (c, col)
                assert got["check"][r][j] == check_hash(val), (c, col)
                # the vocabulary is decoded from span: it must be the field as written
                assert got["span"][r][j] == [bounds[col], bounds[col + 1] - 1], (c, col)
    # equal strings written two ways hash equally; different strings differently
    h = {c: got["hash"][r][0] for r, c in enumerate(cells)}
    assert h['e""f'] == h['"e""""f"'] != h['"e""f"'] == fnv1a(b'e"f')
    assert h["q"] == h['"q"'] != h[' "q" ']
    assert len({h["b"], h[" b"], h["b "], h["\tb"], h['" b "']}) == 5


def test_oracle_hashes():
    """FNV-1a-64 test vectors (the published ones for "", "a" and "foobar")."""
    assert fnv1a(b"a") == 0xaf63dc4c8601ec8c and fnv1a(b"foobar") == 0x85944171f73967e8
    assert fnv1a(b"") == 0xcbf29ce484222325
    assert decode(b'"e""""f"') == b'e""f' and decode(b'e""f') == b'e""f' and decode(b' "q" ') == b' "q" '
    assert check_hash(b"ab") != check_hash(b"ba")
