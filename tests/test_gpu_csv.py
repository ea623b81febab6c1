"""CSV parsed on the GPU (readers/gpu_csv.py, ops/csrc/hip/csv_kernels.hip) against the pyarrow columnar path
(readers/columnar.py csv_dataset): identical float64 / int64 values and validity, identical text codes and
vocabularies -- across chunk boundaries (tiny chunks), quoted fields with separators and escaped quotes, pandas' NA
strings, CRLF line ends, blank lines, a missing final newline and long-mantissa numbers (the host fallback).

The contract on any file: ``gpu_csv_dataset`` returns None or exactly ``csv_dataset``'s dataset, and None where
``csv_dataset`` returns None -- checked cell by cell on the cells where the two grammars could part (padding, quotes,
``_``, non-ASCII digits, signs and exponents in integers, int64 overflow, a newline inside quotes)."""
import numpy as np
import pytest
import torch

from transmogrifai_amd.features import types as T
from transmogrifai_amd.features.builder import FeatureBuilder

gpu = pytest.mark.gpu

# rows of cells pyarrow reads like any other (r1, r2, i1, t1, t2): padded and quoted numbers, infinities, text that
# keeps its padding, and one string written unquoted (e""f) and quoted ("e""""f")
_EXTRA_ROWS = [
    ("+5", "1.5", "007", " b", "p"), ("5.", "2.5", "-007", "b ", "q"), (".5", "0.5", " 5 ", '" b "', "r"),
    (" 5 ", "\t5", '"5"', ' "q" ', "p"), ("\t5", '"5"', '" 5"', 'e""f', "q"), ('"5"', '" 5"', "\t5", '"e""""f"', "r"),
    ('" 5"', "inf", '"NA"', "b", "p"), ("inf", "-inf", "1", "q", "q"), ("-inf", "Infinity", "2", '"q"', "r"),
    ("Infinity", "1e400", "3", " b", "p"), ("1e400", "1.#IND", "4", 'e""f', "q"), ("1.#IND", '"NA"', "5", "x", "r"),
    ('"NA"', "+5", "6", '" NA"', "p"), ("-1e400", " nan", "0000000000000000000000012", "\tb", "q")]


def _write(path, crlf=False, final_newline=True, n=3000, seed=0):
    rng = np.random.default_rng(seed)
    eol = "\r\n" if crlf else "\n"
    lines = ['"r1","r2","i1","t1","t2"']
    words = ["alpha", "beta", "c,d", 'e""f', "NA", "", "gamma delta", "x"]
    for k in range(n):
        r1 = ["%.9g" % np.float32(rng.normal() * 10.0 ** int(rng.integers(-8, 8))), "", "nan", "-0.0", "1e-30",
              "3.14159265358979323846", "12345678901234567890.5", "7", "-2.5E+3", "NULL"][k % 10]
        r2 = repr(float(rng.normal()))
        i1 = ["1", "", "-42", "9007199254740993", "0"][k % 5]
        t1 = words[rng.integers(0, len(words))]
        t1 = f'"{t1}"' if t1 not in ("", "NA") else t1
        t2 = ["p", "q", "r"][k % 3]
        lines.append(",".join([r1, r2, i1, t1, t2]))
        if k % 997 == 5:
            lines.append("")                      # blank line: skipped
        if k == n // 2:
            lines.extend(",".join(r) for r in _EXTRA_ROWS)
    lines.extend(",".join(r) for r in _EXTRA_ROWS)
    text = eol.join(lines) + (eol if final_newline else "")
    path.write_bytes(text.encode())


def _features():
    return [FeatureBuilder.Real("r1").as_predictor(), FeatureBuilder.Real("r2").as_predictor(),
            FeatureBuilder.Integral("i1").as_predictor(), FeatureBuilder.Text("t1").as_predictor(),
            FeatureBuilder.PickList("t2").as_predictor()]


def _assert_same(ref, got, feats):
    assert got.n_rows == ref.n_rows
    for f in feats:
        a, b = ref[f.name], got[f.name]
        if f.wtype.kind == "text":
            assert list(a.vocab) == list(b.vocab), f.name
            assert torch.equal(a.codes.cpu().to(torch.int32), b.codes.cpu()), f.name
        else:
            va = a.valid.cpu() if a.valid is not None else torch.ones(ref.n_rows, dtype=torch.bool)
            vb = b.valid.cpu() if b.valid is not None else torch.ones(got.n_rows, dtype=torch.bool)
            assert torch.equal(va, vb), f.name
            x, y = a.values.cpu(), b.values.cpu()
            assert x.dtype == y.dtype, f.name
            if x.is_floating_point():
                assert torch.equal(x.view(torch.int64)[va], y.view(torch.int64)[vb]), f.name
            else:
                assert torch.equal(x[va], y[vb]), f.name


@gpu
@pytest.mark.parametrize("crlf,final_nl,chunk", [(False, True, 1 << 20), (False, False, 4096), (True, True, 7777)])
def test_gpu_csv_matches_arrow(tmp_path, crlf, final_nl, chunk):
    from transmogrifai_amd.readers.columnar import csv_dataset
    from transmogrifai_amd.readers.gpu_csv import gpu_csv_dataset
    p = tmp_path / "d.csv"
    _write(p, crlf, final_nl)
    feats = _features()
    dev = torch.device("cuda")
    ref = csv_dataset(str(p), feats, dev)
    got = gpu_csv_dataset(str(p), feats, dev, chunk_bytes=chunk)
    assert ref is not None and got is not None
    _assert_same(ref, got, feats)
    # text keeps its padding, and e""f has one code and one vocabulary entry however it is written
    voc = list(got["t1"].vocab)
    assert all(voc.count(w) == 1 for w in (" b", "b ", " b ", ' "q" ', "q", "b", 'e""f', 'e"f', " NA", "\tb"))
    t1 = got["t1"].codes.cpu()
    k0 = 3000 // 2 + 1                              # the first extra row: behind row n // 2 (blank lines are no rows)
    assert int(t1[k0 + 4]) == int(t1[k0 + 5]) == voc.index('e""f')
    r1 = got["r1"].values.cpu()[k0:k0 + 14].tolist()
    inf = float("inf")
    assert r1[:6] == [5.0, 5.0, 0.5, 5.0, 5.0, 5.0] and r1[6:11] == [5.0, inf, -inf, inf, inf] and r1[13] == -inf
    assert got["r1"].valid.cpu()[k0:k0 + 14].tolist() == [True] * 11 + [False, False, True]
    assert got["i1"].values.cpu()[k0:k0 + 6].tolist() == [7, -7, 5, 5, 5, 5]


def test_fixture_reads_on_the_arrow_path(tmp_path):
    """The reference of the comparison above exists: the Arrow path reads the fixture, extra rows included."""
    from transmogrifai_amd.readers.columnar import csv_dataset
    p = tmp_path / "d.csv"
    _write(p, n=40)
    ref = csv_dataset(str(p), _features(), "cpu")
    assert ref is not None and ref.n_rows == 40 + 2 * len(_EXTRA_ROWS)
    voc = list(ref["t1"].vocab)
    assert all(w in voc for w in (" b", "b ", " b ", ' "q" ', 'e""f', " NA", "\tb")) and voc.count('e""f') == 1


# cells on which the GPU reader's grammar could part from pyarrow's: (kind of column b, cell)
_REJECTED = [("real", c) for c in ("1_000", "\u0663", "0x10", "1e", " NA", "NA ", " ", ' "5"', "1d5", "--5")] + \
            [("int", c) for c in ("+5", "1e3", "5.0", "5.", "1_0", " 1_0 ", "99999999999999999999",
                                  "9223372036854775808", "-9223372036854775809", " NA", "\u0663")]
_QUOTED_NEWLINE = 'a,b\n1,"x\n2,y"\n3,z\n'


def _cell_file(tmp_path, kind, cell):
    p = tmp_path / "cell.csv"
    p.write_bytes(f"a,b\nx,{cell}\ny,1\n".encode())
    return str(p), [(FeatureBuilder.Integral if kind == "int" else FeatureBuilder.Real)("b").as_predictor()]


def _newline_file(tmp_path):
    p = tmp_path / "nl.csv"
    p.write_bytes(_QUOTED_NEWLINE.encode())
    return str(p), [FeatureBuilder.Integral("a").as_predictor(), FeatureBuilder.Text("b").as_predictor()]


@pytest.mark.parametrize("kind,cell", _REJECTED)
def test_arrow_rejects_cell(tmp_path, kind, cell):
    """What keeps the contract test below from hiding a failure: on each of these cells ``csv_dataset`` returns
    None, so ``gpu_csv_dataset`` has to."""
    from transmogrifai_amd.readers.columnar import csv_dataset
    path, feats = _cell_file(tmp_path, kind, cell)
    assert csv_dataset(path, feats, "cpu") is None


def test_arrow_reads_quoted_newline_as_two_rows(tmp_path):
    from transmogrifai_amd.readers.columnar import csv_dataset
    path, feats = _newline_file(tmp_path)
    ref = csv_dataset(path, feats, "cpu", text_columns=("b",))
    assert ref.n_rows == 2 and list(ref["b"].vocab) == ["x\n2,y", "z"]
    assert ref["a"].values.tolist() == [1, 3]


def _contract(path, feats, **kw):
    from transmogrifai_amd.readers.columnar import csv_dataset
    from transmogrifai_amd.readers.gpu_csv import gpu_csv_dataset
    dev = torch.device("cuda")
    ref = csv_dataset(path, feats, dev, **kw)
    got = gpu_csv_dataset(path, feats, dev, **kw)
    if ref is None:
        assert got is None
    elif got is not None:
        _assert_same(ref, got, feats)
    return ref, got


@gpu
@pytest.mark.parametrize("kind,cell", _REJECTED)
def test_gpu_none_or_arrow_on_rejected_cell(tmp_path, kind, cell):
    ref, got = _contract(*_cell_file(tmp_path, kind, cell))
    assert ref is None and got is None


@gpu
def test_gpu_none_or_arrow_on_quoted_newline(tmp_path):
    path, feats = _newline_file(tmp_path)
    ref, got = _contract(path, feats, text_columns=("b",))
    assert ref is not None and ref.n_rows == 2
    assert got is None or got.n_rows == 2           # never the three rows of a cut at every newline


@gpu
@pytest.mark.parametrize("cell", ['"a"b', '"a" ', '"a"b"c"', '"5" '])
def test_gpu_none_or_arrow_on_bytes_behind_a_closing_quote(tmp_path, cell):
    """pyarrow reads on behind a closing quote (``"a"b`` is ``ab``); the GPU reader does not parse that."""
    p = tmp_path / "q.csv"
    p.write_bytes(f"a,b\n1,{cell}\n2,7\n".encode())
    if "5" in cell:
        _contract(str(p), [FeatureBuilder.Real("b").as_predictor()])
    else:
        _contract(str(p), [FeatureBuilder.Text("b").as_predictor()], text_columns=("b",))


@gpu
@pytest.mark.parametrize("header", ['"r1","t1","i1"\n', "r1,t1,i1", "r1,t1,i1\r\n\r\n"])
@pytest.mark.parametrize("with_text", [True, False])
def test_header_only_file(tmp_path, header, with_text):
    from transmogrifai_amd.readers.columnar import csv_dataset
    from transmogrifai_amd.readers.gpu_csv import gpu_csv_dataset
    p = tmp_path / "h.csv"
    p.write_bytes(header.encode())
    feats = [FeatureBuilder.Real("r1").as_predictor(), FeatureBuilder.Integral("i1").as_predictor()]
    if with_text:
        feats.append(FeatureBuilder.Text("t1").as_predictor())
    dev = torch.device("cuda")
    got = gpu_csv_dataset(str(p), feats, dev, text_columns=("t1",))
    assert got is not None and got.n_rows == 0
    ref = csv_dataset(str(p), feats, dev, text_columns=("t1",))
    if header.endswith("\n"):           # (pyarrow takes a header without its newline for an empty file: an error)
        assert ref is not None and ref.n_rows == 0
    if ref is not None:
        _assert_same(ref, got, feats)
    assert got["r1"].values.dtype == torch.float64 and got["i1"].values.dtype == torch.int64
    if with_text:
        assert list(got["t1"].vocab) == [] and got["t1"].codes.numel() == 0


def test_encode_no_rows():
    from transmogrifai_amd.readers.gpu_csv import _encode_hashes_spans
    e = torch.empty(0, dtype=torch.int64)
    codes, voc = _encode_hashes_spans(e, torch.empty(0, 2, dtype=torch.int64), b"", "cpu", e)
    assert codes.numel() == 0 and codes.dtype == torch.int32 and voc == []


def test_forged_hash_collision_is_reported():
    """Two different strings with one (forged) hash are not merged into one code: the second hash tells them apart
    and the encoder reports it. The same cells with honest hashes encode by first appearance."""
    from transmogrifai_amd.readers.gpu_csv import _encode_hashes_spans
    mm = b'ab,cd,"ab",,cd\n'
    span = torch.tensor([[0, 2], [3, 5], [6, 10], [11, 11], [12, 14]], dtype=torch.int64)
    check = torch.tensor([11, 22, 11, 0, 22], dtype=torch.int64)
    honest = torch.tensor([-5, 9, -5, 0, 9], dtype=torch.int64)
    codes, voc = _encode_hashes_spans(honest, span, mm, "cpu", check)
    assert codes.tolist() == [0, 1, 0, -1, 1] and voc == ["ab", "cd"]
    forged = torch.tensor([9, 9, 9, 0, 9], dtype=torch.int64)
    assert _encode_hashes_spans(forged, span, mm, "cpu", check) is None
    # a group that differs only in its last cell, and one that differs only in its first
    assert _encode_hashes_spans(torch.tensor([9, 9, 9, 0, 9]), span, mm, "cpu", torch.tensor([1, 1, 1, 0, 2])) is None
    assert _encode_hashes_spans(torch.tensor([9, 9, 9, 0, 9]), span, mm, "cpu", torch.tensor([2, 1, 1, 0, 1])) is None


@pytest.mark.parametrize("raw,integral,want", [
    (b"1_000", False, None), ("\u0663".encode(), False, None), (b" 1_0 ", True, None), (b"1_0", True, None),
    (b"99999999999999999999", True, None), (b"9223372036854775808", True, None), (b"+5", True, None),
    (b"1e3", True, None), (b"5.0", True, None), (b"0x10", False, None), (b"1e", False, None), (b" ", False, None),
    (b' "5"', False, None), (b"NA", False, None), (b"infin", False, None),
    (b"9223372036854775807", True, (2 ** 63 - 1, 1)), (b"-9223372036854775808", True, (-2 ** 63, 1)),
    (b' 1234567890123456789\t', True, (1234567890123456789, 1)), (b'" 007"', True, (7, 1)),
    (b"+5", False, 5.0), (b"5.", False, 5.0), (b".5", False, 0.5), (b'" 5"', False, 5.0), (b"1e400", False, float("inf")),
    (b"-Infinity", False, float("-inf")), (b"inf", False, float("inf")), (b"1e-400", False, 0.0),
    (b"12345678901234567890.5", False, 12345678901234567890.5), (b"4.9e-324", False, 5e-324)])
def test_host_number_grammar(raw, integral, want):
    """The host parser of the cells the device leaves over accepts pyarrow's grammar, not Python's."""
    from transmogrifai_amd.readers.gpu_csv import _host_number
    got = _host_number(raw, integral)
    if want is None or integral:
        assert got == want
    else:
        assert got == (int(np.float64(want).view(np.int64)), 1)
    assert _host_number(b" nan", False)[1] == 0         # a NaN is missing


@gpu
def test_ragged_rows_fall_back(tmp_path):
    from transmogrifai_amd.readers.gpu_csv import gpu_csv_dataset
    p = tmp_path / "bad.csv"
    p.write_text('"r1","r2"\n1,2\n3\n')
    assert gpu_csv_dataset(str(p), [FeatureBuilder.Real("r1").as_predictor()], torch.device("cuda")) is None
