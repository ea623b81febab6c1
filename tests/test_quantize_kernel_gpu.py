"""Edge cases of ``quantize_kernel`` (``ops/csrc/hip/quantize_kernels.hip``), the binning in front of the forest
kernels, against a NumPy oracle: ``bin = searchsorted(thresholds_fp32[f], x, side="left")`` (NaN after every
threshold, the +inf padding included), and with a reserved missing bin NaN and the missing value map to it. Driven
through ``binning.quantize`` on hand-built ``BinSpec``s and once through the C entry; every comparison is exact."""
import numpy as np
import pytest
import torch

from transmogrifai_amd.models.binning import BinSpec, quantize

NS = [1, 63, 64, 65]                 # 64-row blocks
FS = [1, 63, 64, 65, 129]            # 64-feature blocks (lane = feature)


def _loaded():
    from transmogrifai_amd.ops import _native
    return _native.hip_loaded()


def _oracle(X, thr32, missing_bin, mv):
    out = np.empty(X.shape, np.int64)
    for f in range(X.shape[1]):
        out[:, f] = np.searchsorted(thr32[f], X[:, f], side="left")
    if missing_bin >= 0:
        miss = np.isnan(X)
        if mv is not None:
            miss |= X == np.float32(mv)
        out[miss] = missing_bin
    assert out.min() >= 0 and out.max() <= 255
    return out.astype(np.uint8)


def _thresholds(rng, F, MS):
    """fp32 [F, MS]: feature f has between 0 and MS distinct ascending thresholds (0.0 among them for every third
    feature), the rest is +inf padding; the first feature is full, the last one has a single threshold (when MS > 1)."""
    thr = np.full((F, MS), np.inf, np.float32)
    n_real = rng.integers(0, MS + 1, F)
    n_real[0], n_real[-1] = MS, min(MS, 1)
    for f in range(F):
        t = np.unique((rng.standard_normal(3 * MS + 3) * 4).astype(np.float32))
        t = rng.permutation(t)[:n_real[f]]
        if f % 3 == 0 and n_real[f]:
            t[0] = 0.0
        t = np.unique(t)                                   # ascending, distinct
        thr[f, :len(t)] = t
        n_real[f] = len(t)
    return thr, n_real


def _data(rng, N, thr, n_real):
    """Every value class in every column: thresholds, one ulp either side, +-inf, NaN, +-0.0, ordinary draws."""
    F = thr.shape[0]
    X = (rng.standard_normal((N, F)) * 4).astype(np.float32)
    kind = rng.integers(0, 10, (N, F))
    pick = thr[np.arange(F)[None, :], rng.integers(0, np.maximum(n_real, 1), (N, F))]     # +inf where no threshold
    X = np.where(kind == 0, pick, X)
    X = np.where(kind == 1, np.nextafter(pick, np.float32(-np.inf)), X)
    X = np.where(kind == 2, np.nextafter(pick, np.float32(np.inf)), X)
    X = np.where(kind == 3, np.float32(np.inf), X)
    X = np.where(kind == 4, np.float32(-np.inf), X)
    X = np.where(kind == 5, np.float32(np.nan), X)
    X = np.where(kind == 6, np.float32(0.0), X)
    X = np.where(kind == 7, np.float32(-0.0), X)
    return np.ascontiguousarray(X, np.float32)


MODES = {"plain": (False, None), "reserved-nan": (True, None), "reserved-mv0": (True, 0.0)}


@pytest.mark.gpu
@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("MS", [1, 2, 3, 5, 127, 255])
def test_quantize_edges(monkeypatch, MS, mode):
    """Every N x F of 1 / 63 / 64 / 65 rows and 1 / 63 / 64 / 65 / 129 columns: the non-power-of-two ``top`` search
    (MS = 3, 5, 127, 255), MS = 255 at the 64 KiB LDS edge, columns with fewer than MS thresholds (down to none)."""
    monkeypatch.setenv("TMOG_HIP_QUANTIZE", "1")
    reserve, mv = MODES[mode]
    missing_bin = min(MS + 1, 255) if reserve else -1
    rng = np.random.default_rng(MS * 3 + len(mode))
    seen = set()
    for F in FS:
        thr, n_real = _thresholds(rng, F, MS)
        spec = BinSpec(thr.astype(np.float64), n_real.astype(np.int32), 256, missing_bin, mv)
        for N in NS:
            X = _data(rng, N, thr, n_real)
            got = quantize(torch.from_numpy(X).cuda(), spec)
            assert got.dtype == torch.uint8
            want = _oracle(X, thr, missing_bin, mv)
            np.testing.assert_array_equal(got.cpu().numpy(), want)
            seen |= set(np.unique(want).tolist())
    assert set(range(MS + 1)) <= seen if MS <= 5 else len(seen) > 100          # every bin occurs, NaN's MS included
    assert _loaded()


@pytest.mark.gpu
def test_quantize_stated_bins(monkeypatch):
    """Thresholds (-1, 0, 1, +inf pad): a value equal to a threshold is not past it; 0.0 and -0.0 are the same value
    (bin 1, and with ``missing_value = 0.0`` both are missing, as ``xt == missing_value`` in the torch path has it);
    +inf counts the three real thresholds and not the padding; NaN counts all four, or is missing."""
    monkeypatch.setenv("TMOG_HIP_QUANTIZE", "1")
    f32 = np.float32
    thr = np.array([[-1, 0, 1, np.inf]], np.float64)
    up, dn = (lambda v: np.nextafter(f32(v), f32(np.inf))), (lambda v: np.nextafter(f32(v), f32(-np.inf)))
    x = np.array([-np.inf, dn(-1), -1, up(-1), dn(0), -0.0, 0.0, up(0), dn(1), 1, up(1), np.inf, np.nan], f32)
    plain = [0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 3, 3, 4]
    for missing_bin, mv, want in [(-1, None, plain), (5, None, plain[:-1] + [5]),
                                  (5, 0.0, plain[:5] + [5, 5] + plain[7:-1] + [5])]:
        spec = BinSpec(thr, np.array([3], np.int32), 6, missing_bin, mv)
        got = quantize(torch.from_numpy(x[:, None].copy()).cuda(), spec)
        assert got[:, 0].cpu().tolist() == want
        assert _oracle(x[:, None], thr.astype(f32), missing_bin, mv)[:, 0].tolist() == want
        monkeypatch.setenv("TMOG_HIP_QUANTIZE", "0")
        assert quantize(torch.from_numpy(x[:, None].copy()).cuda(), spec)[:, 0].cpu().tolist() == want   # torch path
        monkeypatch.setenv("TMOG_HIP_QUANTIZE", "1")
    assert _loaded()


@pytest.mark.gpu
def test_quantize_entry_guards_and_write_region():
    """The C entry: MS = 256 (and 0) -> -2 without a launch; a 65 x 65 call writes exactly its N x F bytes of a
    sentinel-filled buffer."""
    from transmogrifai_amd.ops import _native
    lib, st = _native.hip(), _native.stream()
    rng = np.random.default_rng(3)
    N, F, MS = 65, 65, 5
    thr, n_real = _thresholds(rng, F, MS)
    X = _data(rng, N, thr, n_real)
    Xd, td = torch.from_numpy(X).cuda(), torch.from_numpy(thr).cuda()
    pad = 128
    buf = torch.full((pad + N * F + pad,), 0xA5, dtype=torch.uint8, device="cuda")
    big = torch.full((F, 256), float("inf"), dtype=torch.float32, device="cuda")
    assert lib.tmog_hip_quantize(Xd.data_ptr(), N, F, big.data_ptr(), 256, -1, 0, 0.0, buf.data_ptr() + pad, st) == -2
    assert lib.tmog_hip_quantize(Xd.data_ptr(), N, F, big.data_ptr(), 0, -1, 0, 0.0, buf.data_ptr() + pad, st) == -2
    torch.cuda.synchronize()
    assert bool((buf == 0xA5).all())
    assert lib.tmog_hip_quantize(Xd.data_ptr(), N, F, td.data_ptr(), MS, 7, 1, 0.0, buf.data_ptr() + pad, st) == 0
    torch.cuda.synchronize()
    got = buf.cpu().numpy()
    assert (got[:pad] == 0xA5).all() and (got[pad + N * F:] == 0xA5).all()
    np.testing.assert_array_equal(got[pad:pad + N * F].reshape(N, F), _oracle(X, thr, 7, 0.0))
    assert _loaded()
