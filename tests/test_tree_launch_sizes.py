"""The launch arithmetic of the tree level kernels that can be asked for without a launch:
``tmog_hip_hist_stat_chunk`` (the histogram LDS size, ``tree_hist_kernels.hip``) and ``tmog_hip_split_cand_bytes``
(the scans' feature-block bound, ``tree_split_kernels.hip``) against values recorded before those formulas were
given one definition each (``tests/golden/tree_launch_sizes.json``; ``TMOG_SPLIT_FPB`` unset).

Neither entry touches the device, and the library loads without one, so this needs no GPU: it loads the library
itself (``N.hip()`` initialises the device first)."""
import ctypes
import json
import pathlib

from transmogrifai_amd.ops import _native as N, build


def test_launch_sizes_match_the_recorded_values(monkeypatch):
    monkeypatch.delenv("TMOG_SPLIT_FPB", raising=False)
    path = build.build_hip()
    build.verify(path, "hip")
    lib = ctypes.CDLL(str(path))
    N._declare(lib, {k: N._HIP_SIGS[k] for k in ("tmog_hip_hist_stat_chunk", "tmog_hip_split_cand_bytes")})
    g = json.loads((pathlib.Path(__file__).parent / "golden" / "tree_launch_sizes.json").read_text())
    Bs, Ss, Fs, Ns = g["B"], g["S"], g["max_nfeat"], g["n_nodes"]
    assert (Bs, Ss, Fs, Ns) == ([2, 32, 64, 65, 256], [1, 2, 3, 4, 5, 16, 17, 256], [1, 15, 16, 17, 329], [1, 7])
    assert [[lib.tmog_hip_hist_stat_chunk(b, s) for s in Ss] for b in Bs] == g["hist_stat_chunk"]
    got = [[[[lib.tmog_hip_split_cand_bytes(n, f, b, s) for s in Ss] for b in Bs] for f in Fs] for n in Ns]
    assert got == g["split_cand_bytes"]
