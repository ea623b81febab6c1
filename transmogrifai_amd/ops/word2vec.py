"""Window-batched skip-gram with negative sampling on the device (``ops/csrc/hip/w2v_kernels.hip``).

The corpus is its token ids (:class:`TokenCorpus`); a training step takes a batch of positions, forms every
position's window inside ``w2v_window_kernel`` (contexts against the centre word and ``S`` negatives shared by the
window) and scatter-adds the two gradient slabs into the tables with ``w2v_apply_kernel`` over stably sorted keys.
A step is minibatch-synchronous: every window reads the tables as they were at its start, no atomics, so a fit is
bitwise reproducible for a seed. Roles are word2vec.c's: contexts read ``emb_in``, the centre and the negatives
read ``emb_out`` (the pairs trainer of ``OpWord2Vec`` has them the other way round).
"""
from __future__ import annotations

import os

import numpy as np
import torch

MAX_WINDOW = 8         # 2 w <= 16 context slots: the rows of one MFMA tile
MAX_NEGATIVE = 15      # 1 + S <= 16 columns
MAX_DP = 256           # two 16 x Dp fp32 tiles per wave in LDS
# In-vocabulary tokens from which trainer="auto" takes the windows path on a device column. Measured
# (benchmarks/bench_word2vec.py, profiles/word2vec_windows.txt): the windows trainer's fit was faster than the pairs
# trainer's at every swept size, 7x at 1024 tokens, 18x at 4096, 53x at 200 000; no crossover was found above 1024.
# 4096 keeps corpora of a few documents, where both take milliseconds, on the pairs trainer.
AUTO_MIN_TOKENS = 1 << 12


def padded(dim: int) -> int:
    return (int(dim) + 15) // 16 * 16


class TokenCorpus:
    """Token ids of the in-vocabulary tokens of a list of documents, on ``device``: ``tok [T]`` int32, ``doc_ptr
    [N + 1]`` int64 and ``doc_id [T]`` int32. Built once per fit or transform."""

    def __init__(self, tok, doc_ptr, device):
        self.device = torch.device(device)
        self.tok = torch.as_tensor(np.asarray(tok, np.int32)).to(self.device)
        self.doc_ptr = torch.as_tensor(np.asarray(doc_ptr, np.int64)).to(self.device)
        self.n_docs = int(self.doc_ptr.numel()) - 1
        self.n_tokens = int(self.tok.numel())
        if self.n_tokens >= 2**31:
            raise ValueError("TokenCorpus: positions are int32, the corpus has 2**31 tokens or more")
        lens = self.doc_ptr[1:] - self.doc_ptr[:-1]
        self.doc_id = torch.repeat_interleave(torch.arange(self.n_docs, device=self.device), lens) \
            .to(torch.int32).contiguous()

    @classmethod
    def from_docs(cls, docs, index: dict, device) -> "TokenCorpus":
        """``docs``: lists of tokens (None: empty); ``index``: the vocabulary dictionary. Other tokens are dropped."""
        ids, ptr = [], [0]
        for d in docs:
            ids.extend(index[t] for t in (d or ()) if t in index)
            ptr.append(len(ids))
        return cls(ids, ptr, device)

    def valid_slots(self, w: int) -> torch.Tensor:
        """``[T]`` int64: the number of positions within ``w`` of each position inside its document."""
        t = torch.arange(self.n_tokens, device=self.device)
        d = self.doc_id.long()
        return (t - self.doc_ptr[d]).clamp(max=w) + (self.doc_ptr[d + 1] - 1 - t).clamp(max=w)


def limit_violated(vector_size: int, window_size: int, num_negative: int):
    """The limit of the windows trainer that these parameters break, as text, or None."""
    if not 1 <= int(window_size) <= MAX_WINDOW:
        return f"window_size must be in 1..{MAX_WINDOW}, got {window_size}"
    if not 1 <= int(num_negative) <= MAX_NEGATIVE:
        return f"num_negative must be in 1..{MAX_NEGATIVE}, got {num_negative}"
    if not 1 <= int(vector_size) <= MAX_DP:
        return f"vector_size must be in 1..{MAX_DP}, got {vector_size}"
    return None


def worthwhile(device, params, n_tokens: int) -> bool:
    """Whether ``trainer="auto"`` (``params`` of ``OpWord2Vec``) or the model's transform (``params`` None) runs on
    the HIP kernels: a device column within the limits with at least ``AUTO_MIN_TOKENS`` in-vocabulary tokens.
    ``TMOG_W2V_WINDOWS=1`` / ``0`` force the choice. Then the HIP library is needed: if it cannot be built or
    loaded this raises, it does not run the other path."""
    if torch.device(device).type != "cuda" or n_tokens < 1:
        return False
    if params is not None and limit_violated(params["vector_size"], params["window_size"], params["num_negative"]):
        return False
    force = os.environ.get("TMOG_W2V_WINDOWS")
    if force == "0" or (force != "1" and n_tokens < AUTO_MIN_TOKENS):
        return False
    from . import _native as N_
    N_.hip()
    return True


def seg_cap() -> int:
    """Slab rows that ``w2v_apply_kernel`` sums before it cuts a run of equal keys."""
    from . import _native as N_
    return int(N_.hip().tmog_hip_w2v_seg_cap())


def _table(t: torch.Tensor, name: str):
    if t.dtype != torch.float32 or t.dim() != 2 or not t.is_contiguous() or not t.is_cuda or t.shape[1] % 16 or \
            not 16 <= t.shape[1] <= MAX_DP or t.shape[0] < 1:
        raise ValueError(f"{name} must be a contiguous device fp32 [V, Dp] tensor, Dp a multiple of 16 up to {MAX_DP}")


def window_grads(emb_in, emb_out, corpus: TokenCorpus, pos, neg, w: int, n_pos, lr: float):
    """``w2v_window_kernel``: ``(gin, gout [B, 16, Dp], key_in, key_out [B, 16] int32)`` for positions ``pos [B]``
    and negatives ``neg [B, S]`` (int32); ``n_pos``: one int32 on the device, ``a_pos = lr / n_pos``."""
    from . import _native as N_
    _table(emb_in, "emb_in")
    _table(emb_out, "emb_out")
    V, Dp = emb_in.shape
    B = int(pos.numel())
    S = int(neg.shape[1])
    bad = limit_violated(Dp, w, S)
    if bad or tuple(emb_out.shape) != (V, Dp) or tuple(neg.shape) != (B, S):
        raise ValueError(bad or "emb_out must have the shape of emb_in, neg must be [B, S]")
    dev = emb_in.device
    pos = pos.to(device=dev, dtype=torch.int32).contiguous()
    neg = neg.to(device=dev, dtype=torch.int32).contiguous()
    n_pos = n_pos.to(device=dev, dtype=torch.int32).contiguous()
    gin = torch.empty(B, 16, Dp, dtype=torch.float32, device=dev)
    gout = torch.empty(B, 16, Dp, dtype=torch.float32, device=dev)
    key_in = torch.empty(B, 16, dtype=torch.int32, device=dev)
    key_out = torch.empty(B, 16, dtype=torch.int32, device=dev)
    N_.check(N_.hip().tmog_hip_w2v_window(N_.ptr(emb_in), N_.ptr(emb_out), V, Dp, N_.ptr(corpus.tok), corpus.n_tokens,
                                          N_.ptr(corpus.doc_ptr), N_.ptr(corpus.doc_id), N_.ptr(pos), N_.ptr(neg), B,
                                          int(w), S, N_.ptr(n_pos), float(lr), N_.ptr(gin), N_.ptr(gout),
                                          N_.ptr(key_in), N_.ptr(key_out), N_.stream(dev)), "w2v_window")
    return gin, gout, key_in, key_out


def apply_rows(emb: torch.Tensor, slab: torch.Tensor, keys: torch.Tensor) -> None:
    """``emb[keys[i]] += slab[i]`` for every slab row whose key is below ``V``, in place, in an order fixed by a
    stable sort of the keys (``w2v_apply_kernel``)."""
    from . import _native as N_
    _table(emb, "emb")
    V, Dp = emb.shape
    slab = slab.reshape(-1, Dp)
    M = int(slab.shape[0])
    if slab.dtype != torch.float32 or not slab.is_contiguous() or keys.numel() != M or keys.dtype != torch.int32:
        raise ValueError("slab must be contiguous fp32 [M, Dp] and keys int32 [M]")
    skey, order = torch.sort(keys.reshape(-1), stable=True)
    n_chunk = (M + seg_cap() - 1) // seg_cap()
    partial = torch.empty(max(n_chunk, 1) * 2 * Dp, dtype=torch.float32, device=emb.device)
    tail = torch.empty(max(n_chunk, 1), dtype=torch.int32, device=emb.device)
    N_.check(N_.hip().tmog_hip_w2v_apply(N_.ptr(emb), V, Dp, N_.ptr(slab), N_.ptr(skey), N_.ptr(order), M,
                                         N_.ptr(partial), N_.ptr(tail), N_.stream(emb.device)), "w2v_apply")


def step(emb_in, emb_out, corpus: TokenCorpus, pos, neg, w: int, step_size: float, n_pos=None) -> None:
    """One minibatch-synchronous SGD step at rate ``40 * step_size`` on the loss of the pairs trainer (mean log
    sigmoid over the positive cells plus mean over the negative cells): in place on both tables. ``n_pos`` (the
    valid context slots of the batch, one int32 on the device) is computed here when not given."""
    if n_pos is None:
        n_pos = corpus.valid_slots(int(w))[pos.long()].sum().to(torch.int32).reshape(1)
    gin, gout, key_in, key_out = window_grads(emb_in, emb_out, corpus, pos, neg, w, n_pos, 40.0 * float(step_size))
    apply_rows(emb_in, gin, key_in)
    apply_rows(emb_out, gout, key_out)


def train(corpus: TokenCorpus, counts, params) -> torch.Tensor:
    """``emb_in [V, Dp]`` after ``max_iter`` epochs of ``ceil(T / batch_size)`` steps (``batch_size`` windows each).
    ``counts``: the vocabulary's term counts (negatives follow ``count ** 0.75``). ``emb_in`` starts as in the pairs
    trainer (seeded CPU generator); permutations and negatives come from a seeded device generator."""
    dev = corpus.device
    dim, w, S = int(params["vector_size"]), int(params["window_size"]), int(params["num_negative"])
    bs, T, Vn = int(params["batch_size"]), corpus.n_tokens, len(counts)
    g = torch.Generator(device="cpu").manual_seed(int(params["seed"]))
    emb_in = torch.zeros(Vn, padded(dim), device=dev)
    emb_in[:, :dim] = ((torch.rand(Vn, dim, generator=g) - 0.5) / dim).to(dev)
    emb_out = torch.zeros(Vn, padded(dim), device=dev)
    freq = torch.as_tensor(list(counts), dtype=torch.float64) ** 0.75
    neg_dist = (freq / freq.sum()).to(torch.float32).to(dev)
    gd = torch.Generator(device=dev).manual_seed(int(params["seed"]))
    slots = corpus.valid_slots(w)
    steps = (T + bs - 1) // bs
    for _ in range(int(params["max_iter"])):
        perm = torch.randperm(T, generator=gd, device=dev)
        neg = torch.multinomial(neg_dist, T * S, replacement=True, generator=gd).view(T, S).to(torch.int32)
        n_pos = torch.zeros(steps * bs, dtype=torch.int64, device=dev)
        n_pos[:T] = slots[perm]
        n_pos = n_pos.view(steps, bs).sum(1).to(torch.int32)       # per step, on the device: no synchronisation
        pos = perm.to(torch.int32)
        for s in range(steps):
            a = s * bs
            step(emb_in, emb_out, corpus, pos[a:a + bs], neg[a:a + bs], w, params["step_size"], n_pos[s:s + 1])
    return emb_in


def doc_mean(corpus: TokenCorpus, vectors: torch.Tensor) -> torch.Tensor:
    """``[N, D]`` fp32: the mean of ``vectors[tok]`` over each document's tokens in fp64, zeros for an empty one
    (``w2v_doc_mean_kernel``)."""
    from . import _native as N_
    dev = corpus.device
    vectors = vectors.to(device=dev, dtype=torch.float32).contiguous()
    V, D = vectors.shape
    out = torch.empty(corpus.n_docs, D, dtype=torch.float32, device=dev)
    N_.check(N_.hip().tmog_hip_w2v_doc_mean(N_.ptr(vectors), V, D, N_.ptr(corpus.tok), N_.ptr(corpus.doc_ptr),
                                            corpus.n_docs, N_.ptr(out), N_.stream(dev)), "w2v_doc_mean")
    return out
