"""Text-modeling stages: Spark ML text wrappers and the NLP detectors of the reference.

Reference (``core/.../stages/impl/feature/``): ``OpStopWordsRemover.scala``, ``OpNGram.scala``, ``OpCountVectorizer.scala``,
``OpWord2Vec.scala``, ``OpLDA.scala``, ``OpStringIndexer.scala`` / ``OpIndexToString.scala``, ``LangDetector.scala``
(Optimaize), ``NameEntityRecognizer.scala`` (OpenNLP), ``HumanNameDetector.scala`` (+ ``NameDetectUtils.scala``
dictionaries), ``MimeTypeDetector.scala`` (Tika) and ``PhoneNumberParser.scala`` (libphonenumber).

Word2Vec (skip-gram with negative sampling) and LDA (batch variational Bayes) are trained with
dense tensor ops on the engine device (embedding gathers + batched GEMMs); LDA on a wide, mostly zero device
matrix runs its E-step over the non-zeros instead (``ops/lda.py``, HIP). Word2Vec has a second trainer,
``trainer="windows"`` (``ops/word2vec.py``, HIP): whole skip-gram windows from token ids on MFMA tiles, the
negatives shared by a window, minibatch-synchronous and bitwise reproducible for a seed; ``"auto"`` takes it for
a large corpus in a dataset on the device, and the model's transform then averages on the device too. Token
lists are host-resident: such a column counts as a device column when its dataset lives on the device. The
``"pairs"`` trainer is the autograd one over materialised (centre, context) pairs. The JVM NLP libraries and
their model binaries / dictionaries are not available (the reference mount also lacks the large
blobs, ``.MISSING_LARGE_BLOBS``); the detectors here are compact, documented replacements whose exact
outputs are "parity unpinned".
"""
from __future__ import annotations

import math
import re
from collections import Counter
from typing import Dict, List, Optional

import numpy as np
import torch

from ...config import vector_dtype
from ...data.columns import NumericColumn, ObjectColumn, TextColumn, VectorColumn, column_from_values
from ...data.vector_metadata import OpVectorColumnMetadata, OpVectorMetadata
from ...features import types as T
from ...ops import lda as LDA
from ...ops import word2vec as W2V
from ...utils import text as TU
from ..base import UnaryEstimator, UnaryTransformer, register_stage
from .text_stages import detect_mime, is_valid_phone
from .vectorizers import VectorizerMixin, col_meta


# ----------------------------------------------------------------------------------- token list ops
@register_stage
class OpStopWordsRemover(UnaryTransformer):
    operation_name = "stopWordsRemover"
    output_type = T.TextList
    _defaults = {"stop_words": None, "case_sensitive": False}

    def transform_fn(self, v):
        sw = self.params["stop_words"]
        sw = set(sw) if sw is not None else TU.ENGLISH_STOPWORDS
        cs = self.params["case_sensitive"]
        if not cs:
            sw = {w.lower() for w in sw}
        return [t for t in (v or []) if (t if cs else t.lower()) not in sw]


@register_stage
class OpNGram(UnaryTransformer):
    operation_name = "ngram"
    output_type = T.TextList
    _defaults = {"n": 2}

    def transform_fn(self, v):
        n = int(self.params["n"])
        v = list(v or [])
        return [" ".join(v[i:i + n]) for i in range(len(v) - n + 1)]


class _ListVectorModel(VectorizerMixin, UnaryTransformer):
    """Shared: vocabulary-indexed vector output with per-term column metadata."""
    output_type = T.OPVector

    def _meta_terms(self, terms):
        tf = self.get_transient_features()[0]
        return self.vector_metadata([col_meta(tf, descriptor=str(t)) for t in terms])


@register_stage
class OpCountVectorizerModel(_ListVectorModel):
    operation_name = "countVec"

    def __init__(self, vocabulary=None, binary=False, min_tf=1.0, uid=None, **kw):
        super().__init__(None, uid=uid, **kw)
        self.vocabulary = list(vocabulary or [])
        self.binary = binary
        self.min_tf = min_tf

    def _row(self, toks):
        idx = {t: i for i, t in enumerate(self.vocabulary)}
        out = np.zeros(len(self.vocabulary))
        cnt = Counter(t for t in (toks or []) if t in idx)
        n = sum(cnt.values())
        thr = self.min_tf if self.min_tf >= 1 else self.min_tf * max(n, 1)
        for t, c in cnt.items():
            if c >= thr:
                out[idx[t]] = 1.0 if self.binary else float(c)
        return out

    def transform_fn(self, v):
        return self._row(v)

    def transform_columns(self, *cols, ds=None):
        rows = [self._row(v) for v in cols[0].to_list()]
        dev = cols[0].device
        X = torch.as_tensor(np.stack(rows) if rows else np.zeros((0, len(self.vocabulary))),
                            dtype=vector_dtype(dev), device=dev)
        self.metadata["vector_metadata"] = self._meta_terms(self.vocabulary)
        return self._vec(X)

    def ctor_args(self):
        return {"vocabulary": self.vocabulary, "binary": self.binary, "minTF": self.min_tf}

    def load_ctor_args(self, a):
        self.vocabulary, self.binary, self.min_tf = list(a["vocabulary"]), a["binary"], a["minTF"]


@register_stage
class OpCountVectorizer(VectorizerMixin, UnaryEstimator):
    """Vocabulary of the ``vocab_size`` most frequent terms with document frequency >= ``min_df``."""
    operation_name = "countVec"
    output_type = T.OPVector
    _defaults = {"vocab_size": 1 << 18, "min_df": 1.0, "min_tf": 1.0, "binary": False}

    def fit_columns(self, c, ds=None):
        p = self.params
        docs = c.to_list()
        df, tf = Counter(), Counter()
        for d in docs:
            d = d or []
            tf.update(d)
            df.update(set(d))
        n = max(len(docs), 1)
        min_df = p["min_df"] if p["min_df"] >= 1 else p["min_df"] * n
        terms = [t for t in tf if df[t] >= min_df]
        terms.sort(key=lambda t: (-tf[t], t))
        return OpCountVectorizerModel(terms[:int(p["vocab_size"])], p["binary"], p["min_tf"])


@register_stage
class OpWord2VecModel(_ListVectorModel):
    operation_name = "word2Vec"

    def __init__(self, vocabulary=None, vectors=None, uid=None, **kw):
        super().__init__(None, uid=uid, **kw)
        self.vocabulary = list(vocabulary or [])
        self.vectors = None if vectors is None else np.asarray(vectors, np.float32)

    def _row(self, toks):
        idx = {t: i for i, t in enumerate(self.vocabulary)}
        ids = [idx[t] for t in (toks or []) if t in idx]
        dim = 0 if self.vectors is None else self.vectors.shape[1]
        if not ids:
            return np.zeros(dim)
        return self.vectors[ids].mean(0).astype(np.float64)

    def transform_fn(self, v):
        return self._row(v)

    def transform_columns(self, *cols, ds=None):
        dev = cols[0].device
        dim = self.vectors.shape[1]
        docs = cols[0].to_list()
        tdev = _token_device(cols[0], ds)
        if self.vocabulary and W2V.worthwhile(tdev, None, sum(len(d or ()) for d in docs)):
            # document means on the device (ops/csrc/hip/w2v_kernels.hip), in the device's vector dtype
            corpus = W2V.TokenCorpus.from_docs(docs, {t: i for i, t in enumerate(self.vocabulary)}, tdev)
            X = W2V.doc_mean(corpus, torch.from_numpy(self.vectors)).to(vector_dtype(tdev))
        else:
            rows = [self._row(v) for v in docs]
            X = torch.as_tensor(np.stack(rows) if rows else np.zeros((0, dim)), dtype=vector_dtype(dev), device=dev)
        tf = self.get_transient_features()[0]
        self.metadata["vector_metadata"] = self.vector_metadata([col_meta(tf, descriptor=f"w2v_{i}")
                                                                 for i in range(dim)])
        return self._vec(X)

    def find_synonyms(self, word: str, num: int = 5):
        idx = {t: i for i, t in enumerate(self.vocabulary)}
        if word not in idx:
            return []
        V = self.vectors / np.linalg.norm(self.vectors, axis=1, keepdims=True).clip(1e-12)
        s = V @ V[idx[word]]
        order = [i for i in np.argsort(-s) if i != idx[word]][:num]
        return [(self.vocabulary[i], float(s[i])) for i in order]

    def ctor_args(self):
        return {"vocabulary": self.vocabulary, "vectors": self.vectors}

    def load_ctor_args(self, a):
        self.vocabulary = list(a["vocabulary"])
        self.vectors = np.asarray(a["vectors"], np.float32)


def _token_device(c, ds) -> torch.device:
    """Where a token-list column lives: the lists themselves are host-resident, the device is its dataset's."""
    return ds.device if ds is not None and ds.device.type == "cuda" else c.device


@register_stage
class OpWord2Vec(VectorizerMixin, UnaryEstimator):
    """Skip-gram word vectors (negative sampling) trained on the device; a document vector is the mean
    of its word vectors (Spark ``Word2VecModel.transform``). ``trainer``: ``"pairs"`` (autograd over materialised
    pairs, ``batch_size`` pairs a step), ``"windows"`` (``ops/word2vec.py``: HIP, a device column, ``window_size <=
    8``, ``num_negative <= 15``, ``vector_size <= 256``, ``batch_size`` windows a step) or ``"auto"``."""
    operation_name = "word2Vec"
    output_type = T.OPVector
    _defaults = {"vector_size": 100, "window_size": 5, "min_count": 5, "max_iter": 1, "step_size": 0.025,
                 "num_negative": 5, "seed": 0, "batch_size": 4096, "trainer": "auto"}

    def _use_windows(self, c, ds, n_tokens: int) -> bool:
        p = self.params
        if p["trainer"] not in ("auto", "pairs", "windows"):
            raise ValueError(f"trainer must be auto, pairs or windows, got {p['trainer']!r}")
        if p["trainer"] == "auto":
            return W2V.worthwhile(_token_device(c, ds), p, n_tokens)
        if p["trainer"] == "windows":
            bad = W2V.limit_violated(p["vector_size"], p["window_size"], p["num_negative"])
            if bad is None and _token_device(c, ds).type != "cuda":
                bad = "the column must be in a dataset on the device"
            if bad:
                raise ValueError(f'trainer="windows": {bad}')
            from ...ops import _native
            _native.hip()                           # a library that cannot be loaded is an error, not a pairs run
            return True
        return False

    def fit_columns(self, c, ds=None):
        p = self.params
        docs = [list(d or []) for d in c.to_list()]
        cnt = Counter(t for d in docs for t in d)
        vocab = sorted((t for t, n in cnt.items() if n >= p["min_count"]), key=lambda t: (-cnt[t], t))
        dim = int(p["vector_size"])
        if not vocab:
            return OpWord2VecModel([], np.zeros((0, dim), np.float32))
        idx = {t: i for i, t in enumerate(vocab)}
        if self._use_windows(c, ds, sum(cnt[t] for t in vocab)):
            corpus = W2V.TokenCorpus.from_docs(docs, idx, _token_device(c, ds))
            emb = W2V.train(corpus, [cnt[t] for t in vocab], p)
            return OpWord2VecModel(vocab, emb[:, :dim].cpu().numpy())
        dev = torch.device("cuda") if torch.cuda.is_available() and c.device.type == "cuda" else torch.device("cpu")
        pairs = []
        w = int(p["window_size"])
        for d in docs:
            ids = [idx[t] for t in d if t in idx]
            for i, a in enumerate(ids):
                for j in range(max(0, i - w), min(len(ids), i + w + 1)):
                    if j != i:
                        pairs.append((a, ids[j]))
        g = torch.Generator(device="cpu").manual_seed(int(p["seed"]))
        Vn = len(vocab)
        emb_in = ((torch.rand(Vn, dim, generator=g) - 0.5) / dim).to(dev).requires_grad_()
        emb_out = torch.zeros(Vn, dim, device=dev, requires_grad=True)
        if pairs:
            P = torch.as_tensor(pairs, dtype=torch.int64, device=dev)
            freq = torch.as_tensor([cnt[t] for t in vocab], dtype=torch.float64) ** 0.75
            neg_dist = (freq / freq.sum()).to(torch.float32).to(dev)
            opt = torch.optim.SGD([emb_in, emb_out], lr=float(p["step_size"]) * 40)
            bs = int(p["batch_size"])
            for _ in range(int(p["max_iter"])):
                perm = torch.randperm(P.shape[0], generator=g).to(dev)
                for a in range(0, P.shape[0], bs):
                    b = P[perm[a:a + bs]]
                    neg = torch.multinomial(neg_dist, b.shape[0] * int(p["num_negative"]), replacement=True)
                    vi = emb_in[b[:, 0]]
                    pos = (vi * emb_out[b[:, 1]]).sum(1)
                    ng = (vi.repeat_interleave(int(p["num_negative"]), 0) * emb_out[neg]).sum(1)
                    loss = -(torch.nn.functional.logsigmoid(pos).mean() + torch.nn.functional.logsigmoid(-ng).mean())
                    opt.zero_grad()
                    loss.backward()
                    opt.step()
        return OpWord2VecModel(vocab, emb_in.detach().cpu().numpy())


@register_stage
class OpLDAModel(VectorizerMixin, UnaryTransformer):
    operation_name = "lda"
    output_type = T.OPVector

    def __init__(self, topics=None, alpha=None, max_iter=100, uid=None, **kw):
        super().__init__(None, uid=uid, **kw)
        self.topics = None if topics is None else np.asarray(topics, np.float64)   # [K, V] word distributions
        self.alpha = None if alpha is None else np.asarray(alpha, np.float64)
        self.doc_iter = max_iter

    def _infer(self, X: torch.Tensor) -> torch.Tensor:
        lam = torch.as_tensor(self.topics, dtype=torch.float64, device=X.device)
        if LDA.worthwhile(X, lam.shape[0]):         # sparse E-step kernel (ops/csrc/hip/lda_kernels.hip)
            return LDA.e_step(LDA.DocTermCSR(X), torch.log(lam.clamp_min(1e-100)),
                              torch.as_tensor(self.alpha, dtype=torch.float64, device=X.device), self.doc_iter,
                              sstats=False)[0]
        return lda_e_step(X.to(torch.float64), torch.log(lam.clamp_min(1e-100)),
                          torch.as_tensor(self.alpha, dtype=torch.float64, device=X.device), self.doc_iter)[0]

    def transform_fn(self, v):
        x = torch.as_tensor(np.asarray(v, np.float64))[None, :]
        return self._infer(x)[0].numpy()

    def transform_columns(self, *cols, ds=None):
        X = cols[0].values
        th = self._infer(X)
        tf = self.get_transient_features()[0]
        self.metadata["vector_metadata"] = self.vector_metadata(
            [col_meta(tf, descriptor=f"topic_{k}") for k in range(th.shape[1])])
        return self._vec(th.to(vector_dtype(X.device)))

    def describe_topics(self, max_terms: int = 10):
        return [np.argsort(-t)[:max_terms].tolist() for t in self.topics]

    def ctor_args(self):
        return {"topics": self.topics, "alpha": self.alpha, "maxIter": self.doc_iter}

    def load_ctor_args(self, a):
        self.topics, self.alpha = np.asarray(a["topics"]), np.asarray(a["alpha"])
        self.doc_iter = int(a["maxIter"])


def lda_e_step(X, Elogbeta, alpha, iters: int = 100, tol: float = 1e-3):
    """Batched variational E-step: doc-topic Dirichlet ``gamma`` [N, K] and expected topic counts."""
    N, V = X.shape
    K = Elogbeta.shape[0]
    expEb = torch.exp(Elogbeta)                                     # [K, V]
    gamma = torch.ones(N, K, dtype=X.dtype, device=X.device) + X.sum(1, keepdim=True) / K
    # per-document convergence (mean |change| over topics < tol, as Spark's online LDA): a document's
    # result does not depend on the batch it is scored in, so row and batch scoring agree
    active = torch.ones(N, dtype=torch.bool, device=X.device)
    for _ in range(iters):
        Elt = torch.digamma(gamma) - torch.digamma(gamma.sum(1, keepdim=True))
        expEt = torch.exp(Elt)                                      # [N, K]
        phinorm = expEt @ expEb + 1e-100                            # [N, V]
        new = alpha[None, :] + expEt * ((X / phinorm) @ expEb.t())
        conv = (new - gamma).abs().mean(1) < tol
        gamma = torch.where(active[:, None], new, gamma)
        active = active & ~conv
        if not bool(active.any()):
            break
    Elt = torch.digamma(gamma) - torch.digamma(gamma.sum(1, keepdim=True))
    expEt = torch.exp(Elt)
    phinorm = expEt @ expEb + 1e-100
    sstats = expEt.t() @ (X / phinorm) * expEb                      # [K, V]
    theta = gamma / gamma.sum(1, keepdim=True)
    return theta, sstats


@register_stage
class OpLDA(VectorizerMixin, UnaryEstimator):
    """Latent Dirichlet allocation on term-count vectors by batch variational Bayes (Spark ``LDA``)."""
    operation_name = "lda"
    output_type = T.OPVector
    _defaults = {"k": 10, "max_iter": 20, "doc_concentration": None, "topic_concentration": None, "seed": 0}

    def fit_columns(self, c, ds=None):
        p = self.params
        K = int(p["k"])
        # a wide, mostly zero corpus on the device runs the sparse E-step kernel over a CSR built once
        # (ops/csrc/hip/lda_kernels.hip); everything else the dense fp64 E-step below
        csr = LDA.DocTermCSR(c.values) if LDA.worthwhile(c.values, K) else None
        X = c.values.to(torch.float64) if csr is None else c.values
        N, V = X.shape
        alpha = torch.full((K,), float(p["doc_concentration"] or 1.0 / K), dtype=torch.float64, device=X.device)
        eta = float(p["topic_concentration"] or 1.0 / K)
        g = torch.Generator(device="cpu").manual_seed(int(p["seed"]))
        lam = (torch.rand(K, V, generator=g, dtype=torch.float64) * 0.5 + 0.75).to(X.device)
        for _ in range(int(p["max_iter"])):
            Elogbeta = torch.digamma(lam) - torch.digamma(lam.sum(1, keepdim=True))
            if csr is not None:
                sstats = LDA.e_step(csr, Elogbeta, alpha, 50)[1]
            else:
                _, sstats = lda_e_step(X, Elogbeta, alpha, 50)
            lam = eta + sstats
        topics = lam / lam.sum(1, keepdim=True)
        return OpLDAModel(topics.cpu().numpy(), alpha.cpu().numpy())


# -------------------------------------------------------------------------------- string indexing
@register_stage
class OpStringIndexerModel(UnaryTransformer):
    operation_name = "strIdx"
    output_type = T.RealNN

    def __init__(self, labels=None, handle_invalid="error", uid=None, **kw):
        super().__init__(None, uid=uid, **kw)
        self.labels = list(labels or [])
        self.handle_invalid = handle_invalid

    def transform_fn(self, v):
        idx = {l: i for i, l in enumerate(self.labels)}
        if v in idx:
            return float(idx[v])
        if self.handle_invalid == "keep":
            return float(len(self.labels))
        if self.handle_invalid == "skip":
            return None
        raise ValueError(f"Unseen label: {v}. To handle unseen labels, set handle_invalid to skip or keep")

    def transform_columns(self, *cols, ds=None):
        vals = [self.transform_fn(v) for v in cols[0].to_list()]
        if self.handle_invalid == "skip":
            return column_from_values(T.Real, vals, cols[0].device)
        return column_from_values(T.RealNN, vals, cols[0].device)

    def ctor_args(self):
        return {"labels": self.labels, "handleInvalid": self.handle_invalid}

    def load_ctor_args(self, a):
        self.labels, self.handle_invalid = list(a["labels"]), a["handleInvalid"]


@register_stage
class OpStringIndexer(UnaryEstimator):
    """Spark ``StringIndexer`` (frequency-descending labels); ``handle_invalid`` error | skip | keep."""
    operation_name = "strIdx"
    output_type = T.RealNN
    _defaults = {"handle_invalid": "error", "string_order_type": "frequencyDesc"}

    def fit_columns(self, c, ds=None):
        cnt = Counter(v for v in c.to_list() if v is not None)
        order = self.params["string_order_type"]
        if order == "frequencyDesc":
            labels = [v for v, _ in sorted(cnt.items(), key=lambda kv: (-kv[1], kv[0]))]
        elif order == "frequencyAsc":
            labels = [v for v, _ in sorted(cnt.items(), key=lambda kv: (kv[1], kv[0]))]
        elif order == "alphabetDesc":
            labels = sorted(cnt, reverse=True)
        else:
            labels = sorted(cnt)
        self.metadata["labels"] = labels
        return OpStringIndexerModel(labels, self.params["handle_invalid"])


# ``OpIndexToString`` lives in ``indexers.py`` (one class per reference name: the checkpoint registry resolves
# ``com.salesforce.op.stages.impl.feature.OpIndexToString`` by its short name)
from .indexers import OpIndexToString  # noqa: E402,F401


# ---------------------------------------------------------------------------------- NLP detectors
def detect_languages(text: Optional[str]) -> Dict[str, float]:
    """Language identification -> {language: confidence} (Optimaize replacement, ``utils/lang.py``)."""
    from ...utils.lang import detect_languages as _dl
    return _dl(text)


@register_stage
class LangDetector(UnaryTransformer):
    operation_name = "langDet"
    output_type = T.RealMap

    def transform_fn(self, v):
        return detect_languages(v)


_ORG_SUFFIX = {"inc", "inc.", "corp", "corp.", "llc", "ltd", "ltd.", "co", "co.", "company", "corporation",
               "university", "bank", "group", "foundation", "institute"}
_LOC_WORDS = {"street", "avenue", "city", "county", "river", "mountain", "lake", "island", "state", "kingdom"}
_TITLES = {"mr", "mr.", "mrs", "mrs.", "ms", "ms.", "dr", "dr.", "prof", "prof.", "sir", "madam", "miss"}


def recognize_entities(text: Optional[str]) -> Dict[str, frozenset]:
    """Capitalization + cue-word entity tagger -> {Person|Organization|Location: tokens} (OpenNLP replacement)."""
    out: Dict[str, set] = {}
    if not text:
        return {}
    words = re.findall(r"[A-Za-z][\w.'-]*", text)
    i = 0
    while i < len(words):
        w = words[i]
        if w[0].isupper() and i > 0:
            j = i
            while j < len(words) and words[j][0].isupper():
                j += 1
            span = words[i:j]
            nxt = words[j].lower() if j < len(words) else ""
            prev = words[i - 1].lower()
            low = {s.lower() for s in span}
            if low & _ORG_SUFFIX or nxt in _ORG_SUFFIX:
                kind = "Organization"
            elif low & _LOC_WORDS or prev in ("in", "at", "from", "to", "near"):
                kind = "Location"
            else:
                kind = "Person"
            out.setdefault(kind, set()).update(span)
            i = j
        else:
            if w.lower() in _TITLES and i + 1 < len(words):
                out.setdefault("Person", set()).add(words[i + 1])
            i += 1
    return {k: frozenset(v) for k, v in out.items()}


@register_stage
class NameEntityRecognizer(UnaryTransformer):
    operation_name = "nameEntityRec"
    output_type = T.MultiPickListMap

    def transform_fn(self, v):
        return recognize_entities(v)


# Built-in name / gender dictionaries. The reference's (Names_JRC_Combined.txt, GenderDictionary_USandUK.csv,
# NameDetectUtils.scala:217-252) are not in the mount: these are common US first names (with gender) and
# surnames, so which entries count as names is "parity unpinned"; the algorithm around them is the reference's.
_FEMALE = set("""mary patricia jennifer linda elizabeth barbara susan jessica sarah karen nancy lisa betty margaret
sandra ashley kimberly emily donna michelle dorothy carol amanda melissa deborah stephanie rebecca sharon laura
cynthia kathleen amy shirley angela helen anna brenda pamela nicole emma samantha katherine christine debra rachel
catherine carolyn janet ruth maria heather diane virginia julie joyce victoria olivia kelly christina lauren joan
evelyn judith megan cheryl andrea hannah martha jacqueline frances gloria ann teresa kathryn sara janice jean alice
madison doris abigail julia judy grace denise amber marilyn beverly danielle theresa sophia marie diana brittany
natalie isabella charlotte rose alexis kayla florence elsa louisa ellen alyssa shelby ava mia harper chloe ella
lily zoe leah audrey claire lucy paige sydney morgan jasmine haley brooke molly vanessa erin erica monica tiffany
crystal april wendy tina dana valerie gina lori tracy kristen holly kathy peggy connie sally carmen rosa yolanda
""".split())
_MALE = set("""james robert john michael william david richard joseph thomas charles christopher daniel matthew
anthony mark donald steven paul andrew joshua kenneth kevin brian george timothy ronald edward jason jeffrey ryan
jacob gary nicholas eric jonathan stephen larry justin scott brandon benjamin samuel gregory alexander frank
patrick raymond jack dennis jerry tyler aaron jose adam nathan henry douglas zachary peter kyle ethan walter noah
jeremy christian keith roger terry gerald harold sean austin carl arthur lawrence dylan jesse jordan bryan billy
joe bruce gabriel logan albert willie alan juan wayne elijah randy roy vincent ralph eugene russell bobby mason
philip louis owen harry oscar sherrod liam lucas luke isaac caleb connor evan hunter ian jared marcus miguel
carlos luis antonio victor martin travis shawn craig todd derek troy chad curtis dale glenn howard leonard
""".split())
_SURNAMES = set("""smith johnson williams brown jones garcia miller davis rodriguez martinez hernandez lopez gonzalez
wilson anderson thomas taylor moore jackson martin lee perez thompson white harris sanchez clark ramirez lewis
robinson walker young allen king wright scott torres nguyen hill flores green adams nelson baker hall rivera
campbell mitchell carter roberts gomez phillips evans turner diaz parker cruz edwards collins reyes stewart morris
morales murphy cook rogers gutierrez ortiz morgan cooper peterson bailey reed kelly howard ramos kim cox ward
richardson watson brooks chavez wood james bennett gray mendoza ruiz hughes price alvarez castillo sanders patel
myers long ross foster jimenez powell jenkins perry russell sullivan bell coleman butler henderson barnes gonzales
fisher vasquez simmons romero jordan patterson alexander hamilton graham reynolds griffin wallace moreno west cole
hayes bryant herrera gibson ellis tran medina aguilar stevens murray ford castro marshall owens harrison fernandez
mcdonald woods washington kennedy wells vargas henry chen freeman webb tucker guzman burns crawford olson simpson
porter hunter gordon mendez silva shaw snyder mason dixon munoz hunt hicks holmes palmer wagner black robertson
boyd rose stone salazar fox warren mills meyer rice schmidt garza daniels ferguson nichols stephens soto weaver
ryan gardner payne grant dunn kelley spencer hawkins arnold pierce vazquez hansen peters santos hart bradley knight
elliott cunningham duncan armstrong hudson carroll lane riley andrews alvarado ray delgado berry perkins hoffman
""".split())
_NAME_DICT = _FEMALE | _MALE | _SURNAMES
_GENDER_DICT = {**{n: 0.0 for n in _FEMALE}, **{n: 1.0 for n in _MALE}}     # name -> probability male
_MALE_HONORIFICS = frozenset(("mr", "mister", "sir"))
_FEMALE_HONORIFICS = frozenset(("ms", "mrs", "miss", "madam"))
# NameDetectUtils.scala:271-275: the gender strategies, in the reference's (tie-breaking) order
_AFTER_COMMA = r".*,(.*)"
_AFTER_COMMA_NEXT = r".*,\s+.*?\s+(.*)"
GENDER_STRATEGIES = ("FindHonorific", "ByIndex WITH VALUE 0", "ByLast", "ByRegex WITH VALUE " + _AFTER_COMMA,
                     "ByRegex WITH VALUE " + _AFTER_COMMA_NEXT)


def _name_tokens(s: Optional[str]):
    from ...utils.text import tokenize
    return tokenize(s, stopwords=()) if s else []


def _gender_of(name: Optional[str]) -> str:
    p = _GENDER_DICT.get(name) if name is not None else None
    return "GenderNA" if p is None else ("Male" if p >= 0.5 else "Female")


def identify_gender(text: Optional[str], tokens, strategy: str) -> str:
    """One gender strategy on one entry (``NameDetectFun.identifyGender``, NameDetectUtils.scala:120-149)."""
    import re
    if text is None:
        return "GenderNA"
    kind, _, arg = strategy.partition(" WITH VALUE ")
    if kind == "FindHonorific":
        hits = ["Male" if t in _MALE_HONORIFICS else "Female" for t in tokens
                if t in _MALE_HONORIFICS or t in _FEMALE_HONORIFICS]
        return hits[0] if len(hits) == 1 else "GenderNA"
    if kind == "ByIndex":
        i = int(arg)
        return _gender_of(tokens[i] if 0 <= i < len(tokens) else None)
    if kind == "ByLast":
        return _gender_of(tokens[-1] if tokens else None)
    if kind == "ByRegex":
        m = re.fullmatch(arg, text)            # Scala's `case pattern(g)` matches the whole string
        if m is None:
            return "GenderNA"
        toks = _name_tokens(m.group(1))
        return _gender_of(toks[0] if toks else None)
    return "GenderNA"


def parse_name(s: Optional[str]) -> Dict[str, str]:
    """Name map of one entry with every strategy in the reference's order (first inferred gender wins)."""
    if not s:
        return {}
    toks = _name_tokens(s)
    g = next((x for x in (identify_gender(s, toks, st) for st in GENDER_STRATEGIES) if x != "GenderNA"), "GenderNA")
    return {"IsName": "true", "OriginalValue": s, "Gender": g}


@register_stage
class HumanNameDetectorModel(UnaryTransformer):
    """``HumanNameDetectorModel`` (HumanNameDetector.scala:87-116): when the column was judged a name column,
    each entry maps to ``{IsName, OriginalValue, Gender}`` with the gender of the first strategy (in the fitted
    order) that infers one; otherwise the empty map."""
    operation_name = "humanNameDetect"
    output_type = T.NameStats

    def __init__(self, treat_as_name: bool = False, strategies=(), uid=None, **kw):
        super().__init__(None, uid=uid, **kw)
        self.treat_as_name = treat_as_name
        self.ordered_gender_detect_strategies = list(strategies)

    def transform_fn(self, v):
        if not self.treat_as_name:
            return {}
        toks = _name_tokens(v)
        gender = "GenderNA"
        for st in self.ordered_gender_detect_strategies:
            g = identify_gender(v, toks, st)
            if g != "GenderNA":
                gender = g
                break
        return {"IsName": "true", "OriginalValue": v if v is not None else "", "Gender": gender}

    def ctor_args(self):
        return {"treatAsName": self.treat_as_name, "orderedGenderDetectStrategies": self.ordered_gender_detect_strategies}

    def load_ctor_args(self, a):
        self.treat_as_name = bool(a["treatAsName"])
        self.ordered_gender_detect_strategies = list(a.get("orderedGenderDetectStrategies") or
                                                     (GENDER_STRATEGIES if self.treat_as_name else ()))


@register_stage
class HumanNameDetector(UnaryEstimator):
    """``HumanNameDetector`` (HumanNameDetector.scala:56-85, NameDetectUtils.scala:55-198). One pass over the
    column accumulates, per entry: the guard-check quantities (token count below ``guard_max_tokens``, text
    length at least ``guard_min_text_length``, text-length moments, distinct entries -- exact here, HyperLogLog
    in the reference), the fraction of the entry's tokens found in the name dictionary (averaged over entries)
    and each gender strategy's male / female / undetermined counts. Nulls are skipped when ``ignore_nulls``
    (else they count as entries with no name tokens). The column is a name column when every guard passes and
    the average dictionary fraction reaches ``threshold``; the strategies are then ordered by their count of
    undetermined genders (stable: the reference's strategy order breaks ties)."""
    operation_name = "humanNameDetect"
    output_type = T.NameStats
    _defaults = {"threshold": 0.50, "ignore_nulls": True, "guard_max_tokens": 10, "guard_pct_max_tokens": 0.75,
                 "guard_min_text_length": 3, "guard_pct_min_text_length": 0.75, "guard_min_count_std": 10,
                 "guard_min_std": 0.05, "guard_min_count_unique": 10, "guard_min_unique": 10}

    def set_threshold(self, v: float):
        self.params["threshold"] = float(v)
        return self

    def set_ignore_nulls(self, v: bool):
        self.params["ignore_nulls"] = bool(v)
        return self

    def fit_columns(self, c, ds=None):
        import math
        P = self.params
        below = above = 0
        n_len, s_len, s2_len = 0, 0.0, 0.0
        uniq = set()
        dict_sum, dict_n = 0.0, 0
        stats = {st: [0, 0, 0] for st in GENDER_STRATEGIES}
        for v in c.to_list():
            if v is None and P["ignore_nulls"]:
                continue
            toks = _name_tokens(v)
            if v is not None:
                below += len(toks) < P["guard_max_tokens"]
                above += len(v) >= P["guard_min_text_length"]
                n_len += 1
                s_len += len(v)
                s2_len += len(v) * len(v)
                uniq.add(v)
            dict_sum += (sum(t in _NAME_DICT for t in toks) / len(toks)) if toks else 0.0
            dict_n += 1
            for st in GENDER_STRATEGIES:
                g = identify_gender(v, toks, st)
                stats[st][0 if g == "Male" else 1 if g == "Female" else 2] += 1
        N = float(n_len)
        std = math.sqrt(max(s2_len / N - (s_len / N) ** 2, 0.0)) if n_len else 0.0
        guards = n_len > 0 and below / N > P["guard_pct_max_tokens"] and above / N > P["guard_pct_min_text_length"] \
            and (N < P["guard_min_count_std"] or std > P["guard_min_std"]) \
            and (N < P["guard_min_count_unique"] or len(uniq) >= P["guard_min_unique"])
        prob = dict_sum / dict_n if dict_n else 0.0
        treat = bool(guards and prob >= P["threshold"])
        self.metadata["treatAsName"] = treat
        self.metadata["predictedNameProb"] = prob
        self.metadata["genderResultsByStrategy"] = {st: [float(x) for x in v] for st, v in stats.items()}
        order = [st for st, _ in sorted(stats.items(), key=lambda kv: kv[1][2])] if treat else []
        return HumanNameDetectorModel(treat, order)


@register_stage
class MimeTypeDetector(UnaryTransformer):
    """Base64 -> MIME type text (``MimeTypeDetector.scala:47-54``; magic-byte table in place of Tika,
    ``text_stages.detect_mime``). ``type_hint`` / ``max_bytes_to_parse`` as ``MimeTypeDetectorParams``
    (``:86-103``)."""
    operation_name = "mimeDetect"
    output_type = T.Text
    _defaults = {"type_hint": "", "max_bytes_to_parse": 1024}

    def transform_fn(self, v):
        return detect_mime(v, self.params["max_bytes_to_parse"], self.params["type_hint"])


@register_stage
class MimeTypeMapDetector(UnaryTransformer):
    """Base64Map -> PickListMap of each value's MIME type (``MimeTypeDetector.scala:61-77``): keys whose
    value is empty or undecodable are dropped, as the reference's ``collect { case (k, Some(v)) }``."""
    operation_name = "mimeMapDetect"
    output_type = T.PickListMap
    _defaults = {"type_hint": "", "max_bytes_to_parse": 1024}

    def transform_fn(self, m):
        mb, hint = self.params["max_bytes_to_parse"], self.params["type_hint"]
        out = {}
        for k, v in (m or {}).items():
            d = detect_mime(v, mb, hint)
            if d is not None:
                out[k] = d
        return out


def parse_phone(s: Optional[str], region: str = "US", strict: bool = False) -> Optional[str]:
    """E.164 form of a valid number of ``region`` (``PhoneNumberParser.parse``; utils/phone.py)."""
    from ...utils import phone as PH
    return PH.parse(s, region, strict)


@register_stage
class ParsePhoneNumber(UnaryTransformer):
    operation_name = "parsePhone"
    output_type = T.Phone
    _defaults = {"default_region": "US", "strict": False}

    def transform_fn(self, v):
        return parse_phone(v, self.params["default_region"], self.params.get("strict", False))


@register_stage
class IsValidPhoneMapDefaultCountry(UnaryTransformer):
    """PhoneMap -> BinaryMap of validity against the default region (``PhoneNumberParser.scala:241-253``):
    values that cannot be judged (empty / too short) are dropped from the map, as the reference's
    ``collect { case (k, SomeValue(Some(b))) }``."""
    operation_name = "validatePhoneMapNoCC"
    output_type = T.BinaryMap
    _defaults = {"default_region": "US", "strict": False}

    def transform_fn(self, m):
        region, strict = self.params["default_region"], self.params.get("strict", False)
        out = {}
        for k, v in (m or {}).items():
            b = is_valid_phone(v, region, strict) if v is not None else None
            if b is not None:
                out[k] = bool(b)
        return out
