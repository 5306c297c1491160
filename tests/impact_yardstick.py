"""numpy restatement of the impact index's contract (include/lrx.h, lrx_impact_search): Lucene impact search over a
JsonVectorCollection.  S(q, r) = sum_t count_q[t] * weight_r[t] accumulated in int64, a row is a hit iff S >= 1, the returned score is
np.float32(S) (one round-to-nearest-even conversion), the hits are ranked by that float descending with ties to the lower row, a list
shorter than k is padded with (-FLT_MAX, -1).  Terms the documents never brought contribute nothing."""
from collections import Counter

import numpy as np

FLT_MAX = np.finfo(np.float32).max


class Yardstick:
    """Documents as a ragged CSR (doc_terms / doc_weights [nnz], doc_offsets [n + 1]), rows in that order."""

    def __init__(self, doc_terms, doc_weights, doc_offsets):
        terms, weights, off = (np.asarray(a, dtype=np.int64) for a in (doc_terms, doc_weights, doc_offsets))
        self.n = off.size - 1
        rows = np.repeat(np.arange(self.n, dtype=np.int64), np.diff(off))
        order = np.argsort(terms, kind="stable")
        self.terms, self.rows, self.weights = terms[order], rows[order], weights[order]

    def scores(self, q_terms, q_counts) -> np.ndarray:
        """The exact integer scores of one query, int64 [n]."""
        S = np.zeros(self.n, dtype=np.int64)
        for t, c in zip(np.asarray(q_terms, dtype=np.int64).tolist(), np.asarray(q_counts, dtype=np.int64).tolist()):
            a, b = np.searchsorted(self.terms, t, "left"), np.searchsorted(self.terms, t, "right")
            np.add.at(S, self.rows[a:b], c * self.weights[a:b])
        return S

    def search(self, queries, k: int):
        """queries: [(term ids, counts), ...] -> (D fp32 [Q, k], I int64 [Q, k])."""
        D = np.full((len(queries), k), -FLT_MAX, np.float32)
        I = np.full((len(queries), k), -1, np.int64)
        for i, (t, c) in enumerate(queries):
            S = self.scores(t, c)
            hits = np.flatnonzero(S >= 1)
            f = S[hits].astype(np.float32)
            o = np.argsort(-f, kind="stable")[:k]                # hits ascend by row: stable = ties to the lower row
            D[i, :o.size], I[i, :o.size] = f[o], hits[o]
        return D, I


def csr_of(pairs):
    """[(ids, values), ...] -> (ids [nnz], values [nnz], offsets [n + 1]) int64."""
    off = np.zeros(len(pairs) + 1, dtype=np.int64)
    off[1:] = np.cumsum([len(t) for t, _ in pairs])
    cat = lambda xs: np.concatenate([np.asarray(x, dtype=np.int64).reshape(-1) for x in xs]) if xs else np.zeros(0, np.int64)
    return cat([t for t, _ in pairs]), cat([v for _, v in pairs]), off


def vocabulary(docs, vocab=None) -> dict:
    """str -> int in first-seen order over a list of {term: weight} dicts."""
    vocab = {} if vocab is None else vocab
    for d in docs:
        for t in d:
            vocab.setdefault(t, len(vocab))
    return vocab


def query_pairs(vocab: dict, query):
    """A {term: count} dict or pseudo text ("tok tok ...": split on whitespace, counted) -> (term ids, counts); unknown terms dropped."""
    if isinstance(query, str):
        query = Counter(query.split())
    kept = [(vocab[t], int(c)) for t, c in query.items() if t in vocab]
    return [t for t, _ in kept], [c for _, c in kept]


def search_dicts(docs, doc_ids, queries, query_ids, k: int) -> dict:
    """The engine-level form: {term: weight} documents, dict / pseudo-text queries -> {qid: {pid: float score}}."""
    vocab = vocabulary(docs)
    y = Yardstick(*csr_of([([vocab[t] for t in d], [int(w) for w in d.values()]) for d in docs]))
    D, I = y.search([query_pairs(vocab, q) for q in queries], k)
    return {qid: {doc_ids[r]: float(s) for s, r in zip(D[i], I[i]) if r >= 0} for i, qid in enumerate(query_ids)}
