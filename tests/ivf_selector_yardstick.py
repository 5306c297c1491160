"""numpy restatement of the row selector of the inverted-file searches (include/lrx.h, ROW SELECTOR): the bit packing, and a
filtered result as the UNFILTERED full result restricted to the selected rows -- every scanned (query, row) pair is scored independently of
the others, so the restriction is exact on bits.  Nothing here knows how a score is computed: the inputs are an index's own unfiltered
results in ORIGINAL row numbers (id_base = 0, no row_map)."""
import numpy as np


def pack(mask) -> np.ndarray:
    """bool [n] -> int32 [ceil(n / 32)]: bit r is (words[r >> 5] >> (r & 31)) & 1, the bits at and beyond n are 0."""
    mask = np.asarray(mask, dtype=bool).reshape(-1)
    n = mask.shape[0]
    words = np.zeros((n + 31) // 32, dtype=np.uint32)
    for r in np.flatnonzero(mask):
        words[r >> 5] |= np.uint32(1) << np.uint32(r & 31)
    return words.view(np.int32)


def unpack(words, n: int) -> np.ndarray:
    """int32 words -> bool [n]."""
    w = np.asarray(words).astype(np.int32).view(np.uint32)
    return np.array([bool((int(w[r >> 5]) >> (r & 31)) & 1) for r in range(n)], dtype=bool)


def tail_is_clear(words, n: int) -> bool:
    w = np.asarray(words).astype(np.int32).view(np.uint32)
    return len(w) == (n + 31) // 32 and (n % 32 == 0 or int(w[-1]) >> (n % 32) == 0)


def filter_range(lims, D, I, mask):
    """(lims, D, I) of an unfiltered range search -> the same of the search under `mask`: the hits whose row is selected, order kept."""
    lims, D, I = np.asarray(lims, np.int64), np.asarray(D, np.float32), np.asarray(I, np.int64)
    mask = np.asarray(mask, dtype=bool)
    keep = mask[I] if len(I) else np.zeros(0, bool)
    csum = np.concatenate([[0], np.cumsum(keep)]).astype(np.int64)
    return csum[lims], D[keep], I[keep]


def _key(d: np.ndarray) -> np.ndarray:
    """The order of the packed score words: the fp32 bit patterns as a monotone uint32."""
    b = np.asarray(d, np.float32).view(np.uint32).astype(np.uint64)
    return np.where(b >> 31, (~b) & 0xFFFFFFFF, b | 0x80000000).astype(np.int64)


def filter_topk(full_D, full_I, mask, k: int):
    """The top k under `mask` from each query's unfiltered FULL result: full_D / full_I are per-query sequences (rows of a 2-D array, or a
    list of 1-D arrays of any lengths, e.g. the slices of a range search at radius -inf), ids < 0 are padding.  -> (D f32[Q, k], I i64[Q, k]):
    score descending, ties to the lower row, (-FLT_MAX, -1) where fewer than k selected rows were scanned."""
    mask = np.asarray(mask, dtype=bool)
    Q = len(full_D)
    D = np.full((Q, k), -np.finfo(np.float32).max, np.float32)
    I = np.full((Q, k), -1, np.int64)
    for i in range(Q):
        d, r = np.asarray(full_D[i], np.float32), np.asarray(full_I[i], np.int64)
        keep = r >= 0
        keep[keep] = mask[r[keep]]
        d, r = d[keep], r[keep]
        order = np.lexsort((r, -_key(d)))[:k]
        D[i, :len(order)], I[i, :len(order)] = d[order], r[order]
    return D, I


def split(lims, D, I):
    """(lims, D, I) -> the per-query lists filter_topk takes."""
    lims = np.asarray(lims, np.int64)
    return [np.asarray(D)[a:b] for a, b in zip(lims[:-1], lims[1:])], [np.asarray(I)[a:b] for a, b in zip(lims[:-1], lims[1:])]
