"""Numpy / plain-Python model of the graph index (lightretriever_amd/graph.py, lrx_graph_ip_search / lrx_graph_detour_counts):
the four build steps over a score table, and the beam search over a score row -- with an exact visited set, or one that forgets everything
but the beam at chosen steps (what the kernel's LDS table does when it fills).  A helper, not a test.

Every order is (score descending, row ascending) on the bits of the fp32 scores -- the order of the library's packed words."""
from __future__ import annotations

import math

import numpy as np


def score_keys(scores: np.ndarray) -> np.ndarray:
    """fp32 scores -> int64 keys, larger = better: the library's monotone map of the float bits (f2key)."""
    u = np.ascontiguousarray(scores, dtype=np.float32).view(np.uint32).astype(np.int64)
    return np.where(u & 0x80000000, 0xFFFFFFFF - u, u | 0x80000000)


def ranking(keys: np.ndarray) -> np.ndarray:
    """Rows in (key descending, row ascending) order."""
    return np.lexsort((np.arange(keys.shape[0]), -keys))


# -- build ------------------------------------------------------------------------------------------------------------------------------
def knn_lists(S: np.ndarray, K: int) -> np.ndarray:
    """Step 1: S fp32 [n, n], S[u, v] = score of row v for query row u -> int32 [n, K].  The K + 1 best rows of u (u itself competes), u
    dropped -- or the last of them when u is not among them -- and -1 where n - 1 < K."""
    n = S.shape[0]
    keys = score_keys(S)
    out = np.full((n, K), -1, dtype=np.int32)
    for u in range(n):
        top = [int(v) for v in ranking(keys[u])[:K + 1]]
        if u in top:
            top.remove(u)
        else:
            top.pop()
        out[u, :len(top)] = top[:K]
    return out


def detour_counts(knn: np.ndarray) -> np.ndarray:
    """Step 2: counts[u][c] = the pairs (a, b) with v = knn[u][a], w = knn[v][b], w at position c > max(a, b) of knn[u] (its first position);
    -1 entries take no part."""
    n, K = knn.shape
    counts = np.zeros((n, K), dtype=np.int32)
    pos = np.arange(K)
    floor = np.maximum(pos[:, None], pos[None, :])            # max(a, b)
    where = np.full(n + 1, -1, dtype=np.int64)                # row -> its first position in knn[u]; slot n serves the -1 entries
    for u in range(n):
        mine = knn[u]
        valid = mine >= 0
        where[mine[valid][::-1]] = pos[valid][::-1]
        two_hop = knn[np.where(valid, mine, 0)]               # [a, b] = w
        c = np.where(valid[:, None], where[np.where(two_hop >= 0, two_hop, n)], -1)
        counts[u] = np.bincount(c[c > floor], minlength=K)
        where[mine[valid]] = -1
    return counts


def prune(knn: np.ndarray, counts: np.ndarray, R: int) -> np.ndarray:
    """Step 3: the rows at the R positions with the fewest detours, ties to the lower position; empty slots after every row."""
    n, K = knn.shape
    out = np.full((n, R), -1, dtype=np.int32)
    for u in range(n):
        pos = sorted(range(K), key=lambda c: (knn[u, c] < 0, int(counts[u, c]), c))[:R]
        out[u, :len(pos)] = knn[u, pos]
    return out


def merge_reverse(pruned: np.ndarray) -> np.ndarray:
    """Step 4: rev[v] = rows u with v in pruned[u] by (position of v in pruned[u], u), cut to R / 2; graph[u] = the first R distinct entries of
    pruned[u][:R/2] ++ rev[u] ++ pruned[u][R/2:], padded with -1."""
    n, R = pruned.shape
    h = R // 2
    rev = [[] for _ in range(n)]
    for j in range(R):
        for u in range(n):
            v = int(pruned[u, j])
            if v >= 0 and len(rev[v]) < h:
                rev[v].append(u)
    graph = np.full((n, R), -1, dtype=np.int32)
    for u in range(n):
        seen, row = set(), []
        for v in [int(x) for x in pruned[u, :h]] + rev[u] + [int(x) for x in pruned[u, h:]]:
            if v >= 0 and v not in seen:
                seen.add(v)
                row.append(v)
        graph[u, :min(len(row), R)] = row[:R]
    return graph


def build_graph(knn: np.ndarray, R: int) -> np.ndarray:
    return merge_reverse(prune(knn, detour_counts(knn), R))


def entry_rows(n: int, n_entry: int) -> np.ndarray:
    return (np.arange(n_entry, dtype=np.int64) * n) // max(n_entry, 1)


def best_entries(score_row: np.ndarray, entries: np.ndarray, m: int) -> np.ndarray:
    """What the index hands the kernel: the best m of the entry rows for this query, -1 padded."""
    order = ranking(score_keys(score_row[entries]))[:m]
    out = np.full(m, -1, dtype=np.int64)
    out[:order.shape[0]] = entries[order]
    return out


# -- search -----------------------------------------------------------------------------------------------------------------------------
def beam_search(score_row: np.ndarray, graph: np.ndarray, entries, k: int, beam: int, width: int, max_iterations: int = 0, forget_at=()):
    """-> (ids int64 [k], scores fp32 [k], steps, rows scored): the traversal of lrx_graph_ip_search for one query over its score row (fp32 [n]).
    forget_at: steps (0-based) before whose gather the visited set is cut down to the beam's rows."""
    n = graph.shape[0]
    keys = score_keys(score_row)
    order = lambda rows: sorted(rows, key=lambda r: (-int(keys[r]), r))
    visited, scored = set(), 0

    def fresh(rows):
        out = []
        for r in rows:
            r = int(r)
            if 0 <= r < n and r not in visited:
                visited.add(r)
                out.append(r)
        return out

    new = fresh(entries)
    scored += len(new)
    members = order(new)[:beam]
    expanded = set()
    steps = 0
    limit = max_iterations if max_iterations > 0 else math.ceil(beam / width) + 32
    while steps < limit:
        parents = [r for r in members if r not in expanded][:width]
        if not parents:
            break
        if steps in forget_at:
            visited = set(members)
        expanded.update(parents)
        new = fresh(v for p in parents for v in graph[p])
        scored += len(new)
        members = order(members + new)[:beam]
        expanded &= set(members)          # a mark travels with its entry and leaves with it
        steps += 1
    ids = np.full(k, -1, dtype=np.int64)
    out = np.full(k, -np.finfo(np.float32).max, dtype=np.float32)
    top = members[:k]
    ids[:len(top)] = top
    out[:len(top)] = score_row[top]
    return ids, out, steps, scored


def clustered_corpus(n: int, d: int, n_clusters: int, n_queries: int, seed: int = 0):
    """(x fp32 [n, d], q fp32 [n_queries, d]): Gaussian clusters (centres N(0, 1), noise 0.5), rows normalised; the queries are drawn the
    same way."""
    rng = np.random.default_rng(seed)
    centres = rng.standard_normal((n_clusters, d))

    def draw(m):
        v = centres[rng.integers(0, n_clusters, m)] + 0.5 * rng.standard_normal((m, d))
        return (v / np.linalg.norm(v, axis=1, keepdims=True)).astype(np.float32)
    return draw(n), draw(n_queries)
