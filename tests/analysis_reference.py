"""Numpy restatement of the embedding analysis (clibd_amd.analysis, include/clibd_hip_analysis.h): the oracle of the analysis tests.

  silhouette_fp64          sklearn's silhouette_samples in float64, distances in the difference form (no cancellation)
  silhouette_fp32_gram     the kernel's formula in float32 — fp32 norms, an fp32 Gram product, d = sqrt(max(n_i + n_j - 2 g, 0)), fp32 sums
                           and means — whose error against silhouette_fp64 sizes the GPU tests' gate
  silhouette_chunked       the kernel's bookkeeping in float64: per (row, column chunk) a head and a tail partial sum, the segments strictly
                           inside a chunk folded at once, then the chunks stitched in order (the finalize step)
  nearest_fp64             per query the distance to (and the row of) the nearest key with the query's label
  confusion_np             np.add.at counts, -1 codes skipped
"""
from __future__ import annotations

import numpy as np


def _runs(codes):
    order = np.argsort(codes, kind="stable")
    _, counts = np.unique(codes, return_counts=True)
    seg = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    return order, seg


def _from_distances(d: np.ndarray, codes: np.ndarray, dtype) -> np.ndarray:
    """a, b and s from a full distance matrix with a zero diagonal, every sum and quotient in `dtype`"""
    N = len(codes)
    uniq, inv, counts = np.unique(codes, return_inverse=True, return_counts=True)
    sums = np.zeros((N, len(uniq)), dtype=dtype)
    for c in range(len(uniq)):
        sums[:, c] = d[:, inv == c].sum(axis=1, dtype=dtype)
    own = counts[inv]
    a = sums[np.arange(N), inv] / np.maximum(own - 1, 1).astype(dtype)
    means = sums / counts[None, :].astype(dtype)
    means[np.arange(N), inv] = np.inf
    b = means.min(axis=1)
    m = np.maximum(a, b)
    with np.errstate(invalid="ignore", divide="ignore"):
        s = np.where(m > 0, (b - a) / m, 0).astype(dtype)
    s[own == 1] = 0
    return s


def silhouette_fp64(X, codes) -> np.ndarray:
    X = np.asarray(X, dtype=np.float64)
    codes = np.asarray(codes)
    d = np.sqrt(((X[:, None, :] - X[None, :, :]) ** 2).sum(axis=2)) if X.shape[0] * X.shape[0] * X.shape[1] <= 5e7 else None
    if d is None:
        d = np.empty((len(X), len(X)))
        for i in range(len(X)):
            d[i] = np.sqrt(((X[i][None, :] - X) ** 2).sum(axis=1))
    np.fill_diagonal(d, 0.0)
    return _from_distances(d, codes, np.float64)


def distances_fp32_gram(X) -> np.ndarray:
    X = np.asarray(X, dtype=np.float32)
    n = (X * X).sum(axis=1, dtype=np.float32)
    g = X @ X.T
    d2 = (n[:, None] + n[None, :]) - np.float32(2) * g
    d = np.sqrt(np.maximum(d2, np.float32(0)))
    np.fill_diagonal(d, np.float32(0))
    assert d.dtype == np.float32
    return d


def silhouette_fp32_gram(X, codes) -> np.ndarray:
    return _from_distances(distances_fp32_gram(X), np.asarray(codes), np.float32)


def silhouette_chunked(X_sorted, seg, col_chunk: int) -> np.ndarray:
    """float64, rows already sorted by cluster, with the kernel's head / tail / fold bookkeeping (a transliteration, row by row)"""
    X = np.asarray(X_sorted, dtype=np.float64)
    seg = np.asarray(seg, dtype=np.int64)
    N, C = len(X), len(seg) - 1
    cid = np.repeat(np.arange(C), np.diff(seg))
    size = np.diff(seg)
    chunks = [(c0, min(c0 + col_chunk, N)) for c0 in range(0, N, col_chunk)]
    out = np.zeros(N)
    for i in range(N):
        d = np.sqrt(((X[i][None, :] - X) ** 2).sum(axis=1))
        d[i] = 0.0
        my = cid[i]
        part = []
        for c0, c1 in chunks:           # the tile kernel: one (row, chunk) pair
            first, cur, run = cid[c0], cid[c0], 0.0
            head = tail = own = 0.0
            bmin = np.inf
            for c in range(c0, c1):
                if cid[c] != cur:
                    if cur == first:
                        head = run
                    elif cur == my:
                        own = run
                    else:
                        bmin = min(bmin, run / size[cur])
                    cur, run = cid[c], 0.0
                run += d[c]
            if cur == first:
                head = run
            else:
                tail = run
            part.append((head, tail, bmin, own))
        bmin, own, run, cur = np.inf, 0.0, 0.0, -1   # the finalize kernel

        def close():
            nonlocal bmin, own
            if cur < 0:
                return
            if cur == my:
                own = run
            else:
                bmin = min(bmin, run / size[cur])

        for (c0, c1), (head, tail, pmin, pown) in zip(chunks, part):
            first, last = cid[c0], cid[c1 - 1]
            if first == cur:
                run += head
            else:
                close()
                cur, run = first, head
            bmin = min(bmin, pmin)
            if first < my < last:
                own = pown
            if last != first:
                close()
                cur, run = last, tail
        close()
        if size[my] > 1:
            a = own / (size[my] - 1)
            m = max(a, bmin)
            out[i] = (bmin - a) / m if m > 0 else 0.0
    return out


def nearest_fp64(Q, K, qlabels, klabels):
    """(dist [Nq], arg [Nq], runner_up [Nq]): the nearest key with the query's label (the lowest row on a tie), and the distance of the
    second nearest such key (+inf if none); +inf / -1 where no key carries the label"""
    Q, K = np.asarray(Q, dtype=np.float64), np.asarray(K, dtype=np.float64)
    klabels = np.asarray(klabels)
    dist = np.full(len(Q), np.inf)
    second = np.full(len(Q), np.inf)
    arg = np.full(len(Q), -1, dtype=np.int64)
    for i, lab in enumerate(qlabels):
        rows = np.nonzero(klabels == lab)[0]
        if len(rows) == 0:
            continue
        d = np.sqrt(((Q[i][None, :] - K[rows]) ** 2).sum(axis=1))
        j = int(np.argmin(d))
        dist[i], arg[i] = d[j], rows[j]
        if len(rows) > 1:
            second[i] = np.partition(d, 1)[1]
    return dist, arg, second


def confusion_np(true_code, pred_code, C: int) -> np.ndarray:
    t, p = np.asarray(true_code), np.asarray(pred_code)
    ok = (t >= 0) & (p >= 0)
    cm = np.zeros((C, C), dtype=np.int64)
    np.add.at(cm, (t[ok], p[ok]), 1)
    return cm
