"""Restatement of the k-means vector quantisation of casualhdrsplat_amd/csrc/vq.hip (hs_vq_assign, hs_vq_update) in numpy.

assign: float32, explicit loops over k and d -- acc = 0; for d ascending: t = x[i,d] - c[k,d]; acc = acc + t * t, every
operation rounded to float32 once (numpy's elementwise float32 arithmetic is IEEE; np.sum is NOT used: its pairwise order
differs) --, then k ascending with a strict < against a running best that starts at +inf.  The kernel must give these bits.
update: float64 weighted means per cluster; a cluster whose weight sum is not positive keeps the previous row.  The kernel adds
in another (fixed) order, so the comparison carries the bound of tests/test_vq_gpu.py.
"""
import numpy as np


def assign(x, codebook):
    """(codes int32 [N], dist2 float32 [N])"""
    x = np.ascontiguousarray(x, np.float32)
    c = np.ascontiguousarray(codebook, np.float32)
    N, D = x.shape
    K = c.shape[0]
    assert c.shape[1] == D
    best = np.full(N, np.inf, np.float32)
    code = np.zeros(N, np.int32)
    with np.errstate(invalid="ignore", over="ignore"):
        for k in range(K):
            acc = np.zeros(N, np.float32)
            for d in range(D):
                t = x[:, d] - c[k, d]
                acc = acc + t * t
            assert acc.dtype == np.float32
            win = acc < best          # False for NaN
            best = np.where(win, acc, best)
            code = np.where(win, np.int32(k), code)
    return code, best


def update(x, codes, codebook, weights=None):
    """(new codebook float32 [K, D], counts int32 [K], bound float64 [K, D]): bound = sum w |x| / S_w per element (0 where the
    previous row is kept), the scale of the fp64 summation error."""
    x64 = np.asarray(x, np.float64)
    prev = np.ascontiguousarray(codebook, np.float32)
    K, D = prev.shape
    N = x64.shape[0]
    w = np.ones(N, np.float64) if weights is None else np.asarray(weights, np.float64)
    codes = np.asarray(codes, np.int64)
    inside = (codes >= 0) & (codes < K)
    counts = np.bincount(codes[inside], minlength=K).astype(np.int32)
    sw = np.zeros(K, np.float64)
    np.add.at(sw, codes[inside], w[inside])
    sd = np.zeros((K, D), np.float64)
    np.add.at(sd, codes[inside], w[inside, None] * x64[inside])
    sa = np.zeros((K, D), np.float64)
    np.add.at(sa, codes[inside], w[inside, None] * np.abs(x64[inside]))
    out = prev.copy()
    bound = np.zeros((K, D), np.float64)
    live = sw > 0
    out[live] = (sd[live] / sw[live, None]).astype(np.float32)
    bound[live] = sa[live] / sw[live, None]
    ref64 = np.where(live[:, None], sd / np.where(live, sw, 1.0)[:, None], prev.astype(np.float64))
    return out, counts, bound, ref64


def objective(dist2, weights=None):
    """sum w dist2 in float64"""
    d = np.asarray(dist2, np.float64)
    return float(d.sum() if weights is None else (np.asarray(weights, np.float64) * d).sum())


def planted(seed=0, K=8, D=45, per=400, spread=4.0, sigma=0.25):
    """K blobs of `per` rows: centres spread * N(0, 1), rows centre + sigma * N(0, 1), shuffled.
    -> (x float32 [K per, D], labels [K per], centres float64 [K, D], one row index per blob)"""
    rng = np.random.default_rng(seed)
    centres = spread * rng.standard_normal((K, D))
    labels = np.repeat(np.arange(K), per)
    x = centres[labels] + sigma * rng.standard_normal((K * per, D))
    order = rng.permutation(K * per)
    x, labels = x[order].astype(np.float32), labels[order]
    first = np.array([int(np.flatnonzero(labels == k)[0]) for k in range(K)])
    return x, labels, centres, first


def lloyd(x, init_rows, iters, weights=None):
    """The loop of vq.kmeans on the restatements: (codebook, codes, dist2, objective per assignment)."""
    book = np.ascontiguousarray(x[init_rows], np.float32)
    trace = []
    for _ in range(iters):
        codes, d2 = assign(x, book)
        trace.append(objective(d2, weights))
        book = update(x, codes, book, weights)[0]
    codes, d2 = assign(x, book)
    trace.append(objective(d2, weights))
    return book, codes, d2, trace
