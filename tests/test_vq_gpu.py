"""k-means SH codebook compression on the GPU (vq.hip): the assignment bit for bit against the numpy float32 restatement,
the update against float64 under a derived bound, reproducibility whatever the workspace held, and the loop on a planted and
on a random problem.  Seconds each."""
import functools

import numpy as np
import pytest
import torch

import vq_reference as R

pytestmark = pytest.mark.gpu
DEV = "cuda"
N = 3001                                                  # no multiple of 64, of 256 or of the 512 rows of a workgroup


def gpu(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def bits(t):
    return t.detach().cpu().contiguous().view(torch.int32).numpy()


# ---- assign ----

@functools.lru_cache(maxsize=None)
def assign_case(D, K):
    """Rows and a codebook with every special the definition names: rows that are copies of centroids (distance 0),
    duplicated codebook rows (the lower index must win), near ties, one NaN row."""
    rng = np.random.default_rng(1000 * D + K)
    x = rng.standard_normal((N, D)).astype(np.float32)
    book = rng.standard_normal((K, D)).astype(np.float32)
    take = rng.permutation(N)[:K]
    book[::2] = x[take[::2]]                                  # every second centroid is a row of x
    if K > 1:
        book[K - 1] = book[0]                                 # duplicates, also across the chunk boundary at 64
    if K > 40:
        book[40] = book[3]
        book[7] = book[33]
    x[11] = book[K // 2]                                      # (after the duplication: an exact copy of a centroid)
    x[N - 1] = book[K - 1]                                    # the last row sits on a duplicated centroid
    x[5, D // 2] = np.nan                                     # one NaN row
    codes, d2 = R.assign(x, book)
    return x, book, codes, d2


@pytest.mark.parametrize("K", [1, 2, 63, 64, 65, 300])
@pytest.mark.parametrize("D", [1, 4, 8, 9, 16, 24, 32, 45, 48])   # (4, 8, 16, 32: the sizes at which the padded width changes)
def test_assign_is_the_restatement_bit_for_bit(D, K):
    from casualhdrsplat_amd import vq as V
    x, book, want_codes, want_d2 = assign_case(D, K)
    codes, d2 = V.kmeans_assign(gpu(x), gpu(book))
    assert codes.dtype == torch.int32 and d2.dtype == torch.float32 and codes.shape == d2.shape == (N,)
    codes, d2 = codes.cpu().numpy(), d2.cpu().numpy()
    assert want_codes[5] == 0 and np.isposinf(want_d2[5])                         # the NaN row
    assert want_d2[11] == 0.0 and want_d2[N - 1] == 0.0
    if K > 1:
        assert want_codes[N - 1] == 0                                             # not K - 1: the lower index of the duplicate
    bad = np.flatnonzero(codes != want_codes)
    assert bad.size == 0, (D, K, bad[:8], codes[bad[:8]], want_codes[bad[:8]])
    assert np.array_equal(d2.view(np.int32), want_d2.view(np.int32)), (D, K)


def test_assign_without_rows_and_without_dist2():
    import ctypes as C
    from casualhdrsplat_amd import _lib as L, vq as V
    book = torch.randn(5, 9, device=DEV)
    codes, d2 = V.kmeans_assign(torch.empty(0, 9, device=DEV), book)
    assert codes.shape == (0,) and d2.shape == (0,)
    x, bk, want, _ = assign_case(9, 65)
    xg, bg = gpu(x), gpu(bk)
    out = torch.full((N + 64,), -7, dtype=torch.int32, device=DEV)
    a = V._args(xg, bg)
    a.codes = out.data_ptr()                                                      # dist2 stays NULL
    L.check(L.load().hs_vq_assign(C.byref(a), V._stream(xg.device)), "hs_vq_assign")
    assert np.array_equal(out[:N].cpu().numpy(), want) and bool((out[N:] == -7).all())


# ---- update ----

def check_update(x, codes, book, w, out, counts):
    want, want_counts, bound, ref64 = R.update(x, codes, book, w)
    out, counts = out.cpu().numpy(), counts.cpu().numpy()
    assert np.array_equal(counts, want_counts)
    sw = np.zeros(book.shape[0])
    np.add.at(sw, codes, np.ones(len(codes)) if w is None else w.astype(np.float64))
    kept = ~(sw > 0)
    assert np.array_equal(out[kept].view(np.int32), book[kept].view(np.int32))    # the previous bits exactly
    # one fp32 rounding of the quotient + the fp64 sums: numerator and denominator each within 2^-36 relative for <= 2^17
    # members, i.e. 2^-35 (sum w |x|) / S_w with 32 x headroom -> 2^-30
    tol = 2.0 ** -23 * np.abs(ref64) + 2.0 ** -30 * bound
    err = np.abs(out.astype(np.float64) - ref64)
    assert np.all(err[~kept] <= tol[~kept]), (float((err[~kept] / np.maximum(tol[~kept], 1e-300)).max()))
    return out, counts


@functools.lru_cache(maxsize=None)
def update_inputs(n, D, K, seed):
    rng = np.random.default_rng(seed)
    x = (rng.standard_normal((n, D)) * 3.0 + 1.0).astype(np.float32)
    book = rng.standard_normal((K, D)).astype(np.float32)
    w = rng.random(n).astype(np.float32)
    return x, book, w


@pytest.mark.parametrize("D,K", [(45, 300), (24, 65), (1, 1), (48, 7), (9, 9000)])
def test_update_random_codes_against_float64(D, K):
    from casualhdrsplat_amd import vq as V
    x, book, w = update_inputs(N, D, K, 7 + D)
    codes = np.random.default_rng(D * K).integers(0, K, N).astype(np.int32)
    out, counts = V.kmeans_update(gpu(x), gpu(codes), gpu(book), gpu(w))
    check_update(x, codes, book, w, out, counts)


def test_update_one_cluster_larger_than_a_workgroup():
    """Every one of 70 000 rows in cluster 3 of 5: the cluster is cut into slices that separate workgroups sum."""
    from casualhdrsplat_amd import vq as V
    n = 70000
    x, book, w = update_inputs(n, 45, 5, 3)
    codes = np.full(n, 3, np.int32)
    out, counts = V.kmeans_update(gpu(x), gpu(codes), gpu(book), gpu(w))
    _, counts = check_update(x, codes, book, w, out, counts)
    assert counts.tolist() == [0, 0, 0, n, 0]
    out1, counts1 = V.kmeans_update(gpu(x), gpu(np.zeros(n, np.int32)), gpu(book[:1]), None)     # K = 1: 64 slices
    check_update(x, np.zeros(n, np.int32), book[:1], None, out1, counts1)


def test_update_empty_and_zero_weight_clusters_keep_the_previous_bits():
    from casualhdrsplat_amd import vq as V
    x, book, w = update_inputs(N, 45, 300, 11)
    book = book.copy()
    book[17, 3], book[18, 0] = np.float32("nan"), np.float32(-0.0)                # bits, not values
    rng = np.random.default_rng(2)
    used = np.sort(rng.permutation(300)[:10])
    codes = used[rng.integers(0, 10, N)].astype(np.int32)
    w = w.copy()
    w[codes == used[4]] = 0.0                                                      # a cluster with members and no weight
    out, counts = V.kmeans_update(gpu(x), gpu(codes), gpu(book), gpu(w))
    out, counts = check_update(x, codes, book, w, out, counts)
    empty = np.setdiff1d(np.arange(300), used)
    assert empty.size == 290 and not counts[empty].any()
    assert np.array_equal(out[empty].view(np.int32), book[empty].view(np.int32))
    assert counts[used[4]] > 0 and np.array_equal(out[used[4]].view(np.int32), book[used[4]].view(np.int32))
    # no rows at all: the codebook is copied and the counts are zero
    out0, counts0 = V.kmeans_update(torch.empty(0, 45, device=DEV), torch.empty(0, dtype=torch.int32, device=DEV), gpu(book))
    assert np.array_equal(bits(out0), book.view(np.int32)) and not counts0.any()


def test_update_without_weights_is_update_with_ones():
    from casualhdrsplat_amd import vq as V
    x, book, _ = update_inputs(N, 24, 65, 5)
    codes = np.random.default_rng(9).integers(0, 65, N).astype(np.int32)
    a, ca = V.kmeans_update(gpu(x), gpu(codes), gpu(book))
    b, cb = V.kmeans_update(gpu(x), gpu(codes), gpu(book), torch.ones(N, device=DEV))
    assert np.array_equal(bits(a), bits(b)) and torch.equal(ca, cb)
    check_update(x, codes, book, None, a, ca)


# ---- reproducibility ----

@pytest.mark.parametrize("n,D,K", [(N, 45, 300), (70000, 24, 3)])
def test_same_bits_every_run_whatever_the_workspace_held(n, D, K):
    from casualhdrsplat_amd import vq as V
    x, book, w = update_inputs(n, D, K, 21)
    xg, bg, wg = gpu(x), gpu(book), gpu(w)
    c1, d1 = V.kmeans_assign(xg, bg)
    c2, d2 = V.kmeans_assign(xg, bg)
    assert torch.equal(c1, c2) and np.array_equal(bits(d1), bits(d2))
    ws = V._workspace(n, D, K, xg.device)
    got = []
    for fill in (0x00, 0xFF, None, 0xFF):
        if fill is not None:
            ws.fill_(fill)
        out, counts = torch.empty_like(bg), torch.empty(K, dtype=torch.int32, device=DEV)
        V._update(xg, c1, bg, wg, out, counts, ws)
        got.append((bits(out), counts.cpu().numpy()))
    for o, c in got[1:]:
        assert np.array_equal(o, got[0][0]) and np.array_equal(c, got[0][1])
    check_update(x, c1.cpu().numpy(), book, w, torch.from_numpy(got[0][0].view(np.float32)), torch.from_numpy(got[0][1]))


# ---- the loop ----

def test_kmeans_recovers_planted_clusters():
    from casualhdrsplat_amd import vq as V
    x, labels, centres, first = R.planted()
    r = V.kmeans(gpu(x), 8, iters=5, init=first.tolist())
    assert isinstance(r, V.VQResult) and r.codebook.shape == (8, 45) and r.codes.shape == (3200,) and r.dist2.shape == (3200,)
    codes, book = r.codes.cpu().numpy(), r.codebook.cpu().numpy()
    assert np.array_equal(codes, labels)
    means = np.stack([x[labels == k].astype(np.float64).mean(0) for k in range(8)])
    assert np.abs(book - means).max() <= 0.1 and np.abs(book - centres).max() <= 0.1
    want_codes, want_d2 = R.assign(x, book)                   # the exact argmin against the RETURNED codebook
    assert np.array_equal(codes, want_codes) and np.array_equal(bits(r.dist2), want_d2.view(np.int32))
    # the same through an index tensor and through a codebook
    r2 = V.kmeans(gpu(x), 8, iters=5, init=torch.from_numpy(first))
    r3 = V.kmeans(gpu(x), 8, iters=5, init=gpu(x[first]))
    assert np.array_equal(bits(r2.codebook), bits(r.codebook)) and np.array_equal(bits(r3.codebook), bits(r.codebook))
    # the default initialisation is the CPU generator's permutation
    g = torch.Generator().manual_seed(4)
    rows = torch.randperm(3200, generator=torch.Generator().manual_seed(4))[:8]
    r4, r5 = V.kmeans(gpu(x), 8, iters=2, generator=g), V.kmeans(gpu(x), 8, iters=2, init=rows)
    assert np.array_equal(bits(r4.codebook), bits(r5.codebook)) and torch.equal(r4.codes, r5.codes)


def test_weighted_objective_never_rises():
    from casualhdrsplat_amd import vq as V
    rng = np.random.default_rng(5)
    x = rng.standard_normal((N, 24)).astype(np.float32)
    w = rng.random(N).astype(np.float32)
    xg, wg = gpu(x), gpu(w)
    book = gpu(x[rng.permutation(N)[:65]])
    trace = []
    for _ in range(12):
        codes, d2 = V.kmeans_assign(xg, book)
        trace.append(R.objective(d2.cpu().numpy(), w))
        book, _ = V.kmeans_update(xg, codes, book, wg)
    trace.append(R.objective(V.kmeans_assign(xg, book)[1].cpu().numpy(), w))
    print("objective", trace)
    for a, b in zip(trace, trace[1:]):
        assert b <= a * (1.0 + 1e-6), trace
    assert trace[-1] < 0.9 * trace[0]


def test_quantize_sh_end_to_end():
    from casualhdrsplat_amd import synthetic as S, vq as V
    P = 3000
    sc = S.make_scene(P, 160, 120, 2, seed=3)
    shs = sc.shs.to(device=DEV, dtype=torch.float32).contiguous()
    assert shs.shape == (P, 9, 3)
    w = torch.rand(P, generator=torch.Generator().manual_seed(1)).to(DEV)
    book, codes = V.quantize_sh(shs, 64, iters=4, weights=w, generator=torch.Generator().manual_seed(2))
    assert book.shape == (64, 8, 3) and book.dtype == torch.float32 and codes.shape == (P,) and codes.dtype == torch.int32
    assert 0 <= int(codes.min()) and int(codes.max()) < 64
    back = V.dequantize_sh(shs[:, :1], book, codes)
    assert back.shape == shs.shape and np.array_equal(bits(back[:, :1]), bits(shs[:, :1]))
    rows = shs[:, 1:].reshape(P, 24)
    want_codes, _ = R.assign(rows.cpu().numpy(), book.reshape(64, 24).cpu().numpy())
    assert np.array_equal(codes.cpu().numpy(), want_codes)
    # quantising helps: closer than the one-centroid codebook (the weighted mean)
    err = float((w * ((back - shs) ** 2).sum((1, 2))).sum())
    mean = (w[:, None] * rows).sum(0) / w.sum()
    assert err < 0.8 * float((w * ((rows - mean) ** 2).sum(1)).sum())
    # every row its own centroid: the reconstruction is the input exactly
    book, codes = V.quantize_sh(shs, P, iters=2, init=torch.arange(P))
    assert np.array_equal(bits(V.dequantize_sh(shs[:, :1], book, codes)), bits(shs))
