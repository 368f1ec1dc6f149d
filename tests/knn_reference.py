"""numpy restatement of hs_knn_mean_dist_sq (include/hdrsplat.h, knn.hip), in float32 with one ufunc per operation (numpy
contracts nothing and keeps denormals):

    brute(x, queries)   the CONTRACT: every d2(i, j), j != i by index, np.partition for the k = min(3, P - 1) smallest
    pruned(x, B, S)     the ALGORITHM of the kernels: Morton order, boxes of B consecutive points (super-boxes of S boxes),
                        seeds with the cleared list, own box first, both skip rules -- each point deciding for itself, which
                        is the most the ballot of a wave can prune

and the point clouds the CPU and GPU tests share."""
import numpy as np

F = np.float32


def _d2(p, q):
    """((dx dx) + (dy dy)) + (dz dz) of p [..., 3] against q [..., 3] (broadcast), fp32."""
    d = np.subtract(p, q, dtype=F)
    d = np.multiply(d, d, dtype=F)
    return np.add(np.add(d[..., 0], d[..., 1], dtype=F), d[..., 2], dtype=F)


def _mean_of_sorted(b, k):
    """((b0 + b1) + b2) / k of the rows of b [n, k] (ascending), fp32."""
    s = b[:, 0]
    for c in range(1, k):
        s = np.add(s, b[:, c], dtype=F)
    return np.divide(s, F(k), dtype=F)


def brute(x, queries=None):
    x = np.ascontiguousarray(x, F)
    P = x.shape[0]
    q = np.arange(P) if queries is None else np.asarray(queries, np.int64)
    k = min(3, P - 1)
    out = np.zeros(len(q), F)
    if k <= 0:
        return out
    chunk = max(1, (1 << 22) // P)
    with np.errstate(over="ignore"):
        for c0 in range(0, len(q), chunk):
            qi = q[c0:c0 + chunk]
            d2 = _d2(x[qi, None, :], x[None, :, :])
            # (excluded BY INDEX.  +inf in the excluded slot: P - 1 >= k real values remain, so the k smallest of the row are
            # the k smallest of the real values even where those overflowed to +inf themselves)
            d2[np.arange(len(qi)), qi] = np.inf
            part = np.partition(d2, k - 1, axis=1)[:, :k]
            part.sort(axis=1)
            out[c0:c0 + len(qi)] = _mean_of_sorted(part, k)
    return out


def morton_codes(x):
    """30-bit codes, 10 bits per axis; an axis of zero extent gets 0, nothing is divided by zero; a quotient that is not a
    number (an extent that overflowed) gives 0."""
    x = np.ascontiguousarray(x, F)
    mn, mx = x.min(axis=0), x.max(axis=0)
    code = np.zeros(x.shape[0], np.uint32)
    with np.errstate(all="ignore"):
        for c in range(3):
            ext = np.subtract(mx[c], mn[c], dtype=F)
            if not ext > 0:
                continue
            u = np.multiply(np.divide(np.subtract(x[:, c], mn[c], dtype=F), ext, dtype=F), F(1024), dtype=F)
            cell = np.where(u >= 0, np.where(u < 1023, u, 1023), 0)
            cell = np.nan_to_num(cell, nan=0.0).astype(np.uint32)
            v = cell
            v = (v | (v << 16)) & 0x030000FF
            v = (v | (v << 8)) & 0x0300F00F
            v = (v | (v << 4)) & 0x030C30C3
            v = (v | (v << 2)) & 0x09249249
            code |= v << c
    return code


def _lb(p, lo, hi):
    """((ex ex) + (ey ey)) + (ez ez), e = max(0, lo - p, p - hi) per axis: p [n, 1, 3] against boxes [1, m, 3] -> [n, m]."""
    e = np.maximum(F(0), np.maximum(np.subtract(lo, p, dtype=F), np.subtract(p, hi, dtype=F)))
    e = np.multiply(e, e, dtype=F)
    return np.add(np.add(e[..., 0], e[..., 1], dtype=F), e[..., 2], dtype=F)


def _aabb(pts, B):
    n = (pts.shape[0] + B - 1) // B
    lo = np.stack([pts[b * B:(b + 1) * B].min(axis=0) for b in range(n)])
    hi = np.stack([pts[b * B:(b + 1) * B].max(axis=0) for b in range(n)])
    return lo, hi


def pruned(x, B, S=None, stats=None):
    """The search of knn.hip, point by point.  `S`: boxes per super-box (None: one level).  `stats` (a dict) receives the
    number of boxes scanned, for tests that want to see pruning happen."""
    x = np.ascontiguousarray(x, F)
    P = x.shape[0]
    k = min(3, P - 1)
    out = np.zeros(P, F)
    if k <= 0:
        return out
    order = np.argsort(morton_codes(x), kind="stable")
    pts = x[order]
    lo, hi = _aabb(pts, B)
    nbox = lo.shape[0]
    scanned = 0
    with np.errstate(over="ignore"):
        d2 = _d2(pts[:, None, :], pts[None, :, :])                 # [P, P]: what a lane computes when it meets a point
        lb = _lb(pts[:, None, :], lo[None], hi[None])              # [P, nbox]
        if S:
            slo, shi = _aabb(lo, S)[0], _aabb(hi, S)[1]
            lbs = _lb(pts[:, None, :], slo[None], shi[None])
        for s in range(P):
            row = d2[s]
            seeds = sorted(float(row[j]) for j in range(max(0, s - 3), min(P, s + 4)) if j != s)
            reject = seeds[k - 1]
            best = []                                              # CLEARED: the seeds are met again in their boxes
            own = s // B
            best = sorted(float(row[j]) for j in range(own * B, min(P, own * B + B)) if j != s)[:k]
            scanned += 1

            def skip(bound):
                return bound > reject or (len(best) >= k and bound >= best[k - 1])

            for g in range((nbox + S - 1) // S if S else 1):
                if S and skip(float(lbs[s, g])):
                    continue
                for b in range(g * S, min(nbox, g * S + S)) if S else range(nbox):
                    if b == own or skip(float(lb[s, b])):
                        continue
                    scanned += 1
                    best = sorted(best + [float(v) for v in row[b * B:min(P, b * B + B)]])[:k]
            out[order[s]] = _mean_of_sorted(np.asarray([best], F), k)[0]
    if stats is not None:
        stats["scanned"] = scanned
        stats["boxes"] = nbox * P
    return out


def bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


# ---- the clouds ----

def uniform(P, seed=0):
    return np.random.default_rng(1000 + 7 * P + seed).random((P, 3), dtype=F)


def identical(P):
    return np.tile(np.asarray([[0.25, -1.5, 3.0]], F), (P, 1))


def line(P=500, seed=1):
    x = np.zeros((P, 3), F)
    x[:, 0] = 0.5
    x[:, 1] = np.random.default_rng(seed).random(P, dtype=F) * F(10)
    x[:, 2] = -2.0
    return x


def plane(P=600, seed=2):
    x = np.random.default_rng(seed).random((P, 3), dtype=F)
    x[:, 2] = 1.25
    return x


def clusters(n=300, seed=3):
    """Two clusters of sigma 1e-3, 1e3 apart, plus one point at 1e6: all Morton cells of the clusters collapse."""
    g = np.random.default_rng(seed)
    a = g.normal(0.0, 1e-3, (n, 3))
    b = g.normal(0.0, 1e-3, (n, 3)) + np.asarray([1e3, 0.0, 0.0])
    return np.concatenate([a, b, np.asarray([[1e6, 1e6, 1e6]])]).astype(F)


def repeated(n=200, times=4, seed=4):
    """n points, each `times` times, shuffled: every output is exactly 0."""
    x = np.repeat(np.random.default_rng(seed).random((n, 3), dtype=F), times, axis=0)
    return x[np.random.default_rng(seed + 1).permutation(len(x))]


def lattice(n=8, spacing=0.5):
    g = np.stack(np.meshgrid(*[np.arange(n, dtype=F)] * 3, indexing="ij"), -1).reshape(-1, 3)
    return np.multiply(g, F(spacing), dtype=F)


def lattice_interior(n=8):
    i = np.arange(n ** 3)
    c = np.stack([i // (n * n), (i // n) % n, i % n], -1)
    return np.all((c > 0) & (c < n - 1), axis=1)


def denormal(P=400, seed=5):
    """Coordinates of the order of 1e-20: every square is denormal (or zero)."""
    return np.multiply(np.random.default_rng(seed).random((P, 3), dtype=F), F(1e-20), dtype=F)


def degenerate_families(n_identical=300):
    return {"identical": identical(n_identical), "line": line(), "plane": plane(), "clusters": clusters(),
            "repeated": repeated(), "lattice": lattice(), "denormal": denormal()}


def sfm_like(P, seed=0):
    """A reconstruction-like cloud: thin noisy surfaces (planes, a sphere, a cylinder) of uneven density and 2 % sparse
    outliers in a volume ten times as wide."""
    g = np.random.default_rng(seed)
    n_out = P // 50
    n = P - n_out
    parts = np.array_split(np.arange(n), 5)
    out = []
    u, v = g.random(len(parts[0])), g.random(len(parts[0]))
    out.append(np.stack([4 * u - 2, 4 * v - 2, g.normal(0, 2e-3, len(u))], -1))                     # floor
    u, v = g.random(len(parts[1])) ** 2, g.random(len(parts[1]))
    out.append(np.stack([4 * u - 2, g.normal(2.0, 3e-3, len(u)), 3 * v], -1))                       # wall, denser at one end
    d = g.normal(size=(len(parts[2]), 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    out.append(d * (0.5 + g.normal(0, 1e-3, (len(d), 1))) + np.asarray([0.5, -0.5, 0.5]))           # sphere
    t, h = g.random(len(parts[3])) * 2 * np.pi, g.random(len(parts[3]))
    out.append(np.stack([0.2 * np.cos(t) - 1, 0.2 * np.sin(t) + 1, 2 * h], -1) + g.normal(0, 1e-3, (len(t), 3)))   # column
    out.append(g.normal(0, 0.05, (len(parts[4]), 3)) + np.asarray([1.0, 1.0, 0.3]))                 # a dense blob
    out.append((g.random((n_out, 3)) - 0.5) * 40)
    x = np.concatenate(out).astype(F)
    return x[g.permutation(P)]
