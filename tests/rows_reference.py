"""numpy restatement of the score-driven row plans (include/hdrsplat.h, hs_rows_plan): the reference the GPU tests hold
rows.hip to, bit for bit.

The order on scores: NaN ranks below every number and all NaNs are equal; -0 equals +0; everything else is numeric.  `key`
maps a float32 to a uint32 that has exactly this order (NaN -> 0, -0 -> the key of +0, sign flip otherwise), `order` lists the
rows by (score descending, row ascending) -- a STABLE argsort of the descending key -- and "the k best rows" are its first k.
T = the number of rows whose key equals the k-th best one (0 when k == 0).

The three plans give (row_map uint32 [P_out], counts list of 8) in hs_densify_plan's format: survivors | clones | children
k = 0 | children k = 1, each in source order, row_map = kind << 30 | source, counts = {P_out, survivors, clones, children,
sources that left no row, split sources, P, T}.  The gather, the child scales and the child means are densify_reference's.
"""
import numpy as np

import densify_reference as DR

F = np.float32
MASK, KEEP, DENSIFY = 0, 1, 2


def key(score):
    score = np.ascontiguousarray(score, dtype=F)
    b = score.view(np.uint32).copy()
    nan = (b & np.uint32(0x7FFFFFFF)) > np.uint32(0x7F800000)
    b[b == np.uint32(0x80000000)] = 0
    k = np.where(b & np.uint32(0x80000000), ~b, b | np.uint32(0x80000000)).astype(np.uint32)
    k[nan] = 0
    return k


def order(score):
    """Row indices by (score descending, row ascending)."""
    return np.argsort(~key(score), kind="stable")


def select(score, k):
    """(selected bool [P], T)."""
    P = score.shape[0]
    sel = np.zeros(P, dtype=bool)
    if k == 0:
        return sel, 0
    o = order(score)
    sel[o[:k]] = True
    ky = key(score)
    return sel, int((ky == ky[o[k - 1]]).sum())


def _row_map(codes):
    P = codes.shape[0]
    idx = np.arange(P, dtype=np.uint32)
    surv, clone, kept = idx[(codes == 1) | (codes == 2)], idx[codes == 2], idx[codes == 3]
    row_map = np.concatenate([surv, clone | np.uint32(1 << 30), kept | np.uint32(2 << 30), kept | np.uint32(3 << 30)]).astype(np.uint32)
    counts = [int(row_map.size), int(surv.size), int(clone.size), 2 * int(kept.size), P - int(surv.size) - int(kept.size),
              int(kept.size), P, 0]
    return row_map, counts


def plan_mask(mask):
    return _row_map(np.where(np.asarray(mask) != 0, 0, 1).astype(np.uint8))


def plan_keep(score, k):
    sel, T = select(score, k)
    row_map, counts = _row_map(sel.astype(np.uint8))
    counts[7] = T
    return row_map, counts


def plan_densify(score, k, scales, tau_split):
    sel, T = select(score, k)
    scales = np.asarray(scales, dtype=F).reshape(-1, 3)
    with np.errstate(all="ignore"):
        s = scales[:, 0].copy()
        s = np.where(scales[:, 1] > s, scales[:, 1], s)
        s = np.where(scales[:, 2] > s, scales[:, 2], s)
        big = s > F(tau_split)
    row_map, counts = _row_map(np.where(sel, np.where(big, 3, 2), 1).astype(np.uint8))
    counts[7] = T
    return row_map, counts


def gather_bits(src_array, row_map):
    """COPY of a 4-byte element array, bit-preserving whatever the dtype."""
    src = (row_map & np.uint32(DR.SRC_MASK)).astype(np.int64)
    return src_array[src].copy()


def apply(case, row_map, raw_scales, children):
    """The cloud and moments of a densify_reference.make_case after the gather over row_map: (new cloud, new moments)."""
    c = case["cloud"]
    roles = DR.ROLES if children else {k: DR.COPY for k in DR.NAMES}
    new = {k: DR.gather(c[k], row_map, roles[k], raw_scales, c, case["noise"]) for k in DR.NAMES}
    mom = {k: tuple(DR.gather(x, row_map, DR.ZERO_NEW) for x in case["moments"][k]) for k in DR.NAMES}
    return new, mom


# ---- score families of the tests ----

SPECIALS = np.array([np.nan, np.inf, -np.inf, 0.0, -0.0, 1e-45, -1e-45, 1e-39, -1e-39, 1.0, -1.0, -3.5, 2.5,
                     3.4028235e38, -3.4028235e38], dtype=F)


def family(name, P, seed=0):
    """A float32 score array [P] of one family: normal, seven, equal, specials, byte0 .. byte3 (byte b: bit patterns that
    differ only in byte b of the key, b = 0 the most significant)."""
    rng = np.random.default_rng(seed)
    if name == "normal":
        return rng.standard_normal(P).astype(F)
    if name == "seven":
        return rng.integers(0, 7, P).astype(F) - F(3)
    if name == "equal":
        return np.full(P, 0.25, dtype=F)
    if name == "specials":
        s = SPECIALS[rng.integers(0, SPECIALS.size, P)].copy()
        qnan = np.array([0xFFC00001], dtype=np.uint32).view(F)[0]      # a negative NaN with a payload: equal to every NaN
        s[(rng.random(P) < 0.05)] = qnan
        return s
    if name.startswith("byte"):
        b = int(name[4:])
        # keys 0x?0?0?0?0 with only byte b free; every such KEY is turned back into the float whose key it is (key < 2^31:
        # a negative number, bits = ~key; otherwise bits = key & 0x7fffffff); NaN patterns are avoided by the fixed bytes
        fixed = np.uint32(0xC0404040) & ~np.uint32(0xFF << (24 - 8 * b))
        lo = 0x80 if b == 0 else 0                                     # byte 0: positive numbers only (0x80 .. 0xff minus NaN)
        digit = rng.integers(lo, 0xFF if b == 0 else 0x100, P).astype(np.uint32)
        k = fixed | (digit << np.uint32(24 - 8 * b))
        bits = np.where(k & np.uint32(0x80000000), k & np.uint32(0x7FFFFFFF), ~k).astype(np.uint32)
        out = bits.view(F).copy()
        assert not np.isnan(out).any() and np.array_equal(key(out), k)
        return out
    raise KeyError(name)


FAMILIES = ("normal", "seven", "equal", "specials", "byte0", "byte1", "byte2", "byte3")


def ks_of(score):
    """The values of k of the grid: 0, 1, P/2, P-1, P, the number of rows above the threshold class of P/2, that plus one."""
    P = score.shape[0]
    ks = {0, 1, P // 2, P - 1, P}
    if P >= 2:
        ky = key(score)
        thr = np.sort(ky)[::-1][P // 2]
        above = int((ky > thr).sum())
        ks |= {above, above + 1}
    return sorted(k for k in ks if 0 <= k <= P)
