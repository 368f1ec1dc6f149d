#!/usr/bin/env python3
"""The fused k-means steps (casualhdrsplat_amd.vq: hs_vq_assign, hs_vq_update) against the torch formulation a trainer writes
without them,

    codes = cat([cdist(x[chunk], codebook).argmin(1) for chunk in chunks])          # the N x K matrix, a chunk at a time
    sums.index_add_(0, codes, w[:, None] * x); wsum.index_add_(0, codes, w); codebook = where(wsum > 0, sums / wsum, codebook)

alternated in one process on the same inputs.  Each size is a run of its own, under its own time limit:

    timeout -k 10 600 python scripts/time_vq.py --size 1M_45_4096 --out profiles/vq_timing.json && \\
    timeout -k 10 300 python scripts/time_vq.py --size 100k_9_256 --out profiles/vq_timing.json

(a run replaces its own size's entry of the file and keeps the others).  Sizes: N = 1 M, D = 45, K = 4096 (the `f_rest` rows
of a degree-3 cloud) and N = 100 k, D = 9, K = 256.  Device events around each call on the current stream, medians and p10 /
p90 over --iters iterations after a warm-up, the forms alternated in --rounds blocks; every buffer is allocated once.  The
assignment is also set against the floor its definition implies -- 3 N K D lane operations (subtract, multiply, add per term)
at 78.6 T lane-operations / s, half of that where two terms share a packed instruction: a derivation, not a measurement."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch

from casualhdrsplat_amd import _lib as L

SIZES = {"1M_45_4096": (1 << 20, 45, 4096), "100k_9_256": (100_000, 9, 256)}
LANE_OPS = 78.6e12
CHUNK_BYTES = 1 << 30          # the baseline's distance matrix, per chunk


def timed(fn, iters, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return ms


def stats(ms):
    q = statistics.quantiles(ms, n=10)
    return dict(median_ms=statistics.median(ms), p10_ms=q[0], p90_ms=q[-1])


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--size", choices=sorted(SIZES), required=True)
    ap.add_argument("--iters", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=4)
    ap.add_argument("--rounds", type=int, default=4, help="the forms are alternated: --rounds blocks of --iters / --rounds each")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "vq_timing.json"))
    a = ap.parse_args(argv)
    lib = L.load()
    N, D, K = SIZES[a.size]
    gen = torch.Generator().manual_seed(1)
    # rows around K / 8 blob centres, so that clusters have the uneven sizes real ones have
    centres = torch.randn(K // 8, D, generator=gen)
    x = (centres[torch.randint(0, K // 8, (N,), generator=gen)] + 0.3 * torch.randn(N, D, generator=gen)).cuda()
    w = torch.rand(N, generator=gen).cuda()
    book = x[torch.randperm(N, generator=gen)[:K].cuda()].contiguous()
    stream = torch.cuda.current_stream().cuda_stream
    nbytes = int(lib.hs_vq_workspace_bytes(N, D, K))
    codes = torch.empty(N, dtype=torch.int32, device="cuda")
    dist2 = torch.empty(N, device="cuda")
    new_book, counts = torch.empty_like(book), torch.empty(K, dtype=torch.int32, device="cuda")
    ws = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    v = L.hs_vq_args()
    v.N, v.D, v.K = N, D, K
    v.x, v.weights, v.codebook_in = x.data_ptr(), w.data_ptr(), book.data_ptr()
    v.codes, v.dist2, v.codebook_out, v.counts, v.workspace = (codes.data_ptr(), dist2.data_ptr(), new_book.data_ptr(),
                                                               counts.data_ptr(), ws.data_ptr())

    def abi_assign():
        L.check(lib.hs_vq_assign(C.byref(v), stream), "hs_vq_assign")

    def abi_update():
        L.check(lib.hs_vq_update(C.byref(v), stream), "hs_vq_update")

    def abi_iteration():
        abi_assign()
        abi_update()

    rows = max(1, min(N, CHUNK_BYTES // (4 * K)))
    t_codes = torch.empty(N, dtype=torch.int64, device="cuda")
    t_sums, t_wsum = torch.empty(K, D, device="cuda"), torch.empty(K, device="cuda")
    wx = w[:, None] * x

    def torch_assign():
        for i in range(0, N, rows):
            t_codes[i:i + rows] = torch.cdist(x[i:i + rows], book).argmin(1)

    def torch_update():
        t_sums.zero_().index_add_(0, t_codes, wx)
        t_wsum.zero_().index_add_(0, t_codes, w)
        return torch.where(t_wsum[:, None] > 0, t_sums / t_wsum[:, None], book)

    def torch_iteration():
        torch_assign()
        return torch_update()

    # the two formulations compute the same thing: cdist's matrix form rounds differently, so a few near ties may differ
    abi_iteration()
    t_book = torch_iteration()
    live = counts > 0
    agree = dict(codes_differing=int((codes.long() != t_codes).sum()),
                 codebook_max_abs=float((new_book - t_book)[live].abs().max()), clusters_live=int(live.sum()),
                 largest_cluster=int(counts.max()))
    forms = {"abi_assign": abi_assign, "torch_assign": torch_assign, "abi_update": abi_update, "torch_update": torch_update,
             "abi_iteration": abi_iteration, "torch_iteration": torch_iteration}
    ms = {k: [] for k in forms}
    per = max(a.iters // a.rounds, 1)
    for r in range(a.rounds):
        for k, fn in forms.items():
            ms[k] += timed(fn, per, a.warmup if r == 0 else 1)
    res = {k: stats(t) for k, t in ms.items()}
    floor_ms = 3.0 * N * K * D / LANE_OPS * 1e3
    res["assign_floor_ms"] = dict(three_ops_per_term=floor_ms, packed=floor_ms / 2, note="derived from the definition, not measured")
    res["abi_assign"]["over_floor"] = res["abi_assign"]["median_ms"] / floor_ms
    res["abi_assign"]["over_packed_floor"] = res["abi_assign"]["median_ms"] / (floor_ms / 2)
    for k in ("assign", "update", "iteration"):
        res[f"ratio_torch_over_abi_{k}"] = res[f"torch_{k}"]["median_ms"] / res[f"abi_{k}"]["median_ms"]
    entry = dict(N=N, D=D, K=K, iters=a.iters, device=torch.cuda.get_device_name(0), library=os.path.basename(L.LIB_PATH),
                 workspace_bytes=nbytes, baseline_chunk_rows=rows, agreement_with_torch=agree, **res)
    print(a.size, json.dumps(entry), flush=True)
    out = {}
    if os.path.exists(a.out):
        with open(a.out) as f:
            out = json.load(f)
    out["lane_ops_per_s"] = LANE_OPS
    out.setdefault("sizes", {})[a.size] = entry
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
