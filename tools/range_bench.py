#!/usr/bin/env python3
"""Exact range search (HipFlatIndex.range_search) over the flagship corpus shape: 21 M x 768 fp16 rows (squared L2,
synthetic rows of the shared counter-based generator), B in {1, 16, 64} device queries, radii chosen for about 10,
1 000 and 100 000 results per query.  Prints ms per call, the fraction of 8 TB/s on the stored-row bytes, the
candidate and result counts, and next to it `search(q, k=10)` on the direct scan of the same rows (no 8-bit shadow).

  python tools/range_bench.py [--docs 21000000] [--reps 5] [--batches 1,16,64] [--targets 10,1000,100000]

Radii: the median over the queries of the target-th distance (from search for small targets, else from the
per-query quantile over a sample of the rows - the first 2^18, iid like the rest).  Not part of bench.py."""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import probing_rag_amd as pra  # noqa: E402
from oracle import oracle_np as onp  # noqa: E402

HBM = 8e12


def timed(fn, reps):
    fn()
    torch.cuda.synchronize()
    t = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        t.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(t)), float(min(t))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--docs", type=int, default=21_000_000)
    ap.add_argument("--d", type=int, default=768)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--batches", default="1,16,64")
    ap.add_argument("--targets", default="10,1000,100000", help="results per query the radii aim at")
    args = ap.parse_args()
    N, d = args.docs, args.d
    torch.cuda.set_device(0)
    ix = pra.HipFlatIndex(d, "l2", "f16")
    ix.set_shadow(0)                       # search on the direct scan: the same rows, the same bytes
    ix.add_synthetic(42, 0, N)
    row_bytes = N * d * 2
    sample = torch.from_numpy(onp.store_round(onp.synth_rows(42, 0, 1 << 18, d), "f16")).cuda().double()
    out = {"docs": N, "d": d, "store": "f16", "metric": "l2", "rows_bytes": row_bytes, "cases": []}
    for B in (int(v) for v in args.batches.split(",")):
        q = torch.from_numpy(onp.synth_rows(7, 0, B, d)).cuda()
        S = torch.cdist(q.double(), sample) ** 2          # calibration only
        ms_s, _ = timed(lambda: ix.search(q, 10), args.reps)
        out["cases"].append({"B": B, "call": "search k=10", "ms": round(ms_s, 4),
                             "frac_8TBs": round(row_bytes / (ms_s * 1e-3) / HBM, 4), "plan": ix.last_plan().get("family")})
        print(json.dumps(out["cases"][-1]), flush=True)
        for target in (int(v) for v in args.targets.split(",")):
            frac = target / N
            kq = max(1, int(round(frac * S.shape[1])))
            if kq >= 8:     # enough sample rows below the target quantile
                r = float(torch.kthvalue(S, kq, dim=1).values.median())
            else:           # the target-th distance itself, from search
                r = float(ix.search(q, target)[0][:, target - 1].median())
            res = {}

            def call():
                res["out"] = ix.range_search(q, r)
            ms, ms_min = timed(call, args.reps)
            lims = res["out"][0]
            case = {"B": B, "call": "range_search", "target_per_query": target, "radius": r, "ms": round(ms, 4),
                    "ms_min": round(ms_min, 4), "frac_8TBs": round(row_bytes / (ms * 1e-3) / HBM, 4),
                    "results": int(lims[-1]), "results_per_query_median": float(np.median(np.diff(lims))),
                    "candidates": ix.range_candidates(), "vs_search": round(ms / ms_s, 3)}
            out["cases"].append(case)
            print(json.dumps(case), flush=True)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
