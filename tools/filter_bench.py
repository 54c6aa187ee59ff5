#!/usr/bin/env python3
"""Exact filtered search (HipFlatIndex.search(q, k, params=SearchParameters(sel=...))) over the flagship corpus shape:
21 M x 768 fp16 rows (squared L2, synthetic rows of the shared counter-based generator), B in {1, 16, 64} device
queries, k = 10.  Prints, per selector, ms per call, the path the device chose, the rows selected, the 32-row tiles
holding one, the row bytes that path reads over 8 TB/s, and next to it `search(q, k=10)` on the direct scan of the same
rows (no 8-bit shadow).  Selectors are CUDA byte bitmaps (faiss IDSelectorBitmap layout) built before timing.

  python tools/filter_bench.py [--docs 21000000] [--reps 5] [--batches 1,16,64] [--only all,rand50,...]

Not part of bench.py."""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import probing_rag_amd as pra  # noqa: E402

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


def selectors(N, rng):
    """name -> selected rows (bool [N])"""
    out = {}
    out["all"] = np.ones(N, bool)
    out["rand50"] = rng.random(N, dtype=np.float32) < 0.5
    m = np.zeros(N, bool)
    m[N // 3:N // 3 + N // 8] = True
    out["contig1_8"] = m
    out["rand1"] = rng.random(N, dtype=np.float32) < 0.01
    m = np.zeros(N, bool)
    m[rng.choice(N, 10_000, replace=False)] = True
    out["ids10000"] = m
    m = np.zeros(N, bool)
    m[5_000_017:5_001_017] = True
    out["contig1000"] = m
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--docs", type=int, default=21_000_000)
    ap.add_argument("--d", type=int, default=768)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--batches", default="1,16,64")
    ap.add_argument("--only", default="", help="comma-separated selector names (default: all six)")
    ap.add_argument("--no-search", action="store_true", help="skip the unfiltered reference search")
    args = ap.parse_args()
    N, d = args.docs, args.d
    torch.cuda.set_device(0)
    ix = pra.HipFlatIndex(d, "l2", "f16")
    ix.set_shadow(0)                       # search on the direct scan: the same rows, the same bytes
    ix.add_synthetic(42, 0, N)
    sels = selectors(N, np.random.default_rng(0))
    if args.only:
        sels = {k: v for k, v in sels.items() if k in args.only.split(",")}
    bitmaps = {k: torch.from_numpy(np.packbits(v, bitorder="little")).cuda() for k, v in sels.items()}
    row_bytes = d * 2
    out = {"docs": N, "d": d, "store": "f16", "metric": "l2", "k": 10, "cases": []}
    for B in (int(v) for v in args.batches.split(",")):
        q = torch.from_numpy(np.random.default_rng(7).standard_normal((B, d)).astype(np.float32)).cuda()
        ms_s = None
        if not args.no_search:
            ms_s, _ = timed(lambda: ix.search(q, 10), args.reps)
            case = {"B": B, "call": "search k=10", "ms": round(ms_s, 4),
                    "frac_8TBs": round(N * row_bytes / (ms_s * 1e-3) / HBM, 4), "plan": ix.last_plan().get("family")}
            out["cases"].append(case)
            print(json.dumps(case), flush=True)
        for name, bm in bitmaps.items():
            p = pra.SearchParameters(sel=pra.IDSelectorBitmap(bm))
            ms, ms_min = timed(lambda: ix.search(q, 10, params=p), args.reps)
            info = ix.last_filter()
            read = info["n_tiles"] * 32 * row_bytes if info["path"] == 1 else info["n_selected"] * row_bytes
            case = {"B": B, "call": "filtered k=10", "selector": name, "ms": round(ms, 4), "ms_min": round(ms_min, 4),
                    "path": info["path"], "n_selected": info["n_selected"], "n_tiles": info["n_tiles"],
                    "n_flagged": info["n_flagged"], "row_bytes_read": read,
                    "frac_8TBs": round(read / (ms * 1e-3) / HBM, 4)}
            if ms_s:
                case["vs_search"] = round(ms / ms_s, 3)
            out["cases"].append(case)
            print(json.dumps(case), flush=True)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
