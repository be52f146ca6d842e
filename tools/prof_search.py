"""Time of a cosine top-k over a resident bank of embeddings, the torch formulation against eat_embed_search (GPU diagnostic):

    python tools/prof_search.py [--rows 100000 1000000] [--D 2184] [--queries 1 16 64] [--k 10] [--repeats 5] [--inner 10]
                                [--out prof_search.json]

Workload: a bank of `rows` x D rows and Q queries, clip(0.75 + N(0, 1), 0) normalised by ops.rows_normalize.  Two legs:
  (a) torch  torch.topk(qn @ bank.T, k): a (Q, N) score matrix, then a top-k over it
  (b) hip    ops.embed_search: no score matrix, the bank read once per group of up to 16 queries
Both are warmed up, then run alternately `repeats` times; each time is a host clock around `inner` back-to-back calls that
end in a device synchronise, divided by `inner`.  For (b) the bank bytes that the call streams (the bank once per group of
16 queries) are set against its median time and against the device-to-device copy rate.  A bank that does not fit the free
memory is skipped and listed under "skipped".
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from efficientat_amd import ops  # noqa: E402

COPY_TBS = 6.29          # what a device-to-device copy reaches on this part (VERDICT, "What's weak" #6)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, nargs="+", default=[100000, 1000000])
    ap.add_argument("--D", type=int, default=2184)
    ap.add_argument("--queries", type=int, nargs="+", default=[1, 16, 64])
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--inner", type=int, default=10)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "prof_search needs a GPU"
    dev = torch.device("cuda:0")
    result = {"workload": {"D": args.D, "k": args.k, "repeats": args.repeats, "inner": args.inner}, "copy_TBs": COPY_TBS,
              "shapes": [], "skipped": []}
    for N in args.rows:
        free = torch.cuda.mem_get_info(dev)[0]
        if 4 * N * args.D * 1.25 > free:
            result["skipped"].append({"rows": N, "reason": f"bank of {4 * N * args.D} bytes, {free} bytes free"})
            continue
        g = torch.Generator(device=dev).manual_seed(N)
        bank = torch.empty((N, args.D), device=dev)
        step = 65536
        for n0 in range(0, N, step):                       # filled in pieces: no second bank-sized temporary
            piece = bank[n0:n0 + step]
            piece.copy_((0.75 + torch.randn(piece.shape, device=dev, generator=g)).clamp_(min=0))
        ops.rows_normalize(bank, out=bank)
        for Q in args.queries:
            qn = ops.rows_normalize((0.75 + torch.randn((Q, args.D), device=dev, generator=g)).clamp_(min=0))
            a = lambda: torch.topk(qn @ bank.T, args.k)
            b = lambda: ops.embed_search(bank, qn, args.k)
            (sa, ia), (sb, ib) = a(), b()                  # warm-up of both, and how far apart they are
            diff = float((sa - sb).abs().max())
            same = float((ia == ib).float().mean())
            del sa, ia, sb, ib
            times = {"torch": [], "hip": []}
            for _ in range(args.repeats):
                for name, fn in (("torch", a), ("hip", b)):
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    for _ in range(args.inner):
                        fn()
                    torch.cuda.synchronize()
                    times[name].append((time.perf_counter() - t0) / args.inner)
            r = {"rows": N, "Q": Q, "max_abs_score_diff": diff, "same_index_share": same}
            for name, ts in times.items():
                r[name] = {"median_us": 1e6 * statistics.median(ts), "min_us": 1e6 * min(ts), "max_us": 1e6 * max(ts),
                           "all_us": [round(1e6 * x, 1) for x in ts]}
            r["speedup_median"] = r["torch"]["median_us"] / r["hip"]["median_us"]
            passes = -(-Q // ops.SEARCH_GROUP)
            streamed = 4 * N * args.D * passes
            r["hip_bytes"] = {"bank": 4 * N * args.D, "passes": passes, "TBs": streamed / (1e-6 * r["hip"]["median_us"]) / 1e12}
            r["hip_bytes"]["of_copy"] = r["hip_bytes"]["TBs"] / COPY_TBS
            result["shapes"].append(r)
            print(json.dumps(r), flush=True)
        del bank
        torch.cuda.empty_cache()
    line = json.dumps(result)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
