"""Time of an occurrence search over a resident q8 bank of timestamp embeddings, next to the fp32 one (GPU diagnostic):

    python tools/prof_match_q8.py [--rows 100000 1000000] [--D 2184] [--lengths 16 32 64 200] [--k 10] [--file_rows 1200]
                                  [--repeats 5] [--inner 10] [--out prof_match_q8.json]

Workload: that of tools/prof_match.py - a bank of `rows` x D rows in files of `file_rows` rows, clip(0.75 + N(0, 1), 0)
normalised by ops.rows_normalize, and a query clip of L rows cut from the bank; sep = L - and the q8 codes of the same rows
(ops.rows_quantize_q8 of the normalised rows, as EmbeddingIndex.quantized does).  Four legs:
  (a) torch      the torch formulation of tools/prof_match.py on the fp32 bank
  (b) search_q8  ops.embed_search_q8 with Q = L on the codes: what scanning the codes that many times costs, with the
                 selection rounds of the search and without the match
  (c) match      ops.embed_match on the fp32 bank
  (d) match_q8   ops.embed_match_q8 on the codes
All are warmed up, then run alternately `repeats` times; each time is a host clock around `inner` back-to-back calls that
end in a device synchronise, divided by `inner`.  Fidelity of (d) against (c) is reported per shape: the share of the k
places that are the same, and the largest score difference at the places both return.  A bank that does not fit the free
memory is skipped and listed under "skipped"; so is leg (a) where its score matrix does not fit.
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
from tools.prof_match import torch_match  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, nargs="+", default=[100000, 1000000])
    ap.add_argument("--D", type=int, default=2184)
    ap.add_argument("--lengths", type=int, nargs="+", default=[16, 32, 64, 200])
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--file_rows", type=int, default=1200)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--inner", type=int, default=10)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "prof_match_q8 needs a GPU"
    dev = torch.device("cuda:0")
    D = args.D
    result = {"workload": {"D": D, "k": args.k, "file_rows": args.file_rows, "repeats": args.repeats, "inner": args.inner},
              "shapes": [], "skipped": []}
    for N in args.rows:
        free = torch.cuda.mem_get_info(dev)[0]
        if 5 * N * D * 1.25 > free:
            result["skipped"].append({"rows": N, "reason": f"banks of {5 * N * D} bytes, {free} bytes free"})
            continue
        g = torch.Generator(device=dev).manual_seed(N)
        bank = torch.empty((N, D), device=dev)
        step = 65536
        for n0 in range(0, N, step):                       # filled in pieces: no second bank-sized temporary
            piece = bank[n0:n0 + step]
            piece.copy_((0.75 + torch.randn(piece.shape, device=dev, generator=g)).clamp_(min=0))
        ops.rows_normalize(bank, out=bank)
        codes, scale = ops.rows_quantize_q8(bank, normalize=False)
        seg = torch.tensor(list(range(0, N, args.file_rows)) + [N], dtype=torch.int32, device=dev)
        for L in args.lengths:
            at = (N // 2) // args.file_rows * args.file_rows + 7
            qn = bank[at:at + L].clone()
            qcodes, qscale = ops.rows_quantize_q8(qn, normalize=True)
            legs = {"search_q8": lambda: ops.embed_search_q8(codes, scale, D, qcodes, qscale, args.k),
                    "match": lambda: ops.embed_match(bank, seg, qn, args.k, L),
                    "match_q8": lambda: ops.embed_match_q8(codes, scale, D, seg, qcodes, qscale, args.k, L)}
            if 4 * N * L * 3 < torch.cuda.mem_get_info(dev)[0]:
                legs["torch"] = lambda: torch_match(bank, args.file_rows, qn, args.k, L)
            else:
                result["skipped"].append({"rows": N, "L": L, "leg": "torch", "reason": f"score matrix of {4 * N * L} bytes"})
            first = {name: fn() for name, fn in legs.items()}          # warm-up of every leg
            torch.cuda.synchronize()
            s32, i32 = (t.cpu() for t in first["match"])
            s8, i8 = (t.cpu() for t in first["match_q8"])
            both = [(float(s8[a]), float(s32[(i32 == i8[a]).nonzero()[0, 0]])) for a in range(args.k)
                    if int(i8[a]) >= 0 and bool((i32 == i8[a]).any())]
            r = {"rows": N, "L": L, "sep": L, "planted_at": at, "first_place": int(i8[0]), "first_score": float(s8[0]),
                 "first_place_fp32": int(i32[0]), "first_score_fp32": float(s32[0]),
                 "same_places_of_k": len(both), "same_order": bool(torch.equal(i8, i32)),
                 "max_abs_score_diff_fp32": max((abs(a - b) for a, b in both), default=None)}
            del first
            times = {name: [] for name in legs}
            for _ in range(args.repeats):
                for name, fn in legs.items():
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    for _ in range(args.inner):
                        fn()
                    torch.cuda.synchronize()
                    times[name].append((time.perf_counter() - t0) / args.inner)
            for name, ts in times.items():
                r[name] = {"median_us": 1e6 * statistics.median(ts), "min_us": 1e6 * min(ts), "max_us": 1e6 * max(ts),
                           "all_us": [round(1e6 * x, 1) for x in ts]}
            r["match_q8_over_search_q8"] = r["match_q8"]["median_us"] / r["search_q8"]["median_us"]
            r["match_over_match_q8"] = r["match"]["median_us"] / r["match_q8"]["median_us"]
            if "torch" in r:
                r["torch_over_match_q8"] = r["torch"]["median_us"] / r["match_q8"]["median_us"]
            passes = -(-L // ops.MATCH_Q8_GROUP)
            bank_bytes = N * (codes.shape[1] + 4)                        # codes and the scale of every row
            r["match_q8_bytes"] = {"bank": bank_bytes, "passes": passes, "scores": 8 * N * L,
                                   "bank_TBs": bank_bytes * passes / (1e-6 * r["match_q8"]["median_us"]) / 1e12,
                                   "TBs": (bank_bytes * passes + 8 * N * L) / (1e-6 * r["match_q8"]["median_us"]) / 1e12}
            result["shapes"].append(r)
            print(json.dumps(r), flush=True)
        del bank, codes, scale
        torch.cuda.empty_cache()
    line = json.dumps(result)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
