"""Time of an occurrence search over a resident bank of timestamp embeddings (GPU diagnostic):

    python tools/prof_match.py [--rows 100000 1000000] [--D 2184] [--lengths 16 32 200] [--k 10] [--file_rows 1200]
                               [--repeats 5] [--inner 10] [--out prof_match.json]

Workload: a bank of `rows` x D rows in files of `file_rows` rows, clip(0.75 + N(0, 1), 0) normalised by ops.rows_normalize,
and a query clip of L rows cut from the bank; sep = L.  Three legs:
  (a) torch   qn @ bank.T, the L diagonal slices summed in ascending j, / L, windows that leave their file masked,
              max_pool1d over 2 sep + 1 starts as the peak rule, topk - a (L, N) score matrix and several (N,) passes
  (b) search  ops.embed_search with Q = L on the same bank: what scanning the bank that many times costs, without the match
  (c) match   ops.embed_match
All are warmed up, then run alternately `repeats` times; each time is a host clock around `inner` back-to-back calls that
end in a device synchronise, divided by `inner`.  (a) differs from (c) where a file boundary lies within sep of a peak
(max_pool1d looks across it) and in ties; the share of equal places is reported, not asserted.  A bank that does not fit the
free memory is skipped and listed under "skipped"; so is leg (a) where its score matrix does not fit.
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


def torch_match(bank, seg_len, qn, k, sep):
    """Leg (a): files of seg_len rows (the last one shorter)."""
    L, N = qn.shape[0], bank.shape[0]
    S = qn @ bank.T
    n = N - L + 1
    acc = S[0, :n].clone()
    for j in range(1, L):
        acc += S[j, j:j + n]
    m = acc / L
    start = torch.arange(n, device=bank.device)
    file_end = torch.clamp((start // seg_len + 1) * seg_len, max=N)
    m = torch.where(start + L <= file_end, m, torch.full_like(m, float("-inf")))
    top = torch.nn.functional.max_pool1d(m[None, None], 2 * sep + 1, stride=1, padding=sep)[0, 0]
    m = torch.where(m == top, m, torch.full_like(m, float("-inf")))
    return torch.topk(m, k)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, nargs="+", default=[100000, 1000000])
    ap.add_argument("--D", type=int, default=2184)
    ap.add_argument("--lengths", type=int, nargs="+", default=[16, 32, 200])
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--file_rows", type=int, default=1200)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--inner", type=int, default=10)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "prof_match needs a GPU"
    dev = torch.device("cuda:0")
    result = {"workload": {"D": args.D, "k": args.k, "file_rows": args.file_rows, "repeats": args.repeats, "inner": args.inner},
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
        seg = torch.tensor(list(range(0, N, args.file_rows)) + [N], dtype=torch.int32, device=dev)
        for L in args.lengths:
            at = (N // 2) // args.file_rows * args.file_rows + 7
            qn = bank[at:at + L].clone()
            legs = {"search": lambda: ops.embed_search(bank, qn, args.k),
                    "match": lambda: ops.embed_match(bank, seg, qn, args.k, L)}
            if 4 * N * L * 3 < torch.cuda.mem_get_info(dev)[0]:
                legs["torch"] = lambda: torch_match(bank, args.file_rows, qn, args.k, L)
            else:
                result["skipped"].append({"rows": N, "L": L, "leg": "torch", "reason": f"score matrix of {4 * N * L} bytes"})
            first = {name: fn() for name, fn in legs.items()}          # warm-up of every leg
            torch.cuda.synchronize()
            r = {"rows": N, "L": L, "sep": L, "first_place": int(first["match"][1][0]), "planted_at": at,
                 "first_score": float(first["match"][0][0])}
            if "torch" in first:
                r["same_place_share_torch"] = float((first["torch"][1] == first["match"][1]).float().mean())
                r["max_abs_score_diff_torch"] = float((first["torch"][0] - first["match"][0]).abs().max())
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
            r["match_over_search"] = r["match"]["median_us"] / r["search"]["median_us"]
            if "torch" in r:
                r["torch_over_match"] = r["torch"]["median_us"] / r["match"]["median_us"]
            passes = -(-L // ops.SEARCH_GROUP)
            r["match_bytes"] = {"bank": 4 * N * args.D, "passes": passes, "scores": 8 * N * L,
                                "TBs": (4 * N * args.D * passes + 8 * N * L) / (1e-6 * r["match"]["median_us"]) / 1e12}
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
