"""Time and fidelity of the 8-bit search index against the fp32 index and the torch formulation (GPU diagnostic):

    python tools/prof_search_q8.py [--rows 100000 1000000] [--D 2184] [--queries 1 16 64] [--k 10] [--repeats 5] [--inner 10]
                                   [--out profiles/embed_search_q8.json]

Workload, as tools/prof_search.py: a bank of `rows` x D rows and Q queries, clip(0.75 + N(0, 1), 0), normalised by
ops.rows_normalize; the q8 bank is ops.rows_quantize_q8 of the normalised rows.  Three legs:
  (a) torch  torch.topk(qn @ bank.T, k)
  (b) fp32   ops.embed_search: the bank read once per group of up to 16 queries
  (c) q8     ops.embed_search_q8: a quarter of the bytes, read once per group of up to 64 queries
All are warmed up, then run alternately `repeats` times; each time is a host clock around `inner` back-to-back calls that
end in a device synchronise, divided by `inner`.  For (b) and (c) the bank bytes that the call streams are set against the
median time and against the device-to-device copy rate.

Fidelity, per shape: recall@k of the q8 result against the fp32 result (the share of the fp32 index's k rows that the q8
index returns too) and the largest |s_q8 - s_fp32| over the rows that both return.  On this distribution random rows'
cosines crowd together (they differ in the fourth decimal at D = 2184), so recall between random rows says little; the
planted leg says what a search is for: per query three rows query + noise x N(0, 1), clipped at 0, are written into the
smallest bank at the noise levels of --noise, and the share of them that each index returns in its top k is reported,
with recall@k on that bank.
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


def _fidelity(fp32, q8, k):
    """(recall@k, largest |score difference| over the rows both return) of two (score, index) results."""
    (sa, ia), (sb, ib) = fp32, q8
    both = ia.unsqueeze(2) == ib.unsqueeze(1)                            # (Q, k, k): fp32 slot x q8 slot
    recall = float(both.any(dim=2).float().mean())
    diff = (sa.unsqueeze(2) - sb.unsqueeze(1)).abs()
    worst = float(diff[both].max()) if bool(both.any()) else float("nan")
    return recall, worst


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, nargs="+", default=[100000, 1000000])
    ap.add_argument("--D", type=int, default=2184)
    ap.add_argument("--queries", type=int, nargs="+", default=[1, 16, 64])
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--inner", type=int, default=10)
    ap.add_argument("--noise", type=float, nargs="+", default=[0.25, 0.5, 1.0])
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "prof_search_q8 needs a GPU"
    dev = torch.device("cuda:0")
    D, k = args.D, args.k
    ld = ops.q8_ld(D)
    result = {"workload": {"D": D, "k": k, "repeats": args.repeats, "inner": args.inner}, "copy_TBs": COPY_TBS,
              "shapes": [], "planted": None, "skipped": []}
    for N in args.rows:
        free = torch.cuda.mem_get_info(dev)[0]
        if (4 * D + ld) * N * 1.25 > free:
            result["skipped"].append({"rows": N, "reason": f"banks of {(4 * D + ld) * N} bytes, {free} bytes free"})
            continue
        g = torch.Generator(device=dev).manual_seed(N)
        bank = torch.empty((N, D), device=dev)
        step = 65536
        for n0 in range(0, N, step):                       # filled in pieces: no second bank-sized temporary
            piece = bank[n0:n0 + step]
            piece.copy_((0.75 + torch.randn(piece.shape, device=dev, generator=g)).clamp_(min=0))
        ops.rows_normalize(bank, out=bank)
        codes, scale = ops.rows_quantize_q8(bank, normalize=False)
        for Q in args.queries:
            raw = (0.75 + torch.randn((Q, D), device=dev, generator=g)).clamp_(min=0)
            qn = ops.rows_normalize(raw)
            qc, qs = ops.rows_quantize_q8(raw, normalize=True)
            legs = {"torch": lambda: torch.topk(qn @ bank.T, k), "fp32": lambda: ops.embed_search(bank, qn, k),
                    "q8": lambda: ops.embed_search_q8(codes, scale, D, qc, qs, k)}
            warm = {name: fn() for name, fn in legs.items()}          # warm-up of all three, and how far apart they are
            recall, worst = _fidelity(warm["fp32"], warm["q8"], k)
            del warm
            times = {name: [] for name in legs}
            for _ in range(args.repeats):
                for name, fn in legs.items():
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    for _ in range(args.inner):
                        fn()
                    torch.cuda.synchronize()
                    times[name].append((time.perf_counter() - t0) / args.inner)
            r = {"rows": N, "Q": Q, "recall_at_k_vs_fp32": recall, "max_abs_score_diff_vs_fp32": worst}
            for name, ts in times.items():
                r[name] = {"median_us": 1e6 * statistics.median(ts), "min_us": 1e6 * min(ts), "max_us": 1e6 * max(ts),
                           "all_us": [round(1e6 * x, 1) for x in ts]}
            r["q8_over_torch"] = r["torch"]["median_us"] / r["q8"]["median_us"]
            r["q8_over_fp32"] = r["fp32"]["median_us"] / r["q8"]["median_us"]
            for name, row_bytes, group in (("fp32", 4 * D, ops.SEARCH_GROUP), ("q8", ld, ops.SEARCH_Q8_GROUP)):
                passes = -(-Q // group)
                tbs = row_bytes * N * passes / (1e-6 * r[name]["median_us"]) / 1e12
                r[name + "_bytes"] = {"bank": row_bytes * N, "passes": passes, "TBs": tbs, "of_copy": tbs / COPY_TBS}
            r["rows_per_us"] = {name: N / r[name]["median_us"] for name in legs}
            result["shapes"].append(r)
            print(json.dumps(r), flush=True)

        if result["planted"] is None:                      # the planted leg, on the first bank that fits
            Q = max(args.queries)
            raw = (0.75 + torch.randn((Q, D), device=dev, generator=g)).clamp_(min=0)
            qn = ops.rows_normalize(raw)
            qc, qs = ops.rows_quantize_q8(raw, normalize=True)
            rows = {}
            for j, noise in enumerate(args.noise):
                at = torch.arange(Q, device=dev) * (N // Q) + 7 * j + 1
                near = (raw + noise * torch.randn((Q, D), device=dev, generator=g)).clamp_(min=0)
                bank[at] = ops.rows_normalize(near)
                c, s = ops.rows_quantize_q8(bank[at].contiguous(), normalize=False)
                codes[at], scale[at] = c, s
                rows[noise] = at
            fp32, q8 = ops.embed_search(bank, qn, k), ops.embed_search_q8(codes, scale, D, qc, qs, k)
            recall, worst = _fidelity(fp32, q8, k)
            planted = {"rows": N, "Q": Q, "recall_at_k_vs_fp32": recall, "max_abs_score_diff_vs_fp32": worst, "levels": []}
            for noise, at in rows.items():
                cos = (bank[at] * qn).sum(dim=1)
                planted["levels"].append({"noise": noise, "mean_cosine": float(cos.mean()),
                                          "found_fp32": float((fp32[1] == at.unsqueeze(1).int()).any(dim=1).float().mean()),
                                          "found_q8": float((q8[1] == at.unsqueeze(1).int()).any(dim=1).float().mean())})
            # the same order among the rows that matter: the fp32 index's first three against the q8 index's
            planted["same_top3"] = float((fp32[1][:, :3] == q8[1][:, :3]).all(dim=1).float().mean())
            result["planted"] = planted
            print(json.dumps(planted), flush=True)
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
