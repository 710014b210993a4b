"""Cost of the median filter between warps (KM, hs_flow_median_kernel), 1080p,
batch 1 and 8:

  (w0) flow_warped_device, 3 levels, 2 warps, w 5, 100 it, median = 0
  (w3) the same with median = 3
  (w5) the same with median = 5
  (k3) median_device alone, 3 x 3          (k5) median_device alone, 5 x 5

Device events around each eager call, a warm-up of every variant, the
variants alternated inside every round of one process; median, min and max
over the rounds.  w5 - w0 is what the filter costs a solve: 6 KM launches
(3 levels x 2 warps) and their copies back.  The byte model's figures are
printed beside them.  (w0)'s inputs are those of scripts/warped_timing.py's
(d), so the two scripts' figures can be set side by side.

    python scripts/median_timing.py                  # -> profiles/median_timing.json
    python scripts/median_timing.py --only k3,k5 --rounds 3 --out ''   # under rocprofv3
    python scripts/median_timing.py --trace-csv X_kernel_trace.csv     # per-kernel means
"""
import argparse
import csv
import json
import os
import sys
from collections import defaultdict

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "cpp-optical-flow_amd"))

ROWS, COLS, WINDOW, ITERS, LEVELS, WARPS, ALPHA = 1080, 1920, 5, 100, 3, 2, 400.0
HBM_BYTES_PER_S = 8.0e12  # MI355X spec
B_KM = 8 + 8        # (u, v) read, (u, v) written
B_COPY_BACK = 16    # the second planes read, (u, v) written: two device copies
# min/max per pixel and plane (scripts/median_network_check.cpp)
OPS = {3: 18, 5: 158}


def level_pixels():
    r, c, px = ROWS, COLS, []
    for _ in range(LEVELS):
        px.append(r * c)
        r, c = (r + 1) // 2, (c + 1) // 2
    return px


def model(batch):
    px = level_pixels()
    to_ms = lambda b: round(b * batch / HBM_BYTES_PER_S * 1e3, 4)  # noqa: E731
    return {"km_alone_ms": to_ms(B_KM * px[0]),
            "filter_in_solve_ms": to_ms((B_KM + B_COPY_BACK) * WARPS * sum(px)),
            "minmax_per_pixel_both_planes": {k: 2 * n for k, n in OPS.items()}}


def run(args):
    import numpy as np
    import torch
    import hsflow

    only = [x for x in args.only.split(",") if x]
    out = {"shape": f"{COLS}x{ROWS}", "window": WINDOW, "iters_per_level": ITERS,
           "levels": LEVELS, "warps": WARPS, "alpha": ALPHA, "rounds": args.rounds,
           "timing": "device events around one eager call; median, min and max over the "
                     "rounds, variants alternated inside every round",
           "model": "algorithmic bytes at 8 TB/s", "batches": {}}
    for batch in (1, 8):
        pairs = [hsflow.synth_pair(3000 + k, ROWS, COLS) for k in range(batch)]
        I0 = torch.from_numpy(np.stack([p[0] for p in pairs])).cuda()
        I1 = torch.from_numpy(np.stack([p[1] for p in pairs])).cuda()
        J0 = I0 * 0.9 + 0.3  # non-integer, as warped_timing.py's warped variants
        u, v = torch.empty_like(I0), torch.empty_like(I0)
        fu, fv = torch.empty_like(I0), torch.empty_like(I0)
        ws = torch.empty(hsflow.pyramid_workspace_bytes(ROWS, COLS, batch, LEVELS),
                         dtype=torch.uint8, device="cuda")

        def solve(median):
            return lambda: hsflow.flow_warped_device(J0, I1, LEVELS, WARPS, WINDOW, ITERS, ALPHA,
                                                     u, v, ws, median=median)

        def alone(k):
            return lambda: hsflow.median_device(u, v, k, fu, fv)

        variants = {"w0": solve(0), "w3": solve(3), "w5": solve(5), "k3": alone(3),
                    "k5": alone(5)}
        variants = {k: f for k, f in variants.items() if k in only}
        solve(0)()  # (u, v) hold a flow whatever runs first
        for _ in range(args.warmup):
            for f in variants.values():
                f()
        torch.cuda.synchronize()
        ms = defaultdict(list)
        for _ in range(args.rounds):
            for k, f in variants.items():
                e0 = torch.cuda.Event(enable_timing=True)
                e1 = torch.cuda.Event(enable_timing=True)
                e0.record()
                f()
                e1.record()
                e1.synchronize()
                ms[k].append(e0.elapsed_time(e1))
        res = {k: {"median_ms": round(float(np.median(t)), 4), "min_ms": round(min(t), 4),
                   "max_ms": round(max(t), 4)} for k, t in ms.items()}
        med = {k: r["median_ms"] for k, r in res.items()}
        for k in ("w3", "w5"):
            if "w0" in med and k in med:
                res[f"{k}_minus_w0_ms"] = round(med[k] - med["w0"], 4)
        res["model"] = model(batch)
        out["batches"][str(batch)] = res
        print(json.dumps({"batch": batch, **res}), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(args.out), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")


def summarise_trace(path):
    """Mean duration of KM and of the warp kernel per launch size, from a
    rocprofv3 --kernel-trace CSV."""
    rows = defaultdict(list)
    with open(path) as f:
        for r in csv.DictReader(f):
            name = r["Kernel_Name"]
            key = next((k for k in ("hs_flow_median_kernel<3>", "hs_flow_median_kernel<5>",
                                    "hs_flow_median_kernel", "hs_warp_gradients_kernel",
                                    "hs_jacobi") if k in name), None)
            if key is None:
                continue
            grid = (int(r["Grid_Size_X"]), int(r["Grid_Size_Y"]), int(r["Grid_Size_Z"]))
            rows[(key if key != "hs_jacobi" else name.split("(")[0][-60:], grid)].append(
                int(r["End_Timestamp"]) - int(r["Start_Timestamp"]))
    for (key, grid), ns in sorted(rows.items()):
        mean = sum(ns) / len(ns)
        print(json.dumps({"kernel": key, "grid": grid, "launches": len(ns),
                          "mean_us": round(mean / 1e3, 2), "min_us": round(min(ns) / 1e3, 2)}))


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", default="w0,w3,w5,k3,k5")
    ap.add_argument("--rounds", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "median_timing.json"))
    ap.add_argument("--trace-csv", default="")
    a = ap.parse_args()
    if a.trace_csv:
        summarise_trace(a.trace_csv)
    else:
        run(a)
