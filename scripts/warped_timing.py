"""Cost of the warped coarse-to-fine solve next to the plain pyramid, 1080p,
w 5, 100 it per level, 3 levels, batch 1 and 8:

  (a) flow_pyramid_device, integer pair      packed-gradient Jacobi, 20 B/px per pass
  (b) flow_pyramid_device, non-integer pair  f32-plane Jacobi, 28 B/px per pass
  (c) flow_warped_device, warps = 1          (b)'s Jacobi + hs_warp_gradients_kernel
  (d) flow_warped_device, warps = 2

Device events around each eager call, a warm-up of every variant, the
variants alternated inside every round of one process.  (c) - (b) is what the
warp kernels cost, (b) / (a) what leaving the packed gradients costs; the
byte model's figures are printed beside them.

    python scripts/warped_timing.py                  # -> profiles/warped_timing.json
    python scripts/warped_timing.py --only b,c --rounds 3 --out ''   # under rocprofv3
    python scripts/warped_timing.py --trace-csv X_kernel_trace.csv   # per-kernel, per-size rates
"""
import argparse
import csv
import json
import os
import sys
from collections import defaultdict

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "cpp-optical-flow_amd"))

ROWS, COLS, WINDOW, ITERS, LEVELS, ALPHA = 1080, 1920, 5, 100, 3, 400.0
HBM_BYTES_PER_S = 8.0e12  # MI355X spec
# algorithmic bytes per pixel
B_JACOBI_PACKED, B_JACOBI_F32 = 20, 28   # per pass: gradients + (u, v) in + (u, v) out
B_K1_F32 = 8 + 4 + 8 + 12                # K1 (I0, I1 -> packed) + K1f (I0, I1 -> planes)
B_K1_INT = 8 + 4
B_WARP = 4 + 4 + 8 + 12                  # I0, I1, (u0, v0) -> gx, gy, gt'


def level_pixels():
    r, c, px = ROWS, COLS, []
    for _ in range(LEVELS):
        px.append(r * c)
        r, c = (r + 1) // 2, (c + 1) // 2
    return px


def model_ms(hsflow, batch):
    """Milliseconds at the HBM spec rate by algorithmic bytes."""
    px = level_pixels()
    r, c, passes = ROWS, COLS, []
    for _ in range(LEVELS):
        kb = hsflow.iters_per_launch(r, c, batch, WINDOW)
        passes.append(-(-ITERS // kb))
        r, c = (r + 1) // 2, (c + 1) // 2
    jac = lambda bpp, warps: sum(p * n * bpp * warps for p, n in zip(px, passes))  # noqa: E731
    # both solves run K1 once at level 0 for the pairs' integrality flags
    k1_a = B_K1_INT * (px[0] + sum(px))
    k1_b = B_K1_F32 * (px[0] + sum(px))
    warp = lambda warps: B_K1_F32 * px[0] + B_WARP * warps * sum(px)  # noqa: E731
    to_ms = lambda b: round(b * batch / HBM_BYTES_PER_S * 1e3, 4)  # noqa: E731
    m = {"a": to_ms(jac(B_JACOBI_PACKED, 1) + k1_a), "b": to_ms(jac(B_JACOBI_F32, 1) + k1_b),
         "c": to_ms(jac(B_JACOBI_F32, 1) + warp(1)), "d": to_ms(jac(B_JACOBI_F32, 2) + warp(2))}
    m["b_over_a"] = round(m["b"] / m["a"], 3)
    m["c_minus_b"] = round(m["c"] - m["b"], 4)
    m["warp_kernels_one_warp"] = to_ms(B_WARP * sum(px))
    return m


def run(args):
    import numpy as np
    import torch
    import hsflow

    only = [x for x in args.only.split(",") if x]
    out = {"shape": f"{COLS}x{ROWS}", "window": WINDOW, "iters_per_level": ITERS,
           "levels": LEVELS, "alpha": ALPHA, "rounds": args.rounds,
           "timing": "device events around one eager call; median and min over the rounds, "
                     "variants alternated inside every round",
           "model": "algorithmic bytes at 8 TB/s", "batches": {}}
    for batch in (1, 8):
        pairs = [hsflow.synth_pair(3000 + k, ROWS, COLS) for k in range(batch)]
        I0 = torch.from_numpy(np.stack([p[0] for p in pairs])).cuda()
        I1 = torch.from_numpy(np.stack([p[1] for p in pairs])).cuda()
        J0 = I0 * 0.9 + 0.3  # non-integer: the f32 gradient planes
        u, v = torch.empty_like(I0), torch.empty_like(I0)
        ws = torch.empty(hsflow.pyramid_workspace_bytes(ROWS, COLS, batch, LEVELS),
                         dtype=torch.uint8, device="cuda")
        variants = {
            "a": lambda: hsflow.flow_pyramid_device(I0, I1, LEVELS, WINDOW, ITERS, ALPHA, u, v, ws),
            "b": lambda: hsflow.flow_pyramid_device(J0, I1, LEVELS, WINDOW, ITERS, ALPHA, u, v, ws),
            "c": lambda: hsflow.flow_warped_device(J0, I1, LEVELS, 1, WINDOW, ITERS, ALPHA, u, v,
                                                   ws),
            "d": lambda: hsflow.flow_warped_device(J0, I1, LEVELS, 2, WINDOW, ITERS, ALPHA, u, v,
                                                   ws),
        }
        variants = {k: f for k, f in variants.items() if k in only}
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
        if "a" in med and "b" in med:
            res["b_over_a"] = round(med["b"] / med["a"], 3)
        if "b" in med and "c" in med:
            res["c_minus_b_ms"] = round(med["c"] - med["b"], 4)
        if "c" in med and "d" in med:
            res["d_minus_c_ms"] = round(med["d"] - med["c"], 4)
        res["model_ms"] = model_ms(hsflow, batch)
        res["jacobi_kernel_level0"] = hsflow.jacobi_kernel_name(ROWS, COLS, batch, WINDOW)
        out["batches"][str(batch)] = res
        print(json.dumps({"batch": batch, **res}), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(args.out), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")


def summarise_trace(path):
    """Mean duration and algorithmic bytes/s of K1, K1f and the warp kernel
    per launch size, from a rocprofv3 --kernel-trace CSV."""
    rows = defaultdict(list)
    with open(path) as f:
        for r in csv.DictReader(f):
            name = r["Kernel_Name"]
            key = next((k for k in ("hs_warp_gradients_kernel", "hs_gradients_f32_kernel",
                                    "hs_gradients_kernel") if k in name), None)
            if key is None:
                continue
            grid = (int(r["Grid_Size_X"]), int(r["Grid_Size_Y"]), int(r["Grid_Size_Z"]))
            rows[(key, grid)].append(int(r["End_Timestamp"]) - int(r["Start_Timestamp"]))
    px_levels = level_pixels()
    for (key, grid), ns in sorted(rows.items()):
        mean = sum(ns) / len(ns)
        print(json.dumps({"kernel": key, "grid": grid, "launches": len(ns),
                          "mean_us": round(mean / 1e3, 2), "min_us": round(min(ns) / 1e3, 2),
                          "level_pixels": px_levels}))


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", default="a,b,c,d")
    ap.add_argument("--rounds", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "warped_timing.json"))
    ap.add_argument("--trace-csv", default="")
    a = ap.parse_args()
    if a.trace_csv:
        summarise_trace(a.trace_csv)
    else:
        run(a)
