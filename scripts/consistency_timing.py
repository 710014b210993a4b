"""Cost of the bidirectional warped solve and its forward-backward check,
1080p, w 5, 100 it per level, 3 levels, 2 warps, batch 1 and 8:

  (a) two flow_warped_device calls (I0 -> I1, I1 -> I0) + two consistency_device
      calls (err off, mask + counts each way)
  (b) one flow_bidir_device call with both masks and counts

Device events around each variant, a warm-up of both, the variants alternated
inside every round of one process.  The spread between rounds is recorded
next to the medians: (b) - (a) means something only beyond it.

    python scripts/consistency_timing.py               # -> profiles/consistency_timing.json
    python scripts/consistency_timing.py --kernels     # KC and KW alone at 1080p, under
                                                       # rocprofv3 --kernel-trace
    python scripts/consistency_timing.py --trace-csv X_kernel_trace.csv
                                                       # their rates into the same JSON
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
# algorithmic bytes per pixel
B_KC = 8 + 8 + 4 + 1   # (uf, vf), (ub, vb) once each -> err, mask
B_KC_MASK = 8 + 8 + 1  # mask and counts only
B_KW = 4 + 4 + 8 + 12  # f32 I0, I1, (u0, v0) -> gx, gy, gt'
KERNELS = {"hs_flow_consistency_kernel": B_KC, "hs_warp_gradients_kernel": B_KW}


def _pairs(hsflow, batch):
    import numpy as np
    import torch
    pairs = [hsflow.synth_pair(3000 + k, ROWS, COLS) for k in range(batch)]
    I0 = torch.from_numpy(np.stack([p[0] for p in pairs])).cuda()
    I1 = torch.from_numpy(np.stack([p[1] for p in pairs])).cuda()
    return I0 * 0.9 + 0.3, I1  # non-integer, as scripts/warped_timing.py's (c), (d)


def run(args):
    import numpy as np
    import torch
    import hsflow

    out = {"shape": f"{COLS}x{ROWS}", "window": WINDOW, "iters_per_level": ITERS,
           "levels": LEVELS, "warps": WARPS, "alpha": ALPHA, "rounds": args.rounds,
           "timing": "device events around each variant; median, min and max over the rounds, "
                     "variants alternated inside every round",
           "a": "2 x flow_warped_device + 2 x consistency_device (mask, counts)",
           "b": "1 x flow_bidir_device (both masks, both counts)", "batches": {}}
    for batch in (1, 8):
        I0, I1 = _pairs(hsflow, batch)
        uf, vf, ub, vb = (torch.empty_like(I0) for _ in range(4))
        mf, mb = (torch.empty(I0.shape, dtype=torch.uint8, device="cuda") for _ in range(2))
        cf, cb = (torch.empty((batch, 3), dtype=torch.int32, device="cuda") for _ in range(2))
        ws = torch.empty(hsflow.bidir_workspace_bytes(ROWS, COLS, batch, LEVELS),
                         dtype=torch.uint8, device="cuda")

        def separate():
            hsflow.flow_warped_device(I0, I1, LEVELS, WARPS, WINDOW, ITERS, ALPHA, uf, vf, ws)
            hsflow.flow_warped_device(I1, I0, LEVELS, WARPS, WINDOW, ITERS, ALPHA, ub, vb, ws)
            hsflow.consistency_device(uf, vf, ub, vb, mask=mf, counts=cf)
            hsflow.consistency_device(ub, vb, uf, vf, mask=mb, counts=cb)

        def fused():
            hsflow.flow_bidir_device(I0, I1, LEVELS, WARPS, WINDOW, ITERS, ALPHA,
                                     uf=uf, vf=vf, ub=ub, vb=vb, mask_f=mf, counts_f=cf,
                                     mask_b=mb, counts_b=cb, workspace=ws)

        variants = {"a": separate, "b": fused}
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
                   "max_ms": round(max(t), 4),
                   "spread_pct": round(100.0 * (max(t) - min(t)) / float(np.median(t)), 2)}
               for k, t in ms.items()}
        res["b_minus_a_ms"] = round(res["b"]["median_ms"] - res["a"]["median_ms"], 4)
        res["b_over_a"] = round(res["b"]["median_ms"] / res["a"]["median_ms"], 4)
        res["counts_forward"] = cf.cpu().numpy().sum(axis=0).tolist()
        res["kc_model_ms_at_8TBps"] = round(
            2 * B_KC_MASK * ROWS * COLS * batch / HBM_BYTES_PER_S * 1e3, 4)
        out["batches"][str(batch)] = res
        print(json.dumps({"batch": batch, **res}), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(args.out), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")


def run_kernels(args):
    """KC (err + mask + counts) and KW alone on 1080p f32 planes, batch 1 and
    8, for a kernel trace: same shape, same process, same box."""
    import torch
    import hsflow

    for batch in (1, 8):
        I0, I1 = _pairs(hsflow, batch)
        ws = torch.empty(hsflow.bidir_workspace_bytes(ROWS, COLS, batch, LEVELS),
                         dtype=torch.uint8, device="cuda")
        r = hsflow.flow_bidir_device(I0, I1, LEVELS, 1, WINDOW, 20, ALPHA, mask_f=None,
                                     workspace=ws)
        err = torch.empty_like(I0)
        mask = torch.empty(I0.shape, dtype=torch.uint8, device="cuda")
        counts = torch.empty((batch, 3), dtype=torch.int32, device="cuda")
        for _ in range(args.rounds):
            hsflow.consistency_device(r.uf, r.vf, r.ub, r.vb, err=err, mask=mask, counts=counts)
            hsflow.warp_gradients_device(I0, I1, r.uf, r.vf, ws)
        torch.cuda.synchronize()
        print(json.dumps({"batch": batch, "counts": counts.cpu().numpy().sum(axis=0).tolist()}),
              flush=True)


def summarise_trace(path, out_path):
    """Mean duration and algorithmic bytes/s of KC and KW per batch at 1080p,
    from a rocprofv3 --kernel-trace CSV of a --kernels run."""
    rows = defaultdict(list)
    with open(path) as f:
        for r in csv.DictReader(f):
            key = next((k for k in KERNELS if k in r["Kernel_Name"]), None)
            if key is None:
                continue
            # the pair index is the grid's last used axis, one workgroup thick
            batch = int(r["Grid_Size_Y"]) if key == "hs_flow_consistency_kernel" \
                else int(r["Grid_Size_Z"])
            rows[(key, batch)].append(int(r["End_Timestamp"]) - int(r["Start_Timestamp"]))
    res = []
    for (key, batch), ns in sorted(rows.items()):
        ns = ns[len(ns) // 4:]  # the first quarter warms caches and clocks
        mean = sum(ns) / len(ns)
        nbytes = KERNELS[key] * ROWS * COLS * batch
        res.append({"kernel": key, "batch": batch, "launches": len(ns),
                    "mean_us": round(mean / 1e3, 2), "min_us": round(min(ns) / 1e3, 2),
                    "bytes_per_px": KERNELS[key],
                    "tb_per_s": round(nbytes / mean / 1e3, 3)})
        print(json.dumps(res[-1]))
    if out_path and os.path.exists(out_path):
        with open(out_path) as f:
            out = json.load(f)
        out["kernel_trace"] = {"what": "rocprofv3 --kernel-trace of --kernels, 1080p f32 planes; "
                                       "algorithmic bytes over mean kernel time", "kernels": res}
        with open(out_path, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "consistency_timing.json"))
    ap.add_argument("--kernels", action="store_true")
    ap.add_argument("--trace-csv", default="")
    a = ap.parse_args()
    if a.trace_csv:
        summarise_trace(a.trace_csv, a.out)
    elif a.kernels:
        run_kernels(a)
    else:
        run(a)
