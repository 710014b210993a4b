"""Cost of the flow-driven smoothness term (KG hs_diffusivity_kernel, KJ
hs_jacobi_weighted_kernel) alone and inside the bidirectional solve, 1080p,
batch 1 and 8, window 5:

  (a)      flow_bidir_device, 100 it, 3 levels, 2 warps, median 5, alpha 100
  (b)      the same with smoothness=Smoothness(1, 0.3)
  (plain)  jacobi_device, 100 warm-started iterations on the f32 gradient
           planes warp_gradients_device left (the pass (a) runs)
  (kj_d<k>) jacobi_weighted_device, the same 100 iterations on the same planes
           at every depth KJ is built for (hsflow_set_iters_per_launch(k))
  (plain_w3, kj_w3_d<k>) the two at window 3, for KJ's depth there
  (kg)     diffusivity_device alone

Device events around each variant, a warm-up of all, the variants alternated
inside every round of one process.  KG runs REPS launches back to back between
its events.  The Jacobi variants are given per iteration and per pass (launch),
with the algorithmic bytes per pass over the time per pass; (b) as a ratio to
(a), next to (a)'s own spread between rounds.  No pass/fail number for speed.

Each batch runs in a child process of its own under a time limit; the parent
stops at the first child that fails.

    python scripts/smoothness_timing.py          # -> profiles/smoothness_timing.json
"""
import argparse
import json
import os
import subprocess
import sys
from collections import defaultdict

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "cpp-optical-flow_amd"))

ROWS, COLS, WINDOW, ITERS, LEVELS, WARPS, MEDIAN, ALPHA = 1080, 1920, 5, 100, 3, 2, 5, 100.0
LAM = 0.3
DEPTHS = (2, 3, 4)  # the depths KJ is built for at window 5
DEPTHS_W3 = (3, 4, 6)  # ... and at window 3
REPS = 10  # launches between the events of KG
STEP_LIMIT_S = 240  # one batch: warm-up and 15 rounds take a few seconds
# algorithmic bytes per pixel and pass
B_PLAIN = 8 + 12 + 8   # (u, v), (gx, gy, gt') -> (u, v)
B_KJ = 8 + 12 + 4 + 8  # ... and g
B_KG = 8 + 4           # (u, v) -> g


def _pairs(hsflow, batch):
    import numpy as np
    import torch
    pairs = [hsflow.synth_pair(3000 + k, ROWS, COLS) for k in range(batch)]
    I0 = torch.from_numpy(np.stack([p[0] for p in pairs])).cuda()
    I1 = torch.from_numpy(np.stack([p[1] for p in pairs])).cuda()
    return I0, I1


def run_batch(batch, rounds, warmup):
    import numpy as np
    import torch
    import hsflow

    I0, I1 = _pairs(hsflow, batch)
    S0, S1 = I0 * 0.9 + 0.3, I1  # non-integer f32, as prefilter_timing.py's
    uf, vf, ub, vb, g, u, v = (torch.empty_like(I0) for _ in range(7))
    mf, mb = (torch.empty(I0.shape, dtype=torch.uint8, device="cuda") for _ in range(2))
    ws = torch.empty(hsflow.bidir_workspace_bytes(ROWS, COLS, batch, LEVELS), dtype=torch.uint8,
                     device="cuda")
    jws = hsflow.alloc_workspace(ROWS, COLS, batch)
    solve = (LEVELS, WARPS, WINDOW, ITERS, ALPHA)
    sm = hsflow.Smoothness(hsflow.SMOOTH_FLOW_DRIVEN, LAM)

    def bidir(smoothness):
        return lambda: hsflow.flow_bidir_device(S0, S1, *solve, uf=uf, vf=vf, ub=ub, vb=vb,
                                                mask_f=mf, mask_b=mb, workspace=ws, median=MEDIAN,
                                                smoothness=smoothness)

    def plain(window=WINDOW):
        return lambda: hsflow.jacobi_device(ROWS, COLS, batch, window, ITERS, ALPHA, u, v, jws,
                                            warm_start=True)

    def kj(depth, window=WINDOW):
        def f():
            hsflow.set_iters_per_launch(depth)
            try:
                hsflow.jacobi_weighted_device(ROWS, COLS, batch, window, ITERS, ALPHA, g, u, v, jws)
            finally:
                hsflow.set_iters_per_launch(0)
        return f

    def kg():
        for _ in range(REPS):
            hsflow.diffusivity_device(uf, vf, LAM, g)

    variants = {"a": bidir(None), "b": bidir(sm), "plain": plain(), "kg": kg,
                "plain_w3": plain(3)}
    for d in DEPTHS:
        variants[f"kj_d{d}"] = kj(d)
    for d in DEPTHS_W3:
        variants[f"kj_w3_d{d}"] = kj(d, 3)
    passes = {"plain": -(-ITERS // hsflow.iters_per_launch(ROWS, COLS, batch, WINDOW)),
              "plain_w3": -(-ITERS // hsflow.iters_per_launch(ROWS, COLS, batch, 3))}
    passes.update({f"kj_d{d}": -(-ITERS // d) for d in DEPTHS})
    passes.update({f"kj_w3_d{d}": -(-ITERS // d) for d in DEPTHS_W3})
    bidir(sm)()  # the flows KG reads and the Jacobi variants start from
    hsflow.warp_gradients_device(S0, S1, uf, vf, jws)
    hsflow.diffusivity_device(uf, vf, LAM, g)
    u.copy_(uf)
    v.copy_(vf)
    for _ in range(warmup):
        for f in variants.values():
            f()
    torch.cuda.synchronize()
    ms = defaultdict(list)
    for _ in range(rounds):
        for k, f in variants.items():
            e0 = torch.cuda.Event(enable_timing=True)
            e1 = torch.cuda.Event(enable_timing=True)
            e0.record()
            f()
            e1.record()
            e1.synchronize()
            ms[k].append(e0.elapsed_time(e1) / (REPS if k == "kg" else 1))
    res = {k: {"median_ms": round(float(np.median(t)), 4), "min_ms": round(min(t), 4),
               "max_ms": round(max(t), 4),
               "spread_pct": round(100.0 * (max(t) - min(t)) / float(np.median(t)), 2)}
           for k, t in ms.items()}
    px = ROWS * COLS * batch
    for k, n in passes.items():
        r, b = res[k], (B_PLAIN if k.startswith("plain") else B_KJ)
        r["passes"] = n
        r["us_per_iteration"] = round(1e3 * r["median_ms"] / ITERS, 3)
        r["us_per_pass"] = round(1e3 * r["median_ms"] / n, 3)
        r["mpix_iter_per_s"] = round(px * ITERS / (r["median_ms"] * 1e-3) / 1e6, 0)
        r["bytes_per_px_pass"] = b
        r["tb_per_s"] = round(b * px * n / (r["median_ms"] * 1e-3) / 1e12, 3)
    res["plain"]["kernel"] = hsflow.jacobi_kernel_name(ROWS, COLS, batch, WINDOW)
    res["plain"]["depth"] = hsflow.iters_per_launch(ROWS, COLS, batch, WINDOW)
    res["plain_w3"]["kernel"] = hsflow.jacobi_kernel_name(ROWS, COLS, batch, 3)
    res["plain_w3"]["depth"] = hsflow.iters_per_launch(ROWS, COLS, batch, 3)
    for d in DEPTHS:
        res[f"kj_d{d}"]["time_over_plain"] = round(
            res[f"kj_d{d}"]["median_ms"] / res["plain"]["median_ms"], 3)
    for d in DEPTHS_W3:
        res[f"kj_w3_d{d}"]["time_over_plain"] = round(
            res[f"kj_w3_d{d}"]["median_ms"] / res["plain_w3"]["median_ms"], 3)
    res["kj_fastest_depth"] = {"w5": max(DEPTHS, key=lambda d: res[f"kj_d{d}"]["mpix_iter_per_s"]),
                               "w3": max(DEPTHS_W3,
                                         key=lambda d: res[f"kj_w3_d{d}"]["mpix_iter_per_s"])}
    res["kg"]["bytes_per_px"] = B_KG
    res["kg"]["tb_per_s"] = round(B_KG * px / (res["kg"]["median_ms"] * 1e-3) / 1e12, 3)
    res["b_over_a"] = round(res["b"]["median_ms"] / res["a"]["median_ms"], 3)
    res["a_spread_pct"] = res["a"]["spread_pct"]
    return res


def main(args):
    if args.batch:
        print(json.dumps(run_batch(args.batch, args.rounds, args.warmup)), flush=True)
        return 0
    variants = {"a": "flow_bidir_device, median 5, both masks",
                "b": f"the same with smoothness (flow-driven, lambda {LAM})",
                "plain": "jacobi_device, 100 warm-started iterations on f32 gradient planes",
                "kj_d<k>": "jacobi_weighted_device (KJ), the same iterations, k per launch",
                "plain_w3, kj_w3_d<k>": "the two at window 3",
                "kg": "diffusivity_device (KG)"}
    out = {"shape": f"{COLS}x{ROWS}", "window": WINDOW, "iters_per_level": ITERS,
           "levels": LEVELS, "warps": WARPS, "median": MEDIAN, "alpha": ALPHA, "lambda": LAM,
           "rounds": args.rounds,
           "timing": "device events around each variant; median, min and max over the rounds, "
                     f"variants alternated inside every round; KG: {REPS} launches between the "
                     "events, time per launch",
           "variants": variants, "batches": {}}
    for batch in (1, 8):
        # a fresh process per batch, under its own time limit; stop at a failure
        p = subprocess.run([sys.executable, os.path.abspath(__file__), "--batch", str(batch),
                            "--rounds", str(args.rounds), "--warmup", str(args.warmup)],
                           capture_output=True, text=True, timeout=STEP_LIMIT_S)
        if p.returncode != 0:
            sys.stderr.write(p.stdout + p.stderr)
            return p.returncode
        res = json.loads(p.stdout.strip().splitlines()[-1])
        out["batches"][str(batch)] = res
        print(json.dumps({"batch": batch, **res}), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(args.out), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")
    return 0


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--batch", type=int, default=0, help="one batch, result to stdout (child)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "smoothness_timing.json"))
    sys.exit(main(ap.parse_args()))
