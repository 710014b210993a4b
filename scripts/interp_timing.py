"""Cost of the frame interpolation next to the bidirectional solve it consumes,
1080p, non-integer f32 pair, w 5, 100 it per level, 3 levels, 2 warps, batch 1
and 8:

  (a)  flow_bidir_device alone (both masks, both counts: consistency_timing.py's (b))
  (b)  flow_interp_device, nt = 1 (frames, flags, trusted)
  (c)  flow_interp_device, nt = 3
  (d1) frame_interp_device alone, nt = 1   (KI: masks in, frames, flags, trusted out)
  (d3) frame_interp_device alone, nt = 3
  (e)  warp_image_device alone             (KR)
  (kc) consistency_device alone (err, mask, counts)        the neighbours KI and
  (kw) warp_gradients_device alone                         KR are compared with

Device events around each variant, a warm-up of all, the variants alternated
inside every round of one process.  The kernels alone run REPS launches back
to back between their events, so the figure per launch holds little of the
events' own cost.  Achieved bytes per second = algorithmic bytes (below) over
the median time per launch; KI's and KR's are also given as ratios to KC's and
KW's of the same run, with the rounds' min-max.  No pass/fail number for speed.

Each batch runs in a child process of its own under a time limit; the parent
stops at the first child that fails.

    python scripts/interp_timing.py               # -> profiles/interp_timing.json
"""
import argparse
import json
import os
import subprocess
import sys
from collections import defaultdict

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "cpp-optical-flow_amd"))

ROWS, COLS, WINDOW, ITERS, LEVELS, WARPS, ALPHA = 1080, 1920, 5, 100, 3, 2, 400.0
TIMES = {1: (0.5,), 3: (0.25, 0.5, 0.75)}
REPS = 10  # launches between the events of a kernel timed alone
STEP_LIMIT_S = 240  # one batch: warm-up and 15 rounds take a few seconds
# algorithmic bytes per pixel (f32 frames)
B_KC = 8 + 8 + 4 + 1   # (uf, vf), (ub, vb) once each -> err, mask
B_KW = 4 + 4 + 8 + 12  # I0, I1, (u0, v0) -> gx, gy, gt'
B_KR = 4 + 8 + 4       # I, (u, v) -> out


def b_ki(nt):
    """16 B of flows once; per time 8 B of frames and 2 B of masks in, 4 B of
    frame and 1 B of flags out."""
    return 16 + nt * (8 + 2 + 4 + 1)


def _pairs(hsflow, batch):
    import numpy as np
    import torch
    pairs = [hsflow.synth_pair(3000 + k, ROWS, COLS) for k in range(batch)]
    I0 = torch.from_numpy(np.stack([p[0] for p in pairs])).cuda()
    I1 = torch.from_numpy(np.stack([p[1] for p in pairs])).cuda()
    return I0 * 0.9 + 0.3, I1  # non-integer, as scripts/consistency_timing.py's


def run_batch(batch, rounds, warmup):
    import numpy as np
    import torch
    import hsflow

    I0, I1 = _pairs(hsflow, batch)
    uf, vf, ub, vb, err, warped = (torch.empty_like(I0) for _ in range(6))
    mf, mb = (torch.empty(I0.shape, dtype=torch.uint8, device="cuda") for _ in range(2))
    cf, cb = (torch.empty((batch, 3), dtype=torch.int32, device="cuda") for _ in range(2))
    out = {nt: torch.empty((batch, nt, ROWS, COLS), dtype=torch.float32, device="cuda")
           for nt in TIMES}
    flags = {nt: torch.empty((batch, nt, ROWS, COLS), dtype=torch.uint8, device="cuda")
             for nt in TIMES}
    trusted = {nt: torch.empty((batch, nt), dtype=torch.int32, device="cuda") for nt in TIMES}
    ws = torch.empty(hsflow.flow_interp_workspace_bytes(ROWS, COLS, batch, LEVELS),
                     dtype=torch.uint8, device="cuda")
    solve = (LEVELS, WARPS, WINDOW, ITERS, ALPHA)

    def bidir():
        hsflow.flow_bidir_device(I0, I1, *solve, uf=uf, vf=vf, ub=ub, vb=vb, mask_f=mf,
                                 counts_f=cf, mask_b=mb, counts_b=cb, workspace=ws)

    def fused(nt):
        return lambda: hsflow.flow_interp_device(I0, I1, TIMES[nt], *solve, out=out[nt],
                                                 flags=flags[nt], trusted=trusted[nt],
                                                 workspace=ws)

    def ki(nt):
        def f():
            for _ in range(REPS):
                hsflow.frame_interp_device(I0, I1, uf, vf, ub, vb, TIMES[nt], mask_f=mf,
                                           mask_b=mb, out=out[nt], flags=flags[nt],
                                           trusted=trusted[nt])
        return f

    def kr():
        for _ in range(REPS):
            hsflow.warp_image_device(I1, uf, vf, out=warped)

    def kc():
        for _ in range(REPS):
            hsflow.consistency_device(uf, vf, ub, vb, err=err, mask=mf, counts=cf)

    def kw():
        for _ in range(REPS):
            hsflow.warp_gradients_device(I0, I1, uf, vf, ws)

    variants = {"a": bidir, "b": fused(1), "c": fused(3), "d1": ki(1), "d3": ki(3), "e": kr,
                "kc": kc, "kw": kw}
    per_launch = {"d1": REPS, "d3": REPS, "e": REPS, "kc": REPS, "kw": REPS}
    bidir()  # the flows and masks the kernels alone read
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
            ms[k].append(e0.elapsed_time(e1) / per_launch.get(k, 1))
    res = {k: {"median_ms": round(float(np.median(t)), 4), "min_ms": round(min(t), 4),
               "max_ms": round(max(t), 4),
               "spread_pct": round(100.0 * (max(t) - min(t)) / float(np.median(t)), 2)}
           for k, t in ms.items()}
    px = ROWS * COLS * batch
    nbytes = {"d1": b_ki(1), "d3": b_ki(3), "e": B_KR, "kc": B_KC, "kw": B_KW}
    for k, b in nbytes.items():
        r = res[k]
        r["bytes_per_px"] = b
        r["tb_per_s"] = round(b * px / (r["median_ms"] * 1e-3) / 1e12, 3)
        r["tb_per_s_min_max"] = [round(b * px / (r[m] * 1e-3) / 1e12, 3)
                                 for m in ("max_ms", "min_ms")]
    for k in ("d1", "d3", "e"):
        for other in ("kc", "kw"):
            res[k][f"rate_over_{other}"] = round(res[k]["tb_per_s"] / res[other]["tb_per_s"], 3)
            res[k][f"rate_over_{other}_min_max"] = [
                round(res[k]["tb_per_s_min_max"][0] / res[other]["tb_per_s_min_max"][1], 3),
                round(res[k]["tb_per_s_min_max"][1] / res[other]["tb_per_s_min_max"][0], 3)]
    res["b_minus_a_ms"] = round(res["b"]["median_ms"] - res["a"]["median_ms"], 4)
    res["c_minus_a_ms"] = round(res["c"]["median_ms"] - res["a"]["median_ms"], 4)
    res["trusted_share"] = {str(nt): [round(float(x), 4) for x in
                                      (trusted[nt].cpu().numpy().sum(axis=0) / px)]
                            for nt in TIMES}
    return res


def main(args):
    if args.batch:
        print(json.dumps(run_batch(args.batch, args.rounds, args.warmup)), flush=True)
        return 0
    out = {"shape": f"{COLS}x{ROWS}", "window": WINDOW, "iters_per_level": ITERS,
           "levels": LEVELS, "warps": WARPS, "alpha": ALPHA, "rounds": args.rounds,
           "times": {str(k): list(v) for k, v in TIMES.items()},
           "timing": "device events around each variant; median, min and max over the rounds, "
                     f"variants alternated inside every round; kernels alone: {REPS} launches "
                     "between the events, time per launch",
           "variants": {"a": "flow_bidir_device (both masks, both counts)",
                        "b": "flow_interp_device nt 1 (frames, flags, trusted)",
                        "c": "flow_interp_device nt 3",
                        "d1": "frame_interp_device nt 1 (KI)", "d3": "frame_interp_device nt 3",
                        "e": "warp_image_device (KR)", "kc": "consistency_device err + mask + "
                        "counts (KC)", "kw": "warp_gradients_device (KW)"},
           "batches": {}}
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "interp_timing.json"))
    sys.exit(main(ap.parse_args()))
