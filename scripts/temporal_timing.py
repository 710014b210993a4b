"""Cost of the temporal warm start (KD hs_downflow_kernel, KP
hs_flow_predict_kernel, the *_init_device solves) at 1080p, batch 1 and 8,
window 5, 100 iterations, median 5, alpha 100:

  (a)   flow_bidir_device cold, 3 levels, 4 warps
  (b)   temporal.flow_bidir_device from a predicted start, 3 levels, 2 warps
  (c)   the same, 1 level, 1 warp
  (kd)  downflow_device alone, (kp) predict_device alone: REPS launches back to
        back between the events, with the algorithmic bytes per pixel over the
        time per launch

The iteration counts predict (b)/(a) = 0.5 and (c)/(a) = 1 / 5.25 = 0.19; what
is measured is reported next to them.  Device events around each variant, a
warm-up of all, the variants alternated inside every round of one process;
median, min and max over the rounds.  No pass/fail number for speed.

Each batch runs in a child process of its own under a time limit; the parent
stops at the first child that fails.

    python scripts/temporal_timing.py            # -> profiles/temporal_timing.json

--ab OTHER_LIBHSFLOW_SO: (a) alone on this build and on another build of the
library (the parent commit's), in child processes alternated this, other, this,
other: the cold path's time on both, next to the spread of two runs of one
build.  The result joins the JSON as "cold_path_ab".
"""
import argparse
import ctypes
import json
import os
import subprocess
import sys
from collections import defaultdict

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "cpp-optical-flow_amd"))

ROWS, COLS, WINDOW, ITERS, MEDIAN, ALPHA = 1080, 1920, 5, 100, 5, 100.0
COLD, WARM, WARM1 = (3, 4), (3, 2), (1, 1)  # (levels, warps) of (a), (b), (c)
REPS = 10  # launches between the events of KD and KP
STEP_LIMIT_S = 300  # one child: warm-up and 15 rounds take some seconds
B_KD = 8 + 2    # per fine pixel: (u, v) read, a quarter of (uc, vc) written
B_KP = 8 + 16   # (ub, vb) read (the taps hit the same lines), four planes written


def _hsflow(only_present):
    """hsflow; for another build of the library (HSFLOW_LIB) the prototypes it
    does not export yet are left out, so that it loads."""
    import hsflow
    if only_present:
        L = ctypes.CDLL(hsflow.LIB_PATH)
        for name in list(hsflow._PROTOTYPES):
            if not hasattr(L, name):
                del hsflow._PROTOTYPES[name]
    return hsflow


def _pairs(hsflow, batch):
    import numpy as np
    import torch
    pairs = [hsflow.synth_pair(3000 + k, ROWS, COLS) for k in range(batch)]
    I0 = torch.from_numpy(np.stack([p[0] for p in pairs])).cuda()
    I1 = torch.from_numpy(np.stack([p[1] for p in pairs])).cuda()
    return I0, I1


def _stats(np, t, reps=1):
    t = [x / reps for x in t]
    med = float(np.median(t))
    return {"median_ms": round(med, 4), "min_ms": round(min(t), 4), "max_ms": round(max(t), 4),
            "spread_pct": round(100.0 * (max(t) - min(t)) / med, 2)}


def run_batch(batch, rounds, warmup, cold_only):
    import numpy as np
    import torch
    hsflow = _hsflow(cold_only)

    I0, I1 = _pairs(hsflow, batch)
    S0, S1 = I0 * 0.9 + 0.3, I1  # non-integer f32, as smoothness_timing.py's
    uf, vf, ub, vb = (torch.empty_like(I0) for _ in range(4))
    mf, mb = (torch.empty(I0.shape, dtype=torch.uint8, device="cuda") for _ in range(2))
    ws = torch.empty(hsflow.bidir_workspace_bytes(ROWS, COLS, batch, COLD[0]), dtype=torch.uint8,
                     device="cuda")

    def cold():
        hsflow.flow_bidir_device(S0, S1, *COLD, WINDOW, ITERS, ALPHA, uf=uf, vf=vf, ub=ub, vb=vb,
                                 mask_f=mf, mask_b=mb, workspace=ws, median=MEDIAN)

    variants, reps = {"a": cold}, defaultdict(lambda: 1)
    if not cold_only:
        import temporal
        cold()
        start = temporal.predict_device(ub, vb)  # of the pair itself: realistic magnitudes
        nxt = temporal.FlowInit(*[torch.empty_like(I0) for _ in range(4)])
        rc, cc = hsflow.pyramid_level_size(ROWS, COLS, 1)
        uc, vc = (torch.empty((batch, rc, cc), dtype=torch.float32, device="cuda")
                  for _ in range(2))

        def warm(levels, warps):
            return lambda: temporal.flow_bidir_device(
                S0, S1, levels, warps, WINDOW, ITERS, ALPHA, uf=uf, vf=vf, ub=ub, vb=vb,
                mask_f=mf, mask_b=mb, workspace=ws, median=MEDIAN, init=start)

        def kd():
            for _ in range(REPS):
                temporal.downflow_device(start.uf, start.vf, uc, vc)

        def kp():
            for _ in range(REPS):
                temporal.predict_device(start.ub, start.vb, out=nxt)

        variants.update({"b": warm(*WARM), "c": warm(*WARM1), "kd": kd, "kp": kp})
        reps.update({"kd": REPS, "kp": REPS})
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
            ms[k].append(e0.elapsed_time(e1))
    res = {k: _stats(np, t, reps[k]) for k, t in ms.items()}
    if cold_only:
        return res
    px = ROWS * COLS * batch
    for k, b in (("kd", B_KD), ("kp", B_KP)):
        res[k]["bytes_per_px"] = b
        res[k]["tb_per_s"] = round(b * px / (res[k]["median_ms"] * 1e-3) / 1e12, 3)
    res["b_over_a"] = round(res["b"]["median_ms"] / res["a"]["median_ms"], 3)
    res["c_over_a"] = round(res["c"]["median_ms"] / res["a"]["median_ms"], 3)
    res["predicted"] = {"b_over_a": 0.5, "c_over_a": round(1 / 5.25, 3)}
    res["a_spread_pct"] = res["a"]["spread_pct"]
    return res


def _child(batch, args, lib=None):
    """One batch in a fresh process under its own time limit -> its result."""
    env = dict(os.environ)
    cmd = [sys.executable, os.path.abspath(__file__), "--batch", str(batch), "--rounds",
           str(args.rounds), "--warmup", str(args.warmup)]
    if lib is not None:
        cmd.append("--cold-only")
        if lib:
            env["HSFLOW_LIB"] = os.path.abspath(lib)
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=STEP_LIMIT_S, env=env)
    if p.returncode != 0:
        sys.stderr.write(p.stdout + p.stderr)
        return None
    return json.loads(p.stdout.strip().splitlines()[-1])


def main(args):
    if args.batch:
        print(json.dumps(run_batch(args.batch, args.rounds, args.warmup, args.cold_only)),
              flush=True)
        return 0
    variants = {"a": f"flow_bidir_device cold, {COLD[0]} levels, {COLD[1]} warps, both masks",
                "b": f"from a predicted start, {WARM[0]} levels, {WARM[1]} warps",
                "c": f"from a predicted start, {WARM1[0]} level, {WARM1[1]} warp",
                "kd": "downflow_device (KD)", "kp": "predict_device (KP)"}
    out = {"shape": f"{COLS}x{ROWS}", "window": WINDOW, "iters_per_warp": ITERS, "median": MEDIAN,
           "alpha": ALPHA, "rounds": args.rounds,
           "timing": "device events around each variant; median, min and max over the rounds, "
                     f"variants alternated inside every round; KD, KP: {REPS} launches between "
                     "the events, time per launch",
           "variants": variants, "batches": {}}
    for batch in (1, 8):
        res = _child(batch, args)
        if res is None:
            return 1
        out["batches"][str(batch)] = res
        print(json.dumps({"batch": batch, **res}), flush=True)
    if args.ab:
        ab = {"other": os.path.basename(args.ab), "order": "this, other, this, other",
              "batches": {}}
        for batch in (1, 8):
            runs = {"this": [], "other": []}
            for who in ("this", "other", "this", "other"):
                res = _child(batch, args, lib=args.ab if who == "other" else "")
                if res is None:
                    return 1
                runs[who].append(res["a"])
            med = {w: [r["median_ms"] for r in rs] for w, rs in runs.items()}
            ab["batches"][str(batch)] = {
                "a_median_ms": med,
                "this_over_other": round(sum(med["this"]) / sum(med["other"]), 4),
                "run_to_run_pct": {w: round(100.0 * abs(m[0] - m[1]) / min(m), 2)
                                   for w, m in med.items()}}
            print(json.dumps({"ab_batch": batch, **ab["batches"][str(batch)]}), flush=True)
        out["cold_path_ab"] = ab
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
    ap.add_argument("--cold-only", action="store_true", help="(a) alone (child of --ab)")
    ap.add_argument("--ab", default="", help="another build of libhsflow.so to time (a) against")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "temporal_timing.json"))
    sys.exit(main(ap.parse_args()))
