"""Cost of the coarse solve (KB hs_upflow_bilinear_kernel, the *_lv_device
solves) at 1080p and 4K, batch 1 and 8, window 5, 100 iterations, median 5,
alpha 100; the bidirectional cold solve, 3 levels, 4 warps, both masks:

  (a)   finest = 0: every level solved, the call as it was
  (b)   finest = 1: levels 2 and 1 solved, one KB launch per direction
  (c)   finest = 2: level 2 solved, two KB launches per direction
  (kb)  upflow_bilinear_device alone, level 1 -> level 0: REPS launches back to
        back between the events, with the algorithmic bytes per fine pixel (8
        written, 2 read) over the time per launch, next to the 8 TB/s of HBM

By pixel x iterations (b)/(a) = (1/4 + 1/16) / (1 + 1/4 + 1/16) = 0.238 and
(c)/(a) = (1/16) / (1 + 1/4 + 1/16) = 0.048; what is measured is reported next
to them.  Device events around each variant, a warm-up of all, the variants
alternated inside every round of one process; median, min and max over the
rounds.  No pass/fail number for speed.

Each (shape, batch) runs in a child process of its own under a time limit; the
parent stops at the first child that fails.

    python scripts/finest_timing.py            # -> profiles/finest_timing.json

--ab OTHER_LIBHSFLOW_SO: (a) alone on this build and on another build of the
library (the parent commit's), in child processes alternated this, other, this,
other: the default path's time on both -- it may not pay for the feature --
next to the spread of two runs of one build.  The result joins the JSON as
"default_path_ab" ((e) is its "other").
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

SHAPES = {"1080p": (1080, 1920), "4k": (2160, 3840)}
WINDOW, ITERS, MEDIAN, ALPHA = 5, 100, 5, 100.0
LEVELS, WARPS = 3, 4
REPS = 10  # launches between the events of KB
STEP_LIMIT_S = 300  # one child: warm-up and 15 rounds take some seconds
B_KB = 8 + 2  # per fine pixel: (u, v) written, a quarter of (uc, vc) read
HBM_TB_S = 8.0
PREDICTED = {"b_over_a": round((1 / 4 + 1 / 16) / (1 + 1 / 4 + 1 / 16), 3),
             "c_over_a": round((1 / 16) / (1 + 1 / 4 + 1 / 16), 3)}


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


def _pairs(hsflow, rows, cols, batch):
    import numpy as np
    import torch
    pairs = [hsflow.synth_pair(3000 + k, rows, cols) for k in range(batch)]
    I0 = torch.from_numpy(np.stack([p[0] for p in pairs])).cuda()
    I1 = torch.from_numpy(np.stack([p[1] for p in pairs])).cuda()
    return I0, I1


def _stats(np, t, reps=1):
    t = [x / reps for x in t]
    med = float(np.median(t))
    return {"median_ms": round(med, 4), "min_ms": round(min(t), 4), "max_ms": round(max(t), 4),
            "spread_pct": round(100.0 * (max(t) - min(t)) / med, 2)}


def run_case(shape, batch, rounds, warmup, default_only):
    import numpy as np
    import torch
    hsflow = _hsflow(default_only)
    rows, cols = SHAPES[shape]

    I0, I1 = _pairs(hsflow, rows, cols, batch)
    S0, S1 = I0 * 0.9 + 0.3, I1  # non-integer f32, as temporal_timing.py's
    uf, vf, ub, vb = (torch.empty_like(I0) for _ in range(4))
    mf, mb = (torch.empty(I0.shape, dtype=torch.uint8, device="cuda") for _ in range(2))
    ws = torch.empty(hsflow.bidir_workspace_bytes(rows, cols, batch, LEVELS), dtype=torch.uint8,
                     device="cuda")

    def solve(finest):
        kw = {"finest": finest} if finest else {}  # finest = 0: the call as it was
        return lambda: hsflow.flow_bidir_device(
            S0, S1, LEVELS, WARPS, WINDOW, ITERS, ALPHA, uf=uf, vf=vf, ub=ub, vb=vb, mask_f=mf,
            mask_b=mb, workspace=ws, median=MEDIAN, **kw)

    variants, reps = {"a": solve(0)}, defaultdict(lambda: 1)
    if not default_only:
        import coarse
        rc, cc = hsflow.pyramid_level_size(rows, cols, 1)
        uc, vc = (torch.randn((batch, rc, cc), dtype=torch.float32, device="cuda")
                  for _ in range(2))

        def kb():
            for _ in range(REPS):
                coarse.upflow_bilinear_device(uc, vc, uf, vf)

        variants.update({"b": solve(1), "c": solve(2), "kb": kb})
        reps.update({"kb": REPS})
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
    if default_only:
        return res
    px = rows * cols * batch
    res["kb"]["us"] = round(1e3 * res["kb"]["median_ms"], 2)
    res["kb"]["bytes_per_px"] = B_KB
    res["kb"]["tb_per_s"] = round(B_KB * px / (res["kb"]["median_ms"] * 1e-3) / 1e12, 3)
    res["kb"]["of_hbm"] = round(res["kb"]["tb_per_s"] / HBM_TB_S, 3)
    res["b_over_a"] = round(res["b"]["median_ms"] / res["a"]["median_ms"], 3)
    res["c_over_a"] = round(res["c"]["median_ms"] / res["a"]["median_ms"], 3)
    res["predicted"] = PREDICTED
    res["a_spread_pct"] = res["a"]["spread_pct"]
    return res


def _child(shape, batch, args, lib=None):
    """One (shape, batch) in a fresh process under its own time limit -> its result."""
    env = dict(os.environ)
    cmd = [sys.executable, os.path.abspath(__file__), "--shape", shape, "--batch", str(batch),
           "--rounds", str(args.rounds), "--warmup", str(args.warmup)]
    if lib is not None:
        cmd.append("--default-only")
        if lib:
            env["HSFLOW_LIB"] = os.path.abspath(lib)
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=STEP_LIMIT_S, env=env)
    if p.returncode != 0:
        sys.stderr.write(p.stdout + p.stderr)
        return None
    return json.loads(p.stdout.strip().splitlines()[-1])


def main(args):
    if args.batch:
        print(json.dumps(run_case(args.shape, args.batch, args.rounds, args.warmup,
                                  args.default_only)), flush=True)
        return 0
    what = f"flow_bidir_device cold, {LEVELS} levels, {WARPS} warps, both masks"
    variants = {"a": what + ", finest 0", "b": what + ", finest 1", "c": what + ", finest 2",
                "kb": "upflow_bilinear_device (KB), level 1 -> level 0"}
    out = {"shapes": {k: f"{c}x{r}" for k, (r, c) in SHAPES.items()}, "window": WINDOW,
           "iters_per_warp": ITERS, "median": MEDIAN, "alpha": ALPHA, "rounds": args.rounds,
           "timing": "device events around each variant; median, min and max over the rounds, "
                     f"variants alternated inside every round; KB: {REPS} launches between the "
                     "events, time per launch",
           "variants": variants, "cases": {}}
    cases = [(s, b) for s in SHAPES for b in (1, 8)]
    for shape, batch in cases:
        res = _child(shape, batch, args)
        if res is None:
            return 1
        out["cases"][f"{shape} x {batch}"] = res
        print(json.dumps({"shape": shape, "batch": batch, **res}), flush=True)
    if args.ab:
        ab = {"other": os.path.basename(args.ab), "order": "this, other, this, other", "cases": {}}
        for shape, batch in cases:
            runs = {"this": [], "other": []}
            for who in ("this", "other", "this", "other"):
                res = _child(shape, batch, args, lib=args.ab if who == "other" else "")
                if res is None:
                    return 1
                runs[who].append(res["a"])
            med = {w: [r["median_ms"] for r in rs] for w, rs in runs.items()}
            ab["cases"][f"{shape} x {batch}"] = {
                "a_median_ms": med,
                "this_over_other": round(sum(med["this"]) / sum(med["other"]), 4),
                "run_to_run_pct": {w: round(100.0 * abs(m[0] - m[1]) / min(m), 2)
                                   for w, m in med.items()},
                "in_round_spread_pct": {w: [r["spread_pct"] for r in rs]
                                        for w, rs in runs.items()}}
            print(json.dumps({"ab": f"{shape} x {batch}", **ab["cases"][f"{shape} x {batch}"]}),
                  flush=True)
        out["default_path_ab"] = ab
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
    ap.add_argument("--shape", default="1080p", choices=sorted(SHAPES), help="(child)")
    ap.add_argument("--batch", type=int, default=0, help="one case, result to stdout (child)")
    ap.add_argument("--default-only", action="store_true", help="(a) alone (child of --ab)")
    ap.add_argument("--ab", default="", help="another build of libhsflow.so to time (a) against")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "finest_timing.json"))
    sys.exit(main(ap.parse_args()))
