"""Cost of the brightness-robust prefilter (KN, hs_prefilter_kernel) alone and in
front of the bidirectional solve, 1080p, batch 1 and 8:

  (kn_<in>_m<mode>_s<sigma>)  prefilter_device alone: u8 and f32 input, modes 1
        (high-pass) and 2 (normalise), sigma 1.7 (r = 6) and 4 (r = 12)
  (kw)  warp_gradients_device alone          the byte-rate yardsticks KN is
  (kr)  warp_image_device alone              compared with
  (km)  median_device alone, 5 x 5           (KW + KM: one warp's own kernels)
  (a)   flow_bidir_device, 100 it, 3 levels, 2 warps, median 5, alpha 100
  (b)   the same with prefilter=Prefilter(2, 4, 4, 32)

Device events around each variant, a warm-up of all, the variants alternated
inside every round of one process.  The kernels alone run REPS launches back
to back between their events, so the figure per launch holds little of the
events' own cost.  Achieved bytes per second = algorithmic bytes (below) over
the median time per launch; KN's is also given as a ratio to KW's and KR's of
the same run, with the rounds' min-max.  The fused call's extra time is given
as a percentage of the unfiltered call, next to that call's own spread between
rounds.  No pass/fail number for speed.

Each batch runs in a child process of its own under a time limit; the parent
stops at the first child that fails.

    python scripts/prefilter_timing.py            # -> profiles/prefilter_timing.json
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
PREFILTER = (2, 4.0, 4.0, 32.0)  # mode, sigma, eps, scale of the fused call
SIGMAS = (1.7, 4.0)
REPS = 10  # launches between the events of a kernel timed alone
STEP_LIMIT_S = 240  # one batch: warm-up and 15 rounds take a few seconds
# algorithmic bytes per pixel
B_KW = 4 + 4 + 8 + 12  # I0, I1, (u0, v0) -> gx, gy, gt' (f32 frames)
B_KR = 4 + 8 + 4       # I, (u, v) -> out
B_KM = 8 + 8           # (u, v) -> (u, v)
B_KN = {"u8": 1 + 4, "f32": 4 + 4}  # I -> out


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
    frames = {"u8": I0.to(torch.uint8), "f32": I0 * 0.9 + 0.3}
    S0, S1 = frames["f32"], I1  # the solves' pair: non-integer f32, as interp_timing.py's
    uf, vf, ub, vb, plane, u2, v2 = (torch.empty_like(I0) for _ in range(7))
    mf, mb = (torch.empty(I0.shape, dtype=torch.uint8, device="cuda") for _ in range(2))
    ws = torch.empty(hsflow.bidir_workspace_bytes(ROWS, COLS, batch, LEVELS) +
                     hsflow.prefilter_planes_bytes(ROWS, COLS, batch), dtype=torch.uint8,
                     device="cuda")
    solve = (LEVELS, WARPS, WINDOW, ITERS, ALPHA)
    pf = hsflow.Prefilter(*PREFILTER)

    def bidir(prefilter):
        return lambda: hsflow.flow_bidir_device(S0, S1, *solve, uf=uf, vf=vf, ub=ub, vb=vb,
                                                mask_f=mf, mask_b=mb, workspace=ws, median=MEDIAN,
                                                prefilter=prefilter)

    def kn(kind, mode, sigma):
        p = hsflow.Prefilter(mode, sigma, 1.0, 32.0)

        def f():
            for _ in range(REPS):
                hsflow.prefilter_device(frames[kind], p, out=plane)
        return f

    def kw():
        for _ in range(REPS):
            hsflow.warp_gradients_device(S0, S1, uf, vf, ws)

    def kr():
        for _ in range(REPS):
            hsflow.warp_image_device(S1, uf, vf, out=plane)

    def km():
        for _ in range(REPS):
            hsflow.median_device(uf, vf, MEDIAN, u2, v2)

    variants = {"a": bidir(None), "b": bidir(pf), "kw": kw, "kr": kr, "km": km}
    nbytes = {"kw": B_KW, "kr": B_KR, "km": B_KM}
    for kind in ("u8", "f32"):
        for mode in (1, 2):
            for sigma in SIGMAS:
                name = f"kn_{kind}_m{mode}_s{sigma}"
                variants[name] = kn(kind, mode, sigma)
                nbytes[name] = B_KN[kind]
    bidir(None)()  # the flows the kernels alone read
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
            ms[k].append(e0.elapsed_time(e1) / (REPS if k in nbytes else 1))
    res = {k: {"median_ms": round(float(np.median(t)), 4), "min_ms": round(min(t), 4),
               "max_ms": round(max(t), 4),
               "spread_pct": round(100.0 * (max(t) - min(t)) / float(np.median(t)), 2)}
           for k, t in ms.items()}
    px = ROWS * COLS * batch
    for k, b in nbytes.items():
        r = res[k]
        r["bytes_per_px"] = b
        r["tb_per_s"] = round(b * px / (r["median_ms"] * 1e-3) / 1e12, 3)
        r["tb_per_s_min_max"] = [round(b * px / (r[m] * 1e-3) / 1e12, 3)
                                 for m in ("max_ms", "min_ms")]
    for k in nbytes:
        if not k.startswith("kn_"):
            continue
        for other in ("kw", "kr"):
            res[k][f"rate_over_{other}"] = round(res[k]["tb_per_s"] / res[other]["tb_per_s"], 3)
            res[k][f"rate_over_{other}_min_max"] = [
                round(res[k]["tb_per_s_min_max"][0] / res[other]["tb_per_s_min_max"][1], 3),
                round(res[k]["tb_per_s_min_max"][1] / res[other]["tb_per_s_min_max"][0], 3)]
        # against one warp's own kernels of the same run
        res[k]["time_over_kw_plus_km"] = round(
            res[k]["median_ms"] / (res["kw"]["median_ms"] + res["km"]["median_ms"]), 3)
    extra = res["b"]["median_ms"] - res["a"]["median_ms"]
    res["b_minus_a_ms"] = round(extra, 4)
    res["b_minus_a_pct_of_a"] = round(100.0 * extra / res["a"]["median_ms"], 2)
    res["a_spread_pct"] = res["a"]["spread_pct"]
    return res


def main(args):
    if args.batch:
        print(json.dumps(run_batch(args.batch, args.rounds, args.warmup)), flush=True)
        return 0
    variants = {"a": "flow_bidir_device, median 5, both masks",
                "b": "the same with prefilter (mode 2, sigma 4, eps 4, scale 32)",
                "kw": "warp_gradients_device (KW)", "kr": "warp_image_device (KR)",
                "km": "median_device 5 x 5 (KM)",
                "kn_<in>_m<mode>_s<sigma>": "prefilter_device (KN), eps 1, scale 32"}
    out = {"shape": f"{COLS}x{ROWS}", "window": WINDOW, "iters_per_level": ITERS,
           "levels": LEVELS, "warps": WARPS, "median": MEDIAN, "alpha": ALPHA,
           "prefilter": list(PREFILTER), "rounds": args.rounds,
           "timing": "device events around each variant; median, min and max over the rounds, "
                     f"variants alternated inside every round; kernels alone: {REPS} launches "
                     "between the events, time per launch",
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "prefilter_timing.json"))
    sys.exit(main(ap.parse_args()))
