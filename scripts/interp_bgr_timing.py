"""Cost of the colour frame interpolation (KIC, hsflow_interp_bgr.hip) next to
the route a caller had before it, 1080p 8-bit BGR pair, batch 1 and 8, nt 1 and
3, u8 output:

  (a1, a3)   frame_interp_bgr_device alone (KIC: masks in; frames, flags,
             trusted out), the wide tap loads (set_interp_bgr_loads(True))
  (ab1, ab3) the same with single-byte tap loads (the default)
  (b1, b3)   three frame_interp_device launches (KI) on the pre-split u8
             channel planes, u8 output, flags and trusted from each; the split
             and the re-interleave are left out, which favours (b)
  (c1, c3)   flow_interp_bgr_device (grey conversion, bidirectional solve, KIC)
  (g1, g3)   flow_interp_device on the grey frames of the same pair

Device events around each variant, a warm-up of all, the variants alternated
inside every round of one process; the kernels alone run REPS launches back to
back between their events.  Median and min-max of the rounds.  (a) and (ab) are
compared with (b) against the min-max spread of (b)'s own rounds, not a fixed
ratio; no pass/fail number for speed.

Each batch runs in a child process of its own under a time limit; the parent
stops at the first child that fails.

    python scripts/interp_bgr_timing.py        # -> profiles/interp_bgr_timing.json
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
STEP_LIMIT_S = 240


def b_kic(nt):
    """16 B of flows once; per time 6 B of u8 BGR frames and 2 B of masks in,
    3 B of frame and 1 B of flags out."""
    return 16 + nt * (6 + 2 + 3 + 1)


def b_ki3(nt):
    """Three KI launches on u8 planes: each 16 B of flows and per time 2 B of
    frames and 2 B of masks in, 1 B of frame and 1 B of flags out."""
    return 3 * (16 + nt * (2 + 2 + 1 + 1))


def _pairs(hsflow, batch):
    import numpy as np
    import torch
    frames = [[], []]
    for k in range(batch):
        chans = [hsflow.synth_pair(3000 + 100 * c + k, ROWS, COLS) for c in range(3)]
        for j in range(2):
            frames[j].append(np.stack([ch[j] for ch in chans], axis=-1).astype(np.uint8))
    return tuple(torch.from_numpy(np.stack(f)).cuda() for f in frames)


def run_batch(batch, rounds, warmup):
    import numpy as np
    import torch
    import hsflow

    B0, B1 = _pairs(hsflow, batch)
    G0, G1 = hsflow.bgr_to_gray_device(B0), hsflow.bgr_to_gray_device(B1)
    P0 = [B0[..., c].contiguous() for c in range(3)]
    P1 = [B1[..., c].contiguous() for c in range(3)]
    solve = (LEVELS, WARPS, WINDOW, ITERS, ALPHA)
    r = hsflow.flow_bidir_device(G0, G1, *solve, mask_f=True, mask_b=True)
    flows, mf, mb = (r.uf, r.vf, r.ub, r.vb), r.mask_f, r.mask_b
    u8 = torch.uint8
    out = {nt: torch.empty((batch, nt, ROWS, COLS, 3), dtype=u8, device="cuda") for nt in TIMES}
    outp = {nt: [torch.empty((batch, nt, ROWS, COLS), dtype=u8, device="cuda") for _ in range(3)]
            for nt in TIMES}
    flags = {nt: torch.empty((batch, nt, ROWS, COLS), dtype=u8, device="cuda") for nt in TIMES}
    trusted = {nt: torch.empty((batch, nt), dtype=torch.int32, device="cuda") for nt in TIMES}
    ws = torch.empty(hsflow.flow_interp_bgr_workspace_bytes(ROWS, COLS, batch, LEVELS), dtype=u8,
                     device="cuda")

    def kic(nt, wide):
        def f():
            was = hsflow.set_interp_bgr_loads(wide)
            for _ in range(REPS):
                hsflow.frame_interp_bgr_device(B0, B1, *flows, TIMES[nt], mask_f=mf, mask_b=mb,
                                               out=out[nt], flags=flags[nt], trusted=trusted[nt])
            hsflow.set_interp_bgr_loads(was)
        return f

    def ki3(nt):
        def f():
            for _ in range(REPS):
                for c in range(3):
                    hsflow.frame_interp_device(P0[c], P1[c], *flows, TIMES[nt], mask_f=mf,
                                               mask_b=mb, out=outp[nt][c], flags=flags[nt],
                                               trusted=trusted[nt])
        return f

    def fused_bgr(nt):
        return lambda: hsflow.flow_interp_bgr_device(B0, B1, TIMES[nt], *solve, out=out[nt],
                                                     flags=flags[nt], trusted=trusted[nt],
                                                     workspace=ws)

    def fused_grey(nt):
        return lambda: hsflow.flow_interp_device(G0, G1, TIMES[nt], *solve, out=outp[nt][0],
                                                 flags=flags[nt], trusted=trusted[nt],
                                                 workspace=ws)

    variants = {}
    for nt in TIMES:
        variants[f"a{nt}"] = kic(nt, True)
        variants[f"ab{nt}"] = kic(nt, False)
        variants[f"b{nt}"] = ki3(nt)
        variants[f"c{nt}"] = fused_bgr(nt)
        variants[f"g{nt}"] = fused_grey(nt)
    per_launch = {k: REPS for k in variants if k[0] in "ab"}
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
    for nt in TIMES:
        for k, b in ((f"a{nt}", b_kic(nt)), (f"ab{nt}", b_kic(nt)), (f"b{nt}", b_ki3(nt))):
            res[k]["bytes_per_px"] = b
            res[k]["tb_per_s"] = round(b * px / (res[k]["median_ms"] * 1e-3) / 1e12, 3)
        a, ab, b = res[f"a{nt}"], res[f"ab{nt}"], res[f"b{nt}"]
        res[f"a{nt}_over_b{nt}"] = round(a["median_ms"] / b["median_ms"], 3)
        res[f"ab{nt}_over_b{nt}"] = round(ab["median_ms"] / b["median_ms"], 3)
        res[f"a{nt}_over_ab{nt}"] = round(a["median_ms"] / ab["median_ms"], 3)
        # (a), (ab) are no slower than (b) beyond (b)'s own spread
        res[f"a{nt}_within_b{nt}_spread"] = bool(a["median_ms"] <= b["max_ms"])
        res[f"ab{nt}_within_b{nt}_spread"] = bool(ab["median_ms"] <= b["max_ms"])
        res[f"c{nt}_minus_g{nt}_ms"] = round(res[f"c{nt}"]["median_ms"] -
                                             res[f"g{nt}"]["median_ms"], 4)
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
                     "(b: 3 x that) between the events, time per launch (b: per three)",
           "variants": {"a": "frame_interp_bgr_device (KIC), wide tap loads, u8 out",
                        "ab": "frame_interp_bgr_device (KIC), single-byte tap loads, u8 out",
                        "b": "3 x frame_interp_device (KI) on pre-split u8 planes, u8 out",
                        "c": "flow_interp_bgr_device (frames, flags, trusted)",
                        "g": "flow_interp_device on the grey frames, u8 out"},
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "interp_bgr_timing.json"))
    sys.exit(main(ap.parse_args()))
