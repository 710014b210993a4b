"""Cost of the fallback for a failed pair next to the fused call it follows:
1080p BGR frames, uint8 frames out with flags and trusted, w 5, 100 it per
level, 3 levels, 2 warps, three times, batch 1 and 8:

  pj       hsflow_flow_interp_bgr_pj_device, projection 0: on this build the
           fallback-off path (the *_fb_ call with a null setting)
  on_pass  hsflow_flow_interp_bgr_fb_device, NEAREST, related pairs: both counts,
           then one launch of KF whose blocks leave at once
  on_fail  the same on unrelated pairs with min_share = 1: KF rewrites every
           frame
  kf_pass, kf_fail   fallback.frame_fallback_bgr_device alone on those counts

The timed schedule is projection_timing.py's (alpha 400, no median), under
which the unrelated 1080p pairs keep a share of consistent pixels above the
default threshold -- both flows stay near zero, and two zero flows agree -- so
the failing case is forced with min_share = 1 (the related pairs' share is
exactly 1, which passes any threshold).  `consistent_share` records the shares
of the timed schedule, `consistent_share_alpha100_median5` those of the
schedule the fallback is meant for.

projection_timing.py's method: device events around each variant, a warm-up of
all, the variants alternated inside every round of one process; KF alone runs
REPS launches back to back between its events.  Achieved bytes per second of
kf_fail = algorithmic bytes (b_kf) over the median time per launch.  No
pass/fail number for speed.

Each batch runs in a child process of its own under a time limit; the parent
process stops at the first child that fails.

    python scripts/fallback_timing.py --ab PARENT_LIBHSFLOW_SO
                                               # -> profiles/fallback_timing.json

--ab: `pj` alone on another build of the library (the parent commit's), in
child processes: other, other first -- the A/A spread of one build -- then
this, other, this, other.  The three ratios off / on_pass / on_fail are this
build's medians over the other build's `pj`.
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

ROWS, COLS, WINDOW, ITERS, LEVELS, WARPS, ALPHA = 1080, 1920, 5, 100, 3, 2, 400.0
TIMES = (0.25, 0.5, 0.75)
REPS = 10  # launches between the events of KF timed alone
STEP_LIMIT_S = 300


def b_kf(nt):
    """Two BGR pixels read once; per time one BGR pixel and one flag byte written."""
    return 6 + nt * (3 + 1)


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


def _bgr(grey):
    import numpy as np
    return np.ascontiguousarray(np.stack([grey, 255 - grey, grey[:, ::-1]], axis=-1))


def _clips(hsflow, batch):
    """(bgr0, related bgr1, unrelated bgr1) uint8 [batch, rows, cols, 3] on the device."""
    import numpy as np
    import torch
    a = [hsflow.synth_pair(3000 + k, ROWS, COLS) for k in range(batch)]
    b = [hsflow.synth_pair(7000 + k, ROWS, COLS) for k in range(batch)]
    g0 = np.stack([p[0] for p in a]).astype(np.uint8)
    g1 = np.stack([p[1] for p in a]).astype(np.uint8)
    gx = np.stack([p[0] for p in b]).astype(np.uint8)
    return tuple(torch.from_numpy(_bgr(g)).cuda() for g in (g0, g1, gx))


def _fused(hsflow, name, b0, b1, out, flags, trusted, ws, extra_out=(), extra_in=()):
    """One fused C call on the current stream: `name` is the *_pj_ or the *_fb_
    entry point (extra_out: cut; extra_in: the setting)."""
    import torch
    tm = hsflow._times_array(TIMES)
    batch = b0.shape[0]

    def call():
        rc = getattr(hsflow.lib(), name)(
            b0.data_ptr(), b1.data_ptr(), ROWS, COLS, batch, LEVELS, 0, WARPS, 0, WINDOW, ITERS,
            ALPHA, hsflow.CONSISTENCY_REL, hsflow.CONSISTENCY_ABS, tm, len(TIMES), 0,
            out.data_ptr(), hsflow.U8, flags.data_ptr(), trusted.data_ptr(), *extra_out, None,
            None, None, *extra_in, ws.data_ptr(), ws.numel(),
            torch.cuda.current_stream().cuda_stream)
        if rc:
            raise RuntimeError(f"{name}: {rc} {hsflow.lib().hsflow_last_error(None).decode()}")
    return call


def _shares(cf, cb):
    return [round((int(a[0]) + int(b[0])) / (2.0 * ROWS * COLS), 4)
            for a, b in zip(cf.tolist(), cb.tolist())]


def _time(variants, alone, rounds, warmup):
    import numpy as np
    import torch
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
            ms[k].append(e0.elapsed_time(e1) / (REPS if k in alone else 1))
    return {k: {"median_ms": round(float(np.median(t)), 4), "min_ms": round(min(t), 4),
                "max_ms": round(max(t), 4),
                "spread_pct": round(100.0 * (max(t) - min(t)) / float(np.median(t)), 2)}
            for k, t in ms.items()}


def run_batch(batch, rounds, warmup, pj_only):
    import torch
    hsflow = _hsflow(pj_only)
    b0, b1, bx = _clips(hsflow, batch)
    nt = len(TIMES)
    out = torch.empty((batch, nt, ROWS, COLS, 3), dtype=torch.uint8, device="cuda")
    flags = torch.empty((batch, nt, ROWS, COLS), dtype=torch.uint8, device="cuda")
    trusted = torch.empty((batch, nt), dtype=torch.int32, device="cuda")
    ws = torch.empty(hsflow.flow_interp_bgr_workspace_bytes(ROWS, COLS, batch, LEVELS) + 4096,
                     dtype=torch.uint8, device="cuda")
    pj = "hsflow_flow_interp_bgr_pj_device"
    variants = {"pj": _fused(hsflow, pj, b0, b1, out, flags, trusted, ws)}
    if pj_only:
        return _time(variants, set(), rounds, warmup)
    import fallback
    settings = {"pass": fallback.Fallback(fallback.FALLBACK_NEAREST),
                "fail": fallback.Fallback(fallback.FALLBACK_NEAREST, 1.0)}
    c = {k: hsflow._CFallback(*v) for k, v in settings.items()}
    cut = torch.empty((batch,), dtype=torch.uint8, device="cuda")
    fbn = "hsflow_flow_interp_bgr_fb_device"
    for name, other in (("pass", b1), ("fail", bx)):
        variants["on_" + name] = _fused(hsflow, fbn, b0, other, out, flags, trusted, ws,
                                        extra_out=(cut.data_ptr(),),
                                        extra_in=(ctypes.byref(c[name]),))
    verdicts, counts, meant = {}, {}, {}
    for name, other in (("pass", b1), ("fail", bx)):
        variants["on_" + name]()
        torch.cuda.synchronize()
        verdicts[name] = cut.tolist()
        g0, g1 = hsflow.bgr_to_gray_device(b0), hsflow.bgr_to_gray_device(other)
        r = hsflow.flow_bidir_device(g0, g1, LEVELS, WARPS, WINDOW, ITERS, ALPHA, mask_f=None,
                                     counts_f=True, counts_b=True)
        counts[name] = (r.counts_f, r.counts_b)
        r = hsflow.flow_bidir_device(g0, g1, LEVELS, WARPS, WINDOW, ITERS, 100.0, mask_f=None,
                                     counts_f=True, counts_b=True, median=5)
        meant[name] = _shares(r.counts_f, r.counts_b)
        del g0, g1, r
    if verdicts != {"pass": [0] * batch, "fail": [1] * batch}:
        raise RuntimeError(f"the timed cases are not what they are called: {verdicts}")

    def kf(name, other):
        cf, cb = counts[name]

        def f():
            for _ in range(REPS):
                fallback.frame_fallback_bgr_device(b0, other, cf, cb, settings[name], TIMES, out,
                                                   flags=flags, trusted=trusted, cut=cut)
        return f

    variants["kf_pass"], variants["kf_fail"] = kf("pass", b1), kf("fail", bx)
    res = _time(variants, {"kf_pass", "kf_fail"}, rounds, warmup)
    px = ROWS * COLS * batch
    res["verdicts"] = verdicts
    res["min_share"] = {k: v.min_share for k, v in settings.items()}
    res["consistent_share"] = {k: _shares(*v) for k, v in counts.items()}
    res["consistent_share_alpha100_median5"] = meant
    r = res["kf_fail"]
    r["bytes_per_px"] = b_kf(nt)
    r["tb_per_s"] = round(b_kf(nt) * px / (r["median_ms"] * 1e-3) / 1e12, 3)
    for k in ("kf_pass", "kf_fail"):
        res[k]["us"] = round(res[k]["median_ms"] * 1e3, 2)
    for k in ("on_pass", "on_fail"):
        res[k + "_over_pj"] = round(res[k]["median_ms"] / res["pj"]["median_ms"], 4)
        res[k + "_minus_pj_ms"] = round(res[k]["median_ms"] - res["pj"]["median_ms"], 4)
    return res


def _child(batch, args, lib=None):
    """One batch in a fresh process under its own time limit -> its result;
    lib: a path: `pj` alone on that build of the library."""
    env = dict(os.environ)
    cmd = [sys.executable, os.path.abspath(__file__), "--batch", str(batch), "--rounds",
           str(args.rounds), "--warmup", str(args.warmup)]
    if lib:
        cmd.append("--pj-only")
        env["HSFLOW_LIB"] = os.path.abspath(lib)
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=STEP_LIMIT_S, env=env)
    if p.returncode != 0:
        sys.stderr.write(p.stdout + p.stderr)
        return None
    return json.loads(p.stdout.strip().splitlines()[-1])


def main(args):
    if args.batch:
        print(json.dumps(run_batch(args.batch, args.rounds, args.warmup, args.pj_only)),
              flush=True)
        return 0
    out = {"shape": f"{COLS}x{ROWS} BGR, uint8 out", "window": WINDOW, "iters_per_level": ITERS,
           "levels": LEVELS, "warps": WARPS, "alpha": ALPHA, "rounds": args.rounds,
           "times": list(TIMES),
           "timing": "device events around each variant; median, min and max over the rounds, "
                     f"variants alternated inside every round; KF alone: {REPS} launches "
                     "between the events, time per launch",
           "batches": {}}
    for batch in (1, 8):
        if not args.ab:
            res = _child(batch, args)
            if res is None:
                return 1
            out["batches"][str(batch)] = {"this": [res]}
            print(json.dumps({"batch": batch, **res}), flush=True)
            continue
        runs = {"aa": [], "this": [], "other": []}
        for who in ("aa", "aa", "this", "other", "this", "other"):
            res = _child(batch, args, lib=None if who == "this" else args.ab)
            if res is None:
                return 1
            runs[who].append(res)
            print(json.dumps({"batch": batch, "run": who, **res}), flush=True)
        aa = [r["pj"]["median_ms"] for r in runs["aa"]]
        other = sum(r["pj"]["median_ms"] for r in runs["other"]) / 2
        summary = {"other": os.path.basename(args.ab),
                   "order": "other, other (A/A), this, other, this, other",
                   "aa_run_to_run_pct": round(100.0 * abs(aa[0] - aa[1]) / min(aa), 2),
                   "other_pj_median_ms": [r["pj"]["median_ms"] for r in runs["other"]]}
        for k, name in (("pj", "off"), ("on_pass", "on_pass"), ("on_fail", "on_fail")):
            this = [r[k]["median_ms"] for r in runs["this"]]
            summary[name + "_median_ms"] = this
            summary[name + "_over_parent_pj"] = round(sum(this) / 2 / other, 4)
        out["batches"][str(batch)] = {"ab": summary, **runs}
        print(json.dumps({"batch": batch, "ab": summary}), flush=True)
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
    ap.add_argument("--pj-only", action="store_true", help="`pj` alone (child of --ab)")
    ap.add_argument("--ab", default="", help="another build of libhsflow.so to time `pj` on")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fallback_timing.json"))
    sys.exit(main(ap.parse_args()))
