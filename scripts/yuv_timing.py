"""Cost of the YUV 4:2:0 interpolation ("YUV 4:2:0 frame
interpolation"), uint8 frames out:

  (a) kiy   KIY alone (yuv.chroma_interp_device) against the launches it
            replaces, at 1080p and 4K, batch 1 and 8, nt 1 and 3:
              i420        one launch
              i420_pieces two KD (temporal.downflow_device) and four KI
                          (hsflow.frame_interp_device on the U and V planes)
              nv12, nv12_wide   one launch, a row's two taps as four bytes or as
                          one unaligned dword (yuv.set_nv12_loads)
              nv12_pieces the same six launches plus the copies that take the
                          interleaved planes apart and put the result together
            Achieved bytes per second of KIY against its algorithmic traffic:
            16 B per luma pixel of flows, 2 x 2 B per chroma sample of both
            frames' chroma read per time and 2 B written (b_kiy).
  (b) fused yuv.flow_interp_yuv_device against hsflow.flow_interp_bgr_device on
            the same content and schedule, 1080p, batch 1 and 8, three times,
            flags and trusted out.
  (c) ab    the unchanged grey and BGR fused calls on this build against
            another build of the library (the parent commit's), in child
            processes: other, other first -- the A/A spread of one build --
            then this, other, this, other.

fallback_timing.py's method: device events around each variant, a warm-up of
all, the variants alternated inside every round of one process; the kernels
of (a) run REPS times back to back between their events.  No pass/fail number
for speed.  Every part runs in child processes of its own under a time limit;
the parent process stops at the first child that fails.

    python scripts/yuv_timing.py --ab PARENT_LIBHSFLOW_SO   # -> profiles/yuv_timing.json
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

SIZES = {"1080p": (1080, 1920), "4k": (2160, 3840)}
WINDOW, ITERS, LEVELS, WARPS, ALPHA = 5, 100, 3, 2, 400.0
TIMES = {1: (0.5,), 3: (0.25, 0.5, 0.75)}
REPS = 10  # launches between the events of the kernels timed alone
STEP_LIMIT_S = 300


def b_kiy(nt):
    """Per luma pixel: 16 B of flows once; per time a quarter of (4 B of chroma
    read, 2 B written)."""
    return 16 + nt * (4 + 2) / 4.0


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
                "max_ms": round(max(t), 4)} for k, t in ms.items()}


def _flows(batch, rows, cols):
    """Smooth flows of a few px, the backward one the forward one negated plus a
    little noise (float32 [batch, rows, cols] each)."""
    import torch
    g = torch.Generator(device="cuda").manual_seed(7)
    yy = torch.arange(rows, device="cuda", dtype=torch.float32)[None, :, None]
    xx = torch.arange(cols, device="cuda", dtype=torch.float32)[None, None, :]
    k = torch.arange(batch, device="cuda", dtype=torch.float32)[:, None, None]
    uf = (0.3 * torch.sin(xx / 97.0 + k) + 0.2 * torch.cos(yy / 61.0)).contiguous()
    vf = (0.25 * torch.cos(xx / 83.0) - 0.15 * torch.sin(yy / 45.0 + k)).contiguous()
    n = 0.02 * torch.randn((2, batch, rows, cols), device="cuda", generator=g)
    return uf, vf, (-uf + n[0]).contiguous(), (-vf + n[1]).contiguous()


def run_kiy(size, batch, rounds, warmup):
    import temporal
    import torch
    import yuv
    hsflow = _hsflow(False)
    rows, cols = SIZES[size]
    rc, cc = rows // 2, cols // 2
    flows = _flows(batch, rows, cols)
    g = torch.Generator(device="cuda").manual_seed(3)
    i0, i1 = ((torch.rand((batch, 2, rc, cc), device="cuda", generator=g) * 256).to(torch.uint8)
              for _ in range(2))
    n0, n1 = (c.permute(0, 2, 3, 1).contiguous() for c in (i0, i1))
    down = [torch.empty((batch, rc, cc), device="cuda") for _ in range(4)]
    # the U and V planes of an I420 batch, [B][2][rc][cc], as dense batch planes
    dense = [i0[:, 0].contiguous(), i0[:, 1].contiguous(), i1[:, 0].contiguous(),
             i1[:, 1].contiguous()]
    res = {}
    for nt, times in TIMES.items():
        oi = torch.empty((batch, nt, 2, rc, cc), dtype=torch.uint8, device="cuda")
        on = torch.empty((batch, nt, rc, cc, 2), dtype=torch.uint8, device="cuda")
        op = [torch.empty((batch, nt, rc, cc), dtype=torch.uint8, device="cuda") for _ in range(2)]
        planes = [torch.empty((batch, rc, cc), dtype=torch.uint8, device="cuda") for _ in range(4)]

        def kiy(c0, c1, lay, out, wide=False):
            def f():
                yuv.set_nv12_loads(wide)
                for _ in range(REPS):
                    yuv.chroma_interp_device(c0, c1, *flows, times, lay, out=out)
                yuv.set_nv12_loads(False)
            return f

        def six(src):
            temporal.downflow_device(flows[0], flows[1], uc=down[0], vc=down[1])
            temporal.downflow_device(flows[2], flows[3], uc=down[2], vc=down[3])
            for ch in range(2):
                hsflow.frame_interp_device(src[ch], src[2 + ch], *down, times, out=op[ch])

        def i420_pieces():  # on dense copies of the planes, made once: no copy is timed
            for _ in range(REPS):
                six(dense)

        def nv12_pieces():
            for _ in range(REPS):
                for p, c, ch in ((planes[0], n0, 0), (planes[1], n0, 1), (planes[2], n1, 0),
                                 (planes[3], n1, 1)):
                    p.copy_(c[..., ch])
                six(planes)
                on[..., 0].copy_(op[0])
                on[..., 1].copy_(op[1])

        variants = {"i420": kiy(i0, i1, 1, oi), "i420_pieces": i420_pieces,
                    "nv12": kiy(n0, n1, 2, on), "nv12_wide": kiy(n0, n1, 2, on, True),
                    "nv12_pieces": nv12_pieces}
        alone = set(variants)
        r = _time(variants, alone, rounds, warmup)
        px = rows * cols * batch
        for k in ("i420", "nv12", "nv12_wide"):
            r[k]["us"] = round(r[k]["median_ms"] * 1e3, 2)
            r[k]["tb_per_s"] = round(b_kiy(nt) * px / (r[k]["median_ms"] * 1e-3) / 1e12, 3)
        r["bytes_per_luma_px"] = b_kiy(nt)
        r["i420_pieces_over_kiy"] = round(r["i420_pieces"]["median_ms"] / r["i420"]["median_ms"], 3)
        r["nv12_pieces_over_kiy"] = round(r["nv12_pieces"]["median_ms"] / r["nv12"]["median_ms"], 3)
        res[f"nt{nt}"] = r
    return res


def _content(hsflow, batch, rows, cols):
    """(y0, y1) uint8 [batch, rows, cols]: textured pairs under a small shift."""
    import numpy as np
    import torch
    a = [hsflow.synth_pair(3000 + k, rows, cols) for k in range(batch)]
    return tuple(torch.from_numpy(np.stack([p[j] for p in a]).astype(np.uint8)).cuda()
                 for j in range(2))


def run_fused(batch, rounds, warmup, other):
    """The fused calls at 1080p.  other: the grey and the BGR call alone, on
    whatever build HSFLOW_LIB names."""
    import torch
    hsflow = _hsflow(other)
    rows, cols = SIZES["1080p"]
    times = TIMES[3]
    y0, y1 = _content(hsflow, batch, rows, cols)
    b0, b1 = (torch.stack([y, 255 - y, y.flip(2)], dim=-1).contiguous() for y in (y0, y1))
    args = (LEVELS, WARPS, WINDOW, ITERS, ALPHA)
    ws = torch.empty(hsflow.flow_interp_bgr_workspace_bytes(rows, cols, batch, LEVELS) + 4096,
                     dtype=torch.uint8, device="cuda")
    og = torch.empty((batch, 3, rows, cols), dtype=torch.uint8, device="cuda")
    ob = torch.empty((batch, 3, rows, cols, 3), dtype=torch.uint8, device="cuda")
    flags = torch.empty((batch, 3, rows, cols), dtype=torch.uint8, device="cuda")
    trusted = torch.empty((batch, 3), dtype=torch.int32, device="cuda")
    variants = {
        "grey": lambda: hsflow.flow_interp_device(y0, y1, times, *args, out=og, flags=flags,
                                                  trusted=trusted, workspace=ws),
        "bgr": lambda: hsflow.flow_interp_bgr_device(b0, b1, times, *args, out=ob, flags=flags,
                                                     trusted=trusted, workspace=ws)}
    if not other:
        import yuv
        c0, c1 = (b[:, :rows // 2, :cols // 2, :2].contiguous() for b in (b0, b1))  # NV12 chroma
        oc = torch.empty((batch, 3, rows // 2, cols // 2, 2), dtype=torch.uint8, device="cuda")
        variants["yuv_nv12"] = lambda: yuv.flow_interp_yuv_device(
            y0, c0, y1, c1, times, *args, layout=2, out_y=og, out_c=oc, flags=flags,
            trusted=trusted, workspace=ws)
        i0, i1 = (c.permute(0, 3, 1, 2).contiguous() for c in (c0, c1))
        oi = torch.empty((batch, 3, 2, rows // 2, cols // 2), dtype=torch.uint8, device="cuda")
        variants["yuv_i420"] = lambda: yuv.flow_interp_yuv_device(
            y0, i0, y1, i1, times, *args, layout=1, out_y=og, out_c=oi, flags=flags,
            trusted=trusted, workspace=ws)
    r = _time(variants, set(), rounds, warmup)
    if not other:
        for k in ("yuv_nv12", "yuv_i420"):
            r[k + "_over_bgr"] = round(r[k]["median_ms"] / r["bgr"]["median_ms"], 4)
            r[k + "_minus_grey_ms"] = round(r[k]["median_ms"] - r["grey"]["median_ms"], 4)
    return r


def _child(args, part, *what, lib=None):
    """One part in a fresh process under its own time limit -> its result."""
    env = dict(os.environ)
    cmd = [sys.executable, os.path.abspath(__file__), "--part", part, "--what", *map(str, what),
           "--rounds", str(args.rounds), "--warmup", str(args.warmup)]
    if lib:
        cmd.append("--other")
        env["HSFLOW_LIB"] = os.path.abspath(lib)
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=STEP_LIMIT_S, env=env)
    if p.returncode != 0:
        sys.stderr.write(p.stdout + p.stderr)
        return None
    return json.loads(p.stdout.strip().splitlines()[-1])


def main(args):
    if args.part == "kiy":
        print(json.dumps(run_kiy(args.what[0], int(args.what[1]), args.rounds, args.warmup)),
              flush=True)
        return 0
    if args.part == "fused":
        print(json.dumps(run_fused(int(args.what[0]), args.rounds, args.warmup, args.other)),
              flush=True)
        return 0
    out = {"window": WINDOW, "iters_per_level": ITERS, "levels": LEVELS, "warps": WARPS,
           "alpha": ALPHA, "rounds": args.rounds, "times": {str(k): list(v) for k, v in TIMES.items()},
           "timing": "device events around each variant; median, min and max over the rounds, "
                     f"variants alternated inside every round; (a): {REPS} runs between the "
                     "events, time per run",
           "kiy": {}, "fused": {}}
    for size in SIZES:
        for batch in (1, 8):
            res = _child(args, "kiy", size, batch)
            if res is None:
                return 1
            out["kiy"][f"{size}_b{batch}"] = res
            print(json.dumps({"kiy": size, "batch": batch, **res}), flush=True)
    for batch in (1, 8):
        runs = {"this": [], "aa": [], "other": []}
        order = ("aa", "aa", "this", "other", "this", "other") if args.ab else ("this",)
        for who in order:
            res = _child(args, "fused", batch, lib=None if who == "this" else args.ab)
            if res is None:
                return 1
            runs[who].append(res)
            print(json.dumps({"fused": batch, "run": who, **res}), flush=True)
        entry = dict(runs)
        if args.ab:
            summary = {"other": os.path.basename(os.path.dirname(os.path.abspath(args.ab))) + "/" +
                       os.path.basename(args.ab),
                       "order": "other, other (A/A), this, other, this, other"}
            for k in ("grey", "bgr"):
                aa = [r[k]["median_ms"] for r in runs["aa"]]
                this = [r[k]["median_ms"] for r in runs["this"]]
                other = [r[k]["median_ms"] for r in runs["other"]]
                summary[k] = {"aa_run_to_run_pct": round(100.0 * abs(aa[0] - aa[1]) / min(aa), 2),
                              "this_median_ms": this, "other_median_ms": other,
                              "this_over_other": round(sum(this) / sum(other), 4)}
            entry["ab"] = summary
            print(json.dumps({"fused": batch, "ab": summary}), flush=True)
        out["fused"][f"1080p_b{batch}"] = entry
    if args.out:
        os.makedirs(os.path.dirname(args.out), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")
    return 0


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--part", default="", help="kiy or fused: one part, result to stdout (child)")
    ap.add_argument("--what", nargs="*", default=[], help="the part's size and batch (child)")
    ap.add_argument("--other", action="store_true", help="grey and bgr alone (child of --ab)")
    ap.add_argument("--ab", default="", help="another build of libhsflow.so for part (c)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "yuv_timing.json"))
    sys.exit(main(ap.parse_args()))
