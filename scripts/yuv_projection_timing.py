"""Cost of the projected YUV 4:2:0 interpolation ("YUV 4:2:0 with
projection"), uint8 frames out; yuv_timing.py's method and helpers:

  (a) kiyp  KIYP alone (yuv.chroma_interp_proj_device) against KIY and against
            the launches it replaces, at 1080p and 4K, batch 1 and 8, nt 1 and 3:
              i420_kiy, nv12_kiy   KIY, the unprojected kernel
              i420, nv12           KIYP, one launch
              i420_pieces  two KD (temporal.downflow_device), KSD
                           (yuv.cells_down_device) and KIP
                           (projection.frame_interp_device) on the U and on the
                           V planes
              nv12_pieces  the same plus the copies that take the interleaved
                           planes apart and put the result together
            Achieved bytes per second of KIYP against its algorithmic traffic,
            per chroma sample and time: 32 B of cells, 32 B of gathered flows,
            4 B of chroma read and 2 B written (b_kiyp).
  (b) fused yuv.flow_interp_yuv_proj_device with projection 1 against
            projection 0 and against hsflow.flow_interp_bgr_device(projection=1)
            on the same luma content and schedule, 1080p, batch 1 and 8, three
            times, flags and trusted out.
  (c) ab    the unchanged fused calls -- unprojected YUV, grey and BGR -- on
            this build against another build of the library (the parent
            commit's), in child processes: other, other first -- the A/A spread
            of one build -- then this, other, this, other.

No pass/fail number for speed.  Every part runs in child processes of its own
under a time limit; the parent process stops at the first child that fails.

    python scripts/yuv_projection_timing.py --ab PARENT_LIBHSFLOW_SO
        # -> profiles/yuv_projection_timing.json
"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "cpp-optical-flow_amd"))
sys.path.insert(0, os.path.join(ROOT, "scripts"))

from yuv_timing import (ALPHA, ITERS, LEVELS, REPS, SIZES, STEP_LIMIT_S, TIMES, WARPS,  # noqa: E402
                        WINDOW, _content, _flows, _hsflow, _time)


def b_kiyp(nt):
    """Per luma pixel and time, a quarter of a chroma sample's 32 B of cells,
    32 B of gathered flows, 4 B of chroma read and 2 B written."""
    return nt * (32 + 32 + 4 + 2) / 4.0


def run_kiyp(size, batch, rounds, warmup):
    import projection
    import temporal
    import torch
    import yuv
    _hsflow(False)
    rows, cols = SIZES[size]
    rc, cc = rows // 2, cols // 2
    flows = _flows(batch, rows, cols)
    g = torch.Generator(device="cuda").manual_seed(3)
    y0, y1 = ((torch.rand((batch, rows, cols), device="cuda", generator=g) * 256).to(torch.uint8)
              for _ in range(2))
    i0, i1 = ((torch.rand((batch, 2, rc, cc), device="cuda", generator=g) * 256).to(torch.uint8)
              for _ in range(2))
    n0, n1 = (c.permute(0, 2, 3, 1).contiguous() for c in (i0, i1))
    down = [torch.empty((batch, rc, cc), device="cuda") for _ in range(4)]
    dense = [i0[:, 0].contiguous(), i0[:, 1].contiguous(), i1[:, 0].contiguous(),
             i1[:, 1].contiguous()]
    res = {}
    for nt, times in TIMES.items():
        cells = projection.project_device(y0, y1, *flows, times)
        cells_c = torch.empty((batch, nt, rc, cc), dtype=torch.int64, device="cuda")
        oi = torch.empty((batch, nt, 2, rc, cc), dtype=torch.uint8, device="cuda")
        on = torch.empty((batch, nt, rc, cc, 2), dtype=torch.uint8, device="cuda")
        op = [torch.empty((batch, nt, rc, cc), dtype=torch.uint8, device="cuda") for _ in range(2)]
        planes = [torch.empty((batch, rc, cc), dtype=torch.uint8, device="cuda") for _ in range(4)]

        def kiy(c0, c1, lay, out):
            def f():
                for _ in range(REPS):
                    yuv.chroma_interp_device(c0, c1, *flows, times, lay, out=out)
            return f

        def kiyp(c0, c1, lay, out):
            def f():
                for _ in range(REPS):
                    yuv.chroma_interp_proj_device(c0, c1, *flows, times, cells, lay, out=out)
            return f

        def pieces(src):
            temporal.downflow_device(flows[0], flows[1], uc=down[0], vc=down[1])
            temporal.downflow_device(flows[2], flows[3], uc=down[2], vc=down[3])
            yuv.cells_down_device(cells, cells_c)
            for ch in range(2):
                projection.frame_interp_device(src[ch], src[2 + ch], *down, times, cells_c,
                                               out=op[ch])

        def i420_pieces():  # on dense copies of the planes, made once: no copy is timed
            for _ in range(REPS):
                pieces(dense)

        def nv12_pieces():
            for _ in range(REPS):
                for p, c, ch in ((planes[0], n0, 0), (planes[1], n0, 1), (planes[2], n1, 0),
                                 (planes[3], n1, 1)):
                    p.copy_(c[..., ch])
                pieces(planes)
                on[..., 0].copy_(op[0])
                on[..., 1].copy_(op[1])

        variants = {"i420_kiy": kiy(i0, i1, 1, oi), "i420": kiyp(i0, i1, 1, oi),
                    "i420_pieces": i420_pieces, "nv12_kiy": kiy(n0, n1, 2, on),
                    "nv12": kiyp(n0, n1, 2, on), "nv12_pieces": nv12_pieces}
        r = _time(variants, set(variants), rounds, warmup)
        px = rows * cols * batch
        for k in ("i420", "nv12"):
            r[k]["us"] = round(r[k]["median_ms"] * 1e3, 2)
            r[k]["tb_per_s"] = round(b_kiyp(nt) * px / (r[k]["median_ms"] * 1e-3) / 1e12, 3)
            r[k + "_pieces_over_kiyp"] = round(r[k + "_pieces"]["median_ms"] / r[k]["median_ms"], 3)
            r[k + "_kiyp_over_kiy"] = round(r[k]["median_ms"] / r[k + "_kiy"]["median_ms"], 3)
        r["bytes_per_luma_px"] = b_kiyp(nt)
        res[f"nt{nt}"] = r
    return res


def run_fused(batch, rounds, warmup, other):
    """The fused calls at 1080p.  other: the unchanged paths alone -- the
    unprojected YUV, the grey and the BGR call -- on whatever build HSFLOW_LIB
    names."""
    import torch
    hsflow = _hsflow(other)
    import yuv
    rows, cols = SIZES["1080p"]
    times = TIMES[3]
    y0, y1 = _content(hsflow, batch, rows, cols)
    b0, b1 = (torch.stack([y, 255 - y, y.flip(2)], dim=-1).contiguous() for y in (y0, y1))
    args = (LEVELS, WARPS, WINDOW, ITERS, ALPHA)
    import projection
    ws = torch.empty(projection.flow_interp_bgr_workspace_bytes(rows, cols, batch, LEVELS, 3) + 4096,
                     dtype=torch.uint8, device="cuda")
    og = torch.empty((batch, 3, rows, cols), dtype=torch.uint8, device="cuda")
    ob = torch.empty((batch, 3, rows, cols, 3), dtype=torch.uint8, device="cuda")
    flags = torch.empty((batch, 3, rows, cols), dtype=torch.uint8, device="cuda")
    trusted = torch.empty((batch, 3), dtype=torch.int32, device="cuda")
    c0, c1 = (b[:, :rows // 2, :cols // 2, :2].contiguous() for b in (b0, b1))  # NV12 chroma
    oc = torch.empty((batch, 3, rows // 2, cols // 2, 2), dtype=torch.uint8, device="cuda")
    variants = {
        "grey": lambda: hsflow.flow_interp_device(y0, y1, times, *args, out=og, flags=flags,
                                                  trusted=trusted, workspace=ws),
        "bgr": lambda: hsflow.flow_interp_bgr_device(b0, b1, times, *args, out=ob, flags=flags,
                                                     trusted=trusted, workspace=ws),
        "yuv_nv12": lambda: yuv.flow_interp_yuv_device(
            y0, c0, y1, c1, times, *args, layout=2, out_y=og, out_c=oc, flags=flags,
            trusted=trusted, workspace=ws)}
    if not other:
        for proj in (0, 1):
            variants[f"yuv_nv12_pj{proj}"] = lambda proj=proj: yuv.flow_interp_yuv_proj_device(
                y0, c0, y1, c1, times, *args, layout=2, out_y=og, out_c=oc, flags=flags,
                trusted=trusted, workspace=ws, projection=proj)
        variants["grey_pj1"] = lambda: hsflow.flow_interp_device(
            y0, y1, times, *args, out=og, flags=flags, trusted=trusted, workspace=ws, projection=1)
        variants["bgr_pj1"] = lambda: hsflow.flow_interp_bgr_device(
            b0, b1, times, *args, out=ob, flags=flags, trusted=trusted, workspace=ws, projection=1)
    r = _time(variants, set(), rounds, warmup)
    if not other:
        m = {k: v["median_ms"] for k, v in r.items()}
        r["yuv_pj1_over_pj0"] = round(m["yuv_nv12_pj1"] / m["yuv_nv12_pj0"], 4)
        r["yuv_pj1_over_bgr_pj1"] = round(m["yuv_nv12_pj1"] / m["bgr_pj1"], 4)
        r["yuv_pj1_minus_grey_pj1_ms"] = round(m["yuv_nv12_pj1"] - m["grey_pj1"], 4)
        r["yuv_pj0_over_yuv"] = round(m["yuv_nv12_pj0"] / m["yuv_nv12"], 4)
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
    if args.part == "kiyp":
        print(json.dumps(run_kiyp(args.what[0], int(args.what[1]), args.rounds, args.warmup)),
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
           "kiyp": {}, "fused": {}}
    for size in SIZES:
        for batch in (1, 8):
            res = _child(args, "kiyp", size, batch)
            if res is None:
                return 1
            out["kiyp"][f"{size}_b{batch}"] = res
            print(json.dumps({"kiyp": size, "batch": batch, **res}), flush=True)
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
            summary = {"other": "the parent commit's libhsflow.so",
                       "order": "other, other (A/A), this, other, this, other"}
            for k in ("yuv_nv12", "grey", "bgr"):
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
    ap.add_argument("--part", default="", help="kiyp or fused: one part, result to stdout (child)")
    ap.add_argument("--what", nargs="*", default=[], help="the part's size and batch (child)")
    ap.add_argument("--other", action="store_true", help="the unchanged paths alone (child of --ab)")
    ap.add_argument("--ab", default="", help="another build of libhsflow.so for part (c)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "yuv_projection_timing.json"))
    sys.exit(main(ap.parse_args()))
