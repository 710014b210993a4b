"""Cost of the 16-bit YUV 4:2:0 interpolation ("16-bit YUV 4:2:0"),
uint16 frames out:

  (a) kiy16  KIY and KIYP on 16-bit chroma (yuv.chroma_interp_device,
             yuv.chroma_interp_proj_device on uint16 tensors) against the chain
             of launches and copies they replace, at 1080p and 4K, eight pairs,
             nt 1 and 3, I420 and NV12:
               pieces   the chroma planes to float32 (NV12: taken apart on the
                        way), two KD (temporal.downflow_device), KI on the U and
                        on the V planes with float32 out (projected: KSD and
                        KIP), floor(x + 0.5) clamped and narrowed to 16 bits
                        (NV12: interleaved on the way)
             A cell passes when the chain's median exceeds the fused kernel's
             median by more than the two (max - min) spreads added together.
  (b) the traffic model: per chroma sample 64 B of flows once and, per time,
             8 B read and 4 B (U16) written; the achieved bytes per second next
             to the 8-bit kernel's (4 B read, 2 B written) on the same shapes,
             and NV12-16 with a row's two taps as one 8-byte load.
  (c) fused16  yuv.flow_interp_yuv_proj_device on 10-bit content (uint16, alpha
             x 4) against the 8-bit call on the same content divided by four,
             1080p, batch 1 and 8, three times, flags and trusted out.
  (d) ab     the unchanged 8-bit grey, BGR and YUV fused calls on this build
             against another build of the library (the parent commit's), in
             child processes: other, other first -- the A/A spread of one build
             -- then this, other, this, other.

yuv_timing.py's method: device events around each variant, a warm-up of all, the
variants alternated inside every round of one process; the kernels of (a) and
(b) run REPS times back to back between their events.  Every part runs in child
processes of its own under a time limit; the parent process stops at the first
child that fails.

    python scripts/yuv16_timing.py --ab PARENT_LIBHSFLOW_SO  # -> profiles/yuv16_timing.json

profiles/yuv16_timing.json was made with
    python scripts/yuv16_timing.py --rounds 5 --warmup 2 --ab PARENT_LIBHSFLOW_SO
"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "cpp-optical-flow_amd"))
sys.path.insert(0, os.path.join(ROOT, "scripts"))

from yuv_timing import (ALPHA, ITERS, LEVELS, REPS, SIZES, TIMES, WARPS, WINDOW,  # noqa: E402
                        _content, _flows, _hsflow, _time)

BATCH = 8
STEP_LIMIT_S = 240


def b_sample(nt, read, written):
    """The model's bytes per chroma sample: 64 B of flows once; per time `read`
    B of chroma and `written` B of output."""
    return 64 + nt * (read + written)


def _spread(r):
    return r["max_ms"] - r["min_ms"]


def run_kiy16(size, rounds, warmup):
    import numpy as np
    import projection
    import temporal
    import torch
    import yuv
    hsflow = _hsflow(False)
    rows, cols = SIZES[size]
    rc, cc = rows // 2, cols // 2
    batch = BATCH
    flows = _flows(batch, rows, cols)
    g = torch.Generator(device="cuda").manual_seed(3)
    f32 = [torch.floor(torch.rand((batch, 2, rc, cc), device="cuda", generator=g) * 65536.0)
           .clamp_(0.0, 65535.0) for _ in range(2)]
    i0, i1 = (torch.from_numpy(f.cpu().numpy().astype(np.int64).astype(np.uint16)).cuda()
              for f in f32)
    n0, n1 = (c.permute(0, 2, 3, 1).contiguous() for c in (i0, i1))
    b0, b1 = ((f / 256.0).to(torch.uint8) for f in f32)  # the 8-bit kernel's chroma
    m0, m1 = (c.permute(0, 2, 3, 1).contiguous() for c in (b0, b1))
    del f32
    y0, y1 = _content(hsflow, batch, rows, cols)
    down = [torch.empty((batch, rc, cc), device="cuda") for _ in range(4)]
    planes = [torch.empty((batch, rc, cc), device="cuda") for _ in range(4)]
    res = {}
    for nt, times in TIMES.items():
        cells = projection.project_device(y0, y1, *flows, times)
        cells_c = torch.empty((batch, nt, rc, cc), dtype=torch.int64, device="cuda")
        oi = torch.empty((batch, nt, 2, rc, cc), dtype=torch.uint16, device="cuda")
        on = torch.empty((batch, nt, rc, cc, 2), dtype=torch.uint16, device="cuda")
        o8i = torch.empty((batch, nt, 2, rc, cc), dtype=torch.uint8, device="cuda")
        o8n = torch.empty((batch, nt, rc, cc, 2), dtype=torch.uint8, device="cuda")
        op = [torch.empty((batch, nt, rc, cc), device="cuda") for _ in range(2)]
        tmp = torch.empty((batch, nt, rc, cc), device="cuda")

        def kiy(c0, c1, lay, out, proj=False, wide=False):
            def f():
                yuv.set_nv12_loads(wide)
                for _ in range(REPS):
                    if proj:
                        yuv.chroma_interp_proj_device(c0, c1, *flows, times, cells, lay, out=out)
                    else:
                        yuv.chroma_interp_device(c0, c1, *flows, times, lay, out=out)
                yuv.set_nv12_loads(False)
            return f

        def sources(lay):  # the four chroma planes as they lie in the layout
            if lay == 1:
                return (i0[:, 0], i0[:, 1], i1[:, 0], i1[:, 1])
            return (n0[..., 0], n0[..., 1], n1[..., 0], n1[..., 1])

        def pieces(lay, proj):
            def f():
                out = oi if lay == 1 else on
                for _ in range(REPS):
                    for p, c in zip(planes, sources(lay)):
                        p.copy_(c)  # uint16 -> float32
                    temporal.downflow_device(flows[0], flows[1], uc=down[0], vc=down[1])
                    temporal.downflow_device(flows[2], flows[3], uc=down[2], vc=down[3])
                    if proj:
                        yuv.cells_down_device(cells, cells_c)
                    for ch in range(2):
                        if proj:
                            projection.frame_interp_device(planes[ch], planes[2 + ch], *down, times,
                                                           cells_c, out=op[ch])
                        else:
                            hsflow.frame_interp_device(planes[ch], planes[2 + ch], *down, times,
                                                       out=op[ch])
                        torch.add(op[ch], 0.5, out=tmp)
                        tmp.floor_().clamp_(0.0, 65535.0)
                        (out[:, :, ch] if lay == 1 else out[..., ch]).copy_(tmp)
            return f

        variants = {}
        for lay, name, c0, c1, out in ((1, "i420", i0, i1, oi), (2, "nv12", n0, n1, on)):
            for proj, stem in ((False, "kiy16"), (True, "kiyp16")):
                variants[f"{stem}_{name}"] = kiy(c0, c1, lay, out, proj)
                variants[f"{stem}_{name}_pieces"] = pieces(lay, proj)
        variants["kiy16_nv12_wide"] = kiy(n0, n1, 2, on, False, True)
        variants["kiy8_i420"] = kiy(b0, b1, 1, o8i)
        variants["kiy8_nv12"] = kiy(m0, m1, 2, o8n)
        r = _time(variants, set(variants), rounds, warmup)
        samples = rc * cc * batch
        for k in list(variants):
            if k.endswith("_pieces"):
                fused = r[k[:-len("_pieces")]]
                r[k + "_over_fused"] = round(r[k]["median_ms"] / fused["median_ms"], 3)
                r[k[:-len("_pieces")] + "_faster_by_more_than_both_spreads"] = bool(
                    r[k]["median_ms"] - fused["median_ms"] > _spread(r[k]) + _spread(fused))
            else:
                eight = k.startswith("kiy8")
                b = b_sample(nt, 4 if eight else 8, 2 if eight else 4)
                r[k]["model_bytes_per_sample"] = b
                r[k]["tb_per_s"] = round(b * samples / (r[k]["median_ms"] * 1e-3) / 1e12, 3)
        res[f"nt{nt}"] = r
    return res


def run_fused(batch, rounds, warmup, other):
    """The fused calls at 1080p, three times, flags and trusted out.  other: the
    8-bit grey, BGR and YUV calls alone, on whatever build HSFLOW_LIB names."""
    import torch
    hsflow = _hsflow(other)
    import yuv
    rows, cols = SIZES["1080p"]
    times = TIMES[3]
    y0, y1 = _content(hsflow, batch, rows, cols)
    b0, b1 = (torch.stack([y, 255 - y, y.flip(2)], dim=-1).contiguous() for y in (y0, y1))
    c0, c1 = (b[:, :rows // 2, :cols // 2, :2].contiguous() for b in (b0, b1))  # NV12 chroma
    args = (LEVELS, WARPS, WINDOW, ITERS, ALPHA)
    ws = torch.empty(hsflow.flow_interp_bgr_workspace_bytes(rows, cols, batch, LEVELS) + 4096,
                     dtype=torch.uint8, device="cuda")
    og = torch.empty((batch, 3, rows, cols), dtype=torch.uint8, device="cuda")
    ob = torch.empty((batch, 3, rows, cols, 3), dtype=torch.uint8, device="cuda")
    oc = torch.empty((batch, 3, rows // 2, cols // 2, 2), dtype=torch.uint8, device="cuda")
    flags = torch.empty((batch, 3, rows, cols), dtype=torch.uint8, device="cuda")
    trusted = torch.empty((batch, 3), dtype=torch.int32, device="cuda")
    variants = {
        "grey": lambda: hsflow.flow_interp_device(y0, y1, times, *args, out=og, flags=flags,
                                                  trusted=trusted, workspace=ws),
        "bgr": lambda: hsflow.flow_interp_bgr_device(b0, b1, times, *args, out=ob, flags=flags,
                                                     trusted=trusted, workspace=ws),
        "yuv_nv12": lambda: yuv.flow_interp_yuv_device(
            y0, c0, y1, c1, times, *args, layout=2, out_y=og, out_c=oc, flags=flags,
            trusted=trusted, workspace=ws)}
    if not other:
        # 10-bit content whose division by four is the 8-bit content: x 4 + 2 bits
        g = torch.Generator(device="cuda").manual_seed(10)

        def ten(t):
            d = torch.randint(0, 4, t.shape, device="cuda", generator=g, dtype=torch.int16)
            return (t.to(torch.int16) * 4 + d).contiguous()

        w0, w1, d0, d1 = ten(y0), ten(y1), ten(c0), ten(c1)
        args16 = (LEVELS, WARPS, WINDOW, ITERS, ALPHA * 4)
        og16 = torch.empty((batch, 3, rows, cols), dtype=torch.int16, device="cuda")
        oc16 = torch.empty((batch, 3, rows // 2, cols // 2, 2), dtype=torch.int16, device="cuda")
        variants["yuv16_nv12"] = lambda: yuv.flow_interp_yuv_device(
            w0, d0, w1, d1, times, *args16, layout=2, out_y=og16, out_c=oc16, flags=flags,
            trusted=trusted, workspace=ws)
    r = _time(variants, set(), rounds, warmup)
    if not other:
        r["yuv16_over_yuv8"] = round(r["yuv16_nv12"]["median_ms"] / r["yuv_nv12"]["median_ms"], 4)
        r["yuv16_minus_yuv8_ms"] = round(r["yuv16_nv12"]["median_ms"] -
                                         r["yuv_nv12"]["median_ms"], 4)
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
    if args.part == "kiy16":
        print(json.dumps(run_kiy16(args.what[0], args.rounds, args.warmup)), flush=True)
        return 0
    if args.part == "fused":
        print(json.dumps(run_fused(int(args.what[0]), args.rounds, args.warmup, args.other)),
              flush=True)
        return 0
    out = {"window": WINDOW, "iters_per_level": ITERS, "levels": LEVELS, "warps": WARPS,
           "alpha": ALPHA, "alpha_16_bit": ALPHA * 4, "rounds": args.rounds, "batch_kiy16": BATCH,
           "times": {str(k): list(v) for k, v in TIMES.items()},
           "timing": "device events around each variant; median, min and max over the rounds, "
                     f"variants alternated inside every round; kiy16: {REPS} runs between the "
                     "events, time per run",
           "model": "per chroma sample: 64 B of flows once; per time 8 B read and 4 B (U16) "
                    "written; the 8-bit kernel 4 B and 2 B",
           "kiy16": {}, "fused": {}}

    def save():
        if args.out:
            os.makedirs(os.path.dirname(args.out), exist_ok=True)
            with open(args.out, "w") as f:
                json.dump(out, f, indent=1)
                f.write("\n")

    for size in SIZES:
        res = _child(args, "kiy16", size)
        if res is None:
            return 1
        out["kiy16"][f"{size}_b{BATCH}"] = res
        print(json.dumps({"kiy16": size, **res}), flush=True)
        save()
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
            summary = {"other": "the parent commit's build of libhsflow.so",
                       "order": "other, other (A/A), this, other, this, other"}
            for k in ("grey", "bgr", "yuv_nv12"):
                aa = [r[k]["median_ms"] for r in runs["aa"]]
                this = [r[k]["median_ms"] for r in runs["this"]]
                other = [r[k]["median_ms"] for r in runs["other"]]
                spread = 100.0 * abs(aa[0] - aa[1]) / min(aa)
                ratio = sum(this) / sum(other)
                summary[k] = {"aa_run_to_run_pct": round(spread, 2), "this_median_ms": this,
                              "other_median_ms": other, "this_over_other": round(ratio, 4),
                              "inside_aa_spread": bool(abs(ratio - 1.0) * 100.0 <= spread)}
            entry["ab"] = summary
            print(json.dumps({"fused": batch, "ab": summary}), flush=True)
        out["fused"][f"1080p_b{batch}"] = entry
        save()
    return 0


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--part", default="", help="kiy16 or fused: one part, result to stdout (child)")
    ap.add_argument("--what", nargs="*", default=[], help="the part's size or batch (child)")
    ap.add_argument("--other", action="store_true", help="the 8-bit calls alone (child of --ab)")
    ap.add_argument("--ab", default="", help="another build of libhsflow.so for part (d)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "yuv16_timing.json"))
    sys.exit(main(ap.parse_args()))
