"""The bits of everything that samples a plane at (y + 8 v, x + 8 u) -- KW, KC,
KR, KI, KRC, KIC -- and of their neighbours KN, KM, KG, on a fixed list of small
cases, as one sha256 per output.  Two builds of the library (HSFLOW_LIB selects
one) computed the same when their files are equal: the check a refactor of the
device code runs against its parent on the same box and compiler.  A record,
not a golden test: the bits belong to the compiler, and the permanent guards
are the suite's cross-kernel bitwise tests.

Shapes: KC_SHAPES of tests/test_consistency.py -- one-pixel planes, ragged
quads, more than one tile row, KC's shifted tiles (plane 4847: shifts 0, 3, 2).
Flows: that module's smooth flows (all three classes), and the same with NaN,
+-inf and +-1e30 at the corners and a few scattered pixels, which the kernels
clamp by design.  Bases: aligned, and one element past a 16-byte boundary.

The cases run in a child process under a time limit; the first failing step
ends the run.

    HSFLOW_LIB=... python scripts/sampling_bits.py run OUT.json [--label parent]
    python scripts/sampling_bits.py compare A.json B.json [--out RECORD.json]
"""
import argparse
import hashlib
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "cpp-optical-flow_amd"))

SHAPES = [(1, 1, 1), (1, 1, 70), (2, 5, 3), (3, 37, 131), (1, 67, 64), (2, 4, 256)]
BIG = (3, 37, 131)
E2E = (2, 97, 131)
SOLVE = (3, 2, 5, 100, 400.0)  # levels, warps, window, iterations, alpha
HOSTILE = [float("nan"), float("inf"), float("-inf"), 1e30, -1e30]
TIMES = {1: (0.3,), 3: (0.0, 0.5, 1.0)}
FRAME_TYPES = ("uint8", "float16", "float32", "float64")
LIMIT_S = 300


def _box9(np, a):
    c = np.cumsum(np.pad(a, ((0, 0), (0, 0), (1, 0))), axis=2)
    h = c[:, :, 9:] - c[:, :, :-9]
    c = np.cumsum(np.pad(h, ((0, 0), (1, 0), (0, 0))), axis=1)
    return (c[:, 9:, :] - c[:, :-9, :]) / 81.0


def smooth_flows(np, batch, rows, cols):
    """tests/test_consistency.py _smooth_flows: about 1.3 px rms plus an offset
    of up to 3.2 px per plane; the backward flow is -(forward) + noise."""
    rng = np.random.default_rng(77 + 1000 * batch + 10 * rows + cols)

    def field(amp):
        return amp * _box9(np, rng.normal(size=(batch, rows + 8, cols + 8)))

    sx = 1.0 if cols >= 8 else cols / 16.0
    sy = 1.0 if rows >= 8 else rows / 16.0
    off = rng.uniform(-0.4, 0.4, (2, batch, 1, 1))
    uf = (field(1.5) + off[0]) * sx
    vf = (field(1.5) + off[1]) * sy
    ub = -uf + field(0.3) * sx
    vb = -vf + field(0.3) * sy
    return [a.astype(np.float32) for a in (uf, vf, ub, vb)]


def hostile_flows(np, batch, rows, cols):
    flows = smooth_flows(np, batch, rows, cols)
    rng = np.random.default_rng(91 + rows * cols)
    spots = [(0, 0), (0, cols - 1), (rows - 1, 0), (rows - 1, cols - 1)]
    spots += [(int(rng.integers(rows)), int(rng.integers(cols))) for _ in range(6)]
    for b in range(batch):
        for k, (y, x) in enumerate(spots):
            flows[(k + b) % 4][b, y, x] = HOSTILE[(k + 2 * b) % len(HOSTILE)]
    return flows


def frames(np, shape, dtype, seed):
    """Two frames of non-integer values in [0, 255] (integers for uint8)."""
    rng = np.random.default_rng(seed + shape[1] * shape[2])
    return [rng.uniform(0.0, 255.0, shape).astype(dtype) for _ in range(2)]


def child(out_path, label):
    import numpy as np
    import torch
    import hsflow

    hashes = {}

    def put(name, *tensors):
        torch.cuda.synchronize()
        for k, t in enumerate(tensors):
            if t is not None:
                hashes[f"{name} [{k}]"] = hashlib.sha256(t.cpu().numpy().tobytes()).hexdigest()

    def dev(a, shift):
        """a on the device; shift: its base one element past a 16-byte boundary"""
        t = torch.from_numpy(np.ascontiguousarray(a))
        if not shift:
            return t.cuda()
        flat = torch.zeros(t.numel() + 16, dtype=t.dtype, device="cuda")
        view = flat[1:1 + t.numel()].view(t.shape)
        view.copy_(t)
        return view

    def empty(shape, dtype, shift):
        return dev(np.zeros(shape, dtype), shift)

    for shape in SHAPES:
        b, rows, cols = shape
        sid = "x".join(map(str, shape))
        for fname, make in (("smooth", smooth_flows), ("hostile", hostile_flows)):
            fl = make(np, *shape)
            for shift in (0, 1):
                tag = f"{sid} {fname} shift{shift}"
                t = [dev(a, shift) for a in fl]
                err = empty(shape, np.float32, shift)
                mask = empty(shape, np.uint8, shift)
                _, _, counts = hsflow.consistency_device(*t, err=err, mask=mask, counts=True)
                put(f"KC {tag}", err, mask, counts)
                rev = [t[2], t[3], t[0], t[1]]
                mask_b = empty(shape, np.uint8, shift)
                hsflow.consistency_device(*rev, mask=mask_b)
                for ft in FRAME_TYPES:
                    I0, I1 = (dev(a, shift) for a in frames(np, shape, ft, 5))
                    if not shift:
                        ws = hsflow.alloc_workspace(rows, cols, b)
                        g = [torch.empty(shape, dtype=torch.float32, device="cuda")
                             for _ in range(3)]
                        hsflow.warp_gradients_device(I0, I1, t[0], t[1], ws, *g)
                        put(f"KW {tag} {ft}", *g)
                        put(f"KR {tag} {ft}", *hsflow.warp_image_device(I1, t[0], t[1], oof=True))
                    for nt, times in TIMES.items():
                        for odt in (np.float32, np.uint8):
                            for masks in ((mask, mask_b), (None, None)):
                                o = empty((b, nt, rows, cols), odt, shift)
                                f = empty((b, nt, rows, cols), np.uint8, shift)
                                _, _, tr = hsflow.frame_interp_device(
                                    I0, I1, *t, times, mask_f=masks[0], mask_b=masks[1], out=o,
                                    flags=f, trusted=True)
                                put(f"KI {tag} {ft} nt{nt} {np.dtype(odt).name} "
                                    f"masks{int(masks[0] is not None)}", o, f, tr)
                B0, B1 = (dev(a, shift) for a in frames(np, shape + (3,), np.uint8, 9))
                for wide in (False, True):
                    was = hsflow.set_interp_bgr_loads(wide)
                    for odt in (np.float32, np.uint8):
                        o = empty(shape + (3,), odt, shift)
                        oof = empty(shape, np.uint8, shift)
                        hsflow.warp_image_bgr_device(B1, t[0], t[1], out=o, oof=oof)
                        put(f"KRC {tag} wide{int(wide)} {np.dtype(odt).name}", o, oof)
                        for nt, times in TIMES.items():
                            for masks in ((mask, mask_b), (None, None)):
                                o = empty((b, nt, rows, cols, 3), odt, shift)
                                f = empty((b, nt, rows, cols), np.uint8, shift)
                                _, _, tr = hsflow.frame_interp_bgr_device(
                                    B0, B1, *t, times, mask_f=masks[0], mask_b=masks[1], out=o,
                                    flags=f, trusted=True)
                                put(f"KIC {tag} wide{int(wide)} nt{nt} {np.dtype(odt).name} "
                                    f"masks{int(masks[0] is not None)}", o, f, tr)
                    hsflow.set_interp_bgr_loads(was)

    sid = "x".join(map(str, BIG))
    for ft in FRAME_TYPES:
        I = dev(frames(np, BIG, ft, 13)[0], 0)
        for mode in (hsflow.PREFILTER_HIGHPASS, hsflow.PREFILTER_NORMALIZE):
            for sigma in (1.0, 2.5):
                pf = hsflow.Prefilter(mode, sigma, 1.0, 32.0)
                put(f"KN {sid} {ft} mode{mode} sigma{sigma}", hsflow.prefilter_device(I, pf))
    t = [dev(a, 0) for a in smooth_flows(np, *BIG)]
    for k in hsflow.MEDIAN_SIZES:
        put(f"KM {sid} k{k}", *hsflow.median_device(t[0], t[1], k))
    put(f"KG {sid}", hsflow.diffusivity_device(t[0], t[1], 1.0))

    sid = "x".join(map(str, E2E))
    pairs = [hsflow.synth_pair(4000 + k, E2E[1], E2E[2]) for k in range(E2E[0])]
    G0, G1 = (dev(np.stack([p[j] for p in pairs]), 0) for j in range(2))
    r = hsflow.flow_bidir_device(G0, G1, *SOLVE, median=5, err_f=True, mask_f=True, counts_f=True,
                                 err_b=True, mask_b=True, counts_b=True)
    put(f"flow_bidir {sid}", *r)
    put(f"flow_interp {sid}", *hsflow.flow_interp_device(G0, G1, TIMES[3], *SOLVE, median=5,
                                                         flags=True, trusted=True))
    chans = [[hsflow.synth_pair(5000 + 10 * c + k, E2E[1], E2E[2]) for c in range(3)]
             for k in range(E2E[0])]
    B0, B1 = (dev(np.stack([np.stack([ch[j] for ch in p], axis=-1) for p in chans])
                  .astype(np.uint8), 0) for j in range(2))
    put(f"flow_interp_bgr {sid}", *hsflow.flow_interp_bgr_device(
        B0, B1, TIMES[3], *SOLVE, median=5, out_dtype=torch.uint8, flags=True, trusted=True))

    with open(out_path, "w") as f:
        json.dump({"label": label, "lib": os.path.relpath(hsflow.LIB_PATH, ROOT),
                   "outputs": len(hashes), "sha256": hashes}, f, indent=1)
        f.write("\n")
    print(f"{len(hashes)} outputs hashed -> {out_path}")
    return 0


def compare(a_path, b_path, out_path):
    with open(a_path) as f:
        a = json.load(f)
    with open(b_path) as f:
        b = json.load(f)
    ha, hb = a.pop("sha256"), b.pop("sha256")
    differ = sorted(k for k in set(ha) | set(hb) if ha.get(k) != hb.get(k))

    def groups(h):
        """The file folded to one digest per kernel and shape (the first two
        words of an output's name): sha256 of its "name hash" lines, sorted."""
        lines = {}
        for k in sorted(h):
            lines.setdefault(" ".join(k.split()[:2]), []).append(f"{k} {h[k]}\n")
        return {g: {"outputs": len(v), "sha256": hashlib.sha256("".join(v).encode()).hexdigest()}
                for g, v in lines.items()}

    # the record is small: a file is kept as its groups' digests, and in full
    # only the outputs that differ
    ga, gb = groups(ha), groups(hb)
    rec = {"what": "scripts/sampling_bits.py on two builds of the library on one box: the sha256 "
                   "of every output, folded to one digest per kernel and shape",
           "a": a, "b": b, "equal": not differ,
           "differ": {k: [ha.get(k), hb.get(k)] for k in differ},
           "groups": {g: {"outputs": [ga.get(g, {}).get("outputs"), gb.get(g, {}).get("outputs")],
                          "a": ga.get(g, {}).get("sha256"), "b": gb.get(g, {}).get("sha256")}
                      for g in sorted(set(ga) | set(gb))}}
    if out_path:
        with open(out_path, "w") as f:  # one line per entry, one per group
            body = [f' {json.dumps(k)}: {json.dumps(v)}' for k, v in rec.items() if k != "groups"]
            rows = ",\n".join(f'  {json.dumps(g)}: {json.dumps(v)}'
                              for g, v in rec["groups"].items())
            f.write("{\n" + ",\n".join(body) + ',\n "groups": {\n' + rows + "\n }\n}\n")
    print(f"{len(ha)} / {len(hb)} outputs, {len(differ)} differ")
    for k in differ[:20]:
        print("  differs:", k)
    return 1 if differ else 0


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("mode", choices=("run", "child", "compare"))
    ap.add_argument("files", nargs="+")
    ap.add_argument("--out", default="")
    ap.add_argument("--label", default="", help="run: which build this is, kept in the file")
    args = ap.parse_args()
    if args.mode == "compare":
        sys.exit(compare(args.files[0], args.files[1], args.out))
    if args.mode == "child":
        sys.exit(child(args.files[0], args.label))
    # a fresh process under a time limit; an exception in any step ends it
    sys.exit(subprocess.run([sys.executable, os.path.abspath(__file__), "child", args.files[0],
                             "--label", args.label], timeout=LIMIT_S).returncode)
