"""The argument-error table of the warped family, tests/golden/arg_errors.json.

    HSFLOW_LIB=/path/to/libhsflow.so python tests/golden/make_arg_errors.py

Run it against the library the table is to pin (the build of the commit in
front of a change to the host layer); tests/test_arg_errors_table.py then holds
the working tree's library to it.  Needs no GPU and must not see one: every
case fails an argument check, so no call gets as far as a launch.

For every device entry point of the family the table holds, per invalid
argument ("fault"), the status and the text of hsflow_last_error with every
run of digits replaced by N; every status is HSFLOW_ERR_ARG, which the
generator asserts.  For the four *_sm_device solves it also covers every pair
of those faults that can be made at once (pairs() below): each returned the
same status, and the table keeps their number per call.

Conventions (those of the test_argument_errors_without_a_gpu tests): 16 x 16,
batch 1, 3 levels; invented addresses 4096 apart that are never dereferenced;
the workspace far away from them with a large stated size.
"""
from __future__ import annotations

import ctypes
import itertools
import json
import os
import re
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
TABLE = os.path.join(HERE, "arg_errors.json")

A = [4096 * k for k in range(1, 16)]  # an f32 plane is 1024 bytes, an f32 BGR frame 3072
WS, BIG = 1 << 20, 1 << 30
NAN, INF = float("nan"), float("inf")
U8, F32, F64, F16 = 0, 1, 2, 3
PF = dict(mode=2, sigma=1.0, eps=4.0, scale=32.0)
SM = dict(mode=1, lam=0.3)
SOLVE = [("levels", 3), ("warps", 1), ("median", 5), ("window", 5), ("iters", 10),
         ("alpha", 1.0)]
PAIRED = ("hsflow_flow_warped_sm_device", "hsflow_flow_bidir_sm_device",
          "hsflow_flow_interp_sm_device", "hsflow_flow_interp_bgr_sm_device")


def _hsflow():
    pkg = os.path.join(ROOT, "cpp-optical-flow_amd")
    if pkg not in sys.path:
        sys.path.insert(0, pkg)
    import hsflow
    return hsflow


def normalise(text):
    return re.sub(r"\d+", "N", text)


# ------------------------------------------------------------------ the faults
def _sizes(batch=True):
    f = {"rows=0": dict(rows=0), "rows=-1": dict(rows=-1), "rows=262141": dict(rows=4 * 65535 + 1),
         "cols=0": dict(cols=0), "pixels=2^29": dict(rows=32768, cols=16384)}
    if batch:
        f.update({"batch=0": dict(batch=0), "batch=65536": dict(batch=65536)})
    return f


def _nulls(*names):
    return {f"{n}=null": {n: None} for n in names}


def _solve_faults(median=True):
    f = {"levels=0": dict(levels=0), "levels=9": dict(levels=9), "warps=0": dict(warps=0),
         "warps=17": dict(warps=17), "window=0": dict(window=0), "window=64": dict(window=64),
         "iters=-1": dict(iters=-1)}
    if median:
        f["median=4"] = dict(median=4)
    return f


def _threshold_faults():
    return {"rel=nan": dict(rel=NAN), "rel=-1": dict(rel=-1.0), "abs=nan": dict(abs_thr=NAN),
            "abs=inf": dict(abs_thr=INF)}


def _interp_faults(dev=True):
    f = {"nt=0": dict(nt=0), "nt=17": dict(nt=17, times=(0.5,) * 17), "time=1.5": dict(times=(1.5,)),
         "time=nan": dict(times=(NAN,)), "times=null": dict(times=None),
         "dtype_out=9": dict(dtype_out=9), "dtype_out=F16": dict(dtype_out=F16)}
    if dev:
        f["dtype_out=F64"] = dict(dtype_out=F64)
    return f


def _pf_faults():
    return {"pf.mode=3": dict(pf=dict(mode=3)), "pf.mode=-1": dict(pf=dict(mode=-1)),
            "pf.sigma=0.1": dict(pf=dict(sigma=0.1)), "pf.sigma=6": dict(pf=dict(sigma=6.0)),
            "pf.sigma=nan": dict(pf=dict(sigma=NAN)), "pf.eps=0": dict(pf=dict(eps=0.0)),
            "pf.eps=nan": dict(pf=dict(eps=NAN)), "pf.scale=0": dict(pf=dict(scale=0.0)),
            "pf.scale=inf": dict(pf=dict(scale=INF))}


def _sm_faults():
    return {"sm.mode=2": dict(sm=dict(mode=2)), "sm.mode=-1": dict(sm=dict(mode=-1)),
            "sm.lam=0": dict(sm=dict(lam=0.0)), "sm.lam=nan": dict(sm=dict(lam=NAN)),
            "sm.lam=inf": dict(sm=dict(lam=INF)), "window=4 (smoothness on)": dict(window=4)}


def calls(hs):
    """name -> (ordered parameters with their valid values, fault -> overrides)."""
    jac = hs.workspace_bytes(16, 16, 1)
    pyr = hs.pyramid_workspace_bytes(16, 16, 1, 3)
    planes = hs.prefilter_planes_bytes(16, 16, 1)
    out = {}

    def add(name, params, faults):
        assert name not in out
        out[name] = (params + [("stream", None)], faults)

    frames = [("I0", A[0]), ("I1", A[1]), ("dtype_in", F32)]
    shape = [("rows", 16), ("cols", 16), ("batch", 1)]
    ws = [("ws", WS), ("wsb", BIG)]

    add("hsflow_warp_gradients_device",
        frames + shape + [("u0", A[2]), ("v0", A[3]), ("gx", A[4]), ("gy", A[5]), ("gt", A[6])] + ws,
        {**_nulls("I0", "I1", "u0", "v0", "ws"), **_sizes(), "dtype_in=9": dict(dtype_in=9),
         "wsb=need-1": dict(wsb=jac - 1)})

    # the four warped solves; pf / sm: which option structs the entry point takes
    for name, median, pf, sm in (("hsflow_flow_warped_device", False, False, False),
                                 ("hsflow_flow_warped_median_device", True, False, False),
                                 ("hsflow_flow_warped_pf_device", True, True, False),
                                 ("hsflow_flow_warped_sm_device", True, True, True)):
        need = pyr + (planes if pf else 0)
        solve = [p for p in SOLVE if median or p[0] != "median"]
        opts = ([("pf", PF)] if pf else []) + ([("sm", SM)] if sm else [])
        f = {**_nulls("I0", "I1", "u", "v", "ws"), **_sizes(), **_solve_faults(median),
             "dtype_in=9": dict(dtype_in=9), "wsb=need-1": dict(wsb=need - 1)}
        if pf:  # the frames must not share a byte with the workspace
            f.update({**_pf_faults(), "I0 in ws": dict(I0=WS + need - 1),
                      "I1 in ws": dict(I1=WS - 1023)})
        if sm:
            f.update(_sm_faults())
        add(name, frames + shape + solve + [("u", A[2]), ("v", A[3])] + opts + ws, f)

    add("hsflow_flow_median_device",
        [("u", A[0]), ("v", A[1])] + shape + [("ksize", 5), ("u_out", A[2]), ("v_out", A[3])],
        {**_nulls("u", "v", "u_out", "v_out"), **_sizes(), "ksize=0": dict(ksize=0),
         "ksize=4": dict(ksize=4), "u_out=u": dict(u_out=A[0]), "u_out in v": dict(u_out=A[1] + 1020),
         "v_out in u": dict(v_out=A[0] - 1020), "v_out=u_out": dict(v_out=A[2])})

    flows = [("uf", A[2]), ("vf", A[3]), ("ub", A[4]), ("vb", A[5])]
    thr = [("rel", 0.05), ("abs_thr", 0.5)]
    add("hsflow_flow_consistency_device",
        flows + shape + thr + [("err", A[6]), ("mask", A[7]), ("counts", A[8])],
        {**_nulls("uf", "vf", "ub", "vb"), **_sizes(), **_threshold_faults(),
         "no output": dict(err=None, mask=None, counts=None)})

    checks = [("err_f", A[6]), ("mask_f", A[7]), ("counts_f", A[8]), ("err_b", A[9]),
              ("mask_b", A[10]), ("counts_b", A[11])]
    for name, median, pf, sm in (("hsflow_flow_bidir_device", False, False, False),
                                 ("hsflow_flow_bidir_median_device", True, False, False),
                                 ("hsflow_flow_bidir_pf_device", True, True, False),
                                 ("hsflow_flow_bidir_sm_device", True, True, True)):
        need = hs.bidir_workspace_bytes(16, 16, 1, 3) + (planes if pf else 0)
        solve = [p for p in SOLVE if median or p[0] != "median"]
        opts = ([("pf", PF)] if pf else []) + ([("sm", SM)] if sm else [])
        f = {**_nulls("I0", "I1", "uf", "vf", "ub", "vb", "ws"), **_sizes(),
             **_solve_faults(median), **_threshold_faults(), "dtype_in=9": dict(dtype_in=9),
             "wsb=need-1": dict(wsb=need - 1)}
        if pf:
            f.update({**_pf_faults(), "I0 in ws": dict(I0=WS + need - 1),
                      "I1 in ws": dict(I1=WS - 1023)})
        if sm:
            f.update(_sm_faults())
        add(name, frames + shape + solve + thr + flows + checks + opts + ws, f)

    add("hsflow_warp_image_device",
        [("I", A[0]), ("dtype_in", F32)] + shape + [("u", A[1]), ("v", A[2]), ("out", A[3]),
                                                     ("oof", A[4])],
        {**_nulls("I", "u", "v", "out"), **_sizes(), "dtype_in=9": dict(dtype_in=9),
         "out=I": dict(out=A[0]), "out in u": dict(out=A[1] - 1020), "oof in v": dict(oof=A[2] + 1023),
         "oof in out": dict(oof=A[3] + 1023)})
    add("hsflow_warp_image_bgr_device",
        [("I", A[0])] + shape + [("u", A[1]), ("v", A[2]), ("out", A[3]), ("dtype_out", F32),
                                 ("oof", A[4])],
        {**_nulls("I", "u", "v", "out"), **_sizes(), "dtype_out=F64": dict(dtype_out=F64),
         "dtype_out=9": dict(dtype_out=9), "out in I": dict(out=A[0] + 767),
         "out in u": dict(out=A[1] - 3071), "oof=I": dict(oof=A[0]),
         "oof in out": dict(oof=A[3] + 3071)})

    ki_in = flows + [("mf", A[6]), ("mb", A[7])]
    interp = [("times", (0.5,)), ("nt", 1), ("out", A[8]), ("dtype_out", F32), ("flags", A[10]),
              ("trusted", A[12])]
    add("hsflow_frame_interp_device", frames + shape + ki_in + interp,
        {**_nulls("I0", "I1", "uf", "vf", "ub", "vb", "out"), **_sizes(), **_interp_faults(),
         "dtype_in=9": dict(dtype_in=9), "out=I0": dict(out=A[0]), "out in mb": dict(out=A[7] + 255),
         "flags in I1": dict(flags=A[1] + 1023), "flags in out": dict(flags=A[8] + 1023),
         "trusted in ub": dict(trusted=A[4] + 1020), "trusted in flags": dict(trusted=A[10] + 252),
         "second frame reaches flags": dict(times=(0.25, 0.5), nt=2, flags=A[8] + 1024)})
    add("hsflow_frame_interp_bgr_device", [("I0", A[0]), ("I1", A[1])] + shape + ki_in + interp,
        {**_nulls("I0", "I1", "uf", "vf", "ub", "vb", "out"), **_sizes(), **_interp_faults(),
         "out in I0": dict(out=A[0] + 767), "out in mb": dict(out=A[7] + 255),
         "flags=I1": dict(flags=A[1]), "flags in out": dict(flags=A[8] + 3071),
         "trusted in ub": dict(trusted=A[4] + 1020), "trusted in flags": dict(trusted=A[10] + 252),
         "second frame reaches flags": dict(times=(0.25, 0.5), nt=2, flags=A[8] + 3072)})

    # the fused interpolating solves, grey and BGR
    fused = [("times", (0.5,)), ("nt", 1), ("out", A[2]), ("dtype_out", F32), ("flags", A[3]),
             ("trusted", A[4])]
    for bgr in (False, True):
        stem = "hsflow_flow_interp_bgr" if bgr else "hsflow_flow_interp"
        own = (hs.flow_interp_bgr_workspace_bytes if bgr else hs.flow_interp_workspace_bytes)(
            16, 16, 1, 3)
        head = [("I0", A[0]), ("I1", A[1])] + ([] if bgr else [("dtype_in", F32)])
        fb = 768 if bgr else 1024
        for suffix, pf, sm in (("_device", False, False), ("_pf_device", True, False),
                               ("_sm_device", True, True)):
            need = own + (planes if pf else 0)
            opts = ([("pf", PF)] if pf else []) + ([("sm", SM)] if sm else [])
            f = {**_nulls("I0", "I1", "out", "ws"), **_sizes(), **_solve_faults(),
                 **_threshold_faults(), **_interp_faults(), "wsb=need-1": dict(wsb=need - 1),
                 "out=I0": dict(out=A[0]), "flags in I1": dict(flags=A[1] + fb - 1),
                 "out in ws": dict(out=WS + need - 4), "trusted in ws": dict(trusted=WS + 64),
                 "flags in out": dict(flags=A[2] + 512)}
            if not bgr:
                f["dtype_in=9"] = dict(dtype_in=9)
            if bgr or pf:  # the frames must not share a byte with the workspace
                f.update({"I0 in ws": dict(I0=WS + need - 1), "I1 in ws": dict(I1=WS - fb + 1)})
            if pf:
                f.update(_pf_faults())
            if sm:
                f.update(_sm_faults())
            add(stem + suffix, head + shape + SOLVE + thr + fused + opts + ws, f)

    add("hsflow_prefilter_device",
        [("I", A[0]), ("dtype_in", F32)] + shape + [("pf", PF), ("out", A[1])],
        {**_nulls("I", "out", "pf"), **_sizes(), **_pf_faults(), "pf.mode=0": dict(pf=dict(mode=0)),
         "dtype_in=9": dict(dtype_in=9), "out=I": dict(out=A[0]), "out in I": dict(out=A[0] + 1023),
         "I in out": dict(out=A[0] - 1023)})
    add("hsflow_flow_diffusivity_device",
        [("u", A[0]), ("v", A[1])] + shape + [("lam", 0.3), ("g", A[2])],
        {**_nulls("u", "v", "g"), **_sizes(), "lam=0": dict(lam=0.0), "lam=-0.3": dict(lam=-0.3),
         "lam=nan": dict(lam=NAN), "lam=inf": dict(lam=INF), "g=u": dict(g=A[0]),
         "g in v": dict(g=A[1] - 1020)})
    add("hsflow_jacobi_weighted_device",
        shape + [("window", 5), ("iters", 3), ("alpha", 1.0), ("g", A[0]), ("u", A[1]),
                 ("v", A[2])] + ws,
        {**_nulls("g", "u", "v", "ws"), **_sizes(), "window=4": dict(window=4),
         "window=7": dict(window=7), "window=0": dict(window=0), "iters=-1": dict(iters=-1),
         "wsb=need-1": dict(wsb=jac - 1), "g=u": dict(g=A[1]), "v in u": dict(v=A[1] + 1020),
         "u in ws": dict(u=WS + jac - 4), "g=ws": dict(g=WS), "v in ws": dict(v=WS - 1020)})
    return out


def host_calls():
    """The host forms with a null context: name -> arguments (ctypes-ready)."""
    half = (ctypes.c_float * 1)(0.5)
    planes = (ctypes.c_void_p * 1)(A[2])
    img = [None, A[0], A[1], F32, 16, 16, 64, 64]
    bidir_out = [0.05, 0.5, A[2], A[3], A[4], A[5], F32, 64, A[6], A[7], 16, A[8]]
    return {
        "hsflow_flow_warped": img + [3, 1, 5, 10, 1.0, A[2], A[3], F32, 64],
        "hsflow_flow_warped_median": img + [3, 1, 5, 5, 10, 1.0, A[2], A[3], F32, 64],
        "hsflow_flow_bidir": img + [3, 1, 5, 10, 1.0] + bidir_out,
        "hsflow_flow_bidir_median": img + [3, 1, 5, 5, 10, 1.0] + bidir_out,
        "hsflow_flow_interp": img + [3, 1, 5, 5, 10, 1.0, 0.05, 0.5, half, 1, planes, F32, 64, None,
                                     16, None],
        # sets text: its arguments are checked before the context
        "hsflow_flow_interp_bgr": [None, A[0], A[1], 16, 16, 48, 48, 3, 1, 5, 5, 10, 1.0, 0.05, 0.5,
                                   half, 1, planes, U8, 48, None, 16, None],
    }


# ------------------------------------------------------------------ running them
def merged(a, b):
    """Both faults' overrides at once; None where they set the same thing."""
    out = {}
    for k in set(a) | set(b):
        if k in a and k in b:
            if not (isinstance(a[k], dict) and isinstance(b[k], dict)) or set(a[k]) & set(b[k]):
                return None
            out[k] = {**a[k], **b[k]}
        else:
            out[k] = a[k] if k in a else b[k]
    return out


def pairs(faults):
    for a, b in itertools.combinations(sorted(faults), 2):
        both = merged(faults[a], faults[b])
        if both is not None:
            yield a, b, both


def run(hs, name, params, overrides):
    """(status, normalised hsflow_last_error) of one call."""
    L = hs.lib()
    keep, args = [], []
    for key, value in params:
        if key in overrides:
            value = {**value, **overrides[key]} if isinstance(overrides[key], dict) \
                else overrides[key]
        if key == "pf" and value is not None:
            value = hs._CPrefilter(value["mode"], value["sigma"], value["eps"], value["scale"])
            keep.append(value)
            value = ctypes.byref(value)
        elif key == "sm" and value is not None:
            value = hs._CSmoothness(value["mode"], value["lam"])
            keep.append(value)
            value = ctypes.byref(value)
        elif key == "times" and value is not None:
            value = (ctypes.c_float * len(value))(*value)
            keep.append(value)
        args.append(value)
    status = getattr(L, name)(*args)
    return status, normalise(L.hsflow_last_error(None).decode())


def build_table(hs):
    """Every case has the one status (asserted here, so only failing cases get
    in: one whose checks all pass would go on to launch kernels on the invented
    addresses).  single: call -> text -> the faults that give it; pairs: call ->
    how many pairs(faults) there are, each of which gave the status; host: the
    text where the call sets one."""
    E = hs.HSFLOW_ERR_ARG
    single, paired, host = {}, {}, {}
    for name, (params, faults) in calls(hs).items():
        by_text = {}
        for fault, o in faults.items():
            status, text = run(hs, name, params, o)
            assert status == E and text, (name, fault, status, text)
            by_text.setdefault(text, []).append(fault)
        single[name] = by_text
        if name in PAIRED:
            paired[name] = 0
            for a, b, o in pairs(faults):
                assert run(hs, name, params, o)[0] == E, (name, a, b)
                paired[name] += 1
    L = hs.lib()
    for name, args in host_calls().items():
        assert getattr(L, name)(*args) == E, name
        text = normalise(L.hsflow_last_error(None).decode())
        host[name] = text if name == "hsflow_flow_interp_bgr" else None
    return {"status": E, "single": single, "pairs": paired, "host_null_context": host}


def single_texts(table, name):
    """fault -> text of one call."""
    return {f: text for text, faults in table["single"][name].items() for f in faults}


def write_table(table, path):
    """One line per call and text, so that a change of the table reads as a diff."""
    d = json.dumps
    lines = ["{", f' "status": {table["status"]},', ' "single": {']
    names = sorted(table["single"])
    for name in names:
        lines.append(f"  {d(name)}: {{")
        rows = sorted(table["single"][name].items())
        for k, (text, faults) in enumerate(rows):
            lines.append(f"   {d(text)}: {d(sorted(faults))}" + ("," if k + 1 < len(rows) else ""))
        lines.append("  }" + ("," if name != names[-1] else ""))
    lines += [" },", f' "pairs": {d(table["pairs"], sort_keys=True)},',
              f' "host_null_context": {d(table["host_null_context"], sort_keys=True)}', "}"]
    with open(path, "w") as f:
        f.write("\n".join(lines) + "\n")


def main():
    import torch
    assert not torch.cuda.is_available(), "run this where no GPU is visible"
    hs = _hsflow()
    table = build_table(hs)
    write_table(table, TABLE)
    n = sum(len(f) for v in table["single"].values() for f in v.values())
    print(f"{hs.LIB_PATH}: {len(table['single'])} calls, {n} single faults, "
          f"{sum(table['pairs'].values())} pairs, {len(table['host_null_context'])} host forms "
          f"-> {TABLE}")


if __name__ == "__main__":
    main()
