"""The call table of the Python binding, tests/golden/py_calls.json.

    python tests/golden/make_py_calls.py host      # no GPU needed
    python tests/golden/make_py_calls.py device    # needs a GPU, launches nothing

Run it with the hsflow.py the table is to pin (the commit in front of a change
to the binding); tests/test_py_calls_table.py then holds the working tree's
hsflow.py to it.  Each half rewrites its own sections of the table.

A Recorder stands in for the loaded library (hsflow._lib): every entry point
appends (name, args) to a list and returns HSFLOW_OK, so nothing is solved and
nothing is launched.  The pure size/status queries are forwarded to the real
library, so a defaulted workspace's size is part of the record.  For every
public callable of hsflow the table holds, per case, the C calls it made --
which buffer at which byte offset in which slot, every integer and float by
repr, structs by field, the stream as "current" or "given" -- and what it
returned; or, for a case the Python code itself rejects, the HsflowError's
status and text (and the C calls made before it).  The device half keeps its
error cases, none of which gets as far as a C call, as [status, text, cases]
per distinct error (pack_errors): every tensor argument a function checks has
its own faults (on the host, wrong dtype, not contiguous, wrong shape, too
few elements, as far as each can be made), 468 in all.  For PAIRED every two
of a function's faults that are about different arguments are made at once
(1188 pairs of flow_bidir_device's 51 faults, 231 of flow_interp_bgr_device's
22) and kept as the one order of the call's checks that all pairs agree with
(check_order).

Rendering of a pointer: "<buffer>+<offset>", resolved after the call against
the case's named arguments and then against what the call returned ("ret...").
"workspace" is the workspace, given or defaulted; its size is the next
argument.  "copy(I0)+0" is a temporary whose first row holds the first row of
the copy the case says the binding must make of I0 (a widened or re-strided
frame).  A pointer that resolves to nothing raises here.

Frames are 16 x 20 (rows != cols, so a swap shows); the device half runs under
a side stream, so the current stream is not the null stream.
"""
from __future__ import annotations

import ctypes
import itertools
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
TABLE = os.path.join(HERE, "py_calls.json")

R, C = 16, 20
CTX = 0x7C7C0000          # the handle the recorder's hsflow_create hands out
POINTER_MIN = 1 << 20     # integers from here on must resolve to a buffer
SOLVE = dict(levels=2, warps=3, window=5, iters=7, alpha=1.5)
FORWARDED = ("hsflow_workspace_bytes", "hsflow_pyramid_workspace_bytes",
             "hsflow_flow_bidir_workspace_bytes", "hsflow_flow_interp_workspace_bytes",
             "hsflow_flow_interp_bgr_workspace_bytes", "hsflow_prefilter_planes_bytes",
             "hsflow_pyramid_level_size", "hsflow_status_string")
BYTES = ("hsflow_last_error", "hsflow_jacobi_kernel_name")  # char* results

# names of hsflow that are no entry points: constants, types whose methods are
# keyed on their own ("Context.flow"), imports, and the loader
NOT_CALLS = """
    HSFLOW_OK HSFLOW_ERR_ARG HSFLOW_ERR_HIP HSFLOW_ERR_OOM HSFLOW_ERR_NODEV HSFLOW_ERR_SIZE
    U8 F32 F64 F16 MAX_LEVELS MAX_WARPS SOBEL_GAIN CONSISTENT INCONSISTENT OUT_OF_FRAME
    CONSISTENCY_REL CONSISTENCY_ABS MEDIAN_SIZES MAX_TIMES FLAG_I0_OUT FLAG_I1_OUT
    FLAG_FWD_FAILED FLAG_BWD_FAILED EXPORTS PREFILTER_NONE PREFILTER_HIGHPASS
    PREFILTER_NORMALIZE PREFILTER_MAX_RADIUS SMOOTH_QUADRATIC SMOOTH_FLOW_DRIVEN LIB_PATH
    Prefilter Smoothness BidirHost BidirDevice HsflowError Context hornSchunck
    annotations collections contextlib ctypes math os subprocess np torch build lib
""".split()


def _hsflow():
    pkg = os.path.join(ROOT, "cpp-optical-flow_amd")
    if pkg not in sys.path:
        sys.path.insert(0, pkg)
    import hsflow
    return hsflow


def entry_points(hs):
    """Every public callable of hsflow that reaches lib(), as the table keys them."""
    names = [n for n in dir(hs) if not n.startswith("_") and n not in NOT_CALLS]
    for cls in (hs.Context, hs.hornSchunck):
        names += [f"{cls.__name__}.{n}" for n, m in vars(cls).items()
                  if not n.startswith("_") and callable(m)]
    return sorted(names)


# ------------------------------------------------------------------ the recorder
class Recorder:
    def __init__(self, real, copies=()):
        self.real, self.calls, self.copies = real, [], dict(copies)
        self.settings = {"prefilter": {}, "smoothness": {}}

    def __getattr__(self, name):
        if name.startswith("_"):
            raise AttributeError(name)
        if name in FORWARDED:
            return getattr(self.real, name)

        def call(*args):
            kind = name.rsplit("_", 1)[-1]
            if name == "hsflow_create":
                args[0]._obj.value = CTX
            elif name.startswith("hsflow_ctx_set_"):
                s = args[1]._obj if args[1] is not None else None
                self.settings[kind] = {f: getattr(s, f) for f, _ in s._fields_} if s else {}
            elif name.startswith("hsflow_ctx_"):
                for f, _ in args[1]._obj._fields_:
                    setattr(args[1]._obj, f, self.settings[kind].get(f, 0))
            self.calls.append((name, [self._freeze(k, a, args) for k, a in enumerate(args)]))
            return b"" if name in BYTES else 0
        return call

    def _freeze(self, k, a, args):
        """Everything that may be gone or changed after the call, as plain Python."""
        if isinstance(a, ctypes.c_void_p):
            return ("handle", a.value)
        if isinstance(a, ctypes.Array):
            if a._type_ is ctypes.c_void_p:
                return ("pointers", list(a))
            return ("values", [repr(x) for x in a])
        if hasattr(a, "_obj"):  # byref
            o = a._obj
            if isinstance(o, ctypes.Structure):
                return ("struct", {f: repr(getattr(o, f)) for f, _ in o._fields_})
            return ("values", "out")
        # a host frame the binding had to copy: first row against the expected copy
        if k in (1, 2) and isinstance(a, int) and isinstance(args[0], ctypes.c_void_p):
            for name, want in self.copies.items():
                row = want[0].tobytes()
                if ctypes.string_at(a, len(row)) == row:
                    return ("copy", name)
        return a


def _is_buffer(x):
    return isinstance(x, np.ndarray) or type(x).__module__.startswith("torch") and \
        hasattr(x, "data_ptr")


def _span(x):
    if isinstance(x, np.ndarray):
        lo = x.ctypes.data
        return lo, lo + sum((n - 1) * s for n, s in zip(x.shape, x.strides)) + x.itemsize \
            if x.size else lo
    if not x.is_contiguous():
        return 0, 0
    return x.data_ptr(), x.data_ptr() + x.numel() * x.element_size()


def _inside(p, x):
    lo, hi = _span(x)
    return lo <= p < hi


def _named(prefix, x, out):
    if _is_buffer(x):
        out.append((prefix, x))
    elif isinstance(x, (tuple, list)) and not hasattr(x, "mode"):
        for k, y in enumerate(x):
            _named(f"{prefix}.{x._fields[k] if hasattr(x, '_fields') else k}", y, out)
    return out


def _describe(x):
    dt = str(x.dtype).replace("torch.", "")
    return f"{dt}{list(x.shape)}"


class Renderer:
    def __init__(self, kwargs, ret, streams):
        self.bufs = []
        for k, v in kwargs.items():
            _named(k, v, self.bufs)
        self.n_in = len(self.bufs)
        _named("ret", ret, self.bufs)
        self.streams = streams      # {"current": ptr, "given": ptr or None}
        self.ws_default = "workspace" not in kwargs or kwargs["workspace"] is None

    def pointer(self, p, bufs=None):
        for name, x in (self.bufs if bufs is None else bufs):
            if _inside(p, x):
                off = p - _span(x)[0]
                return "workspace" if name == "workspace" and not off else f"{name}+{off}"
        return None

    def call(self, name, args):
        out, unresolved = [], []
        for k, a in enumerate(args):
            if isinstance(a, tuple):
                tag, v = a
                if tag == "handle":
                    assert v == CTX, (name, k, v)
                    v = "ctx"
                elif tag == "pointers":
                    v = [self._int(name, k, p, unresolved) for p in v]
                elif tag == "copy":
                    v = f"copy({v})+0"
                out.append(v)
            else:
                out.append(self._int(name, k, a, unresolved))
        # the one pointer nothing names: a defaulted workspace, its size the next argument
        for k in unresolved:
            ok = self.ws_default and len(unresolved) == 1 and k + 1 < len(args) and \
                isinstance(args[k + 1], int)
            if not ok:
                raise RuntimeError(f"{name}: argument {k} = {args[k]} resolves to nothing")
            out[k], out[k + 1] = "workspace", repr(args[k + 1])
        return [name, out]

    def _int(self, name, k, a, unresolved):
        if a is None or not isinstance(a, int) or isinstance(a, bool):
            return a if a is None else repr(a)
        for label, s in self.streams.items():
            if s is not None and a == s and s >= POINTER_MIN:
                return label
        p = self.pointer(a)
        if p is not None:
            return p
        if a >= POINTER_MIN and not unresolved_size(k, unresolved):
            unresolved.append(k)
        return repr(a)

    def returned(self, ret):
        if _is_buffer(ret):
            p = _span(ret)[0]
            where = self.pointer(p, self.bufs[:self.n_in])
            return _describe(ret) + (f" @{where}" if where else "")
        if isinstance(ret, (tuple, list)) and not hasattr(ret, "mode"):
            return [self.returned(x) for x in ret]
        return None if ret is None else repr(ret)


def unresolved_size(k, unresolved):
    """argument k is the size that follows an unresolved (workspace) pointer"""
    return bool(unresolved) and unresolved[-1] == k - 1


def _target(hs, ctx, key):
    if key.startswith("Context."):
        return getattr(ctx, key.split(".")[1])
    if key.startswith("hornSchunck."):
        return getattr(hs.hornSchunck(5, 7, 1.5, context=ctx), key.split(".")[1])
    return getattr(hs, key)


def record(hs, key, kwargs, copies=(), use=None):
    """One case: `key` called with `kwargs` under a recorder -> its table entry.
    `use` (hs, ctx, **kwargs) replaces the plain call for cases in several steps."""
    real = hs.lib() if not isinstance(hs._lib, Recorder) else hs._lib.real
    rec = Recorder(real, copies)
    saved = hs._lib, hs._default_ctx
    hs._lib, hs._default_ctx = rec, None
    streams = {"current": None, "given": None}
    entry = {}
    try:
        ctx = hs.Context(0)
        if any(_is_buffer(v) and not isinstance(v, np.ndarray) and v.is_cuda
               for _, v in _named("", list(kwargs.values()), [])):
            import torch
            streams["current"] = torch.cuda.current_stream().cuda_stream
            assert streams["current"] >= POINTER_MIN, "run the device half under a side stream"
        if kwargs.get("stream") is not None:
            streams["given"] = kwargs["stream"].cuda_stream
        del rec.calls[:]
        ret = None
        try:
            ret = use(hs, ctx, **kwargs) if use else _target(hs, ctx, key)(**kwargs)
        except hs.HsflowError as e:
            entry["error"] = [e.status, str(e)]
        calls = list(rec.calls)
        r = Renderer(kwargs, ret, streams)
        entry["calls"] = [r.call(n, a) for n, a in calls]
        if "error" not in entry:
            entry["returns"] = r.returned(ret)
    finally:
        # under the recorder still: the real hsflow_destroy must never see CTX
        for c in (locals().get("ctx"), hs._default_ctx):
            if c is not None:
                c.close()
        hs._lib, hs._default_ctx = saved
    return entry


# ------------------------------------------------------------------ host cases
def _rng_frames():
    rng = np.random.default_rng(7)
    return (rng.integers(1, 255, (R, C)).astype(np.uint8),
            rng.integers(1, 255, (R, C)).astype(np.uint8),
            rng.integers(1, 255, (R, C + 8)).astype(np.uint8),
            rng.integers(1, 255, (R, 2 * C)).astype(np.uint8))


def _options(hs):
    return {"median=5": dict(median=5), "prefilter=Prefilter(2)": dict(prefilter=hs.Prefilter(2)),
            "prefilter=tuple": dict(prefilter=(1, 2.0, 4.0, 32.0)),
            "smoothness=Smoothness()": dict(smoothness=hs.Smoothness()),
            "all three": dict(median=5, prefilter=hs.Prefilter(2), smoothness=hs.Smoothness())}


def host_cases(hs):
    """key -> case name -> dict(kwargs=, copies=, use=)."""
    a8, b8, wide, wide2 = _rng_frames()
    forms = {
        "uint8": (a8, b8, {}),
        "float16": (a8.astype(np.float16), b8.astype(np.float16), {}),
        "uint8+float32": (a8, b8.astype(np.float32),
                          {"I0": a8.astype(np.float64), "I1": b8.astype(np.float64)}),
        "column slice": (a8, wide[:, 3:3 + C], {}),
        "column stride 2": (wide2[:, ::2], b8, {"I0": np.ascontiguousarray(wide2[:, ::2])}),
    }
    cases = {}

    def add(key, name, copies=(), use=None, **kw):
        assert name not in cases.setdefault(key, {}), (key, name)
        cases[key][name] = dict(kwargs=kw, copies=copies, use=use)

    times3 = [0.25, 0.5, 0.75]
    grey = {"Context.flow": dict(window=5, iters=7, alpha=1.5),
            "Context.flow_pyramid": dict(levels=2, window=5, iters=7, alpha=1.5),
            "Context.flow_warped": SOLVE, "Context.flow_bidir": SOLVE,
            "Context.interpolate": dict(times=times3, **SOLVE), "Context.gradients": {}}
    for key, base in grey.items():
        for form, (I0, I1, copies) in forms.items():
            add(key, form, copies, I0=I0, I1=I1, **base)
        add(key, "out_dtype=float32", I0=a8, I1=b8, out_dtype=np.float32, **base)
        # errors
        add(key, "I0 3-D", I0=np.zeros((R, C, 3), np.uint8), I1=b8, **base)
        add(key, "I1 1-D", I0=a8, I1=np.zeros(C, np.uint8), **base)
        add(key, "sizes differ", I0=a8, I1=wide, **base)
        add(key, "int32 frames", I0=a8.astype(np.int32), I1=b8.astype(np.int32), **base)
    for key in ("Context.flow_warped", "Context.flow_bidir", "Context.interpolate"):
        for name, opt in _options(hs).items():
            add(key, name, I0=a8, I1=b8, **grey[key], **opt)

    f64 = lambda *s: np.empty(s, np.float64)  # noqa: E731
    add("Context.flow", "out reusable", I0=a8, I1=b8, out=(f64(R, C), f64(R, C)),
        **grey["Context.flow"])
    same = f64(R, C)
    for name, out in (("out float32", (np.empty((R, C), np.float32), f64(R, C))),
                      ("out wrong shape", (f64(C, R), f64(R, C))),
                      ("out a column slice", (f64(R, C + 2)[:, :C], f64(R, C))),
                      ("out twice the same", (same, same)), ("out lists", ([0], [0]))):
        add("Context.flow", name, I0=a8, I1=b8, out=out, **grey["Context.flow"])
    add("Context.flow", "out float32 reusable", I0=a8, I1=b8, out_dtype=np.float32,
        out=(np.empty((R, C), np.float32), np.empty((R, C), np.float32)), **grey["Context.flow"])

    bid = dict(I0=a8, I1=b8, **SOLVE)
    add("Context.flow_bidir", "thresholds", rel=0.02, abs=0.75, **bid)
    add("Context.flow_bidir", "padded out and mask_out", out=f64(4, R, C + 4),
        mask_out=np.empty((2, R, C + 12), np.uint8), **bid)
    add("Context.flow_bidir", "float32 out", out=np.empty((4, R, C), np.float32), **bid)
    for off in ("backward", "masks", "counts"):
        add("Context.flow_bidir", f"{off}=False", **bid, **{off: False})
    for name, out in (("out 3 planes", f64(3, R, C)), ("out too narrow", f64(4, R, C - 1)),
                      ("out rows", f64(4, R + 1, C)), ("out 2-D", f64(R, C)),
                      ("out int32", np.empty((4, R, C), np.int32)),
                      ("out column stride", f64(4, R, 2 * C)[:, :, ::2])):
        add("Context.flow_bidir", name, out=out, **bid)
    for name, m in (("mask_out 1 plane", np.empty((1, R, C), np.uint8)),
                    ("mask_out float32", np.empty((2, R, C), np.float32)),
                    ("mask_out too narrow", np.empty((2, R, C - 1), np.uint8)),
                    ("mask_out column stride", np.empty((2, R, 2 * C), np.uint8)[:, :, ::2])):
        add("Context.flow_bidir", name, mask_out=m, **bid)
    add("Context.flow_bidir", "bad out and bad mask_out", out=f64(3, R, C),
        mask_out=np.empty((1, R, C), np.uint8), **bid)

    rng = np.random.default_rng(11)
    padded = rng.integers(0, 255, (2, R, C + 5, 3)).astype(np.uint8)
    c0, c1 = padded[0, :, :C], padded[1, :, :C]
    d0, d1 = np.ascontiguousarray(c0), np.ascontiguousarray(c1)
    itp = {"Context.interpolate": (dict(I0=a8, I1=b8, **SOLVE), (np.uint8, np.float32, np.float64)),
           "Context.interpolate_bgr": (dict(bgr0=d0, bgr1=d1, **SOLVE), (np.uint8, np.float32))}
    for key, (base, dtypes) in itp.items():
        for times, flags, dt in itertools.product((0.5, times3), (False, True), dtypes):
            add(key, f"times={times} with_flags={flags} {np.dtype(dt).name}", times=times,
                with_flags=flags, out_dtype=dt, **base)
        add(key, "thresholds", times=0.5, rel=0.02, abs=0.75, **base)
        add(key, "out_dtype=float16", times=0.5, out_dtype=np.float16, **base)
    add("Context.interpolate_bgr", "out_dtype=float64", times=0.5, out_dtype=np.float64,
        **itp["Context.interpolate_bgr"][0])
    for name, opt in _options(hs).items():
        add("Context.interpolate_bgr", name, times=times3, **itp["Context.interpolate_bgr"][0], **opt)
    bgr = {"Context.interpolate_bgr": dict(times=0.5, **SOLVE),
           "Context.flow_bgr": dict(window=5, iters=7, alpha=1.5)}
    for key, base in bgr.items():
        add(key, "padded rows", bgr0=c0, bgr1=c1, **base)
        add(key, "dense and padded", bgr0=d0, bgr1=c1, **base)
        add(key, "grey frame", bgr0=a8, bgr1=d1, **base)
        add(key, "float32 frame", bgr0=d0, bgr1=d1.astype(np.float32), **base)
        add(key, "4 channels", bgr0=np.zeros((R, C, 4), np.uint8), bgr1=d1, **base)
        add(key, "sizes differ", bgr0=d0, bgr1=padded[1, :, :C + 1], **base)
        add(key, "grey frame and sizes differ", bgr0=d0, bgr1=np.zeros((R + 1, C), np.uint8), **base)
    add("Context.flow_bgr", "out_dtype=float32", bgr0=d0, bgr1=d1, out_dtype=np.float32,
        **bgr["Context.flow_bgr"])

    P, S = hs.Prefilter(2, 3.0), hs.Smoothness(1, 0.2)
    add("Context.set_prefilter", "Prefilter", prefilter=P)
    add("Context.set_prefilter", "tuple", prefilter=(1, 2.0, 4.0, 32.0))
    add("Context.set_prefilter", "None")
    add("Context.prefilter", "off")
    add("Context.prefilter", "after set", use=lambda hs, ctx: (ctx.set_prefilter(P), ctx.prefilter())[1])
    add("Context.set_smoothness", "Smoothness", smoothness=S)
    add("Context.set_smoothness", "tuple", smoothness=(1, 0.25))
    add("Context.set_smoothness", "None")
    add("Context.smoothness", "off")
    add("Context.smoothness", "after set",
        use=lambda hs, ctx: (ctx.set_smoothness(S), ctx.smoothness())[1])
    add("Context.flow_warped", "per-call options over the context's own", I0=a8, I1=b8,
        use=lambda hs, ctx, **kw: (ctx.set_prefilter(P), ctx.set_smoothness(S),
                                   ctx.flow_warped(prefilter=hs.Prefilter(1), **kw, **SOLVE))[2])
    add("Context.close", "close")
    add("Context.close", "twice", use=lambda hs, ctx: (ctx.close(), ctx.close())[1])
    add("default_context", "twice the same",
        use=lambda hs, ctx: hs.default_context() is hs.default_context())

    for form, (I0, I1, copies) in forms.items():
        add("hornSchunck.getFlow", form, copies, imagePrev=I0, imageNext=I1)
        add("hornSchunck.getGradients", form, copies, imagePrev=I0, imageNext=I1)
    add("hornSchunck.getFlow", "u, v reusable", imagePrev=a8, imageNext=b8, u=f64(R, C), v=f64(R, C))
    add("hornSchunck.getFlow", "u float32", imagePrev=a8, imageNext=b8,
        u=np.empty((R, C), np.float32), v=f64(R, C))
    add("hornSchunck.getFlow", "u only", imagePrev=a8, imageNext=b8, u=f64(R, C))
    add("hornSchunck.getFlow", "sizes differ", imagePrev=a8, imageNext=wide)
    add("hornSchunck.getGradients", "gradX given", imagePrev=a8, imageNext=b8, gradX=f64(R, C))
    add("hornSchunck.getGradients", "sizes differ", imagePrev=a8, imageNext=wide)

    cmp_ = dict(I0=a8, I1=b8, alpha=1.5, nIter=7)
    add("compute", "plain", **cmp_)
    add("compute", "windowSize=3", windowSize=3, **cmp_)
    add("compute", "levels=3", levels=3, **cmp_)
    add("compute", "warps=2", warps=2, levels=3, **cmp_)
    add("compute", "warps=2 levels=1", warps=2, **cmp_)
    for name, opt in _options(hs).items():
        add("compute", f"warps=2 {name}", warps=2, levels=2, **cmp_, **opt)
        add("compute", f"no warps {name}", levels=2, **cmp_, **opt)
    add("compute", "warps=17", warps=17, **cmp_)
    add("compute", "warps=-1", warps=-1, **cmp_)
    add("compute", "sizes differ", I0=a8, I1=wide, alpha=1.5, nIter=7)

    multi = dict(devices=[0, 1], window=5, iters=7, alpha=1.5)
    add("flow_multi", "three pairs", pairs=[(a8, b8), (b8, a8), (a8.copy(), b8.copy())], **multi)
    add("flow_multi", "float32 out", pairs=[(a8, b8)], out_dtype=np.float32, **multi)
    add("flow_multi", "column slices", pairs=[(a8, wide[:, :C]), (b8, wide[:, 8:])], **multi)
    add("flow_multi", "no pairs", pairs=[], **multi)
    add("flow_multi", "sizes differ", pairs=[(a8, b8), (a8, wide)], **multi)
    add("flow_multi", "dtypes differ", pairs=[(a8, b8), (a8, b8.astype(np.float32))], **multi)
    add("flow_multi", "row steps differ", pairs=[(a8, b8), (a8, wide[:, :C])], **multi)
    add("flow_multi", "3-D frame", pairs=[(d0, b8)], **multi)
    add("flow_multi_release", "release")

    add("bgr_to_gray", "dense", bgr=d0)
    add("bgr_to_gray", "grey frame", bgr=a8)
    add("bgr_to_gray", "4 channels", bgr=np.zeros((R, C, 4), np.uint8))
    add("synth_pair", "float32", seed=1000, rows=R, cols=C)
    add("synth_pair", "uint8", seed=1001, rows=R, cols=C, qdy=1, qdx=-2, dtype=np.uint8)
    add("synth_pair", "float64", seed=1000, rows=R, cols=C, dtype=np.float64)

    # settings and queries: one call each
    shape = dict(rows=R, cols=C, batch=2)
    add("build_flags", "call")
    add("is_probe_build", "call")
    add("strip_seg_rows", "call", window=3, **shape)
    add("strip_seg_rows", "defaults", rows=R, cols=C)
    add("set_output_hugepages", "on", on=True)
    add("set_output_hugepages", "off", on=False)
    add("workspace_bytes", "call", **shape)
    add("workspace_bytes", "batch defaulted", rows=R, cols=C)
    add("pyramid_level_size", "call", rows=R, cols=C, level=1)
    add("pyramid_level_size", "level 9", rows=R, cols=C, level=9)
    for name in ("pyramid_workspace_bytes", "bidir_workspace_bytes", "flow_interp_workspace_bytes",
                 "flow_interp_bgr_workspace_bytes"):
        add(name, "call", levels=3, **shape)
    add("prefilter_planes_bytes", "call", **shape)
    add("prefilter_planes_bytes", "batch defaulted", rows=R, cols=C)
    add("set_interp_bgr_loads", "wide", wide=True)
    add("set_iters_per_launch", "call", k=4)
    add("set_max_streams", "call", n=3)
    add("max_streams", "call")
    add("max_streams_as", "with", use=lambda hs, ctx: _with(hs.max_streams_as(3)))
    add("set_first_pass_fusion", "off", on=False)
    add("set_first_pass_fusion", "truthy", on=2)
    add("first_pass_fusion", "call")
    add("first_pass_launches", "call")
    add("first_pass_fusion_as", "with", use=lambda hs, ctx: _with(hs.first_pass_fusion_as(True)))
    add("set_jacobi_kernel", "call", k=4)
    add("set_strip_rows", "call", seg_rows=48)
    add("set_strip_rows", "default")
    add("jacobi_kernel_name", "call", window=5, **shape)
    add("iters_per_launch", "call", window=5, **shape)
    return cases


def _with(manager):
    with manager:
        pass


# ------------------------------------------------------------------ device cases
# every entry point that takes a tensor: only the device half can record it
DEVICE_KEYS = ("flow_device", "flow_pyramid_device", "flow_warped_device", "consistency_device",
               "median_device", "flow_bidir_device", "warp_image_device", "frame_interp_device",
               "flow_interp_device", "warp_image_bgr_device", "frame_interp_bgr_device",
               "flow_interp_bgr_device", "prefilter_device", "warp_gradients_device",
               "pyramid_build_device", "upflow_device", "gradients_device", "jacobi_device",
               "diffusivity_device", "jacobi_weighted_device", "bgr_to_gray_device",
               "download_device", "alloc_workspace")
PAIRED = ("flow_bidir_device", "flow_interp_bgr_device")


def device_cases(hs, torch):
    """key -> case name -> dict(kwargs=); and key -> fault name -> overrides of
    the key's "base" case, for the errors and PAIRED's pairs of them."""
    dev = torch.device("cuda", torch.cuda.current_device())
    u8, f16, f32, f64, i32 = torch.uint8, torch.float16, torch.float32, torch.float64, torch.int32
    E = lambda dt, *s: torch.empty(s, dtype=dt, device=dev)  # noqa: E731
    given = torch.cuda.Stream(dev)
    cases, faults = {}, {}

    def add(key, name, **kw):
        assert name not in cases.setdefault(key, {}), (key, name)
        cases[key][name] = dict(kwargs=kw, copies=(), use=None)

    def pair(lead=(2,), dt=u8):
        return dict(I0=E(dt, *lead, R, C), I1=E(dt, *lead, R, C))

    def bgrs(lead=(2,)):
        return dict(bgr0=E(u8, *lead, R, C, 3), bgr1=E(u8, *lead, R, C, 3))

    def flows(lead=(2,), names=("uf", "vf", "ub", "vb")):
        return {n: E(f32, *lead, R, C) for n in names}

    def common(key, base, leads=((2,), ()), dtypes=(f16, f32, f64), workspace=True):
        """The cases every entry point gets: base(lead, dtype) -> kwargs."""
        add(key, "base", **base((2,), u8))
        for lead in leads[1:]:
            add(key, f"lead {list(lead)}", **base(lead, u8))
        for dt in dtypes:
            add(key, str(dt), **base((2,), dt))
        add(key, "stream given", stream=given, **base((2,), u8))
        if workspace:
            add(key, "workspace given", workspace=E(u8, 1 << 19), **base((2,), u8))

    def frame_faults(names, shape=(2, R, C), dt=u8, bgr=False):
        """One bad frame at a time, and the second frame against the first."""
        f = {}
        for n in names:
            f[f"{n} on the host"] = {n: torch.empty(shape, dtype=dt)}
            f[f"{n} not contiguous"] = {n: E(dt, *shape[:-1], 2 * shape[-1])[..., ::2]}
        n = names[-1]
        wider = shape[:2] + (C + 1,) + shape[3:] if bgr else shape[:-1] + (C + 1,)
        f[f"{n} wider"] = {n: E(dt, *wider)}
        if len(names) == 2:
            f[f"{n} another batch"] = {n: E(dt, 3, *shape[1:])}
            f[f"{n} float32"] = {n: E(f32, *shape)}
        return f

    def plane_faults(names, shape=(2, R, C), sets_batch=None):
        """sets_batch: the plane whose own shape is the call's, so it cannot be short."""
        f = {}
        for n in names:
            f[f"{n} on the host"] = {n: torch.empty(shape)}
            f[f"{n} float64"] = {n: E(f64, *shape)}
            f[f"{n} not contiguous"] = {n: E(f32, *shape[:-1], 2 * shape[-1])[..., ::2]}
            f[f"{n} one plane short"] = {n: E(f32, *shape[1:])}
            f[f"{n} transposed shape"] = {n: E(f32, shape[0], shape[2], shape[1])}
        f.pop(f"{sets_batch} one plane short", None)
        return f

    def output_faults(names, shape, dt):
        f = {}
        for n in names:
            f[f"{n} on the host"] = {n: torch.empty(shape, dtype=dt)}
            f[f"{n} wrong dtype"] = {n: E(f64, *shape)}
            f[f"{n} wrong shape"] = {n: E(dt, *shape, 2)}
            f[f"{n} not contiguous"] = {n: E(dt, *shape[:-1], 2 * shape[-1])[..., ::2]}
        return f

    opts = _options(hs)
    four = ("uf", "vf", "ub", "vb")
    three = ((2,), (), (2, 3))

    # the plain solves
    solves = {"flow_device": dict(window=5, iters=7, alpha=1.5),
              "flow_pyramid_device": dict(levels=2, window=5, iters=7, alpha=1.5),
              "flow_warped_device": SOLVE}
    for key, par in solves.items():
        common(key, lambda lead, dt, par=par: dict(**pair(lead, dt), **par),
               leads=three if key == "flow_device" else three[:2])
        add(key, "u, v given", **pair(), **flows(names=("u", "v")), **par)
        add(key, "u given", **pair(), u=E(f32, 2, R, C), **par)
        add(key, "u, v larger batch", **pair(), u=E(f32, 4, R, C), v=E(f32, 3, R, C), **par)
        faults[key] = {**frame_faults(("I0", "I1")), **plane_faults(("u", "v"))}
    for name, opt in opts.items():
        add("flow_warped_device", name, **pair(), **SOLVE, **opt)
    add("flow_warped_device", "prefilter off", **pair(), prefilter=hs.Prefilter(0), **SOLVE)

    # consistency, median, diffusivity: planes in, planes out
    common("consistency_device", lambda lead, dt: dict(**flows(lead), mask=True), dtypes=(),
           workspace=False)
    full = dict(err=True, mask=True, counts=True)
    add("consistency_device", "all three", **flows(), **full)
    add("consistency_device", "all three, one plane", **flows(()), **full)
    add("consistency_device", "tensors", **flows(), err=E(f32, 2, R, C), mask=E(u8, 2, R, C),
        counts=E(i32, 2, 3), rel=0.02, abs=0.75)
    add("consistency_device", "False", **flows(), err=False, mask=True, counts=None)
    faults["consistency_device"] = {
        **plane_faults(four, sets_batch="uf"),
        **output_faults(("err",), (2, R, C), f32),
        **output_faults(("mask",), (2, R, C), u8), **output_faults(("counts",), (2, 3), i32)}
    common("median_device", lambda lead, dt: dict(**flows(lead, ("u", "v")), ksize=3), dtypes=(),
           workspace=False)
    add("median_device", "outputs given", **flows(names=("u", "v", "u_out", "v_out")), ksize=5)
    add("median_device", "v_out given", **flows(names=("u", "v", "v_out")), ksize=5)
    faults["median_device"] = plane_faults(("u", "v", "u_out", "v_out"), sets_batch="u")
    common("diffusivity_device", lambda lead, dt: dict(**flows(lead, ("u", "v")), lam=0.3),
           dtypes=(), workspace=False)
    add("diffusivity_device", "g given", **flows(names=("u", "v", "g")), lam=0.2)
    faults["diffusivity_device"] = plane_faults(("u", "v", "g"), sets_batch="u")

    # the bidirectional solve
    key = "flow_bidir_device"
    common(key, lambda lead, dt: dict(**pair(lead, dt), **SOLVE))
    add(key, "flows given", **pair(), **flows(), rel=0.02, abs=0.75, **SOLVE)
    add(key, "ub, vb given", **pair(), **flows(names=("ub", "vb")), **SOLVE)
    six = ("err_f", "mask_f", "counts_f", "err_b", "mask_b", "counts_b")
    add(key, "every check output", **pair(), **{n: True for n in six}, **SOLVE)
    add(key, "every check output, one plane", **pair(()), **{n: True for n in six}, **SOLVE)
    add(key, "no check output", **pair(), mask_f=None, **SOLVE)
    add(key, "backward outputs only", **pair(), mask_f=False, err_b=True, mask_b=True,
        counts_b=True, **SOLVE)
    add(key, "check outputs as tensors", **pair(), **SOLVE,
        **{n: E(i32, 2, 3) if n[0] == "c" else E(f32 if n[0] == "e" else u8, 2, R, C) for n in six})
    for name, opt in opts.items():
        add(key, name, **pair(), **SOLVE, **opt)
    faults[key] = {**frame_faults(("I0", "I1")), **plane_faults(four),
                   **output_faults(("err_f", "err_b"), (2, R, C), f32),
                   **output_faults(("mask_f", "mask_b"), (2, R, C), u8),
                   **output_faults(("counts_f", "counts_b"), (2, 3), i32)}

    # warps and interpolation of grey frames
    key = "warp_image_device"
    common(key, lambda lead, dt: dict(I=E(dt, *lead, R, C), **flows(lead, ("u", "v"))), leads=three,
           workspace=False)
    add(key, "out given, oof=True", I=E(u8, 2, R, C), **flows(names=("u", "v", "out")), oof=True)
    add(key, "oof given", I=E(u8, 2, R, C), **flows(names=("u", "v")), oof=E(u8, 2, R, C))
    add(key, "oof=False", I=E(u8, 2, R, C), **flows(names=("u", "v")), oof=False)
    faults[key] = {**frame_faults(("I",)), **plane_faults(("u", "v", "out")),
                   **output_faults(("oof",), (2, R, C), u8)}

    times3 = [0.25, 0.5, 0.75]

    def interp_cases(key, base, trailing):
        shape = lambda nt: (2, nt, R, C) + trailing  # noqa: E731
        common(key, base, dtypes=() if trailing else (f16, f32, f64),
               workspace="flow_interp" in key)
        add(key, "one time", **{**base((2,), u8), "times": 0.5})
        add(key, "one time, one frame", **{**base((), u8), "times": 0.5}, flags=True, trusted=True)
        add(key, "out_dtype=uint8", out_dtype=u8, **base((2,), u8))
        add(key, "flags and trusted", flags=True, trusted=True, **base((2,), u8))
        add(key, "flags=False", flags=False, trusted=None, **base((2,), u8))
        add(key, "outputs as tensors", out=E(u8, *shape(3)), flags=E(u8, 2, 3, R, C),
            trusted=E(i32, 2, 3), **base((2,), u8))
        add(key, "out float32 tensor", out=E(f32, *shape(3)), out_dtype=u8, **base((2,), u8))
        return {"out float64": dict(out=E(f64, *shape(3))), "out_dtype=float64": dict(out_dtype=f64),
                "out for two times": dict(out=E(f32, *shape(2))),
                **output_faults(("out",), shape(3), f32),
                **output_faults(("flags",), (2, 3, R, C), u8),
                **output_faults(("trusted",), (2, 3), i32)}

    def masks(lead=(2,)):
        return dict(mask_f=E(u8, *lead, R, C), mask_b=E(u8, *lead, R, C))

    key = "frame_interp_device"
    f = interp_cases(key, lambda lead, dt: dict(**pair(lead, dt), **flows(lead), times=times3), ())
    add(key, "masks", **pair(), **flows(), **masks(), times=times3)
    add(key, "mask_b only", **pair(), **flows(), mask_b=E(u8, 2, R, C), times=times3)
    faults[key] = {**frame_faults(("I0", "I1")), **plane_faults(four),
                   **output_faults(("mask_f", "mask_b"), (2, R, C), u8), **f}
    key = "flow_interp_device"
    f = interp_cases(key, lambda lead, dt: dict(**pair(lead, dt), times=times3, **SOLVE), ())
    add(key, "thresholds", **pair(), times=times3, rel=0.02, abs=0.75, **SOLVE)
    for name, opt in opts.items():
        add(key, name, **pair(), times=times3, **SOLVE, **opt)
    faults[key] = {**frame_faults(("I0", "I1")), **f}

    # colour frames
    key = "warp_image_bgr_device"
    common(key, lambda lead, dt: dict(bgr=E(u8, *lead, R, C, 3), **flows(lead, ("u", "v"))),
           dtypes=(), workspace=False)
    wb = dict(bgr=E(u8, 2, R, C, 3), **flows(names=("u", "v")))
    add(key, "out_dtype=uint8, oof=True", out_dtype=u8, oof=True, **wb)
    add(key, "out and oof given", out=E(u8, 2, R, C, 3), oof=E(u8, 2, R, C), **wb)
    add(key, "out float32 given", out=E(f32, 2, R, C, 3), out_dtype=u8, **wb)
    faults[key] = {**frame_faults(("bgr",), (2, R, C, 3), bgr=True),
                   "bgr float32": dict(bgr=E(f32, 2, R, C, 3)), "bgr grey": dict(bgr=E(u8, 2, R, C)),
                   "bgr 5-D": dict(bgr=E(u8, 2, 2, R, C, 3)),
                   "bgr an array": dict(bgr=np.zeros((R, C, 3), np.uint8)),
                   **plane_faults(("u", "v")), "out float64": dict(out=E(f64, 2, R, C, 3)),
                   "out_dtype=float64": dict(out_dtype=f64),
                   **output_faults(("out",), (2, R, C, 3), f32),
                   **output_faults(("oof",), (2, R, C), u8)}
    bgr_faults = {**frame_faults(("bgr0", "bgr1"), (2, R, C, 3), bgr=True),
                  "bgr0 float32": dict(bgr0=E(f32, 2, R, C, 3)), "bgr1 grey": dict(bgr1=E(u8, 2, R, C)),
                  "bgr1 4 channels": dict(bgr1=E(u8, 2, R, C, 4))}
    del bgr_faults["bgr1 float32"]
    key = "frame_interp_bgr_device"
    f = interp_cases(key, lambda lead, dt: dict(**bgrs(lead), **flows(lead), times=times3), (3,))
    add(key, "masks", **bgrs(), **flows(), **masks(), times=times3)
    faults[key] = {**bgr_faults, **plane_faults(four),
                   **output_faults(("mask_f", "mask_b"), (2, R, C), u8), **f}
    key = "flow_interp_bgr_device"
    f = interp_cases(key, lambda lead, dt: dict(**bgrs(lead), times=times3, **SOLVE), (3,))
    add(key, "thresholds", **bgrs(), times=times3, rel=0.02, abs=0.75, **SOLVE)
    for name, opt in opts.items():
        add(key, name, **bgrs(), times=times3, **SOLVE, **opt)
    faults[key] = {**bgr_faults, **f}

    key = "bgr_to_gray_device"
    common(key, lambda lead, dt: dict(bgr=E(u8, *lead, R, C, 3)), leads=three, dtypes=(),
           workspace=False)
    add(key, "gray given", bgr=E(u8, 2, R, C, 3), gray=E(u8, 2, R, C))
    add(key, "gray larger", bgr=E(u8, 2, R, C, 3), gray=E(u8, 3 * R * C))
    faults[key] = {**frame_faults(("bgr",), (2, R, C, 3), bgr=True),
                   "bgr float32": dict(bgr=E(f32, 2, R, C, 3)), "bgr 2-D": dict(bgr=E(u8, R, 3)),
                   "bgr grey": dict(bgr=E(u8, 2, R, C)),
                   "gray on the host": dict(gray=torch.empty((2, R, C), dtype=u8)),
                   "gray float32": dict(gray=E(f32, 2, R, C)), "gray short": dict(gray=E(u8, R, C)),
                   "gray not contiguous": dict(gray=E(u8, 2, R, 2 * C)[..., ::2])}
    del faults[key]["bgr wider"]

    # the prefilter and the building blocks
    key = "prefilter_device"
    common(key, lambda lead, dt: dict(I=E(dt, *lead, R, C), prefilter=hs.Prefilter(2)),
           workspace=False)
    add(key, "tuple, out given", I=E(u8, 2, R, C), prefilter=(1, 2.0, 4.0, 32.0), out=E(f32, 2, R, C))
    faults[key] = {**frame_faults(("I",)), "prefilter=None": dict(prefilter=None),
                   **plane_faults(("out",))}
    del faults[key]["I wider"]
    ws = lambda: E(u8, 1 << 19)  # noqa: E731
    key = "warp_gradients_device"
    common(key, lambda lead, dt: dict(**pair(lead, dt), **flows(lead, ("u0", "v0")), workspace=ws()),
           workspace=False)
    add(key, "gx, gy, gt", **pair(), **flows(names=("u0", "v0", "gx", "gy", "gt")), workspace=ws())
    add(key, "gy", **pair(), **flows(names=("u0", "v0", "gy")), workspace=ws())
    faults[key] = {**frame_faults(("I0", "I1")), **plane_faults(("u0", "v0", "gx", "gy", "gt"))}
    key = "gradients_device"
    common(key, lambda lead, dt: dict(**pair(lead, dt), workspace=ws()), workspace=False)
    add(key, "gx, gy, gt", **pair(), **flows(names=("gx", "gy", "gt")), workspace=ws())
    add(key, "gt", **pair(), gt=E(f32, 2, R, C), workspace=ws())
    faults[key] = frame_faults(("I0", "I1"))
    for n in ("I1 another batch", "I1 float32"):
        del faults[key][n]
    key = "pyramid_build_device"
    common(key, lambda lead, dt: dict(**pair(lead, dt), levels=3))
    add(key, "one level", **pair(), levels=1)
    faults[key] = dict(faults["gradients_device"])
    key = "upflow_device"
    up = lambda: dict(uc=E(f32, 8, 10), vc=E(f32, 8, 10), u=E(f32, R, C), v=E(f32, R, C))  # noqa: E731
    add(key, "base", **up())
    add(key, "stream given", stream=given, **up())
    rows = E(f32, R + 4, C)
    add(key, "row slices", **{**up(), "u": rows[2:R + 2], "v": E(f32, 2, R, C)[1]})
    faults[key] = {**plane_faults(("uc", "vc"), (1, 8, 10)), **plane_faults(("u", "v"), (1, R, C))}
    for n in ("uc", "vc", "u", "v"):   # [rows, cols] is the whole of a batch of one
        del faults[key][f"{n} one plane short"]
    jac = lambda: dict(rows=R, cols=C, batch=2, window=5, iters=7, alpha=1.5,  # noqa: E731
                       u=E(f32, 2, R, C), v=E(f32, 2, R, C), workspace=ws())
    key = "jacobi_device"
    add(key, "base", **jac())
    add(key, "warm start", warm_start=True, stream=given, **jac())
    faults[key] = plane_faults(("u", "v"))
    key = "jacobi_weighted_device"
    add(key, "base", g=E(f32, 2, R, C), **jac())
    add(key, "stream given", g=E(f32, 2, R, C), stream=given, **jac())
    faults[key] = plane_faults(("g", "u", "v"))

    key = "download_device"
    pinned = lambda n: torch.empty(n, dtype=u8).pin_memory()  # noqa: E731
    add(key, "base", dst=pinned(4 * R * C), src=E(f32, R, C))
    add(key, "stream given", dst=pinned(4 * R * C), src=E(f32, R, C), stream=given)
    faults[key] = {"sizes differ": dict(dst=pinned(R * C)),
                   "src not contiguous": dict(src=E(f32, R, 2 * C)[:, ::2]),
                   "dst pageable": dict(dst=torch.empty(4 * R * C, dtype=u8)),
                   "dst on the device": dict(dst=E(f32, R, C)),
                   "src on the host": dict(src=torch.empty(R, C))}
    add("alloc_workspace", "call", rows=R, cols=C, batch=2, device=dev)
    return cases, faults


def pairs(faults):
    """Two faults at once, where they are about different arguments."""
    for (a, fa), (b, fb) in itertools.combinations(sorted(faults.items()), 2):
        if not set(fa) & set(fb):
            yield a, b, {**fa, **fb}


def record_all(hs, cases):
    return {key: {name: record(hs, key, **c) for name, c in sorted(named.items())}
            for key, named in sorted(cases.items())}


def record_faults(hs, cases, faults, pairwise=False):
    out = {}
    for key, f in sorted(faults.items()):
        base = cases[key]["base"]["kwargs"]
        todo = ((f"{a} + {b}", both) for a, b, both in pairs(f)) if pairwise else sorted(f.items())
        out[key] = {name: record(hs, key, {**base, **over}) for name, over in todo}
        for name, entry in out[key].items():
            assert "error" in entry, f"{key}: {name} is no fault"
    return out


def pack_errors(entries):
    """name -> entry of cases that all fail before any C call, as the table
    keeps them: [status, text, names], one per distinct error."""
    groups = {}
    for name, e in entries.items():
        assert e["calls"] == [], name
        groups.setdefault(tuple(e["error"]), []).append(name)
    return sorted([status, text, sorted(names)] for (status, text), names in groups.items())


def check_order(single, both):
    """The order of a call's checks, as the table keeps every pair of faults:
    the errors (status, text) such that two faults at once raise the error of
    the one that stands first.  `single`, `both`: record_faults' entries of the
    faults and of their pairs ("a + b").  Errors that no pair tells apart stand
    in the order of their texts; pairs that fit no one order raise."""
    after = {}
    for name, e in both.items():
        ea, eb = (tuple(single[n]["error"]) for n in name.split(" + "))
        got = tuple(e["error"])
        assert e["calls"] == [] and got in (ea, eb), f"{name}: neither fault's own error"
        if ea != eb:
            after.setdefault(got, set()).add(eb if got == ea else ea)
            after.setdefault(eb if got == ea else ea, set())
    order = []
    while after:
        free = sorted(e for e in after if not any(e in later for later in after.values()))
        if not free:
            raise RuntimeError(f"the pairs fit no one order of checks: {sorted(after)}")
        order.append(list(free[0]))
        del after[free[0]]
    return order


def host_half(hs):
    return {"host": record_all(hs, host_cases(hs))}


def device_half(hs, torch):
    with torch.cuda.stream(torch.cuda.Stream()):
        cases, faults = device_cases(hs, torch)
        single = record_faults(hs, cases, faults)
        both = record_faults(hs, cases, {k: faults[k] for k in PAIRED}, pairwise=True)
        return {"device": record_all(hs, cases),
                "device_errors": {k: pack_errors(v) for k, v in single.items()},
                "device_check_order": {k: check_order(single[k], both[k]) for k in PAIRED}}


def dump(table, f):
    """The table with one line per case (or per error), sorted."""
    line = lambda x: json.dumps(x, sort_keys=True)  # noqa: E731
    sections = []
    for sec, keys in sorted(table.items()):
        blocks = []
        for key, v in sorted(keys.items()):
            rows = [f"{line(n)}: {line(e)}" for n, e in sorted(v.items())] \
                if isinstance(v, dict) else [line(e) for e in v]
            a, z = "{}" if isinstance(v, dict) else "[]"
            blocks.append(f"{line(key)}: {a}\n" + ",\n".join(rows) + f"\n{z}")
        sections.append(f"{line(sec)}: {{\n" + ",\n".join(blocks) + "\n}")
    f.write("{\n" + ",\n".join(sections) + "\n}\n")


def main(argv):
    hs = _hsflow()
    half = argv[1] if len(argv) > 1 else "host"
    out = argv[2] if len(argv) > 2 else TABLE
    table = {}
    if os.path.exists(TABLE):
        with open(TABLE) as f:
            table = json.load(f)
    if half == "host":
        table.update(host_half(hs))
    else:
        import torch
        table.update(device_half(hs, torch))
    with open(out, "w") as f:
        dump(table, f)
    print(f"{out}: " + ", ".join(f"{k} {sum(len(v) for v in sec.values())}"
                                 for k, sec in sorted(table.items())))


if __name__ == "__main__":
    main(sys.argv)
