"""Python host binding of libhsflow.so (MI355X Horn-Schunck).

Mirrors the reference's operator interface, HornSchunckOF/hornSchunck.cpp:

    hs = hornSchunck(windowSize, maxIterations, alpha)      # :13-17
    gx, gy, gt = hs.getGradients(imagePrev, imageNext)       # :19-41
    u, v = hs.getFlow(imagePrev, imageNext)                  # :43-75

with numpy arrays standing in for cv::Mat: inputs are 2-D uint8 / float16 /
float32 / float64 (any row stride), outputs are float64 (CV_64FC1, what the reference
returns and plotFlow.cpp:72-75 reads).  Also exposes the stream-ordered
device entry points for torch tensors and the host utilities.

Everything here calls the HIP path in libhsflow.so; there is no CPU fallback.
If the library is missing or no gfx950 device is present, calls raise.
"""
from __future__ import annotations

import collections
import contextlib
import ctypes
import math
import os
import subprocess

import numpy as np

try:  # load torch's HIP runtime first so libhsflow binds to the same one
    import torch  # noqa: F401
except Exception:  # pragma: no cover - torch is optional for the host API
    torch = None

_HERE = os.path.dirname(os.path.abspath(__file__))
# HSFLOW_LIB: load another build of the library (same-box A/B timing only)
LIB_PATH = os.environ.get("HSFLOW_LIB") or os.path.join(_HERE, "libhsflow.so")

HSFLOW_OK = 0
HSFLOW_ERR_ARG = -1
HSFLOW_ERR_HIP = -2
HSFLOW_ERR_OOM = -3
HSFLOW_ERR_NODEV = -4
HSFLOW_ERR_SIZE = -5
U8, F32, F64, F16 = 0, 1, 2, 3
_U16 = 4  # HSFLOW_U16, 16-bit samples: the 16-bit YUV 4:2:0 calls only (yuv.U16)
MAX_LEVELS = 8
MAX_WARPS = 16
SOBEL_GAIN = 8.0
"""Pixels of displacement per unit of (u, v): the reference's Ix, Iy are
unnormalised 3x3 Sobel sums (hornSchunck.cpp:27-28, gain 8), so multiply
(u, v) by SOBEL_GAIN for the motion in pixels."""

# classes of the forward-backward check (HSFLOW_CONSISTENT, ...) and its
# default thresholds (Sundaram, Brox and Keutzer, ECCV 2010)
CONSISTENT, INCONSISTENT, OUT_OF_FRAME = 0, 1, 2
CONSISTENCY_REL, CONSISTENCY_ABS = 0.01, 0.5
# sizes of the median filter between warps (median=; 0 = none)
MEDIAN_SIZES = (3, 5)
# frame interpolation: times per call and the bits of its flags plane
# (HSFLOW_INTERP_*): a target outside I0 / I1, a source that fails the forward /
# backward check; flags == 0 marks a pixel both of whose sources pass
MAX_TIMES = 16
FLAG_I0_OUT, FLAG_I1_OUT, FLAG_FWD_FAILED, FLAG_BWD_FAILED = 1, 2, 4, 8


# modes of the brightness-robust prefilter (HSFLOW_PREFILTER_*)
PREFILTER_NONE, PREFILTER_HIGHPASS, PREFILTER_NORMALIZE = 0, 1, 2
PREFILTER_MAX_RADIUS = 15


class _CPrefilter(ctypes.Structure):
    _fields_ = [("mode", ctypes.c_int), ("sigma", ctypes.c_float), ("eps", ctypes.c_float),
                ("scale", ctypes.c_float)]


class Prefilter(collections.namedtuple("Prefilter", "mode sigma eps scale")):
    """hsflow_prefilter: what the warped, bidirectional and interpolating
    solves run on the frames first.  v = I - G*I with G a Gaussian of `sigma`;
    mode PREFILTER_HIGHPASS gives v, PREFILTER_NORMALIZE gives
    scale * v / (sqrt(G*(v v)) + eps) (include/hsflow.h).  It lowers the
    contrast the solver sees: use alpha ~ 100 with median=5."""
    __slots__ = ()
    _C, _GET, _SET = _CPrefilter, "hsflow_ctx_prefilter", "hsflow_ctx_set_prefilter"

    def __new__(cls, mode, sigma=4.0, eps=4.0, scale=32.0):
        return super().__new__(cls, int(mode), float(sigma), float(eps), float(scale))

    def _c(self):
        return self._C(*self)


# smoothness terms of the warped solves (HSFLOW_SMOOTH_*)
SMOOTH_QUADRATIC, SMOOTH_FLOW_DRIVEN = 0, 1


class _CSmoothness(ctypes.Structure):
    _fields_ = [("mode", ctypes.c_int), ("lam", ctypes.c_float)]


class Smoothness(collections.namedtuple("Smoothness", "mode lam")):
    """hsflow_smoothness: the smoothness term of the warped, bidirectional and
    interpolating solves.  SMOOTH_FLOW_DRIVEN weights each tap of the window
    mean by g = 1 / sqrt(1 + |grad flow|^2 / lam^2), recomputed at every warp
    (include/hsflow.h): motion boundaries stay sharp.  lam: the flow gradient,
    px per px, at which the weight is 1/sqrt(2); 0.1 .. 0.3.  The window must
    be 3 or 5.  Use alpha ~ 100 with median=5 and 4 warps."""
    __slots__ = ()
    _C, _GET, _SET = _CSmoothness, "hsflow_ctx_smoothness", "hsflow_ctx_set_smoothness"

    def __new__(cls, mode=SMOOTH_FLOW_DRIVEN, lam=0.3):
        return super().__new__(cls, int(mode), float(lam))

    def _c(self):
        return self._C(*self)


# what the interpolating calls do with a pair whose flows fail the
# forward-backward check (HSFLOW_FALLBACK_*) and the default share of consistent
# pixels below which a pair fails; fallback.py is their public face
_FALLBACK_OFF, _FALLBACK_NEAREST, _FALLBACK_BLEND = 0, 1, 2
_FALLBACK_MIN_SHARE = 0.4


class _CFallback(ctypes.Structure):
    _fields_ = [("mode", ctypes.c_int), ("min_share", ctypes.c_float)]


class _Fallback(collections.namedtuple("Fallback", "mode min_share")):
    """hsflow_fallback: what becomes of a pair whose share of consistent pixels,
    both directions together, is below `min_share` -- a scene cut, a motion
    beyond the pyramid's reach.  FALLBACK_NEAREST: every frame of the pair is
    the nearer source frame; FALLBACK_BLEND: a cross-fade (include/hsflow.h,
    "fallback for a failed pair"; fallback.Fallback is its public name)."""
    __slots__ = ()
    _C, _GET, _SET = _CFallback, "hsflow_ctx_fallback", "hsflow_ctx_set_fallback"

    def __new__(cls, mode=_FALLBACK_NEAREST, min_share=_FALLBACK_MIN_SHARE):
        return super().__new__(cls, int(mode), float(min_share))

    def _c(self):
        return self._C(*self)


class _CFlowInit(ctypes.Structure):
    """hsflow_flow_init: the planes a warped solve starts from (temporal.py)."""
    _fields_ = [("uf", ctypes.c_void_p), ("vf", ctypes.c_void_p), ("ub", ctypes.c_void_p),
                ("vb", ctypes.c_void_p)]


def _option(kind, value):
    """(keep-alive struct, pointer or None) of an option of `kind` (Prefilter,
    Smoothness or fallback.Fallback): an instance, a plain tuple of its fields, or None."""
    if value is None:
        return None, None
    if not isinstance(value, kind):
        value = kind(*value)
    c = value._c()
    return c, ctypes.byref(c)


BidirHost = collections.namedtuple("BidirHost", "u v ub vb mask_f mask_b counts")
BidirDevice = collections.namedtuple(
    "BidirDevice", "uf vf ub vb err_f mask_f counts_f err_b mask_b counts_b")


class HsflowError(RuntimeError):
    """A non-zero hsflow status (the reference would throw cv::Exception)."""

    def __init__(self, status: int, msg: str):
        super().__init__(f"hsflow status {status}: {msg}")
        self.status = status


def _prototypes():
    """name -> (restype, argtypes) of every symbol include/hsflow.h declares.
    The argument runs the entry points share are named once and the entries
    composed from them, in the header's order."""
    i, f, d, vp, sz = (ctypes.c_int, ctypes.c_float, ctypes.c_double, ctypes.c_void_p,
                       ctypes.c_size_t)
    ip, fp, vpp, text = ctypes.POINTER(i), ctypes.POINTER(f), ctypes.POINTER(vp), ctypes.c_char_p
    pf, sm = [ctypes.POINTER(_CPrefilter)], [ctypes.POINTER(_CSmoothness)]
    init = [ctypes.POINTER(_CFlowInit)]
    fb = [ctypes.POINTER(_CFallback)]
    shape = [i, i, i]                              # rows, cols, batch
    dev_pair = [vp, vp, i] + shape                 # I0, I1, dtype, rows, cols, batch
    dev_bgr_pair = [vp, vp] + shape                # bgr0, bgr1, rows, cols, batch
    host_pair = [vp, vp, vp, i, i, i, sz, sz]      # ctx, prev, next, dtype, rows, cols, steps
    host_bgr_pair = [vp, vp, vp, i, i, sz, sz]     # ctx, bgr0, bgr1, rows, cols, steps
    plain, plain_d = [i, i, f], [i, i, d]          # window, iters, alpha
    pyramid, pyramid_d = [i] + plain, [i] + plain_d            # levels, ...
    warped, warped_d = [i, i] + plain, [i, i] + plain_d        # levels, warps, ...
    solve, solve_d = [i, i, i] + plain, [i, i, i] + plain_d    # levels, warps, median, ...
    solve_lv = [i] + solve                         # levels, finest, warps, median, ...
    thresholds = [f, f]                            # rel, abs
    uv, host_uv = [vp, vp], [vp, vp, i, sz]        # u, v (host: + out dtype, step)
    flows = [vp] * 4                               # uf, vf, ub, vb
    bidir_out = flows + [vp] * 6                   # + err, mask, counts each way
    host_bidir_out = flows + [i, sz, vp, vp, sz, vp]   # + dtype, step, masks, step, counts
    times_out = [fp, i, vp, i, vp, vp]             # times, n, out, out dtype, flags, trusted
    times_pj_out = [fp, i, i, vp, i, vp, vp]       # times, n, projection, out, ...
    times_fb_out = times_pj_out + [vp]             # ... and cut
    host_times_out = [fp, i, vpp, i, sz, vpp, sz, vp]  # planes and their steps
    tail = [vp, sz, vp]                            # workspace, bytes, stream
    sized = (sz, shape + [i])                      # a workspace size of a shape and levels
    return {
        "hsflow_version": (i, []),
        "hsflow_status_string": (text, [i]),
        "hsflow_build_flags": (i, []),
        "hsflow_create": (i, [vpp, i]),
        "hsflow_destroy": (None, [vp]),
        "hsflow_last_error": (text, [vp]),
        "hsflow_stream": (vp, [vp]),
        "hsflow_flow": (i, host_pair + plain_d + host_uv),
        "hsflow_flow_multi": (i, [ip, i, i, vpp, vpp, i, i, i, sz, sz] + plain_d
                              + [vpp, vpp, i, sz]),
        "hsflow_flow_multi_release": (None, []),
        "hsflow_gradients": (i, host_pair + [vp, vp, vp, i, sz]),
        "hsflow_workspace_bytes": (sz, shape),
        "hsflow_flow_device": (i, dev_pair + plain + uv + tail),
        "hsflow_gradients_device": (i, dev_pair + [vp, vp, vp] + tail),
        "hsflow_jacobi_device": (i, shape + plain + [i] + uv + tail),
        "hsflow_set_iters_per_launch": (i, [i]),
        "hsflow_iters_per_launch": (i, shape + [i]),
        "hsflow_set_jacobi_kernel": (i, [i]),
        "hsflow_set_strip_rows": (i, [i]),
        "hsflow_jacobi_kernel_name": (text, shape + [i]),
        "hsflow_strip_seg_rows": (i, shape + [i]),
        "hsflow_set_max_streams": (i, [i]),
        "hsflow_max_streams": (i, []),
        "hsflow_set_first_pass_fusion": (i, [i]),
        "hsflow_first_pass_fusion": (i, []),
        "hsflow_first_pass_launches": (ctypes.c_longlong, []),
        # the interleaved (u, v) between K4 passes: the switch, the plan of a
        # shape (rows, cols, batch, window, iters) and the launch counter;
        # called through lib()
        "hsflow_set_uv_interleave": (i, [i]),
        "hsflow_uv_interleave": (i, []),
        "hsflow_uv_interleave_passes": (i, shape + [i, i]),
        "hsflow_uv_interleave_launches": (ctypes.c_longlong, []),
        "hsflow_set_output_hugepages": (i, [i]),
        "hsflow_download_device": (i, [vp, vp, sz, vp]),
        "hsflow_pyramid_level_size": (i, [i, i, i, ip, ip]),
        "hsflow_pyramid_workspace_bytes": sized,
        "hsflow_flow_pyramid_device": (i, dev_pair + pyramid + uv + tail),
        "hsflow_flow_pyramid": (i, host_pair + pyramid_d + host_uv),
        "hsflow_pyramid_build_device": (i, dev_pair + [i, vpp, vpp] + tail),
        "hsflow_upflow_device": (i, [vp, vp, i, i, vp, vp] + shape + [vp]),
        "hsflow_warp_gradients_device": (i, dev_pair + uv + [vp, vp, vp] + tail),
        "hsflow_flow_warped_device": (i, dev_pair + warped + uv + tail),
        "hsflow_flow_warped": (i, host_pair + warped_d + host_uv),
        "hsflow_flow_consistency_device": (i, flows + shape + thresholds + [vp, vp, vp, vp]),
        "hsflow_flow_bidir_workspace_bytes": sized,
        "hsflow_flow_bidir_device": (i, dev_pair + warped + thresholds + bidir_out + tail),
        "hsflow_flow_bidir": (i, host_pair + warped_d + thresholds + host_bidir_out),
        "hsflow_flow_median_device": (i, uv + shape + [i] + uv + [vp]),
        "hsflow_flow_warped_median_device": (i, dev_pair + solve + uv + tail),
        "hsflow_flow_warped_median": (i, host_pair + solve_d + host_uv),
        "hsflow_flow_bidir_median_device": (i, dev_pair + solve + thresholds + bidir_out + tail),
        "hsflow_flow_bidir_median": (i, host_pair + solve_d + thresholds + host_bidir_out),
        "hsflow_warp_image_device": (i, [vp, i] + shape + uv + [vp, vp, vp]),
        "hsflow_frame_interp_device": (i, dev_pair + flows + [vp, vp] + times_out + [vp]),
        "hsflow_flow_interp_workspace_bytes": sized,
        "hsflow_flow_interp_device": (i, dev_pair + solve + thresholds + times_out + tail),
        "hsflow_flow_interp": (i, host_pair + solve_d + thresholds + host_times_out),
        "hsflow_warp_image_bgr_device": (i, [vp] + shape + uv + [vp, i, vp, vp]),
        "hsflow_frame_interp_bgr_device": (i, dev_bgr_pair + flows + [vp, vp] + times_out + [vp]),
        "hsflow_flow_interp_bgr_workspace_bytes": sized,
        "hsflow_flow_interp_bgr_device": (i, dev_bgr_pair + solve + thresholds + times_out + tail),
        "hsflow_flow_interp_bgr": (i, host_bgr_pair + solve_d + thresholds + host_times_out),
        "hsflow_set_interp_bgr_loads": (i, [i]),
        "hsflow_prefilter_device": (i, [vp, i] + shape + pf + [vp, vp]),
        "hsflow_prefilter_planes_bytes": (sz, shape),
        "hsflow_flow_warped_pf_device": (i, dev_pair + solve + uv + pf + tail),
        "hsflow_flow_bidir_pf_device": (i, dev_pair + solve + thresholds + bidir_out + pf + tail),
        "hsflow_flow_interp_pf_device": (i, dev_pair + solve + thresholds + times_out + pf + tail),
        "hsflow_flow_interp_bgr_pf_device": (i, dev_bgr_pair + solve + thresholds + times_out + pf
                                             + tail),
        "hsflow_ctx_set_prefilter": (i, [vp] + pf),
        "hsflow_ctx_prefilter": (i, [vp] + pf),
        "hsflow_flow_diffusivity_device": (i, uv + shape + [f, vp, vp]),
        "hsflow_jacobi_weighted_device": (i, shape + plain + [vp] + uv + tail),
        "hsflow_flow_warped_sm_device": (i, dev_pair + solve + uv + pf + sm + tail),
        "hsflow_flow_bidir_sm_device": (i, dev_pair + solve + thresholds + bidir_out + pf + sm
                                        + tail),
        "hsflow_flow_interp_sm_device": (i, dev_pair + solve + thresholds + times_out + pf + sm
                                         + tail),
        "hsflow_flow_interp_bgr_sm_device": (i, dev_bgr_pair + solve + thresholds + times_out + pf
                                             + sm + tail),
        "hsflow_ctx_set_smoothness": (i, [vp] + sm),
        "hsflow_ctx_smoothness": (i, [vp] + sm),
        # the temporal warm start (temporal.py is its public face)
        "hsflow_downflow_device": (i, uv + [i, i] + uv + [i, i, i, vp]),
        "hsflow_flow_predict_device": (i, uv + shape + flows + [vp]),
        "hsflow_flow_warped_init_device": (i, dev_pair + solve + uv + pf + sm + init + tail),
        "hsflow_flow_bidir_init_device": (i, dev_pair + solve + thresholds + bidir_out + pf + sm
                                          + init + tail),
        "hsflow_flow_interp_init_device": (i, dev_pair + solve + thresholds + times_out + pf + sm
                                           + init + tail),
        "hsflow_flow_interp_bgr_init_device": (i, dev_bgr_pair + solve + thresholds + times_out
                                               + pf + sm + init + tail),
        "hsflow_ctx_set_temporal": (i, [vp, i]),
        "hsflow_ctx_temporal": (i, [vp]),
        "hsflow_ctx_temporal_reset": (i, [vp]),
        # the coarse solve: finest > 0 stops at that level, KB brings the flow up
        "hsflow_upflow_bilinear_device": (i, [vp, vp, i, i, vp, vp] + shape + [vp]),
        "hsflow_flow_warped_lv_device": (i, dev_pair + solve_lv + uv + pf + sm + init + tail),
        "hsflow_flow_bidir_lv_device": (i, dev_pair + solve_lv + thresholds + bidir_out + pf + sm
                                        + init + tail),
        "hsflow_flow_interp_lv_device": (i, dev_pair + solve_lv + thresholds + times_out + pf + sm
                                         + init + tail),
        "hsflow_flow_interp_bgr_lv_device": (i, dev_bgr_pair + solve_lv + thresholds + times_out
                                             + pf + sm + init + tail),
        "hsflow_ctx_set_finest_level": (i, [vp, i]),
        "hsflow_ctx_finest_level": (i, [vp]),
        # flow projection (projection.py is its public face): KS, KIP on grey and
        # BGR frames, the fused calls with `projection` after nt
        "hsflow_flow_project_device": (i, dev_pair + flows + [fp, i, vp, vp]),
        "hsflow_frame_interp_proj_device": (i, dev_pair + flows + [vp, vp, vp] + times_out + [vp]),
        "hsflow_frame_interp_bgr_proj_device": (i, dev_bgr_pair + flows + [vp, vp, vp] + times_out
                                                + [vp]),
        "hsflow_flow_interp_pj_workspace_bytes": (sz, shape + [i, i]),
        "hsflow_flow_interp_bgr_pj_workspace_bytes": (sz, shape + [i, i]),
        "hsflow_flow_interp_pj_device": (i, dev_pair + solve_lv + thresholds + times_pj_out + pf
                                         + sm + init + tail),
        "hsflow_flow_interp_bgr_pj_device": (i, dev_bgr_pair + solve_lv + thresholds + times_pj_out
                                             + pf + sm + init + tail),
        "hsflow_ctx_set_projection": (i, [vp, i]),
        "hsflow_ctx_projection": (i, [vp]),
        # the fallback for a failed pair (fallback.py is its public face): KF on
        # grey and BGR frames, the fused calls with cut after trusted and the
        # setting after init
        "hsflow_fallback_min_consistent": (sz, [i, i, f]),
        "hsflow_frame_fallback_device": (i, dev_pair + [vp, vp] + fb + times_out + [vp, vp]),
        "hsflow_frame_fallback_bgr_device": (i, dev_bgr_pair + [vp, vp] + fb + times_out
                                             + [vp, vp]),
        "hsflow_fallback_counts_bytes": (sz, [i]),
        "hsflow_flow_interp_fb_device": (i, dev_pair + solve_lv + thresholds + times_fb_out + pf
                                         + sm + init + fb + tail),
        "hsflow_flow_interp_bgr_fb_device": (i, dev_bgr_pair + solve_lv + thresholds + times_fb_out
                                             + pf + sm + init + fb + tail),
        "hsflow_ctx_set_fallback": (i, [vp] + fb),
        "hsflow_ctx_fallback": (i, [vp] + fb),
        "hsflow_ctx_last_cut": (i, [vp]),
        # YUV 4:2:0 (yuv.py is its public face): KIY on the chroma, the fused
        # call on luma and chroma planes, the host call on packed frames
        "hsflow_chroma_interp_device": (i, [vp, vp, i] + shape + flows + [vp, vp] + fb
                                        + [fp, i, vp, i, vp]),
        "hsflow_flow_interp_yuv_workspace_bytes": (sz, shape + [i, i]),
        "hsflow_flow_interp_yuv_device": (i, [vp, vp, vp, vp, i] + shape + solve_lv + thresholds
                                          + [fp, i, vp, vp, i, vp, vp, vp] + pf + sm + init + fb
                                          + tail),
        "hsflow_flow_interp_yuv": (i, [vp, vp, vp, i, i, i] + solve_d + thresholds
                                   + [fp, i, vpp, i, vpp, vp]),
        "hsflow_chroma_interp_blocks_per_cu": (i, []),
        "hsflow_set_chroma_nv12_loads": (i, [i]),
        # ... with the flow projection: KSD, KIYP, the fused and the host call
        # with `projection` after nt
        "hsflow_cells_down_device": (i, [vp] + shape + [i, vp, vp]),
        "hsflow_chroma_interp_proj_device": (i, [vp, vp, i] + shape + flows + [vp, vp, vp] + fb
                                             + [fp, i, vp, i, vp]),
        "hsflow_flow_interp_yuv_pj_workspace_bytes": (sz, shape + [i, i, i, i]),
        "hsflow_flow_interp_yuv_pj_device": (i, [vp, vp, vp, vp, i] + shape + solve_lv + thresholds
                                             + [fp, i, i, vp, vp, i, vp, vp, vp] + pf + sm + init
                                             + fb + tail),
        "hsflow_flow_interp_yuv_pj": (i, [vp, vp, vp, i, i, i] + solve_d + thresholds
                                      + [fp, i, i, vpp, i, vpp, vp]),
        "hsflow_chroma_interp_proj_blocks_per_cu": (i, []),
        # ... on 16-bit samples (yuv420p10le .. p16le, P010 .. P016): KIY / KIYP
        # (cells null or given), the fused and the host call
        "hsflow_chroma_interp16_device": (i, [vp, vp, i] + shape + flows + [vp, vp, vp] + fb
                                          + [fp, i, vp, i, vp]),
        "hsflow_flow_interp_yuv16_device": (i, [vp, vp, vp, vp, i] + shape + solve_lv + thresholds
                                            + [fp, i, i, vp, vp, i, vp, vp, vp] + pf + sm + init
                                            + fb + tail),
        "hsflow_flow_interp_yuv16": (i, [vp, vp, vp, i, i, i] + solve_d + thresholds
                                     + [fp, i, i, vpp, i, vpp, vp]),
        "hsflow_bgr_to_gray": (i, [vp, i, i, sz, vp, sz]),
        "hsflow_bgr_to_gray_device": (i, [vp] + shape + [vp, vp]),
        "hsflow_flow_bgr": (i, host_bgr_pair + plain_d + host_uv),
        "hsflow_synth_pair": (i, [ctypes.c_uint64, i, i, i, i, vp, vp, vp, vp]),
    }


_PROTOTYPES = _prototypes()
# every symbol include/hsflow.h declares
EXPORTS = tuple(_PROTOTYPES)

_lib = None
_vp = ctypes.c_void_p


def build(force: bool = False) -> str:
    if force or not os.path.exists(LIB_PATH):
        subprocess.check_call(["make", "-s", "-C", _HERE, "-j4"])
    return LIB_PATH


def lib():
    """Load libhsflow.so (fails loudly if it was not built)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ImportError(f"{LIB_PATH} is missing: run `make -C {_HERE}` "
                          "(or __graft_entry__.build())")
    L = ctypes.CDLL(LIB_PATH)
    for name, (restype, argtypes) in _PROTOTYPES.items():
        fn = getattr(L, name)
        fn.restype, fn.argtypes = restype, argtypes
    _lib = L
    return L


def _check(rc: int, ctx=None):
    if rc != HSFLOW_OK:
        L = lib()
        msg = L.hsflow_last_error(ctx).decode(errors="replace")
        raise HsflowError(rc, msg or L.hsflow_status_string(rc).decode())


_DTYPE_CODES = {np.dtype(np.uint8): U8, np.dtype(np.float32): F32, np.dtype(np.float64): F64,
                np.dtype(np.float16): F16}


def _dtype_code(a: np.ndarray) -> int:
    code = _DTYPE_CODES.get(a.dtype)
    if code is None:
        raise HsflowError(HSFLOW_ERR_ARG, f"unsupported image dtype {a.dtype}")
    return code


def _float_code(dtype) -> int:
    """The code of a host output: float64, else float32."""
    return F64 if dtype == np.float64 else F32


# --------------------------------------------------- host frames and outputs
def _as_image(a) -> np.ndarray:
    a = np.asarray(a)
    if a.ndim != 2:
        raise HsflowError(HSFLOW_ERR_ARG, "images must be single-channel 2-D "
                          "(convert BGR with bgr_to_gray, as main.cpp:13-14 does)")
    if a.strides[1] != a.itemsize or a.strides[0] < a.shape[1] * a.itemsize:
        a = np.ascontiguousarray(a)
    return a


def _sizes_differ():
    return HsflowError(HSFLOW_ERR_SIZE, "Image sizes are different")


def _host_pair(I0, I1):
    """(a, b, rows, cols) of a pair of grey frames.  Frames of different
    element types are both widened to float64, as hornSchunck.cpp:23-24
    converts each with convertTo(CV_64FC1); each frame keeps its own row step."""
    a, b = _as_image(I0), _as_image(I1)
    if a.shape != b.shape:
        raise _sizes_differ()
    if a.dtype != b.dtype:
        a, b = a.astype(np.float64), b.astype(np.float64)
    return a, b, a.shape[0], a.shape[1]


def _host_bgr(bgr, hint=""):
    """A decoded 8-bit BGR frame, H x W x 3, as the library reads it: dense
    pixels, strided rows accepted (anything else is copied)."""
    x = np.asarray(bgr)
    if x.dtype != np.uint8 or x.ndim != 3 or x.shape[2] != 3:
        raise HsflowError(HSFLOW_ERR_ARG, "need H x W x 3 BGR uint8" + hint)
    if x.strides[1:] != (3, 1) or x.strides[0] < 3 * x.shape[1]:
        x = np.ascontiguousarray(x)
    return x


def _host_bgr_pair(bgr0, bgr1, hint=""):
    """(a, b, rows, cols) of a pair of BGR frames (_host_bgr) of one size."""
    a, b = _host_bgr(bgr0, hint), _host_bgr(bgr1, hint)
    if a.shape != b.shape:
        raise _sizes_differ()
    return a, b, a.shape[0], a.shape[1]


def _pair_args(a, b):
    """The arguments a host entry point takes for its pair of frames: the
    pointers, the dtype code (grey frames only), rows, cols and both row steps."""
    rows, cols = a.shape[:2]
    if a.ndim == 2:
        return a.ctypes.data, b.ctypes.data, _dtype_code(a), rows, cols, a.strides[0], b.strides[0]
    return a.ctypes.data, b.ctypes.data, rows, cols, a.strides[0], b.strides[0]


def _reusable(out, shape, dtype) -> bool:
    """(u, v) can take a solve's output in place: the create() rule."""
    shape, dtype = tuple(shape), np.dtype(dtype)
    for x in out:
        if not (isinstance(x, np.ndarray) and x.shape == shape and x.dtype == dtype and
                x.flags.c_contiguous and x.flags.writeable):
            return False
    return out[0] is not out[1]


def _host_uv(rows, cols, out_dtype, out=None):
    """(u, v, args): the outputs of a host solve -- `out` where it can be
    reused, else new arrays -- and the arguments the entry point takes for
    them: both pointers, the dtype code and the row step."""
    if out is not None and _reusable(out, (rows, cols), out_dtype):
        u, v = out
    else:
        u = np.empty((rows, cols), out_dtype)
        v = np.empty((rows, cols), out_dtype)
    return u, v, (u.ctypes.data, v.ctypes.data, _float_code(u.dtype), u.strides[0])


def _solve_args(levels, warps, median, window, iters, alpha, *finest):
    """levels[, finest], warps, median, window, iters, alpha as the entry points
    take them; `finest`: nothing, or the one value of a *_lv_device call."""
    return (int(levels), *map(int, finest), int(warps), int(median), int(window), int(iters),
            float(alpha))


def _times_array(times):
    """`times` (a number or a sequence) as the C float array the library reads
    at call time; the library checks the count and the range."""
    t = np.atleast_1d(np.asarray(times, np.float64)).tolist()
    return (ctypes.c_float * len(t))(*t)


def _host_interp_out(times, shape, out_dtype, legal, with_flags):
    """(out, flags, trusted, args) of a host interpolation of frames of
    `shape` (rows, cols[, 3]): the outputs and the arguments the entry point
    takes for them, from the times on.  `legal`: the dtypes out may have."""
    tm = _times_array(times)
    nt = len(tm)
    out = np.empty((nt,) + shape, out_dtype)
    if out.dtype not in legal:
        raise HsflowError(HSFLOW_ERR_ARG, "out_dtype: need uint8, float32 or float64"
                          if np.float64 in legal else "out_dtype: need uint8 or float32")
    flags = np.empty((nt,) + shape[:2], np.uint8) if with_flags else None
    trusted = np.zeros(nt, np.uint32) if with_flags else None
    planes = (_vp * nt)(*[out[k].ctypes.data for k in range(nt)])
    fplanes = (_vp * nt)(*[flags[k].ctypes.data for k in range(nt)]) if with_flags else None
    return out, flags, trusted, (tm, nt, planes, _dtype_code(out), out.strides[1] if nt else 0,
                                 fplanes, shape[1], trusted.ctypes.data if with_flags else None)


class Context:
    """Device + stream + cached device buffers (hsflow_ctx)."""

    def __init__(self, device: int = 0):
        L = lib()
        p = _vp()
        rc = L.hsflow_create(ctypes.byref(p), int(device))
        if rc != HSFLOW_OK:
            raise HsflowError(rc, L.hsflow_last_error(None).decode(errors="replace"))
        self._p = p
        self.device = device

    @property
    def handle(self):
        return self._p

    def close(self):
        if getattr(self, "_p", None):
            lib().hsflow_destroy(self._p)
            self._p = None

    def __del__(self):  # pragma: no cover
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
        return False

    def _call(self, name, *args):
        """The one path of a host entry point: on this context, status checked."""
        _check(getattr(lib(), name)(self._p, *args), self._p)

    def _get(self, kind):
        c = kind._C()
        _check(getattr(lib(), kind._GET)(self._p, ctypes.byref(c)))
        return kind(*(getattr(c, f) for f in kind._fields)) if c.mode else None

    def _set(self, kind, value):
        self._call(kind._SET, _option(kind, value)[1])

    @contextlib.contextmanager
    def _setting_as(self, kind, value):
        """`value` (a Prefilter, a Smoothness or a Fallback) on the context for one call,
        the setting before it restored afterwards; None leaves the context's own."""
        if value is None:
            yield
            return
        was = self._get(kind)
        self._set(kind, value)
        try:
            yield
        finally:
            self._set(kind, was)

    @contextlib.contextmanager
    def _finest_as(self, finest):
        """`finest` as the context's finest level for one call, the setting
        before it restored afterwards; None leaves the context's own."""
        if finest is None:
            yield
            return
        was = self._finest_level()
        self._set_finest_level(finest)
        try:
            yield
        finally:
            self._set_finest_level(was)

    @contextlib.contextmanager
    def _projection_as(self, projection):
        """`projection` as the context's for one call, the setting before it
        restored afterwards; None leaves the context's own."""
        if projection is None:
            yield
            return
        was = self._projection()
        self._set_projection(projection)
        try:
            yield
        finally:
            self._set_projection(was)

    def _call_with(self, prefilter, smoothness, name, *args, finest=None, projection=None,
                   fallback=None):
        """_call with `prefilter`, `smoothness`, `finest`, `projection` and
        `fallback` as the context's settings."""
        with self._setting_as(Prefilter, prefilter), self._setting_as(Smoothness, smoothness), \
                self._finest_as(finest), self._projection_as(projection), \
                self._setting_as(_Fallback, fallback):
            rc = getattr(lib(), name)(self._p, *args)
        _check(rc, self._p)

    @property
    def last_cut(self):
        """The verdict of the last interpolate / interpolate_bgr on this context
        (hsflow_ctx_last_cut): True where the pair failed the check and the
        fallback made its frames, False where it passed, None where there was
        no such call or the fallback was off."""
        rc = int(lib().hsflow_ctx_last_cut(self._p))
        return None if rc < 0 else bool(rc)

    def _set_projection(self, projection):
        """hsflow_ctx_set_projection (projection.set_projection is its public face)."""
        self._call("hsflow_ctx_set_projection", int(projection))

    def _projection(self) -> int:
        rc = lib().hsflow_ctx_projection(self._p)
        if rc < 0:
            _check(rc, self._p)
        return int(rc)

    def _set_finest_level(self, finest):
        """hsflow_ctx_set_finest_level (coarse.set_finest_level is its public face)."""
        self._call("hsflow_ctx_set_finest_level", int(finest))

    def _finest_level(self) -> int:
        rc = lib().hsflow_ctx_finest_level(self._p)
        if rc < 0:
            _check(rc, self._p)
        return int(rc)

    def set_prefilter(self, prefilter=None):
        """The context's prefilter (hsflow_ctx_set_prefilter): flow_warped,
        flow_bidir, interpolate and interpolate_bgr run it on the frames first.
        None or mode 0 = off (default).  flow, flow_bgr, flow_pyramid and
        gradients are the reference's semantics and ignore it."""
        self._set(Prefilter, prefilter)

    def prefilter(self):
        """The context's current Prefilter, None when off."""
        return self._get(Prefilter)

    def set_smoothness(self, smoothness=None):
        """The context's smoothness term (hsflow_ctx_set_smoothness) for
        flow_warped, flow_bidir, interpolate and interpolate_bgr.  None or mode
        0 = quadratic (default).  flow, flow_bgr, flow_pyramid and gradients are
        the reference's semantics and ignore it."""
        self._set(Smoothness, smoothness)

    def smoothness(self):
        """The context's current Smoothness, None when quadratic."""
        return self._get(Smoothness)

    def flow(self, I0, I1, window: int, iters: int, alpha: float, out_dtype=np.float64,
             out=None):
        """getFlow on host arrays.  `out` = (u, v): C-contiguous rows x cols
        arrays of out_dtype written in place (cv::Mat::create() keeps an
        existing CV_64FC1 buffer of the right size the same way); else new
        arrays."""
        a, b, rows, cols = _host_pair(I0, I1)
        u, v, uv = _host_uv(rows, cols, out_dtype, out)
        self._call("hsflow_flow", *_pair_args(a, b), int(window), int(iters), float(alpha), *uv)
        return u, v

    def flow_pyramid(self, I0, I1, levels: int, window: int, iters: int, alpha: float,
                     out_dtype=np.float64):
        """Config 5 coarse-to-fine warm start (`iters` per level), see
        hsflow_flow_pyramid in include/hsflow.h."""
        a, b, rows, cols = _host_pair(I0, I1)
        u, v, uv = _host_uv(rows, cols, out_dtype)
        self._call("hsflow_flow_pyramid", *_pair_args(a, b), int(levels), int(window), int(iters),
                   float(alpha), *uv)
        return u, v

    def flow_warped(self, I0, I1, levels: int, warps: int, window: int, iters: int,
                    alpha: float, out_dtype=np.float64, median: int = 0, prefilter=None,
                    smoothness=None, finest=None):
        """Warped coarse-to-fine solve for large displacements (`warps`
        re-linearisations per level, `iters` iterations each), see
        hsflow_flow_warped in include/hsflow.h.  (u, v) * SOBEL_GAIN is the
        motion in pixels.  median = 3 or 5 filters (u, v) with a median of
        that size after every warp's iterations (hsflow_flow_warped_median);
        0 = none.  prefilter: a Prefilter set on the context for this call
        (None: the context's own setting, off by default).  smoothness: a
        Smoothness, likewise (window 3 or 5 then).  finest: the last level
        solved, likewise (coarse.set_finest_level; None: the context's own, 0
        by default); (u, v) are full resolution whatever it is."""
        a, b, rows, cols = _host_pair(I0, I1)
        u, v, uv = _host_uv(rows, cols, out_dtype)
        self._call_with(prefilter, smoothness, "hsflow_flow_warped_median", *_pair_args(a, b),
                        *_solve_args(levels, warps, median, window, iters, alpha), *uv,
                        finest=finest)
        return u, v

    def flow_bidir(self, I0, I1, levels: int, warps: int, window: int, iters: int,
                   alpha: float, rel: float = CONSISTENCY_REL, abs: float = CONSISTENCY_ABS,
                   out_dtype=np.float64, backward: bool = True, masks: bool = True,
                   counts: bool = True, out=None, mask_out=None, median: int = 0,
                   prefilter=None, smoothness=None, finest=None):
        """Warped solve in both directions with the forward-backward check
        (hsflow_flow_bidir in include/hsflow.h).  Returns a BidirHost: u, v
        (I0 -> I1), ub, vb (I1 -> I0, None unless `backward`), mask_f, mask_b
        (uint8: CONSISTENT / INCONSISTENT / OUT_OF_FRAME, None unless `masks`)
        and counts (uint32 [2, 3], forward then backward, None unless
        `counts`).  `out`: an array [4, rows, >= cols] of out_dtype whose
        planes' first `cols` columns receive u, v, ub, vb (a padded row step);
        `mask_out`: likewise uint8 [2, rows, >= cols] for the masks.  median,
        prefilter, smoothness and finest as in flow_warped, for both directions;
        the check runs on the full-resolution flows."""
        a, b, rows, cols = _host_pair(I0, I1)
        if out is None:
            out = np.empty((4, rows, cols), out_dtype)
        if mask_out is None:
            mask_out = np.empty((2, rows, cols), np.uint8)
        if out.ndim != 3 or out.shape[0] != 4 or out.shape[1] != rows or \
                out.shape[2] < cols or out.dtype not in (np.float32, np.float64) or \
                out.strides[2] != out.itemsize:
            raise HsflowError(HSFLOW_ERR_ARG, f"out: need float32/float64 [4, {rows}, >= {cols}]")
        if mask_out.ndim != 3 or mask_out.shape[0] != 2 or mask_out.shape[1] != rows or \
                mask_out.shape[2] < cols or mask_out.dtype != np.uint8 or \
                mask_out.strides[2] != 1:
            raise HsflowError(HSFLOW_ERR_ARG, f"mask_out: need uint8 [2, {rows}, >= {cols}]")
        u, v = out[0, :, :cols], out[1, :, :cols]
        ub, vb = (out[2, :, :cols], out[3, :, :cols]) if backward else (None, None)
        mf, mb = (mask_out[0, :, :cols], mask_out[1, :, :cols]) if masks else (None, None)
        cnt = np.zeros((2, 3), np.uint32) if counts else None
        ptr = (lambda x: x.ctypes.data if x is not None else None)
        self._call_with(prefilter, smoothness, "hsflow_flow_bidir_median", *_pair_args(a, b),
                        *_solve_args(levels, warps, median, window, iters, alpha), float(rel),
                        float(abs), ptr(u), ptr(v), ptr(ub), ptr(vb), _float_code(out.dtype),
                        out.strides[1], ptr(mf), ptr(mb), mask_out.strides[1], ptr(cnt),
                        finest=finest)
        return BidirHost(u, v, ub, vb, mf, mb, cnt)

    def interpolate(self, I0, I1, times, levels: int, warps: int, window: int, iters: int,
                    alpha: float, median: int = 0, rel: float = CONSISTENCY_REL,
                    abs: float = CONSISTENCY_ABS, out_dtype=np.float32,
                    with_flags: bool = False, prefilter=None, smoothness=None, finest=None,
                    projection=None, fallback=None):
        """The frames at `times` (each in [0, 1]; at most MAX_TIMES) between I0
        and I1: the bidirectional warped solve, then the motion-compensated
        blend (hsflow_flow_interp in include/hsflow.h).  Returns an array
        [len(times), rows, cols] of out_dtype (uint8, float32 or float64), or
        with_flags: (frames, flags, trusted) -- flags uint8 like frames (FLAG_*
        bits; 0 = both sources pass the forward-backward check), trusted uint32
        [len(times)], the pixels per frame with flags == 0.  prefilter as in
        flow_warped: the flows come from the prefiltered frames, the frames
        themselves are sampled.  smoothness as in flow_warped.  finest as in
        flow_warped: the flows are solved down to that level only, the frames
        are sampled at full resolution.  projection: 1 carries the flows to each
        time before the blend (projection.set_projection; None: the context's
        own, 0 by default); flags then has FLAG bit 16 where nothing landed.
        fallback: a fallback.Fallback (fallback.set_fallback; None: the context's own,
        off by default): where the pair fails the check every frame is a
        source frame or a cross-fade, flags is fallback.FLAG_FALLBACK, trusted 0 and
        Context.last_cut True."""
        a, b, rows, cols = _host_pair(I0, I1)
        out, flags, trusted, outs = _host_interp_out(times, (rows, cols), out_dtype,
                                                     (np.uint8, np.float32, np.float64), with_flags)
        self._call_with(prefilter, smoothness, "hsflow_flow_interp", *_pair_args(a, b),
                        *_solve_args(levels, warps, median, window, iters, alpha), float(rel),
                        float(abs), *outs, finest=finest, projection=projection,
                        fallback=fallback)
        return (out, flags, trusted) if with_flags else out

    def interpolate_bgr(self, bgr0, bgr1, times, levels: int, warps: int, window: int,
                        iters: int, alpha: float, median: int = 0,
                        rel: float = CONSISTENCY_REL, abs: float = CONSISTENCY_ABS,
                        out_dtype=np.uint8, with_flags: bool = False, prefilter=None,
                        smoothness=None, finest=None, projection=None, fallback=None):
        """The colour frames at `times` between two decoded 8-bit BGR frames
        (H x W x 3, strided rows accepted): uploaded as BGR, converted to grey
        and solved both ways on the GPU, then the motion-compensated blend of
        each channel (hsflow_flow_interp_bgr in include/hsflow.h).  Returns an
        array [len(times), rows, cols, 3] of out_dtype (uint8 or float32), or
        with_flags: (frames, flags, trusted) -- flags uint8 [len(times), rows,
        cols] and trusted uint32 [len(times)] as in interpolate.  prefilter as
        in flow_warped, run on the grey planes; smoothness and finest as in
        flow_warped; projection as in interpolate (the cells come from the grey
        planes); fallback as in interpolate."""
        a, b, rows, cols = _host_bgr_pair(bgr0, bgr1, " (grey frames: Context.interpolate)")
        out, flags, trusted, outs = _host_interp_out(times, (rows, cols, 3), out_dtype,
                                                     (np.uint8, np.float32), with_flags)
        self._call_with(prefilter, smoothness, "hsflow_flow_interp_bgr", *_pair_args(a, b),
                        *_solve_args(levels, warps, median, window, iters, alpha), float(rel),
                        float(abs), *outs, finest=finest, projection=projection,
                        fallback=fallback)
        return (out, flags, trusted) if with_flags else out

    def flow_bgr(self, bgr0, bgr1, window: int, iters: int, alpha: float,
                 out_dtype=np.float64):
        """main.cpp:50-51 + :13-14 + :97-98: decoded 8-bit BGR frames are
        uploaded as BGR and converted to gray on the GPU, then solved."""
        a, b, rows, cols = _host_bgr_pair(bgr0, bgr1)
        u, v, uv = _host_uv(rows, cols, out_dtype)
        self._call("hsflow_flow_bgr", *_pair_args(a, b), int(window), int(iters), float(alpha),
                   *uv)
        return u, v

    def gradients(self, I0, I1, out_dtype=np.float64):
        a, b, rows, cols = _host_pair(I0, I1)
        gx, gy, gt = (np.empty((rows, cols), out_dtype) for _ in range(3))
        self._call("hsflow_gradients", *_pair_args(a, b), gx.ctypes.data, gy.ctypes.data,
                   gt.ctypes.data, _float_code(gx.dtype), gx.strides[0])
        return gx, gy, gt


_default_ctx = None


def flow_multi(devices, pairs, window: int, iters: int, alpha: float,
               out_dtype=np.float64):
    """Frame-parallel getFlow of host pairs over several GPUs from one
    process (hsflow_flow_multi): pair j on devices[j % len(devices)], one
    host thread + context per listed device.  `pairs`: list of (I0, I1)
    arrays of one shape and dtype.  Returns [(u, v), ...] in pair order."""
    pairs = [(_as_image(a), _as_image(b)) for a, b in pairs]
    if not pairs:
        return []
    rows, cols = pairs[0][0].shape
    dt, st0, st1 = pairs[0][0].dtype, pairs[0][0].strides[0], pairs[0][1].strides[0]
    for a, b in pairs:
        if a.shape != (rows, cols) or b.shape != (rows, cols):
            raise _sizes_differ()
        if a.dtype != dt or b.dtype != dt or a.strides[0] != st0 or b.strides[0] != st1:
            raise HsflowError(HSFLOW_ERR_ARG, "pairs must share dtype and row steps")
    out = [(np.empty((rows, cols), out_dtype), np.empty((rows, cols), out_dtype))
           for _ in pairs]
    n = len(pairs)
    P = _vp * n
    devs = (ctypes.c_int * len(devices))(*devices)
    rc = lib().hsflow_flow_multi(
        devs, len(devices), n, P(*[a.ctypes.data for a, _ in pairs]),
        P(*[b.ctypes.data for _, b in pairs]), _dtype_code(pairs[0][0]), rows, cols, st0,
        st1, int(window), int(iters), float(alpha), P(*[u.ctypes.data for u, _ in out]),
        P(*[v.ctypes.data for _, v in out]), _float_code(out_dtype), out[0][0].strides[0])
    _check(rc)
    return out


def flow_multi_release():
    """Destroy the per-device contexts flow_multi keeps (hsflow_flow_multi_release)."""
    lib().hsflow_flow_multi_release()


def default_context() -> Context:
    global _default_ctx
    if _default_ctx is None:
        _default_ctx = Context(0)
    return _default_ctx


class hornSchunck:  # noqa: N801  (reference class name, hornSchunck.cpp:8)
    """Drop-in mirror of `class hornSchunck` (hornSchunck.cpp:8-76)."""

    def __init__(self, inpWindowSize: int, inpMaxIterations: int, inpAlpha: float,
                 context: Context | None = None):
        # hornSchunck.cpp:13-17 -- public fields, same names
        self.windowSize = int(inpWindowSize)
        self.maxIterations = int(inpMaxIterations)
        self.alpha = float(inpAlpha)
        self._ctx = context

    def _c(self):
        return self._ctx if self._ctx is not None else default_context()

    def getGradients(self, imagePrev, imageNext, gradX=None, gradY=None, gradT=None):
        """hornSchunck.cpp:19-41 -> (gradX, gradY, gradT) float64."""
        gx, gy, gt = self._c().gradients(imagePrev, imageNext)
        for dst, src in ((gradX, gx), (gradY, gy), (gradT, gt)):
            if dst is not None:
                dst[...] = src
        return gx, gy, gt

    def getFlow(self, imagePrev, imageNext, u=None, v=None):
        """hornSchunck.cpp:43-75 -> (u, v) float64 (CV_64FC1).  Given u, v
        float64 arrays of the frame size, the solve writes into them (as the
        cv::Mat adapter's create() does); other arrays receive a copy."""
        out = (u, v) if u is not None and v is not None else None
        uu, vv = self._c().flow(imagePrev, imageNext, self.windowSize,
                                self.maxIterations, self.alpha, out=out)
        if u is not None and u is not uu:
            u[...] = uu
        if v is not None and v is not vv:
            v[...] = vv
        return uu, vv


def compute(I0, I1, alpha: float, nIter: int, windowSize: int = 5, levels: int = 1,
            warps: int = 0, median: int = 0, prefilter=None, smoothness=None, finest: int = 0,
            projection: int = 0):
    """compute(I0, I1, alpha, nIter) -> (u, v): the north-star convenience
    wrapper over hornSchunck(windowSize, nIter, alpha).getFlow; levels > 1
    runs the config-5 coarse-to-fine warm start (nIter per level).  warps >= 1
    runs the warped coarse-to-fine solve instead (large displacements:
    `warps` re-linearisations per level, nIter iterations each); warps = 0
    keeps the behaviour above.  median = 3 or 5 (MEDIAN_SIZES) filters the
    flow after every warp's iterations and needs warps >= 1; so does
    prefilter (a Prefilter: the frames are locally normalised first) and so
    does smoothness (a Smoothness: the flow-driven, edge-preserving term) and so
    does finest > 0 (the last level solved; its flow goes up to the full frame
    bilinearly).  projection is a step of frame interpolation (Context.interpolate,
    flow_interp_device), not of the solve: compute returns the flows, which it
    does not change, so anything but 0 is an error here rather than ignored."""
    if projection:
        raise HsflowError(HSFLOW_ERR_ARG, f"projection {projection} belongs to frame "
                          "interpolation (Context.interpolate), not to a flow")
    if median and not warps:
        raise HsflowError(HSFLOW_ERR_ARG, f"median {median} needs the warped solve (warps >= 1)")
    if prefilter is not None and not warps:
        raise HsflowError(HSFLOW_ERR_ARG, "prefilter needs the warped solve (warps >= 1)")
    if smoothness is not None and not warps:
        raise HsflowError(HSFLOW_ERR_ARG, "smoothness needs the warped solve (warps >= 1)")
    if finest and not warps:
        raise HsflowError(HSFLOW_ERR_ARG, f"finest {finest} needs the warped solve (warps >= 1)")
    if warps:
        if not 1 <= int(warps) <= MAX_WARPS:
            raise HsflowError(HSFLOW_ERR_ARG, f"warps {warps} outside [1, {MAX_WARPS}]")
        return default_context().flow_warped(I0, I1, levels, warps, windowSize, nIter, alpha,
                                             median=median, prefilter=prefilter,
                                             smoothness=smoothness, finest=finest or None)
    if levels > 1:
        return default_context().flow_pyramid(I0, I1, levels, windowSize, nIter, alpha)
    return hornSchunck(windowSize, nIter, alpha).getFlow(I0, I1)


# ------------------------------------------------------------ device (torch)
def _stream_ptr(stream, device=None):
    """hipStream_t of `stream`, or of the current stream of `device` (the
    tensors' device) when stream is None.  The library runs a call on the
    device its stream belongs to; the null stream (torch's default stream is
    0 on every device) means the CURRENT device, so _device_call, the one path
    every wrapper below takes, makes the tensors' device current around the
    library call (_on)."""
    if stream is None:
        return torch.cuda.current_stream(device).cuda_stream if torch is not None else None
    return getattr(stream, "cuda_stream", stream)


def _on(device):
    """Context that makes `device` current for one library call (a null
    stream runs on the current device, include/hsflow.h)."""
    return torch.cuda.device(device)


def _device_call(name, device, stream, *args):
    """The one path of a stream-ordered entry point: `device` (the tensors')
    current, the arguments (ending in _ws_args where the entry point takes a
    workspace), then the stream; status checked."""
    with _on(device):
        rc = getattr(lib(), name)(*args, _stream_ptr(stream, device))
    _check(rc)


def download_device(dst, src, stream=None):
    """Stream-ordered download of the CUDA tensor `src` into the pinned host
    tensor `dst` (same byte size) through the runtime's DMA engines
    (hsflow_download_device), so it overlaps Jacobi passes running on other
    streams; torch's own copy_ of pinned memory runs as a blit kernel that
    takes their workgroup slots."""
    if src.numel() * src.element_size() != dst.numel() * dst.element_size():
        raise HsflowError(HSFLOW_ERR_ARG, "download sizes differ")
    if not (src.is_contiguous() and dst.is_contiguous()):
        raise HsflowError(HSFLOW_ERR_ARG, "download tensors must be contiguous")
    # a pageable dst would silently serialise the 'overlapped' copy, and a
    # CUDA dst would get a device-to-host copy kind on a device pointer
    if not src.is_cuda or dst.is_cuda or not dst.is_pinned():
        raise HsflowError(HSFLOW_ERR_ARG,
                          "download_device: src must be a CUDA tensor, dst pinned host memory")
    _device_call("hsflow_download_device", src.device, stream, dst.data_ptr(), src.data_ptr(),
                 src.numel() * src.element_size())


def build_flags() -> int:
    return int(lib().hsflow_build_flags())


def is_probe_build() -> bool:
    """True for a non-product build (hsflow_build_flags() != 0)."""
    return build_flags() != 0


def strip_seg_rows(rows: int, cols: int, batch: int = 1, window: int = 5) -> int:
    """hsflow_strip_seg_rows: K4 segment height a solve of this shape uses
    (0 when its full-depth passes run another kernel)."""
    return int(lib().hsflow_strip_seg_rows(rows, cols, batch, window))


def set_output_hugepages(on: bool) -> bool:
    """hsflow_set_output_hugepages: MADV_HUGEPAGE advice on f64 host outputs
    (default on; the advice stays on the caller's allocation).  Returns the
    previous setting."""
    return bool(lib().hsflow_set_output_hugepages(1 if on else 0))


def workspace_bytes(rows: int, cols: int, batch: int = 1) -> int:
    return int(lib().hsflow_workspace_bytes(rows, cols, batch))


def alloc_workspace(rows: int, cols: int, batch: int = 1, device="cuda"):
    n = workspace_bytes(rows, cols, batch)
    return torch.empty(n, dtype=torch.uint8, device=device)


def pyramid_level_size(rows: int, cols: int, level: int):
    r, c = ctypes.c_int(), ctypes.c_int()
    _check(lib().hsflow_pyramid_level_size(rows, cols, level, ctypes.byref(r),
                                           ctypes.byref(c)))
    return r.value, c.value


def pyramid_workspace_bytes(rows: int, cols: int, batch: int, levels: int) -> int:
    return int(lib().hsflow_pyramid_workspace_bytes(rows, cols, batch, levels))


_TENSOR_CODES = {} if torch is None else {torch.uint8: U8, torch.float32: F32, torch.float16: F16,
                                          torch.float64: F64}


def _tensor_dtype(t) -> int:
    code = _TENSOR_CODES.get(t.dtype)
    if code is None:
        raise HsflowError(HSFLOW_ERR_ARG,
                          f"device input dtype {t.dtype} (want uint8/float16/float32/float64)")
    return code


def _ptr(t):
    return t.data_ptr() if t is not None else None


def _ws_args(workspace):
    return workspace.data_ptr(), workspace.numel()


def _is16(dtype) -> bool:
    """A torch dtype that holds 16-bit samples: uint16, or int16 read as the same
    16 bits (torch has few uint16 operators)."""
    return dtype == torch.int16 or dtype == getattr(torch, "uint16", torch.int16)


def _out_code(out) -> int:
    """The code of a warped or interpolated device output: uint8, 16-bit samples
    (the 16-bit YUV calls), else float32."""
    return U8 if out.dtype == torch.uint8 else (_U16 if _is16(out.dtype) else F32)


def _dims(shape):
    """(rows, cols, batch) of a tensor shape [..., rows, cols]: batch is the
    product of the leading dimensions."""
    rows, cols = shape[-2:]
    return rows, cols, math.prod(shape[:-2])


def _check_dense(t, shape, name):
    if not t.is_cuda or not t.is_contiguous() or tuple(t.shape[-2:]) != tuple(shape):
        raise HsflowError(HSFLOW_ERR_ARG, f"{name}: need a contiguous CUDA tensor "
                          f"[..., {shape[0]}, {shape[1]}]")


def _check_plane(t, shape, batch, name):
    """u, v (and the warm-start planes) are written by the kernels through
    raw pointers: a float32, contiguous CUDA tensor holding at least
    batch x rows x cols elements, or HsflowError (not a GPU fault)."""
    if t is None or not t.is_cuda or t.dtype != torch.float32 or not t.is_contiguous() or \
            tuple(t.shape[-2:]) != tuple(shape) or t.numel() < batch * shape[0] * shape[1]:
        raise HsflowError(HSFLOW_ERR_ARG, f"{name}: need a contiguous float32 CUDA tensor of "
                          f"{batch} x {shape[0]} x {shape[1]}")


def _check_planes(dims, **planes):
    for name, t in planes.items():
        _check_plane(t, dims[:2], dims[2], name)


def _frame(I, name="I"):
    """(rows, cols, batch) of the dense frames I, [B, H, W] or [H, W]."""
    dims = _dims(I.shape)
    _check_dense(I, dims[:2], name)
    return dims


def _frame_pair(I0, I1, same=True):
    """(rows, cols, batch) of the dense frames I0 and I1, of one shape and
    dtype unless not `same` (the entry points that convert each on its own)."""
    dims = _frame(I0, "I0")
    _check_dense(I1, dims[:2], "I1")
    if same and (I1.dtype != I0.dtype or I1.shape != I0.shape):
        raise HsflowError(HSFLOW_ERR_SIZE, "I0/I1 differ in shape or dtype")
    return dims


def _plane(t, like, dims, name):
    """The float32 plane `t`, a new one of the shape of `like` when None; checked."""
    if t is None:
        t = torch.empty(like.shape, dtype=torch.float32, device=like.device)
    _check_plane(t, dims[:2], dims[2], name)
    return t


def _workspace(workspace, device, size_fn, *size_args, prefilter=None, fallback=None):
    """The given workspace, or size_fn(rows, cols, batch[, levels]) bytes on
    `device`, with the prefilter's planes and the fallback's counts where one
    is on."""
    if workspace is None:
        n = size_fn(*size_args) + _pf_extra(prefilter, *size_args[:3]) + \
            _fb_extra(fallback, size_args[2])
        workspace = torch.empty(n, dtype=torch.uint8, device=device)
    return workspace


def _check_output(want, shape, dtype, device, name):
    """An optional output of the consistency check: None / False = not asked
    for, True = allocate, else a contiguous CUDA tensor of `shape`, `dtype`."""
    if want is None or want is False:
        return None
    if want is True:
        return torch.empty(shape, dtype=dtype, device=device)
    if not want.is_cuda or want.dtype != dtype or not want.is_contiguous() or \
            tuple(want.shape) != tuple(shape):
        raise HsflowError(HSFLOW_ERR_ARG, f"{name}: need a contiguous {dtype} CUDA tensor "
                          f"{tuple(shape)}")
    return want


def _out_frames(out, shape, out_dtype, device, wide=False):
    """The `out` of a colour warp or an interpolation: the given tensor, or a
    new one of out_dtype (float32 when None); float32 or uint8, of `shape`.
    wide: of 16-bit frames, float32 or uint16 (int16: the same bits)."""
    if out is None:
        out = torch.empty(shape, dtype=out_dtype or torch.float32, device=device)
    if wide:
        if out.dtype != torch.float32 and not _is16(out.dtype):
            raise HsflowError(HSFLOW_ERR_ARG, "out: need float32 or uint16 (int16) for 16-bit "
                              "frames")
    elif out.dtype not in (torch.float32, torch.uint8):
        raise HsflowError(HSFLOW_ERR_ARG, "out: need float32 or uint8")
    return _check_output(out, shape, out.dtype, device, "out")


def _interp_outputs(frames, channels, nt, out, out_dtype, flags, trusted, wide=False):
    """out / flags / trusted of an interpolation of `nt` times of `frames`,
    [B, H, W] + channels or [H, W] + channels (channels () or (3,)):
    [B, nt, H, W] + channels, [B, nt, H, W] and [B, nt]."""
    plane = tuple(frames.shape[:frames.dim() - len(channels)])
    shape = plane[:-2] + (nt,) + plane[-2:]
    out = _out_frames(out, shape + channels, out_dtype, frames.device, wide)
    flags = _check_output(flags, shape, torch.uint8, frames.device, "flags")
    trusted = _check_output(trusted, (math.prod(plane[:-2]), nt), torch.int32, frames.device,
                            "trusted")
    return out, flags, trusted


def _init_entry(stem, init, dims, finest=0):
    """(entry point, its finest argument, its init argument) of a
    warped-family solve `stem`: the *_sm_device call and nothing for init None,
    else the *_init_device call and the hsflow_flow_init of `init` = (uf, vf, ub,
    vb), float32 CUDA planes like the frames or None each; the library checks
    that pairs are whole.  finest != 0: the *_lv_device call, `finest` for
    _solve_args and the init, NULL for None."""
    name, start = _init_entry_0(stem, init, dims)
    if not finest:
        return name, (), start
    return stem + "_lv_device", (int(finest),), start or (None,)


def _pj_entry(stem, init, dims, finest, projection):
    """_init_entry for the two interpolating solves, plus the projection
    argument: nothing for projection 0, which is _init_entry as it stands; else
    the *_pj_device call, which takes finest, `projection` after nt and an
    init or NULL."""
    name, lv, start = _init_entry(stem, init, dims, finest)
    if not projection:
        return name, lv, start, ()
    return stem + "_pj_device", (int(finest),), start or (None,), (int(projection),)


def _fb_entry(stem, init, dims, finest, projection, fallback, cut, device):
    """_pj_entry plus the fallback's arguments: (name, lv, start, pj, cut
    tensor, arguments after trusted, arguments after the init).  fallback None
    and no cut: _pj_entry as it stands; else the *_fb_device call, which takes
    finest, projection, `cut` (uint8 [B], allocated for True) after trusted and
    the hsflow_fallback (NULL for None) after an init or NULL."""
    if fallback is None and (cut is None or cut is False):
        return _pj_entry(stem, init, dims, finest, projection) + (None, (), ())
    _, _, start = _init_entry(stem, init, dims, finest)
    cut = _check_output(cut, (dims[2],), torch.uint8, device, "cut")
    keep, fb = _option(_Fallback, fallback)
    return (stem + "_fb_device", (int(finest),), start or (None,), (int(projection),), cut,
            (_ptr(cut),), (fb,))


def _fb_extra(fallback, batch):
    """The bytes a fused call's workspace grows by with `fallback` on."""
    on = fallback is not None and int(fallback[0]) != _FALLBACK_OFF
    return int(lib().hsflow_fallback_counts_bytes(batch)) if on else 0


def _pj_size(size_fn, stem, projection, levels, nt):
    """(workspace size function, its arguments past the shape) of an
    interpolating solve: `size_fn` of the levels, or with projection the
    *_pj_workspace_bytes of `stem`, which counts the cell planes of nt times."""
    if not projection:
        return size_fn, (levels,)
    return getattr(lib(), stem + "_pj_workspace_bytes"), (levels, nt)


def _init_entry_0(stem, init, dims):
    if init is None:
        return stem + "_sm_device", ()
    planes = tuple(init)
    if len(planes) != 4:
        raise HsflowError(HSFLOW_ERR_ARG, "init: need (uf, vf, ub, vb), None for a plane not given")
    for t, name in zip(planes, ("uf", "vf", "ub", "vb")):
        if t is not None:
            _check_plane(t, dims[:2], dims[2], "init." + name)
    return stem + "_init_device", (ctypes.byref(_CFlowInit(*[_ptr(t) for t in planes])),)


def flow_device(I0, I1, window: int, iters: int, alpha: float, u=None, v=None,
                workspace=None, stream=None):
    """Stream-ordered solve on torch CUDA tensors [B, H, W] (or [H, W]).
    Returns (u, v) float32 tensors.  No host synchronisation."""
    dims = _frame_pair(I0, I1)
    u, v = _plane(u, I0, dims, "u"), _plane(v, I0, dims, "v")
    workspace = _workspace(workspace, I0.device, workspace_bytes, *dims)
    _device_call("hsflow_flow_device", I0.device, stream, I0.data_ptr(), I1.data_ptr(),
                 _tensor_dtype(I0), *dims, int(window), int(iters), float(alpha), u.data_ptr(),
                 v.data_ptr(), *_ws_args(workspace))
    return u, v


def flow_pyramid_device(I0, I1, levels: int, window: int, iters: int, alpha: float,
                        u=None, v=None, workspace=None, stream=None):
    """Config 5: coarse-to-fine warm start on torch CUDA tensors [B, H, W]
    (uint8 / float16 / float32), `iters` Jacobi iterations per level."""
    dims = _frame_pair(I0, I1)
    u, v = _plane(u, I0, dims, "u"), _plane(v, I0, dims, "v")
    workspace = _workspace(workspace, I0.device, pyramid_workspace_bytes, *dims, levels)
    _device_call("hsflow_flow_pyramid_device", I0.device, stream, I0.data_ptr(), I1.data_ptr(),
                 _tensor_dtype(I0), *dims, int(levels), int(window), int(iters), float(alpha),
                 u.data_ptr(), v.data_ptr(), *_ws_args(workspace))
    return u, v


def flow_warped_device(I0, I1, levels: int, warps: int, window: int, iters: int,
                       alpha: float, u=None, v=None, workspace=None, stream=None,
                       median: int = 0, prefilter=None, smoothness=None, finest: int = 0):
    """Warped coarse-to-fine solve on torch CUDA tensors [B, H, W] (uint8 /
    float16 / float32 / float64): per level `warps` times the gradients
    linearised around the current flow and `iters` Jacobi iterations.
    `workspace`: pyramid_workspace_bytes(rows, cols, batch, levels) bytes.
    (u, v) * SOBEL_GAIN is the motion in pixels.  median = 3 or 5: a median
    of that size over (u, v) after every warp's iterations
    (hsflow_flow_warped_median_device); 0 = none.  prefilter: a Prefilter run
    on both frames first (hsflow_flow_warped_pf_device); the workspace then
    needs prefilter_planes_bytes(rows, cols, batch) more.  smoothness: a
    Smoothness; SMOOTH_FLOW_DRIVEN runs the g-weighted iterations
    (hsflow_flow_warped_sm_device; window 3 or 5, no more workspace).
    finest > 0: only the levels down to `finest` are solved and that flow goes
    up to the full frame through coarse.upflow_bilinear_device
    (hsflow_flow_warped_lv_device; the same workspace); (u, v) are full
    resolution.  Stream-ordered."""
    return _flow_warped_device(I0, I1, levels, warps, window, iters, alpha, u, v, workspace,
                               stream, median, prefilter, smoothness, finest=finest)


def _flow_warped_device(I0, I1, levels, warps, window, iters, alpha, u, v, workspace, stream,
                        median, prefilter, smoothness, init=None, finest=0):
    """flow_warped_device, from `init` (_init_entry) where given."""
    dims = _frame_pair(I0, I1)
    u, v = _plane(u, I0, dims, "u"), _plane(v, I0, dims, "v")
    pf, sm = _option(Prefilter, prefilter)[1], _option(Smoothness, smoothness)[1]
    workspace = _workspace(workspace, I0.device, pyramid_workspace_bytes, *dims, levels,
                           prefilter=prefilter)
    name, lv, start = _init_entry("hsflow_flow_warped", init, dims, finest)
    _device_call(name, I0.device, stream, I0.data_ptr(), I1.data_ptr(),
                 _tensor_dtype(I0), *dims,
                 *_solve_args(levels, warps, median, window, iters, alpha, *lv), u.data_ptr(),
                 v.data_ptr(), pf, sm, *start, *_ws_args(workspace))
    return u, v


def consistency_device(uf, vf, ub, vb, rel: float = CONSISTENCY_REL,
                       abs: float = CONSISTENCY_ABS, err=None, mask=None, counts=None,
                       stream=None):
    """Forward-backward check of the flow (uf, vf) against the opposite flow
    (ub, vb), float32 CUDA tensors [B, H, W] (or [H, W]) in solver units
    (hsflow_flow_consistency_device in include/hsflow.h).  err / mask / counts:
    True to allocate, or a tensor to fill -- float32 like uf (pixels), uint8
    like uf (CONSISTENT / INCONSISTENT / OUT_OF_FRAME), int32 [B, 3] (pixels
    per class; the library's uint32 words); at least one.  Returns (err, mask,
    counts), None for those not asked for.  Stream-ordered."""
    dims = _dims(uf.shape)
    _check_planes(dims, uf=uf, vf=vf, ub=ub, vb=vb)
    err = _check_output(err, uf.shape, torch.float32, uf.device, "err")
    mask = _check_output(mask, uf.shape, torch.uint8, uf.device, "mask")
    counts = _check_output(counts, (dims[2], 3), torch.int32, uf.device, "counts")
    _device_call("hsflow_flow_consistency_device", uf.device, stream, uf.data_ptr(), vf.data_ptr(),
                 ub.data_ptr(), vb.data_ptr(), *dims, float(rel), float(abs), _ptr(err),
                 _ptr(mask), _ptr(counts))
    return err, mask, counts


def median_device(u, v, ksize: int, u_out=None, v_out=None, stream=None):
    """ksize x ksize (3 or 5, MEDIAN_SIZES) median of u and of v, each on its
    own: float32 CUDA tensors [B, H, W] (or [H, W]), border replicated, IEEE
    total order of the bit patterns, so each result is one of its taps bit
    for bit (hsflow_flow_median_device in include/hsflow.h).  Out of place:
    u_out, v_out are allocated unless given and must not overlap u or v.
    Returns (u_out, v_out).  Stream-ordered."""
    dims = _dims(u.shape)
    _check_planes(dims, u=u, v=v)
    u_out, v_out = _plane(u_out, u, dims, "u_out"), _plane(v_out, u, dims, "v_out")
    _device_call("hsflow_flow_median_device", u.device, stream, u.data_ptr(), v.data_ptr(), *dims,
                 int(ksize), u_out.data_ptr(), v_out.data_ptr())
    return u_out, v_out


def bidir_workspace_bytes(rows: int, cols: int, batch: int, levels: int) -> int:
    return int(lib().hsflow_flow_bidir_workspace_bytes(rows, cols, batch, levels))


def flow_bidir_device(I0, I1, levels: int, warps: int, window: int, iters: int, alpha: float,
                      rel: float = CONSISTENCY_REL, abs: float = CONSISTENCY_ABS,
                      uf=None, vf=None, ub=None, vb=None, err_f=None, mask_f=True,
                      counts_f=None, err_b=None, mask_b=None, counts_b=None, workspace=None,
                      stream=None, median: int = 0, prefilter=None, smoothness=None,
                      finest: int = 0):
    """Warped solve of I0 -> I1 (uf, vf) and I1 -> I0 (ub, vb) on torch CUDA
    tensors [B, H, W], then the forward-backward check each way
    (hsflow_flow_bidir_device in include/hsflow.h).  The flows equal
    flow_warped_device's bit for bit.  The six check outputs are as in
    consistency_device (True / tensor / None); a direction with none runs no
    check.  Returns a BidirDevice, None for outputs not asked for.
    `workspace`: bidir_workspace_bytes(rows, cols, batch, levels) bytes.
    median and prefilter (hsflow_flow_bidir_pf_device; prefilter_planes_bytes
    more workspace) as in flow_warped_device, for both directions; so is
    finest (hsflow_flow_bidir_lv_device), and the check runs on the
    full-resolution flows.  Stream-ordered."""
    return _flow_bidir_device(I0, I1, levels, warps, window, iters, alpha, rel, abs, uf, vf, ub,
                              vb, err_f, mask_f, counts_f, err_b, mask_b, counts_b, workspace,
                              stream, median, prefilter, smoothness, finest=finest)


def _flow_bidir_device(I0, I1, levels, warps, window, iters, alpha, rel, abs, uf, vf, ub, vb,
                       err_f, mask_f, counts_f, err_b, mask_b, counts_b, workspace, stream,
                       median, prefilter, smoothness, init=None, finest=0):
    """flow_bidir_device, from `init` (_init_entry) where given."""
    dims = _frame_pair(I0, I1)
    flows = [_plane(t, I0, dims, name)
             for t, name in ((uf, "uf"), (vf, "vf"), (ub, "ub"), (vb, "vb"))]
    outs = []
    for want, name in ((err_f, "err_f"), (mask_f, "mask_f"), (counts_f, "counts_f"),
                       (err_b, "err_b"), (mask_b, "mask_b"), (counts_b, "counts_b")):
        if name.startswith("counts"):
            outs.append(_check_output(want, (dims[2], 3), torch.int32, I0.device, name))
        else:
            outs.append(_check_output(
                want, I0.shape, torch.float32 if name.startswith("err") else torch.uint8,
                I0.device, name))
    pf, sm = _option(Prefilter, prefilter)[1], _option(Smoothness, smoothness)[1]
    workspace = _workspace(workspace, I0.device, bidir_workspace_bytes, *dims, levels,
                           prefilter=prefilter)
    name, lv, start = _init_entry("hsflow_flow_bidir", init, dims, finest)
    _device_call(name, I0.device, stream, I0.data_ptr(), I1.data_ptr(),
                 _tensor_dtype(I0), *dims,
                 *_solve_args(levels, warps, median, window, iters, alpha, *lv), float(rel),
                 float(abs),
                 *[t.data_ptr() for t in flows], *[_ptr(t) for t in outs], pf, sm, *start,
                 *_ws_args(workspace))
    return BidirDevice(*flows, *outs)


def warp_image_device(I, u, v, out=None, oof=None, stream=None):
    """Backward warp of the frames I (CUDA tensor [B, H, W] or [H, W], uint8 /
    float16 / float32 / float64) by the flow (u, v) (float32, solver units):
    out(y, x) = I sampled bilinearly at (y + 8 v, x + 8 u), the I1w of
    warp_gradients_device bit for bit (hsflow_warp_image_device in
    include/hsflow.h).  oof: True / a uint8 tensor like I to get 1 where the
    target leaves the frame by more than half a pixel.  Returns out (float32),
    or (out, oof) when oof was asked for.  Stream-ordered."""
    dims = _frame(I)
    _check_planes(dims, u=u, v=v)
    out = _plane(out, I, dims, "out")
    oof = _check_output(oof, I.shape, torch.uint8, I.device, "oof")
    _device_call("hsflow_warp_image_device", I.device, stream, I.data_ptr(), _tensor_dtype(I),
                 *dims, u.data_ptr(), v.data_ptr(), out.data_ptr(), _ptr(oof))
    return out if oof is None else (out, oof)


def _check_masks(shape, device, mask_f, mask_b):
    """The uint8 masks of the forward-backward check where given, of `shape`
    ([B, H, W], the frames' planes)."""
    for t, name in ((mask_f, "mask_f"), (mask_b, "mask_b")):
        if t is not None:
            _check_output(t, shape, torch.uint8, device, name)


def frame_interp_device(I0, I1, uf, vf, ub, vb, times, mask_f=None, mask_b=None, out=None,
                        out_dtype=None, flags=None, trusted=None, stream=None):
    """The frames at `times` (each in [0, 1]; at most MAX_TIMES) between I0 and
    I1 -- CUDA tensors [B, H, W] or [H, W], uint8 / float16 / float32 / float64
    -- from the flows I0 -> I1 (uf, vf) and I1 -> I0 (ub, vb), float32 in solver
    units (hsflow_frame_interp_device in include/hsflow.h).  mask_f, mask_b: the
    uint8 masks of consistency_device / flow_bidir_device, or None.  out:
    float32 (default) or uint8, [B, len(times), H, W]; flags (True / tensor):
    uint8 like out, FLAG_* bits; trusted (True / tensor): int32 [B, len(times)]
    (the library's uint32 words), pixels with flags == 0.  Returns (out, flags,
    trusted), None for those not asked for.  Stream-ordered."""
    dims = _frame_pair(I0, I1)
    _check_planes(dims, uf=uf, vf=vf, ub=ub, vb=vb)
    _check_masks(I0.shape, I0.device, mask_f, mask_b)
    tm = _times_array(times)
    out, flags, trusted = _interp_outputs(I0, (), len(tm), out, out_dtype, flags, trusted)
    _device_call("hsflow_frame_interp_device", I0.device, stream, I0.data_ptr(), I1.data_ptr(),
                 _tensor_dtype(I0), *dims, uf.data_ptr(), vf.data_ptr(), ub.data_ptr(),
                 vb.data_ptr(), _ptr(mask_f), _ptr(mask_b), tm, len(tm), out.data_ptr(),
                 _out_code(out), _ptr(flags), _ptr(trusted))
    return out, flags, trusted


def flow_interp_workspace_bytes(rows: int, cols: int, batch: int, levels: int) -> int:
    return int(lib().hsflow_flow_interp_workspace_bytes(rows, cols, batch, levels))


def flow_interp_device(I0, I1, times, levels: int, warps: int, window: int, iters: int,
                       alpha: float, median: int = 0, rel: float = CONSISTENCY_REL,
                       abs: float = CONSISTENCY_ABS, out=None, out_dtype=None, flags=None,
                       trusted=None, workspace=None, stream=None, prefilter=None,
                       smoothness=None, finest: int = 0, projection: int = 0, fallback=None,
                       cut=None):
    """flow_bidir_device(median=...) into planes of the workspace, then
    frame_interp_device with both masks: one call, the same bits
    (hsflow_flow_interp_device in include/hsflow.h).  `workspace`:
    flow_interp_workspace_bytes(rows, cols, batch, levels) bytes.  prefilter: a
    Prefilter; the flows then come from the prefiltered frames while the
    frames themselves are sampled (hsflow_flow_interp_pf_device;
    prefilter_planes_bytes more workspace).  finest as in flow_bidir_device
    (hsflow_flow_interp_lv_device): the flows of a coarse solve, the frames
    sampled at full resolution.  projection = 1: projection.project_device on
    the frames the solve ran on stands between the two and the interpolation
    is projection.frame_interp_device (hsflow_flow_interp_pj_device; the
    workspace grows by the cells, projection.flow_interp_workspace_bytes).
    fallback: a fallback.Fallback; both checks then always run and
    fallback.frame_fallback_device follows the interpolation
    (hsflow_flow_interp_fb_device; fallback.counts_bytes more workspace).  cut:
    True or a uint8 tensor [B] for the verdict per pair (zeros with the
    fallback off).  Returns (out, flags, trusted) as frame_interp_device, and
    cut behind them where it was asked for.  Stream-ordered."""
    return _flow_interp_device(I0, I1, times, levels, warps, window, iters, alpha, median, rel,
                               abs, out, out_dtype, flags, trusted, workspace, stream, prefilter,
                               smoothness, finest=finest, projection=projection,
                               fallback=fallback, cut=cut)


def _flow_interp_device(I0, I1, times, levels, warps, window, iters, alpha, median, rel, abs, out,
                        out_dtype, flags, trusted, workspace, stream, prefilter, smoothness,
                        init=None, finest=0, projection=0, fallback=None, cut=None):
    """flow_interp_device, from `init` (_init_entry) where given."""
    dims = _frame_pair(I0, I1)
    tm = _times_array(times)
    out, flags, trusted = _interp_outputs(I0, (), len(tm), out, out_dtype, flags, trusted)
    pf, sm = _option(Prefilter, prefilter)[1], _option(Smoothness, smoothness)[1]
    size_fn, size_args = _pj_size(flow_interp_workspace_bytes, "hsflow_flow_interp", projection,
                                  levels, len(tm))
    workspace = _workspace(workspace, I0.device, size_fn, *dims, *size_args, prefilter=prefilter,
                           fallback=fallback)
    name, lv, start, pj, cut, cut_arg, fb = _fb_entry("hsflow_flow_interp", init, dims, finest,
                                                      projection, fallback, cut, I0.device)
    _device_call(name, I0.device, stream, I0.data_ptr(), I1.data_ptr(),
                 _tensor_dtype(I0), *dims,
                 *_solve_args(levels, warps, median, window, iters, alpha, *lv), float(rel),
                 float(abs), tm, len(tm), *pj, out.data_ptr(), _out_code(out), _ptr(flags),
                 _ptr(trusted), *cut_arg, pf, sm, *start, *fb, *_ws_args(workspace))
    return (out, flags, trusted) if cut is None else (out, flags, trusted, cut)


def _check_bgr(t, name):
    """A batch of dense interleaved BGR frames: uint8, contiguous, CUDA,
    [B, H, W, 3] or [H, W, 3].  Returns (rows, cols, batch)."""
    if torch is None or not isinstance(t, torch.Tensor) or t.dtype != torch.uint8 or \
            t.dim() not in (3, 4) or t.shape[-1] != 3 or not t.is_cuda or not t.is_contiguous():
        raise HsflowError(HSFLOW_ERR_ARG, f"{name}: need a contiguous uint8 CUDA tensor "
                          "[B, H, W, 3] or [H, W, 3]")
    return _dims(t.shape[:-1])


def _bgr_pair(bgr0, bgr1):
    """(rows, cols, batch) of the BGR frames bgr0 and bgr1, of one shape."""
    dims = _check_bgr(bgr0, "bgr0")
    _check_bgr(bgr1, "bgr1")
    if bgr1.shape != bgr0.shape:
        raise HsflowError(HSFLOW_ERR_SIZE, "bgr0/bgr1 differ in shape")
    return dims


def warp_image_bgr_device(bgr, u, v, out=None, out_dtype=None, oof=None, stream=None):
    """warp_image_device for colour frames: bgr a uint8 CUDA tensor [B, H, W, 3]
    or [H, W, 3], (u, v) float32 [B, H, W] in solver units; out(y, x, c) =
    bgr(.., c) at (y + 8 v, x + 8 u), each channel the bits warp_image_device
    gives its plane (hsflow_warp_image_bgr_device in include/hsflow.h).  out:
    float32 (default) or uint8, like bgr; oof: True / a uint8 tensor [B, H, W].
    Returns out, or (out, oof) when oof was asked for.  Stream-ordered."""
    dims = _check_bgr(bgr, "bgr")
    _check_planes(dims, u=u, v=v)
    out = _out_frames(out, bgr.shape, out_dtype, bgr.device)
    oof = _check_output(oof, bgr.shape[:-1], torch.uint8, bgr.device, "oof")
    _device_call("hsflow_warp_image_bgr_device", bgr.device, stream, bgr.data_ptr(), *dims,
                 u.data_ptr(), v.data_ptr(), out.data_ptr(), _out_code(out), _ptr(oof))
    return out if oof is None else (out, oof)


def frame_interp_bgr_device(bgr0, bgr1, uf, vf, ub, vb, times, mask_f=None, mask_b=None,
                            out=None, out_dtype=None, flags=None, trusted=None, stream=None):
    """frame_interp_device for colour frames: bgr0, bgr1 uint8 CUDA tensors
    [B, H, W, 3] or [H, W, 3]; flows, masks and times as there (the flow is a
    grey-level quantity).  out: float32 (default) or uint8, [B, len(times), H,
    W, 3], channel c the bits frame_interp_device gives the plane bgr[..., c];
    flags [B, len(times), H, W] and trusted [B, len(times)] are per pixel
    (hsflow_frame_interp_bgr_device in include/hsflow.h).  Returns (out, flags,
    trusted), None for those not asked for.  Stream-ordered."""
    dims = _bgr_pair(bgr0, bgr1)
    _check_planes(dims, uf=uf, vf=vf, ub=ub, vb=vb)
    _check_masks(bgr0.shape[:-1], bgr0.device, mask_f, mask_b)
    tm = _times_array(times)
    out, flags, trusted = _interp_outputs(bgr0, (3,), len(tm), out, out_dtype, flags, trusted)
    _device_call("hsflow_frame_interp_bgr_device", bgr0.device, stream, bgr0.data_ptr(),
                 bgr1.data_ptr(), *dims, uf.data_ptr(), vf.data_ptr(), ub.data_ptr(),
                 vb.data_ptr(), _ptr(mask_f), _ptr(mask_b), tm, len(tm), out.data_ptr(),
                 _out_code(out), _ptr(flags), _ptr(trusted))
    return out, flags, trusted


def flow_interp_bgr_workspace_bytes(rows: int, cols: int, batch: int, levels: int) -> int:
    return int(lib().hsflow_flow_interp_bgr_workspace_bytes(rows, cols, batch, levels))


def flow_interp_bgr_device(bgr0, bgr1, times, levels: int, warps: int, window: int, iters: int,
                           alpha: float, median: int = 0, rel: float = CONSISTENCY_REL,
                           abs: float = CONSISTENCY_ABS, out=None, out_dtype=None, flags=None,
                           trusted=None, workspace=None, stream=None, prefilter=None,
                           smoothness=None, finest: int = 0, projection: int = 0, fallback=None,
                           cut=None):
    """bgr_to_gray_device of both frames, flow_bidir_device(median=...) on the
    grey planes, then frame_interp_bgr_device with both masks: one call, the
    same bits (hsflow_flow_interp_bgr_device in include/hsflow.h).
    `workspace`: flow_interp_bgr_workspace_bytes(rows, cols, batch, levels)
    bytes.  prefilter: a Prefilter run on the grey planes in front of the
    solve (hsflow_flow_interp_bgr_pf_device; prefilter_planes_bytes more
    workspace).  finest as in flow_interp_device
    (hsflow_flow_interp_bgr_lv_device); projection likewise, the cells made
    from the grey planes (hsflow_flow_interp_bgr_pj_device;
    projection.flow_interp_bgr_workspace_bytes); fallback and cut likewise
    (hsflow_flow_interp_bgr_fb_device).  Returns (out, flags, trusted) as
    frame_interp_bgr_device, and cut where asked for.  Stream-ordered."""
    return _flow_interp_bgr_device(bgr0, bgr1, times, levels, warps, window, iters, alpha, median,
                                   rel, abs, out, out_dtype, flags, trusted, workspace, stream,
                                   prefilter, smoothness, finest=finest, projection=projection,
                                   fallback=fallback, cut=cut)


def _flow_interp_bgr_device(bgr0, bgr1, times, levels, warps, window, iters, alpha, median, rel,
                            abs, out, out_dtype, flags, trusted, workspace, stream, prefilter,
                            smoothness, init=None, finest=0, projection=0, fallback=None,
                            cut=None):
    """flow_interp_bgr_device, from `init` (_init_entry) where given."""
    dims = _bgr_pair(bgr0, bgr1)
    tm = _times_array(times)
    out, flags, trusted = _interp_outputs(bgr0, (3,), len(tm), out, out_dtype, flags, trusted)
    pf, sm = _option(Prefilter, prefilter)[1], _option(Smoothness, smoothness)[1]
    size_fn, size_args = _pj_size(flow_interp_bgr_workspace_bytes, "hsflow_flow_interp_bgr",
                                  projection, levels, len(tm))
    workspace = _workspace(workspace, bgr0.device, size_fn, *dims, *size_args, prefilter=prefilter,
                           fallback=fallback)
    name, lv, start, pj, cut, cut_arg, fb = _fb_entry("hsflow_flow_interp_bgr", init, dims, finest,
                                                      projection, fallback, cut, bgr0.device)
    _device_call(name, bgr0.device, stream, bgr0.data_ptr(), bgr1.data_ptr(), *dims,
                 *_solve_args(levels, warps, median, window, iters, alpha, *lv), float(rel),
                 float(abs), tm, len(tm), *pj, out.data_ptr(), _out_code(out), _ptr(flags),
                 _ptr(trusted), *cut_arg, pf, sm, *start, *fb, *_ws_args(workspace))
    return (out, flags, trusted) if cut is None else (out, flags, trusted, cut)


def prefilter_planes_bytes(rows: int, cols: int, batch: int = 1) -> int:
    """Workspace a solve with prefilter= needs on top of its own size function."""
    return int(lib().hsflow_prefilter_planes_bytes(rows, cols, batch))


def _pf_extra(prefilter, rows, cols, batch) -> int:
    on = prefilter is not None and int(prefilter[0]) != PREFILTER_NONE
    return prefilter_planes_bytes(rows, cols, batch) if on else 0


def prefilter_device(I, prefilter, out=None, stream=None):
    """The prefilter alone (hsflow_prefilter_device in include/hsflow.h): I a
    torch CUDA tensor [B, H, W] or [H, W] (uint8 / float16 / float32 /
    float64) -> float32 of the same shape: v = I - G*I (PREFILTER_HIGHPASS) or
    scale * v / (sqrt(G*(v v)) + eps) (PREFILTER_NORMALIZE).  `out` must not
    overlap I.  One launch, no workspace.  Stream-ordered."""
    dims = _frame(I)
    if prefilter is None:
        raise HsflowError(HSFLOW_ERR_ARG, "prefilter_device needs a Prefilter")
    out = _plane(out, I, dims, "out")
    _device_call("hsflow_prefilter_device", I.device, stream, I.data_ptr(), _tensor_dtype(I),
                 *dims, _option(Prefilter, prefilter)[1], out.data_ptr())
    return out


def set_interp_bgr_loads(wide: bool) -> bool:
    """hsflow_set_interp_bgr_loads: the BGR kernels fetch a row's two adjacent
    taps as six bytes (False, default) or as one unaligned dword and halfword;
    same bits.  Returns the previous setting."""
    return bool(lib().hsflow_set_interp_bgr_loads(1 if wide else 0))


def warp_gradients_device(I0, I1, u0, v0, workspace, gx=None, gy=None, gt=None, stream=None):
    """Gradients linearised around the flow (u0, v0) (float32 tensors of the
    frames' shape) into the workspace's f32 planes, optionally also into
    gx/gy/gt; jacobi_device(warm_start=True) on (u0, v0) then runs one warp's
    iterations.  gx, gy equal gradients_device's planes bit for bit."""
    dims = _frame_pair(I0, I1)
    _check_planes(dims, u0=u0, v0=v0)
    for t, name in ((gx, "gx"), (gy, "gy"), (gt, "gt")):
        if t is not None:
            _check_plane(t, dims[:2], dims[2], name)
    _device_call("hsflow_warp_gradients_device", I0.device, stream, I0.data_ptr(), I1.data_ptr(),
                 _tensor_dtype(I0), *dims, u0.data_ptr(), v0.data_ptr(), _ptr(gx), _ptr(gy),
                 _ptr(gt), *_ws_args(workspace))


def pyramid_build_device(I0, I1, levels: int, workspace=None, stream=None):
    """Levels 1..levels-1 of both frames (f32 tensors [B, h_l, w_l]), the
    same planes hsflow_flow_pyramid_device builds internally."""
    dims = _frame_pair(I0, I1, same=False)
    lead = tuple(I0.shape[:-2])
    P0, P1 = [], []
    for l in range(1, levels):
        r, c = pyramid_level_size(dims[0], dims[1], l)
        P0.append(torch.empty(lead + (r, c), dtype=torch.float32, device=I0.device))
        P1.append(torch.empty(lead + (r, c), dtype=torch.float32, device=I0.device))
    workspace = _workspace(workspace, I0.device, workspace_bytes, *dims)
    n = max(1, levels - 1)
    a0 = (_vp * n)(*[t.data_ptr() for t in P0]) if P0 else (_vp * 1)()
    a1 = (_vp * n)(*[t.data_ptr() for t in P1]) if P1 else (_vp * 1)()
    _device_call("hsflow_pyramid_build_device", I0.device, stream, I0.data_ptr(), I1.data_ptr(),
                 _tensor_dtype(I0), *dims, int(levels), a0, a1, *_ws_args(workspace))
    return P0, P1


def upflow_device(uc, vc, u, v, stream=None):
    """u = 2 uc(y/2, x/2), v likewise (the pyramid's warm start); u, v and
    uc, vc are dense [rows, cols] / [rc, cc] views (row slices allowed)."""
    rc, cc = uc.shape[-2:]
    rows, cols = u.shape[-2:]
    _check_planes((rc, cc, 1), uc=uc, vc=vc)
    _check_planes((rows, cols, 1), u=u, v=v)
    _device_call("hsflow_upflow_device", u.device, stream, uc.data_ptr(), vc.data_ptr(), rc, cc,
                 u.data_ptr(), v.data_ptr(), rows, cols, 1)


def gradients_device(I0, I1, workspace, gx=None, gy=None, gt=None, stream=None):
    dims = _frame_pair(I0, I1, same=False)
    _device_call("hsflow_gradients_device", I0.device, stream, I0.data_ptr(), I1.data_ptr(),
                 _tensor_dtype(I0), *dims, _ptr(gx), _ptr(gy), _ptr(gt), *_ws_args(workspace))


def jacobi_device(rows, cols, batch, window, iters, alpha, u, v, workspace,
                  warm_start=False, stream=None):
    _check_planes((rows, cols, batch), u=u, v=v)
    _device_call("hsflow_jacobi_device", u.device, stream, int(rows), int(cols), int(batch),
                 int(window), int(iters), float(alpha), int(bool(warm_start)), u.data_ptr(),
                 v.data_ptr(), *_ws_args(workspace))


def diffusivity_device(u, v, lam: float, g=None, stream=None):
    """The flow-driven smoothness weights alone (hsflow_flow_diffusivity_device
    in include/hsflow.h): g = 1 / sqrt(1 + |grad (8u, 8v)|^2 / lam^2) of float32
    CUDA tensors [B, H, W] (or [H, W]) in solver units, central differences,
    border replicated.  g is allocated unless given and must not overlap u or
    v.  Returns g.  Stream-ordered."""
    dims = _dims(u.shape)
    _check_planes(dims, u=u, v=v)
    g = _plane(g, u, dims, "g")
    _device_call("hsflow_flow_diffusivity_device", u.device, stream, u.data_ptr(), v.data_ptr(),
                 *dims, float(lam), g.data_ptr())
    return g


def jacobi_weighted_device(rows, cols, batch, window, iters, alpha, g, u, v, workspace,
                           stream=None):
    """`iters` g-weighted iterations warm-started from (u, v), in place, from
    the f32 gradient planes warp_gradients_device left in `workspace`
    (hsflow_jacobi_weighted_device in include/hsflow.h); window 3 or 5."""
    _check_planes((rows, cols, batch), g=g, u=u, v=v)
    _device_call("hsflow_jacobi_weighted_device", u.device, stream, int(rows), int(cols),
                 int(batch), int(window), int(iters), float(alpha), g.data_ptr(), u.data_ptr(),
                 v.data_ptr(), *_ws_args(workspace))


def set_iters_per_launch(k: int):
    _check(lib().hsflow_set_iters_per_launch(int(k)))


def set_max_streams(n: int):
    """Side streams a batch is split over: 0 = automatic (2 for eager calls,
    none under stream capture), n >= 1 = up to n always."""
    _check(lib().hsflow_set_max_streams(int(n)))


def max_streams() -> int:
    """The current set_max_streams setting (0 = automatic)."""
    return int(lib().hsflow_max_streams())


class max_streams_as:
    """Context manager: set_max_streams(n) inside, the previous setting after."""

    def __init__(self, n: int):
        self.n = int(n)

    def __enter__(self):
        self.prev = max_streams()
        set_max_streams(self.n)
        return self

    def __exit__(self, *exc):
        set_max_streams(self.prev)
        return False


def set_first_pass_fusion(on: bool):
    """A cold K4 solve computes its gradients inside its first pass (True,
    the default) or in K1 in front of it (False); identical bits
    (include/hsflow.h)."""
    _check(lib().hsflow_set_first_pass_fusion(int(bool(on))))


def first_pass_fusion() -> bool:
    """The current set_first_pass_fusion setting."""
    return bool(lib().hsflow_first_pass_fusion())


def first_pass_launches() -> int:
    """Fused first passes launched by this process so far (one per side-stream
    chain of a fused solve); its difference across a call tells whether it fused."""
    return int(lib().hsflow_first_pass_launches())


class first_pass_fusion_as:
    """Context manager: set_first_pass_fusion(on) inside, the previous setting after."""

    def __init__(self, on: bool):
        self.on = bool(on)

    def __enter__(self):
        self.prev = first_pass_fusion()
        set_first_pass_fusion(self.on)
        return self

    def __exit__(self, *exc):
        set_first_pass_fusion(self.prev)
        return False


def set_jacobi_kernel(k: int):
    """Jacobi pass kernel: 0 = automatic (K4 streaming strips where built,
    K2 register tiles elsewhere), 2 = K2 everywhere, 4 = K4 where built;
    identical bits (include/hsflow.h)."""
    _check(lib().hsflow_set_jacobi_kernel(int(k)))


def set_strip_rows(seg_rows: int = 0):
    """K4 rows per segment (0 = automatic); identical bits for any choice."""
    _check(lib().hsflow_set_strip_rows(int(seg_rows)))


def jacobi_kernel_name(rows, cols, batch, window) -> str:
    """The kernel that runs this shape's full-depth Jacobi passes."""
    return lib().hsflow_jacobi_kernel_name(int(rows), int(cols), int(batch),
                                           int(window)).decode()


def iters_per_launch(rows, cols, batch, window) -> int:
    return int(lib().hsflow_iters_per_launch(rows, cols, batch, window))


# ------------------------------------------------------------------ host utils
def bgr_to_gray(bgr) -> np.ndarray:
    """main.cpp:13-14 cvtColor(BGR2GRAY), OpenCV 4.x 15-bit fixed point."""
    bgr = _host_bgr(np.asarray(bgr, np.uint8))
    rows, cols = bgr.shape[:2]
    out = np.empty((rows, cols), np.uint8)
    _check(lib().hsflow_bgr_to_gray(bgr.ctypes.data, rows, cols, bgr.strides[0],
                                    out.ctypes.data, out.strides[0]))
    return out


def bgr_to_gray_device(bgr, gray=None, stream=None):
    """Device BGR->gray (same integer formula) on a uint8 CUDA tensor
    [..., H, W, 3] -> [..., H, W].  Stream-ordered."""
    if bgr.dtype != torch.uint8 or bgr.dim() < 3 or bgr.shape[-1] != 3 or \
            not bgr.is_cuda or not bgr.is_contiguous():
        raise HsflowError(HSFLOW_ERR_ARG, "need a contiguous uint8 CUDA tensor [..., H, W, 3]")
    rows, cols, batch = _dims(bgr.shape[:-1])
    if gray is None:
        gray = torch.empty(bgr.shape[:-1], dtype=torch.uint8, device=bgr.device)
    if gray.dtype != torch.uint8 or not gray.is_cuda or not gray.is_contiguous() or \
            gray.numel() < batch * rows * cols or gray.device != bgr.device:
        raise HsflowError(HSFLOW_ERR_ARG, "gray: need a contiguous uint8 CUDA tensor of "
                          f"{batch} x {rows} x {cols} on {bgr.device}")
    _device_call("hsflow_bgr_to_gray_device", bgr.device, stream, bgr.data_ptr(), rows, cols,
                 batch, gray.data_ptr())
    return gray


def synth_pair(seed: int, rows: int, cols: int, qdy: int = -3, qdx: int = 6,
               dtype=np.float32):
    """Deterministic synthetic pair: motion (dy, dx) = (qdy, qdx)/4
    px, default (-0.75, +1.5).  Seed convention: 1000 + pair index."""
    I0 = np.empty((rows, cols), dtype)
    I1 = np.empty((rows, cols), dtype)
    if dtype == np.float32:
        args = (I0.ctypes.data, I1.ctypes.data, None, None)
    elif dtype == np.uint8:
        args = (None, None, I0.ctypes.data, I1.ctypes.data)
    else:
        raise HsflowError(HSFLOW_ERR_ARG, "synth dtype must be float32 or uint8")
    _check(lib().hsflow_synth_pair(int(seed), rows, cols, int(qdy), int(qdx), *args))
    return I0, I1
