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

# every symbol include/hsflow.h declares
EXPORTS = (
    "hsflow_version", "hsflow_status_string", "hsflow_create", "hsflow_destroy",
    "hsflow_last_error", "hsflow_stream", "hsflow_flow", "hsflow_gradients",
    "hsflow_workspace_bytes", "hsflow_flow_device", "hsflow_gradients_device",
    "hsflow_jacobi_device", "hsflow_set_iters_per_launch", "hsflow_iters_per_launch",
    "hsflow_bgr_to_gray", "hsflow_synth_pair", "hsflow_set_max_streams",
    "hsflow_pyramid_level_size", "hsflow_pyramid_workspace_bytes",
    "hsflow_flow_pyramid_device", "hsflow_flow_pyramid", "hsflow_bgr_to_gray_device",
    "hsflow_flow_bgr", "hsflow_pyramid_build_device", "hsflow_upflow_device",
    "hsflow_set_jacobi_kernel", "hsflow_build_flags", "hsflow_flow_multi",
    "hsflow_download_device", "hsflow_jacobi_kernel_name", "hsflow_set_strip_rows",
    "hsflow_max_streams", "hsflow_set_output_hugepages", "hsflow_strip_seg_rows",
    "hsflow_flow_multi_release", "hsflow_warp_gradients_device",
    "hsflow_flow_warped_device", "hsflow_flow_warped",
    "hsflow_flow_consistency_device", "hsflow_flow_bidir_workspace_bytes",
    "hsflow_flow_bidir_device", "hsflow_flow_bidir",
    "hsflow_flow_median_device", "hsflow_flow_warped_median_device",
    "hsflow_flow_warped_median", "hsflow_flow_bidir_median_device",
    "hsflow_flow_bidir_median",
    "hsflow_warp_image_device", "hsflow_frame_interp_device",
    "hsflow_flow_interp_workspace_bytes", "hsflow_flow_interp_device", "hsflow_flow_interp",
    "hsflow_set_first_pass_fusion", "hsflow_first_pass_fusion",
    "hsflow_first_pass_launches",
    "hsflow_warp_image_bgr_device", "hsflow_frame_interp_bgr_device",
    "hsflow_flow_interp_bgr_workspace_bytes", "hsflow_flow_interp_bgr_device",
    "hsflow_flow_interp_bgr", "hsflow_set_interp_bgr_loads",
    "hsflow_prefilter_device", "hsflow_prefilter_planes_bytes",
    "hsflow_flow_warped_pf_device", "hsflow_flow_bidir_pf_device",
    "hsflow_flow_interp_pf_device", "hsflow_flow_interp_bgr_pf_device",
    "hsflow_ctx_set_prefilter", "hsflow_ctx_prefilter",
    "hsflow_flow_diffusivity_device", "hsflow_jacobi_weighted_device",
    "hsflow_flow_warped_sm_device", "hsflow_flow_bidir_sm_device",
    "hsflow_flow_interp_sm_device", "hsflow_flow_interp_bgr_sm_device",
    "hsflow_ctx_set_smoothness", "hsflow_ctx_smoothness",
)

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

    def __new__(cls, mode, sigma=4.0, eps=4.0, scale=32.0):
        return super().__new__(cls, int(mode), float(sigma), float(eps), float(scale))

    def _c(self):
        return _CPrefilter(self.mode, self.sigma, self.eps, self.scale)


def _pf_arg(prefilter):
    """(keep-alive struct, pointer or None) of a Prefilter / None."""
    if prefilter is None:
        return None, None
    if not isinstance(prefilter, Prefilter):
        prefilter = Prefilter(*prefilter)
    c = prefilter._c()
    return c, ctypes.byref(c)


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

    def __new__(cls, mode=SMOOTH_FLOW_DRIVEN, lam=0.3):
        return super().__new__(cls, int(mode), float(lam))

    def _c(self):
        return _CSmoothness(self.mode, self.lam)


def _sm_arg(smoothness):
    """(keep-alive struct, pointer or None) of a Smoothness / None."""
    if smoothness is None:
        return None, None
    if not isinstance(smoothness, Smoothness):
        smoothness = Smoothness(*smoothness)
    c = smoothness._c()
    return c, ctypes.byref(c)


BidirHost = collections.namedtuple("BidirHost", "u v ub vb mask_f mask_b counts")
BidirDevice = collections.namedtuple(
    "BidirDevice", "uf vf ub vb err_f mask_f counts_f err_b mask_b counts_b")


class HsflowError(RuntimeError):
    """A non-zero hsflow status (the reference would throw cv::Exception)."""

    def __init__(self, status: int, msg: str):
        super().__init__(f"hsflow status {status}: {msg}")
        self.status = status


_lib = None
_vp = ctypes.c_void_p
_sz = ctypes.c_size_t


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
    i = ctypes.c_int
    L.hsflow_version.restype = i
    L.hsflow_status_string.restype = ctypes.c_char_p
    L.hsflow_status_string.argtypes = [i]
    L.hsflow_create.argtypes = [ctypes.POINTER(_vp), i]
    L.hsflow_destroy.argtypes = [_vp]
    L.hsflow_destroy.restype = None
    L.hsflow_last_error.argtypes = [_vp]
    L.hsflow_last_error.restype = ctypes.c_char_p
    L.hsflow_stream.argtypes = [_vp]
    L.hsflow_stream.restype = _vp
    L.hsflow_build_flags.restype = i
    L.hsflow_flow.argtypes = [_vp, _vp, _vp, i, i, i, _sz, _sz, i, i, ctypes.c_double,
                              _vp, _vp, i, _sz]
    L.hsflow_gradients.argtypes = [_vp, _vp, _vp, i, i, i, _sz, _sz, _vp, _vp, _vp, i,
                                   _sz]
    L.hsflow_workspace_bytes.argtypes = [i, i, i]
    L.hsflow_workspace_bytes.restype = _sz
    L.hsflow_flow_device.argtypes = [_vp, _vp, i, i, i, i, i, i, ctypes.c_float,
                                     _vp, _vp, _vp, _sz, _vp]
    L.hsflow_gradients_device.argtypes = [_vp, _vp, i, i, i, i, _vp, _vp, _vp,
                                          _vp, _sz, _vp]
    L.hsflow_jacobi_device.argtypes = [i, i, i, i, i, ctypes.c_float, i, _vp, _vp,
                                       _vp, _sz, _vp]
    L.hsflow_set_iters_per_launch.argtypes = [i]
    L.hsflow_iters_per_launch.argtypes = [i, i, i, i]
    L.hsflow_set_max_streams.argtypes = [i]
    L.hsflow_strip_seg_rows.argtypes = [i, i, i, i]
    L.hsflow_strip_seg_rows.restype = i
    L.hsflow_set_output_hugepages.argtypes = [i]
    L.hsflow_set_output_hugepages.restype = i
    L.hsflow_max_streams.argtypes = []
    L.hsflow_set_first_pass_fusion.argtypes = [i]
    L.hsflow_first_pass_fusion.argtypes = []
    L.hsflow_first_pass_launches.argtypes = []
    L.hsflow_first_pass_launches.restype = ctypes.c_longlong
    L.hsflow_set_jacobi_kernel.argtypes = [i]
    L.hsflow_set_strip_rows.argtypes = [i]
    L.hsflow_jacobi_kernel_name.argtypes = [i, i, i, i]
    L.hsflow_jacobi_kernel_name.restype = ctypes.c_char_p
    L.hsflow_pyramid_level_size.argtypes = [i, i, i, ctypes.POINTER(i), ctypes.POINTER(i)]
    L.hsflow_pyramid_workspace_bytes.argtypes = [i, i, i, i]
    L.hsflow_pyramid_workspace_bytes.restype = _sz
    L.hsflow_flow_pyramid_device.argtypes = [_vp, _vp, i, i, i, i, i, i, i,
                                             ctypes.c_float, _vp, _vp, _vp, _sz, _vp]
    L.hsflow_flow_pyramid.argtypes = [_vp, _vp, _vp, i, i, i, _sz, _sz, i, i, i,
                                      ctypes.c_double, _vp, _vp, i, _sz]
    L.hsflow_warp_gradients_device.argtypes = [_vp, _vp, i, i, i, i, _vp, _vp, _vp, _vp,
                                               _vp, _vp, _sz, _vp]
    L.hsflow_flow_warped_device.argtypes = [_vp, _vp, i, i, i, i, i, i, i, i,
                                            ctypes.c_float, _vp, _vp, _vp, _sz, _vp]
    L.hsflow_flow_warped.argtypes = [_vp, _vp, _vp, i, i, i, _sz, _sz, i, i, i, i,
                                     ctypes.c_double, _vp, _vp, i, _sz]
    f = ctypes.c_float
    L.hsflow_flow_consistency_device.argtypes = [_vp, _vp, _vp, _vp, i, i, i, f, f, _vp, _vp,
                                                 _vp, _vp]
    L.hsflow_flow_bidir_workspace_bytes.argtypes = [i, i, i, i]
    L.hsflow_flow_bidir_workspace_bytes.restype = _sz
    L.hsflow_flow_bidir_device.argtypes = [_vp, _vp, i, i, i, i, i, i, i, i, f, f, f,
                                           _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp,
                                           _vp, _sz, _vp]
    L.hsflow_flow_bidir.argtypes = [_vp, _vp, _vp, i, i, i, _sz, _sz, i, i, i, i,
                                    ctypes.c_double, f, f, _vp, _vp, _vp, _vp, i, _sz, _vp,
                                    _vp, _sz, _vp]
    L.hsflow_flow_median_device.argtypes = [_vp, _vp, i, i, i, i, _vp, _vp, _vp]
    L.hsflow_flow_warped_median_device.argtypes = [_vp, _vp, i, i, i, i, i, i, i, i, i, f,
                                                   _vp, _vp, _vp, _sz, _vp]
    L.hsflow_flow_warped_median.argtypes = [_vp, _vp, _vp, i, i, i, _sz, _sz, i, i, i, i, i,
                                            ctypes.c_double, _vp, _vp, i, _sz]
    L.hsflow_flow_bidir_median_device.argtypes = [_vp, _vp, i, i, i, i, i, i, i, i, i, f, f, f,
                                                  _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp,
                                                  _vp, _vp, _sz, _vp]
    L.hsflow_flow_bidir_median.argtypes = [_vp, _vp, _vp, i, i, i, _sz, _sz, i, i, i, i, i,
                                           ctypes.c_double, f, f, _vp, _vp, _vp, _vp, i, _sz,
                                           _vp, _vp, _sz, _vp]
    fp = ctypes.POINTER(f)
    L.hsflow_warp_image_device.argtypes = [_vp, i, i, i, i, _vp, _vp, _vp, _vp, _vp]
    L.hsflow_frame_interp_device.argtypes = [_vp, _vp, i, i, i, i, _vp, _vp, _vp, _vp, _vp, _vp,
                                             fp, i, _vp, i, _vp, _vp, _vp]
    L.hsflow_flow_interp_workspace_bytes.argtypes = [i, i, i, i]
    L.hsflow_flow_interp_workspace_bytes.restype = _sz
    L.hsflow_flow_interp_device.argtypes = [_vp, _vp, i, i, i, i, i, i, i, i, i, f, f, f, fp, i,
                                            _vp, i, _vp, _vp, _vp, _sz, _vp]
    L.hsflow_flow_interp.argtypes = [_vp, _vp, _vp, i, i, i, _sz, _sz, i, i, i, i, i,
                                     ctypes.c_double, f, f, fp, i, ctypes.POINTER(_vp), i, _sz,
                                     ctypes.POINTER(_vp), _sz, _vp]
    L.hsflow_warp_image_bgr_device.argtypes = [_vp, i, i, i, _vp, _vp, _vp, i, _vp, _vp]
    L.hsflow_frame_interp_bgr_device.argtypes = [_vp, _vp, i, i, i, _vp, _vp, _vp, _vp, _vp, _vp,
                                                 fp, i, _vp, i, _vp, _vp, _vp]
    L.hsflow_flow_interp_bgr_workspace_bytes.argtypes = [i, i, i, i]
    L.hsflow_flow_interp_bgr_workspace_bytes.restype = _sz
    L.hsflow_flow_interp_bgr_device.argtypes = [_vp, _vp, i, i, i, i, i, i, i, i, f, f, f, fp, i,
                                                _vp, i, _vp, _vp, _vp, _sz, _vp]
    L.hsflow_flow_interp_bgr.argtypes = [_vp, _vp, _vp, i, i, _sz, _sz, i, i, i, i, i,
                                         ctypes.c_double, f, f, fp, i, ctypes.POINTER(_vp), i,
                                         _sz, ctypes.POINTER(_vp), _sz, _vp]
    L.hsflow_set_interp_bgr_loads.argtypes = [i]
    pfp = ctypes.POINTER(_CPrefilter)
    L.hsflow_prefilter_device.argtypes = [_vp, i, i, i, i, pfp, _vp, _vp]
    L.hsflow_prefilter_planes_bytes.argtypes = [i, i, i]
    L.hsflow_prefilter_planes_bytes.restype = _sz
    L.hsflow_flow_warped_pf_device.argtypes = [_vp, _vp, i, i, i, i, i, i, i, i, i, f,
                                               _vp, _vp, pfp, _vp, _sz, _vp]
    L.hsflow_flow_bidir_pf_device.argtypes = [_vp, _vp, i, i, i, i, i, i, i, i, i, f, f, f,
                                              _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp,
                                              _vp, pfp, _vp, _sz, _vp]
    L.hsflow_flow_interp_pf_device.argtypes = [_vp, _vp, i, i, i, i, i, i, i, i, i, f, f, f, fp,
                                               i, _vp, i, _vp, _vp, pfp, _vp, _sz, _vp]
    L.hsflow_flow_interp_bgr_pf_device.argtypes = [_vp, _vp, i, i, i, i, i, i, i, i, f, f, f, fp,
                                                   i, _vp, i, _vp, _vp, pfp, _vp, _sz, _vp]
    L.hsflow_ctx_set_prefilter.argtypes = [_vp, pfp]
    L.hsflow_ctx_prefilter.argtypes = [_vp, pfp]
    smp = ctypes.POINTER(_CSmoothness)
    L.hsflow_flow_diffusivity_device.argtypes = [_vp, _vp, i, i, i, f, _vp, _vp]
    L.hsflow_jacobi_weighted_device.argtypes = [i, i, i, i, i, f, _vp, _vp, _vp, _vp, _sz, _vp]
    L.hsflow_flow_warped_sm_device.argtypes = [_vp, _vp, i, i, i, i, i, i, i, i, i, f,
                                               _vp, _vp, pfp, smp, _vp, _sz, _vp]
    L.hsflow_flow_bidir_sm_device.argtypes = [_vp, _vp, i, i, i, i, i, i, i, i, i, f, f, f,
                                              _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp,
                                              _vp, pfp, smp, _vp, _sz, _vp]
    L.hsflow_flow_interp_sm_device.argtypes = [_vp, _vp, i, i, i, i, i, i, i, i, i, f, f, f, fp,
                                               i, _vp, i, _vp, _vp, pfp, smp, _vp, _sz, _vp]
    L.hsflow_flow_interp_bgr_sm_device.argtypes = [_vp, _vp, i, i, i, i, i, i, i, i, f, f, f, fp,
                                                   i, _vp, i, _vp, _vp, pfp, smp, _vp, _sz, _vp]
    L.hsflow_ctx_set_smoothness.argtypes = [_vp, smp]
    L.hsflow_ctx_smoothness.argtypes = [_vp, smp]
    L.hsflow_pyramid_build_device.argtypes = [_vp, _vp, i, i, i, i, i,
                                              ctypes.POINTER(_vp), ctypes.POINTER(_vp),
                                              _vp, _sz, _vp]
    L.hsflow_upflow_device.argtypes = [_vp, _vp, i, i, _vp, _vp, i, i, i, _vp]
    L.hsflow_bgr_to_gray_device.argtypes = [_vp, i, i, i, _vp, _vp]
    L.hsflow_flow_bgr.argtypes = [_vp, _vp, _vp, i, i, _sz, _sz, i, i, ctypes.c_double,
                                  _vp, _vp, i, _sz]
    L.hsflow_bgr_to_gray.argtypes = [_vp, i, i, _sz, _vp, _sz]
    L.hsflow_synth_pair.argtypes = [ctypes.c_uint64, i, i, i, i, _vp, _vp, _vp, _vp]
    L.hsflow_download_device.argtypes = [_vp, _vp, _sz, _vp]
    L.hsflow_flow_multi.argtypes = [ctypes.POINTER(i), i, i, ctypes.POINTER(_vp),
                                    ctypes.POINTER(_vp), i, i, i, _sz, _sz, i, i,
                                    ctypes.c_double, ctypes.POINTER(_vp),
                                    ctypes.POINTER(_vp), i, _sz]
    L.hsflow_flow_multi_release.argtypes = []
    L.hsflow_flow_multi_release.restype = None
    _lib = L
    return L


def _check(rc: int, ctx=None):
    if rc != HSFLOW_OK:
        L = lib()
        msg = L.hsflow_last_error(ctx).decode(errors="replace")
        raise HsflowError(rc, msg or L.hsflow_status_string(rc).decode())


def _dtype_code(a: np.ndarray) -> int:
    if a.dtype == np.uint8:
        return U8
    if a.dtype == np.float32:
        return F32
    if a.dtype == np.float64:
        return F64
    if a.dtype == np.float16:
        return F16
    raise HsflowError(HSFLOW_ERR_ARG, f"unsupported image dtype {a.dtype}")


def _common_dtype(a, b):
    """Frames of different element types are both widened to float64, as
    hornSchunck.cpp:23-24 converts each with convertTo(CV_64FC1); each frame
    keeps its own row step."""
    if a.dtype != b.dtype:
        return a.astype(np.float64), b.astype(np.float64)
    return a, b


def _as_image(a) -> np.ndarray:
    a = np.asarray(a)
    if a.ndim != 2:
        raise HsflowError(HSFLOW_ERR_ARG, "images must be single-channel 2-D "
                          "(convert BGR with bgr_to_gray, as main.cpp:13-14 does)")
    if a.strides[1] != a.itemsize or a.strides[0] < a.shape[1] * a.itemsize:
        a = np.ascontiguousarray(a)
    return a


def _reusable(out, shape, dtype) -> bool:
    """(u, v) can take a solve's output in place: the create() rule."""
    return all(isinstance(x, np.ndarray) and x.shape == tuple(shape) and
               x.dtype == np.dtype(dtype) and x.flags.c_contiguous and x.flags.writeable
               for x in out) and out[0] is not out[1]


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

    def set_prefilter(self, prefilter=None):
        """The context's prefilter (hsflow_ctx_set_prefilter): flow_warped,
        flow_bidir, interpolate and interpolate_bgr run it on the frames first.
        None or mode 0 = off (default).  flow, flow_bgr, flow_pyramid and
        gradients are the reference's semantics and ignore it."""
        _, p = _pf_arg(prefilter)
        _check(lib().hsflow_ctx_set_prefilter(self._p, p), self._p)

    def prefilter(self):
        """The context's current Prefilter, None when off."""
        c = _CPrefilter()
        _check(lib().hsflow_ctx_prefilter(self._p, ctypes.byref(c)))
        return Prefilter(c.mode, c.sigma, c.eps, c.scale) if c.mode else None

    @contextlib.contextmanager
    def _prefilter_as(self, prefilter):
        """`prefilter` (a Prefilter) on the context for one call, the setting
        before it restored afterwards; None leaves the context's own."""
        if prefilter is None:
            yield
            return
        was = self.prefilter()
        self.set_prefilter(prefilter)
        try:
            yield
        finally:
            self.set_prefilter(was)

    def set_smoothness(self, smoothness=None):
        """The context's smoothness term (hsflow_ctx_set_smoothness) for
        flow_warped, flow_bidir, interpolate and interpolate_bgr.  None or mode
        0 = quadratic (default).  flow, flow_bgr, flow_pyramid and gradients are
        the reference's semantics and ignore it."""
        _, p = _sm_arg(smoothness)
        _check(lib().hsflow_ctx_set_smoothness(self._p, p), self._p)

    def smoothness(self):
        """The context's current Smoothness, None when quadratic."""
        c = _CSmoothness()
        _check(lib().hsflow_ctx_smoothness(self._p, ctypes.byref(c)))
        return Smoothness(c.mode, c.lam) if c.mode else None

    @contextlib.contextmanager
    def _smoothness_as(self, smoothness):
        """`smoothness` (a Smoothness) on the context for one call, the setting
        before it restored afterwards; None leaves the context's own."""
        if smoothness is None:
            yield
            return
        was = self.smoothness()
        self.set_smoothness(smoothness)
        try:
            yield
        finally:
            self.set_smoothness(was)

    def flow(self, I0, I1, window: int, iters: int, alpha: float, out_dtype=np.float64,
             out=None):
        """getFlow on host arrays.  `out` = (u, v): C-contiguous rows x cols
        arrays of out_dtype written in place (cv::Mat::create() keeps an
        existing CV_64FC1 buffer of the right size the same way); else new
        arrays."""
        a, b = _as_image(I0), _as_image(I1)
        if a.shape != b.shape:
            raise HsflowError(HSFLOW_ERR_SIZE, "Image sizes are different")
        a, b = _common_dtype(a, b)
        rows, cols = a.shape
        if out is not None and _reusable(out, (rows, cols), out_dtype):
            u, v = out
        else:
            u = np.empty((rows, cols), out_dtype)
            v = np.empty((rows, cols), out_dtype)
        code = F64 if u.dtype == np.float64 else F32
        rc = lib().hsflow_flow(self._p, a.ctypes.data, b.ctypes.data, _dtype_code(a),
                               rows, cols, a.strides[0], b.strides[0], int(window),
                               int(iters),
                               float(alpha), u.ctypes.data, v.ctypes.data, code,
                               u.strides[0])
        _check(rc, self._p)
        return u, v

    def flow_pyramid(self, I0, I1, levels: int, window: int, iters: int, alpha: float,
                     out_dtype=np.float64):
        """Config 5 coarse-to-fine warm start (`iters` per level), see
        hsflow_flow_pyramid in include/hsflow.h."""
        a, b = _as_image(I0), _as_image(I1)
        if a.shape != b.shape:
            raise HsflowError(HSFLOW_ERR_SIZE, "Image sizes are different")
        a, b = _common_dtype(a, b)
        rows, cols = a.shape
        u = np.empty((rows, cols), out_dtype)
        v = np.empty((rows, cols), out_dtype)
        code = F64 if u.dtype == np.float64 else F32
        rc = lib().hsflow_flow_pyramid(self._p, a.ctypes.data, b.ctypes.data,
                                       _dtype_code(a), rows, cols, a.strides[0],
                                       b.strides[0], int(levels), int(window), int(iters), float(alpha),
                                       u.ctypes.data, v.ctypes.data, code, u.strides[0])
        _check(rc, self._p)
        return u, v

    def flow_warped(self, I0, I1, levels: int, warps: int, window: int, iters: int,
                    alpha: float, out_dtype=np.float64, median: int = 0, prefilter=None,
                    smoothness=None):
        """Warped coarse-to-fine solve for large displacements (`warps`
        re-linearisations per level, `iters` iterations each), see
        hsflow_flow_warped in include/hsflow.h.  (u, v) * SOBEL_GAIN is the
        motion in pixels.  median = 3 or 5 filters (u, v) with a median of
        that size after every warp's iterations (hsflow_flow_warped_median);
        0 = none.  prefilter: a Prefilter set on the context for this call
        (None: the context's own setting, off by default).  smoothness: a
        Smoothness, likewise (window 3 or 5 then)."""
        a, b = _as_image(I0), _as_image(I1)
        if a.shape != b.shape:
            raise HsflowError(HSFLOW_ERR_SIZE, "Image sizes are different")
        a, b = _common_dtype(a, b)
        rows, cols = a.shape
        u = np.empty((rows, cols), out_dtype)
        v = np.empty((rows, cols), out_dtype)
        code = F64 if u.dtype == np.float64 else F32
        with self._prefilter_as(prefilter), self._smoothness_as(smoothness):
            rc = lib().hsflow_flow_warped_median(
                self._p, a.ctypes.data, b.ctypes.data, _dtype_code(a), rows, cols, a.strides[0],
                b.strides[0], int(levels), int(warps), int(median), int(window), int(iters),
                float(alpha), u.ctypes.data, v.ctypes.data, code, u.strides[0])
        _check(rc, self._p)
        return u, v

    def flow_bidir(self, I0, I1, levels: int, warps: int, window: int, iters: int,
                   alpha: float, rel: float = CONSISTENCY_REL, abs: float = CONSISTENCY_ABS,
                   out_dtype=np.float64, backward: bool = True, masks: bool = True,
                   counts: bool = True, out=None, mask_out=None, median: int = 0,
                   prefilter=None, smoothness=None):
        """Warped solve in both directions with the forward-backward check
        (hsflow_flow_bidir in include/hsflow.h).  Returns a BidirHost: u, v
        (I0 -> I1), ub, vb (I1 -> I0, None unless `backward`), mask_f, mask_b
        (uint8: CONSISTENT / INCONSISTENT / OUT_OF_FRAME, None unless `masks`)
        and counts (uint32 [2, 3], forward then backward, None unless
        `counts`).  `out`: an array [4, rows, >= cols] of out_dtype whose
        planes' first `cols` columns receive u, v, ub, vb (a padded row step);
        `mask_out`: likewise uint8 [2, rows, >= cols] for the masks.  median,
        prefilter and smoothness as in flow_warped, for both directions."""
        a, b = _as_image(I0), _as_image(I1)
        if a.shape != b.shape:
            raise HsflowError(HSFLOW_ERR_SIZE, "Image sizes are different")
        a, b = _common_dtype(a, b)
        rows, cols = a.shape
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
        u, v, ub, vb = (out[k, :, :cols] for k in range(4))
        mf, mb = mask_out[0, :, :cols], mask_out[1, :, :cols]
        cnt = np.zeros((2, 3), np.uint32) if counts else None
        code = F64 if out.dtype == np.float64 else F32
        with self._prefilter_as(prefilter), self._smoothness_as(smoothness):
            rc = lib().hsflow_flow_bidir_median(
                self._p, a.ctypes.data, b.ctypes.data, _dtype_code(a), rows, cols, a.strides[0],
                b.strides[0], int(levels), int(warps), int(median), int(window), int(iters),
                float(alpha),
                float(rel), float(abs), u.ctypes.data, v.ctypes.data,
                ub.ctypes.data if backward else None, vb.ctypes.data if backward else None, code,
                out.strides[1], mf.ctypes.data if masks else None,
                mb.ctypes.data if masks else None, mask_out.strides[1],
                cnt.ctypes.data if counts else None)
        _check(rc, self._p)
        return BidirHost(u, v, ub if backward else None, vb if backward else None,
                         mf if masks else None, mb if masks else None, cnt)

    def interpolate(self, I0, I1, times, levels: int, warps: int, window: int, iters: int,
                    alpha: float, median: int = 0, rel: float = CONSISTENCY_REL,
                    abs: float = CONSISTENCY_ABS, out_dtype=np.float32,
                    with_flags: bool = False, prefilter=None, smoothness=None):
        """The frames at `times` (each in [0, 1]; at most MAX_TIMES) between I0
        and I1: the bidirectional warped solve, then the motion-compensated
        blend (hsflow_flow_interp in include/hsflow.h).  Returns an array
        [len(times), rows, cols] of out_dtype (uint8, float32 or float64), or
        with_flags: (frames, flags, trusted) -- flags uint8 like frames (FLAG_*
        bits; 0 = both sources pass the forward-backward check), trusted uint32
        [len(times)], the pixels per frame with flags == 0.  prefilter as in
        flow_warped: the flows come from the prefiltered frames, the frames
        themselves are sampled.  smoothness as in flow_warped."""
        a, b = _as_image(I0), _as_image(I1)
        if a.shape != b.shape:
            raise HsflowError(HSFLOW_ERR_SIZE, "Image sizes are different")
        a, b = _common_dtype(a, b)
        rows, cols = a.shape
        tm = _times_array(times)
        nt = len(tm)
        out = np.empty((nt, rows, cols), out_dtype)
        if out.dtype not in (np.uint8, np.float32, np.float64):
            raise HsflowError(HSFLOW_ERR_ARG, "out_dtype: need uint8, float32 or float64")
        flags = np.empty((nt, rows, cols), np.uint8) if with_flags else None
        trusted = np.zeros(nt, np.uint32) if with_flags else None
        planes = (_vp * nt)(*[out[k].ctypes.data for k in range(nt)])
        fplanes = (_vp * nt)(*[flags[k].ctypes.data for k in range(nt)]) if with_flags else None
        with self._prefilter_as(prefilter), self._smoothness_as(smoothness):
            rc = lib().hsflow_flow_interp(
                self._p, a.ctypes.data, b.ctypes.data, _dtype_code(a), rows, cols, a.strides[0],
                b.strides[0], int(levels), int(warps), int(median), int(window), int(iters),
                float(alpha), float(rel), float(abs), tm, nt, planes, _dtype_code(out),
                out.strides[1], fplanes, cols, trusted.ctypes.data if with_flags else None)
        _check(rc, self._p)
        return (out, flags, trusted) if with_flags else out

    def interpolate_bgr(self, bgr0, bgr1, times, levels: int, warps: int, window: int,
                        iters: int, alpha: float, median: int = 0,
                        rel: float = CONSISTENCY_REL, abs: float = CONSISTENCY_ABS,
                        out_dtype=np.uint8, with_flags: bool = False, prefilter=None,
                        smoothness=None):
        """The colour frames at `times` between two decoded 8-bit BGR frames
        (H x W x 3, strided rows accepted): uploaded as BGR, converted to grey
        and solved both ways on the GPU, then the motion-compensated blend of
        each channel (hsflow_flow_interp_bgr in include/hsflow.h).  Returns an
        array [len(times), rows, cols, 3] of out_dtype (uint8 or float32), or
        with_flags: (frames, flags, trusted) -- flags uint8 [len(times), rows,
        cols] and trusted uint32 [len(times)] as in interpolate.  prefilter as
        in flow_warped, run on the grey planes; smoothness as in flow_warped."""
        a = np.asarray(bgr0)
        b = np.asarray(bgr1)
        for x in (a, b):
            if x.dtype != np.uint8 or x.ndim != 3 or x.shape[2] != 3:
                raise HsflowError(HSFLOW_ERR_ARG, "need H x W x 3 BGR uint8 (grey frames: "
                                  "Context.interpolate)")
        if a.shape != b.shape:
            raise HsflowError(HSFLOW_ERR_SIZE, "Image sizes are different")
        if a.strides[1:] != (3, 1) or a.strides[0] < 3 * a.shape[1]:
            a = np.ascontiguousarray(a)
        if b.strides[1:] != (3, 1) or b.strides[0] < 3 * b.shape[1]:
            b = np.ascontiguousarray(b)
        rows, cols = a.shape[:2]
        tm = _times_array(times)
        nt = len(tm)
        out = np.empty((nt, rows, cols, 3), out_dtype)
        if out.dtype not in (np.uint8, np.float32):
            raise HsflowError(HSFLOW_ERR_ARG, "out_dtype: need uint8 or float32")
        flags = np.empty((nt, rows, cols), np.uint8) if with_flags else None
        trusted = np.zeros(nt, np.uint32) if with_flags else None
        planes = (_vp * nt)(*[out[k].ctypes.data for k in range(nt)])
        fplanes = (_vp * nt)(*[flags[k].ctypes.data for k in range(nt)]) if with_flags else None
        with self._prefilter_as(prefilter), self._smoothness_as(smoothness):
            rc = lib().hsflow_flow_interp_bgr(
                self._p, a.ctypes.data, b.ctypes.data, rows, cols, a.strides[0], b.strides[0],
                int(levels), int(warps), int(median), int(window), int(iters), float(alpha),
                float(rel), float(abs), tm, nt, planes, _dtype_code(out),
                out.strides[1] if nt else 0, fplanes, cols,
                trusted.ctypes.data if with_flags else None)
        _check(rc, self._p)
        return (out, flags, trusted) if with_flags else out

    def flow_bgr(self, bgr0, bgr1, window: int, iters: int, alpha: float,
                 out_dtype=np.float64):
        """main.cpp:50-51 + :13-14 + :97-98: decoded 8-bit BGR frames are
        uploaded as BGR and converted to gray on the GPU, then solved."""
        a = np.asarray(bgr0)
        b = np.asarray(bgr1)
        for x in (a, b):
            if x.dtype != np.uint8 or x.ndim != 3 or x.shape[2] != 3:
                raise HsflowError(HSFLOW_ERR_ARG, "need H x W x 3 BGR uint8")
        if a.shape != b.shape:
            raise HsflowError(HSFLOW_ERR_SIZE, "Image sizes are different")
        if a.strides[1:] != (3, 1) or a.strides[0] < 3 * a.shape[1]:
            a = np.ascontiguousarray(a)
        if b.strides[1:] != (3, 1) or b.strides[0] < 3 * b.shape[1]:
            b = np.ascontiguousarray(b)
        rows, cols = a.shape[:2]
        u = np.empty((rows, cols), out_dtype)
        v = np.empty((rows, cols), out_dtype)
        code = F64 if u.dtype == np.float64 else F32
        rc = lib().hsflow_flow_bgr(self._p, a.ctypes.data, b.ctypes.data, rows, cols,
                                   a.strides[0], b.strides[0], int(window), int(iters), float(alpha),
                                   u.ctypes.data, v.ctypes.data, code, u.strides[0])
        _check(rc, self._p)
        return u, v

    def gradients(self, I0, I1, out_dtype=np.float64):
        a, b = _as_image(I0), _as_image(I1)
        if a.shape != b.shape:
            raise HsflowError(HSFLOW_ERR_SIZE, "Image sizes are different")
        a, b = _common_dtype(a, b)
        rows, cols = a.shape
        gx, gy, gt = (np.empty((rows, cols), out_dtype) for _ in range(3))
        code = F64 if gx.dtype == np.float64 else F32
        rc = lib().hsflow_gradients(self._p, a.ctypes.data, b.ctypes.data, _dtype_code(a),
                                    rows, cols, a.strides[0], b.strides[0], gx.ctypes.data,
                                    gy.ctypes.data, gt.ctypes.data, code, gx.strides[0])
        _check(rc, self._p)
        return gx, gy, gt


_default_ctx = None


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
    with _on(src.device):
        _check(lib().hsflow_download_device(dst.data_ptr(), src.data_ptr(),
                                            src.numel() * src.element_size(),
                                            _stream_ptr(stream, src.device)))


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
            raise HsflowError(HSFLOW_ERR_SIZE, "Image sizes are different")
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
        P(*[v.ctypes.data for _, v in out]), F64 if out_dtype == np.float64 else F32,
        out[0][0].strides[0])
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
            warps: int = 0, median: int = 0, prefilter=None, smoothness=None):
    """compute(I0, I1, alpha, nIter) -> (u, v): the north-star convenience
    wrapper over hornSchunck(windowSize, nIter, alpha).getFlow; levels > 1
    runs the config-5 coarse-to-fine warm start (nIter per level).  warps >= 1
    runs the warped coarse-to-fine solve instead (large displacements:
    `warps` re-linearisations per level, nIter iterations each); warps = 0
    keeps the behaviour above.  median = 3 or 5 (MEDIAN_SIZES) filters the
    flow after every warp's iterations and needs warps >= 1; so does
    prefilter (a Prefilter: the frames are locally normalised first) and so
    does smoothness (a Smoothness: the flow-driven, edge-preserving term)."""
    if median and not warps:
        raise HsflowError(HSFLOW_ERR_ARG, f"median {median} needs the warped solve (warps >= 1)")
    if prefilter is not None and not warps:
        raise HsflowError(HSFLOW_ERR_ARG, "prefilter needs the warped solve (warps >= 1)")
    if smoothness is not None and not warps:
        raise HsflowError(HSFLOW_ERR_ARG, "smoothness needs the warped solve (warps >= 1)")
    if warps:
        if not 1 <= int(warps) <= MAX_WARPS:
            raise HsflowError(HSFLOW_ERR_ARG, f"warps {warps} outside [1, {MAX_WARPS}]")
        return default_context().flow_warped(I0, I1, levels, warps, windowSize, nIter, alpha,
                                             median=median, prefilter=prefilter,
                                             smoothness=smoothness)
    if levels > 1:
        return default_context().flow_pyramid(I0, I1, levels, windowSize, nIter, alpha)
    return hornSchunck(windowSize, nIter, alpha).getFlow(I0, I1)


# ------------------------------------------------------------ device (torch)
def _stream_ptr(stream, device=None):
    """hipStream_t of `stream`, or of the current stream of `device` (the
    tensors' device) when stream is None.  The library runs a call on the
    device its stream belongs to; the null stream (torch's default stream is
    0 on every device) means the CURRENT device, so every wrapper below makes
    the tensors' device current around its library call (_on)."""
    if stream is None:
        return torch.cuda.current_stream(device).cuda_stream if torch is not None else None
    return getattr(stream, "cuda_stream", stream)


def _on(device):
    """Context that makes `device` current for one library call (a null
    stream runs on the current device, include/hsflow.h)."""
    return torch.cuda.device(device)


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


def _tensor_dtype(t) -> int:
    if t.dtype == torch.uint8:
        return U8
    if t.dtype == torch.float32:
        return F32
    if t.dtype == torch.float16:
        return F16
    if t.dtype == torch.float64:
        return F64
    raise HsflowError(HSFLOW_ERR_ARG,
                      f"device input dtype {t.dtype} (want uint8/float16/float32/float64)")


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


def flow_device(I0, I1, window: int, iters: int, alpha: float, u=None, v=None,
                workspace=None, stream=None):
    """Stream-ordered solve on torch CUDA tensors [B, H, W] (or [H, W]).
    Returns (u, v) float32 tensors.  No host synchronisation."""
    rows, cols = I0.shape[-2:]
    batch = int(np.prod(I0.shape[:-2])) if I0.dim() > 2 else 1
    _check_dense(I0, (rows, cols), "I0")
    _check_dense(I1, (rows, cols), "I1")
    if I1.dtype != I0.dtype or I1.shape != I0.shape:
        raise HsflowError(HSFLOW_ERR_SIZE, "I0/I1 differ in shape or dtype")
    if u is None:
        u = torch.empty(I0.shape, dtype=torch.float32, device=I0.device)
    if v is None:
        v = torch.empty(I0.shape, dtype=torch.float32, device=I0.device)
    _check_plane(u, (rows, cols), batch, "u")
    _check_plane(v, (rows, cols), batch, "v")
    if workspace is None:
        workspace = alloc_workspace(rows, cols, batch, I0.device)
    with _on(I0.device):
        rc = lib().hsflow_flow_device(I0.data_ptr(), I1.data_ptr(), _tensor_dtype(I0), rows,
                                      cols, batch, int(window), int(iters), float(alpha),
                                      u.data_ptr(), v.data_ptr(), workspace.data_ptr(),
                                      workspace.numel(), _stream_ptr(stream, I0.device))
    _check(rc)
    return u, v


def pyramid_level_size(rows: int, cols: int, level: int):
    r, c = ctypes.c_int(), ctypes.c_int()
    _check(lib().hsflow_pyramid_level_size(rows, cols, level, ctypes.byref(r),
                                           ctypes.byref(c)))
    return r.value, c.value


def pyramid_workspace_bytes(rows: int, cols: int, batch: int, levels: int) -> int:
    return int(lib().hsflow_pyramid_workspace_bytes(rows, cols, batch, levels))


def flow_pyramid_device(I0, I1, levels: int, window: int, iters: int, alpha: float,
                        u=None, v=None, workspace=None, stream=None):
    """Config 5: coarse-to-fine warm start on torch CUDA tensors [B, H, W]
    (uint8 / float16 / float32), `iters` Jacobi iterations per level."""
    rows, cols = I0.shape[-2:]
    batch = int(np.prod(I0.shape[:-2])) if I0.dim() > 2 else 1
    _check_dense(I0, (rows, cols), "I0")
    _check_dense(I1, (rows, cols), "I1")
    if I1.dtype != I0.dtype or I1.shape != I0.shape:
        raise HsflowError(HSFLOW_ERR_SIZE, "I0/I1 differ in shape or dtype")
    if u is None:
        u = torch.empty(I0.shape, dtype=torch.float32, device=I0.device)
    if v is None:
        v = torch.empty(I0.shape, dtype=torch.float32, device=I0.device)
    _check_plane(u, (rows, cols), batch, "u")
    _check_plane(v, (rows, cols), batch, "v")
    if workspace is None:
        n = pyramid_workspace_bytes(rows, cols, batch, levels)
        workspace = torch.empty(n, dtype=torch.uint8, device=I0.device)
    with _on(I0.device):
        rc = lib().hsflow_flow_pyramid_device(I0.data_ptr(), I1.data_ptr(), _tensor_dtype(I0),
                                              rows, cols, batch, int(levels), int(window),
                                              int(iters), float(alpha), u.data_ptr(),
                                              v.data_ptr(), workspace.data_ptr(),
                                              workspace.numel(), _stream_ptr(stream, I0.device))
    _check(rc)
    return u, v


def flow_warped_device(I0, I1, levels: int, warps: int, window: int, iters: int,
                       alpha: float, u=None, v=None, workspace=None, stream=None,
                       median: int = 0, prefilter=None, smoothness=None):
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
    Stream-ordered."""
    rows, cols = I0.shape[-2:]
    batch = int(np.prod(I0.shape[:-2])) if I0.dim() > 2 else 1
    _check_dense(I0, (rows, cols), "I0")
    _check_dense(I1, (rows, cols), "I1")
    if I1.dtype != I0.dtype or I1.shape != I0.shape:
        raise HsflowError(HSFLOW_ERR_SIZE, "I0/I1 differ in shape or dtype")
    if u is None:
        u = torch.empty(I0.shape, dtype=torch.float32, device=I0.device)
    if v is None:
        v = torch.empty(I0.shape, dtype=torch.float32, device=I0.device)
    _check_plane(u, (rows, cols), batch, "u")
    _check_plane(v, (rows, cols), batch, "v")
    keep, pf = _pf_arg(prefilter)
    keep_sm, sm = _sm_arg(smoothness)
    if workspace is None:
        n = pyramid_workspace_bytes(rows, cols, batch, levels) + \
            _pf_extra(prefilter, rows, cols, batch)
        workspace = torch.empty(n, dtype=torch.uint8, device=I0.device)
    with _on(I0.device):
        rc = lib().hsflow_flow_warped_sm_device(
            I0.data_ptr(), I1.data_ptr(), _tensor_dtype(I0), rows, cols, batch, int(levels),
            int(warps), int(median), int(window), int(iters), float(alpha), u.data_ptr(),
            v.data_ptr(), pf, sm, workspace.data_ptr(), workspace.numel(),
            _stream_ptr(stream, I0.device))
    _check(rc)
    return u, v


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
    rows, cols = uf.shape[-2:]
    batch = int(np.prod(uf.shape[:-2])) if uf.dim() > 2 else 1
    for t, name in ((uf, "uf"), (vf, "vf"), (ub, "ub"), (vb, "vb")):
        _check_plane(t, (rows, cols), batch, name)
    err = _check_output(err, uf.shape, torch.float32, uf.device, "err")
    mask = _check_output(mask, uf.shape, torch.uint8, uf.device, "mask")
    counts = _check_output(counts, (batch, 3), torch.int32, uf.device, "counts")
    ptr = (lambda t: t.data_ptr() if t is not None else None)
    with _on(uf.device):
        rc = lib().hsflow_flow_consistency_device(
            uf.data_ptr(), vf.data_ptr(), ub.data_ptr(), vb.data_ptr(), rows, cols, batch,
            float(rel), float(abs), ptr(err), ptr(mask), ptr(counts),
            _stream_ptr(stream, uf.device))
    _check(rc)
    return err, mask, counts


def median_device(u, v, ksize: int, u_out=None, v_out=None, stream=None):
    """ksize x ksize (3 or 5, MEDIAN_SIZES) median of u and of v, each on its
    own: float32 CUDA tensors [B, H, W] (or [H, W]), border replicated, IEEE
    total order of the bit patterns, so each result is one of its taps bit
    for bit (hsflow_flow_median_device in include/hsflow.h).  Out of place:
    u_out, v_out are allocated unless given and must not overlap u or v.
    Returns (u_out, v_out).  Stream-ordered."""
    rows, cols = u.shape[-2:]
    batch = int(np.prod(u.shape[:-2])) if u.dim() > 2 else 1
    if u_out is None:
        u_out = torch.empty(u.shape, dtype=torch.float32, device=u.device)
    if v_out is None:
        v_out = torch.empty(u.shape, dtype=torch.float32, device=u.device)
    for t, name in ((u, "u"), (v, "v"), (u_out, "u_out"), (v_out, "v_out")):
        _check_plane(t, (rows, cols), batch, name)
    with _on(u.device):
        rc = lib().hsflow_flow_median_device(u.data_ptr(), v.data_ptr(), rows, cols, batch,
                                             int(ksize), u_out.data_ptr(), v_out.data_ptr(),
                                             _stream_ptr(stream, u.device))
    _check(rc)
    return u_out, v_out


def bidir_workspace_bytes(rows: int, cols: int, batch: int, levels: int) -> int:
    return int(lib().hsflow_flow_bidir_workspace_bytes(rows, cols, batch, levels))


def flow_bidir_device(I0, I1, levels: int, warps: int, window: int, iters: int, alpha: float,
                      rel: float = CONSISTENCY_REL, abs: float = CONSISTENCY_ABS,
                      uf=None, vf=None, ub=None, vb=None, err_f=None, mask_f=True,
                      counts_f=None, err_b=None, mask_b=None, counts_b=None, workspace=None,
                      stream=None, median: int = 0, prefilter=None, smoothness=None):
    """Warped solve of I0 -> I1 (uf, vf) and I1 -> I0 (ub, vb) on torch CUDA
    tensors [B, H, W], then the forward-backward check each way
    (hsflow_flow_bidir_device in include/hsflow.h).  The flows equal
    flow_warped_device's bit for bit.  The six check outputs are as in
    consistency_device (True / tensor / None); a direction with none runs no
    check.  Returns a BidirDevice, None for outputs not asked for.
    `workspace`: bidir_workspace_bytes(rows, cols, batch, levels) bytes.
    median and prefilter (hsflow_flow_bidir_pf_device; prefilter_planes_bytes
    more workspace) as in flow_warped_device, for both directions.
    Stream-ordered."""
    rows, cols = I0.shape[-2:]
    batch = int(np.prod(I0.shape[:-2])) if I0.dim() > 2 else 1
    _check_dense(I0, (rows, cols), "I0")
    _check_dense(I1, (rows, cols), "I1")
    if I1.dtype != I0.dtype or I1.shape != I0.shape:
        raise HsflowError(HSFLOW_ERR_SIZE, "I0/I1 differ in shape or dtype")
    flows = []
    for t, name in ((uf, "uf"), (vf, "vf"), (ub, "ub"), (vb, "vb")):
        if t is None:
            t = torch.empty(I0.shape, dtype=torch.float32, device=I0.device)
        _check_plane(t, (rows, cols), batch, name)
        flows.append(t)
    outs = []
    for want, name in ((err_f, "err_f"), (mask_f, "mask_f"), (counts_f, "counts_f"),
                       (err_b, "err_b"), (mask_b, "mask_b"), (counts_b, "counts_b")):
        if name.startswith("counts"):
            outs.append(_check_output(want, (batch, 3), torch.int32, I0.device, name))
        else:
            outs.append(_check_output(
                want, I0.shape, torch.float32 if name.startswith("err") else torch.uint8,
                I0.device, name))
    keep, pf = _pf_arg(prefilter)
    keep_sm, sm = _sm_arg(smoothness)
    if workspace is None:
        n = bidir_workspace_bytes(rows, cols, batch, levels) + \
            _pf_extra(prefilter, rows, cols, batch)
        workspace = torch.empty(n, dtype=torch.uint8, device=I0.device)
    ptr = (lambda t: t.data_ptr() if t is not None else None)
    with _on(I0.device):
        rc = lib().hsflow_flow_bidir_sm_device(
            I0.data_ptr(), I1.data_ptr(), _tensor_dtype(I0), rows, cols, batch, int(levels),
            int(warps), int(median), int(window), int(iters), float(alpha), float(rel),
            float(abs),
            *[t.data_ptr() for t in flows], *[ptr(t) for t in outs], pf, sm,
            workspace.data_ptr(),
            workspace.numel(), _stream_ptr(stream, I0.device))
    _check(rc)
    return BidirDevice(*flows, *outs)


def _times_array(times):
    """`times` (a number or a sequence) as the C float array the library reads
    at call time; the library checks the count and the range."""
    t = [float(x) for x in np.atleast_1d(np.asarray(times, np.float64))]
    return (ctypes.c_float * len(t))(*t)


def warp_image_device(I, u, v, out=None, oof=None, stream=None):
    """Backward warp of the frames I (CUDA tensor [B, H, W] or [H, W], uint8 /
    float16 / float32 / float64) by the flow (u, v) (float32, solver units):
    out(y, x) = I sampled bilinearly at (y + 8 v, x + 8 u), the I1w of
    warp_gradients_device bit for bit (hsflow_warp_image_device in
    include/hsflow.h).  oof: True / a uint8 tensor like I to get 1 where the
    target leaves the frame by more than half a pixel.  Returns out (float32),
    or (out, oof) when oof was asked for.  Stream-ordered."""
    rows, cols = I.shape[-2:]
    batch = int(np.prod(I.shape[:-2])) if I.dim() > 2 else 1
    _check_dense(I, (rows, cols), "I")
    _check_plane(u, (rows, cols), batch, "u")
    _check_plane(v, (rows, cols), batch, "v")
    if out is None:
        out = torch.empty(I.shape, dtype=torch.float32, device=I.device)
    _check_plane(out, (rows, cols), batch, "out")
    oof = _check_output(oof, I.shape, torch.uint8, I.device, "oof")
    with _on(I.device):
        rc = lib().hsflow_warp_image_device(
            I.data_ptr(), _tensor_dtype(I), rows, cols, batch, u.data_ptr(), v.data_ptr(),
            out.data_ptr(), oof.data_ptr() if oof is not None else None,
            _stream_ptr(stream, I.device))
    _check(rc)
    return out if oof is None else (out, oof)


def _interp_outputs(I0, nt, out, out_dtype, flags, trusted):
    """out / flags / trusted of an interpolation of `nt` times of the frames
    I0 ([B, H, W] or [H, W]): [B, nt, H, W] ([nt, H, W]) and [B, nt]."""
    rows, cols = I0.shape[-2:]
    batch = int(np.prod(I0.shape[:-2])) if I0.dim() > 2 else 1
    shape = tuple(I0.shape[:-2]) + (nt, rows, cols)
    if out is None:
        out = torch.empty(shape, dtype=out_dtype, device=I0.device)
    if out.dtype not in (torch.float32, torch.uint8):
        raise HsflowError(HSFLOW_ERR_ARG, "out: need float32 or uint8")
    out = _check_output(out, shape, out.dtype, I0.device, "out")
    flags = _check_output(flags, shape, torch.uint8, I0.device, "flags")
    trusted = _check_output(trusted, (batch, nt), torch.int32, I0.device, "trusted")
    return out, flags, trusted


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
    if out_dtype is None:
        out_dtype = torch.float32
    rows, cols = I0.shape[-2:]
    batch = int(np.prod(I0.shape[:-2])) if I0.dim() > 2 else 1
    _check_dense(I0, (rows, cols), "I0")
    _check_dense(I1, (rows, cols), "I1")
    if I1.dtype != I0.dtype or I1.shape != I0.shape:
        raise HsflowError(HSFLOW_ERR_SIZE, "I0/I1 differ in shape or dtype")
    for t, name in ((uf, "uf"), (vf, "vf"), (ub, "ub"), (vb, "vb")):
        _check_plane(t, (rows, cols), batch, name)
    for t, name in ((mask_f, "mask_f"), (mask_b, "mask_b")):
        if t is not None:
            _check_output(t, I0.shape, torch.uint8, I0.device, name)
    tm = _times_array(times)
    out, flags, trusted = _interp_outputs(I0, len(tm), out, out_dtype, flags, trusted)
    ptr = (lambda t: t.data_ptr() if t is not None else None)
    with _on(I0.device):
        rc = lib().hsflow_frame_interp_device(
            I0.data_ptr(), I1.data_ptr(), _tensor_dtype(I0), rows, cols, batch, uf.data_ptr(),
            vf.data_ptr(), ub.data_ptr(), vb.data_ptr(), ptr(mask_f), ptr(mask_b), tm, len(tm),
            out.data_ptr(), U8 if out.dtype == torch.uint8 else F32, ptr(flags), ptr(trusted),
            _stream_ptr(stream, I0.device))
    _check(rc)
    return out, flags, trusted


def flow_interp_workspace_bytes(rows: int, cols: int, batch: int, levels: int) -> int:
    return int(lib().hsflow_flow_interp_workspace_bytes(rows, cols, batch, levels))


def flow_interp_device(I0, I1, times, levels: int, warps: int, window: int, iters: int,
                       alpha: float, median: int = 0, rel: float = CONSISTENCY_REL,
                       abs: float = CONSISTENCY_ABS, out=None, out_dtype=None, flags=None,
                       trusted=None, workspace=None, stream=None, prefilter=None,
                       smoothness=None):
    """flow_bidir_device(median=...) into planes of the workspace, then
    frame_interp_device with both masks: one call, the same bits
    (hsflow_flow_interp_device in include/hsflow.h).  `workspace`:
    flow_interp_workspace_bytes(rows, cols, batch, levels) bytes.  prefilter: a
    Prefilter; the flows then come from the prefiltered frames while the
    frames themselves are sampled (hsflow_flow_interp_pf_device;
    prefilter_planes_bytes more workspace).  Returns (out, flags, trusted) as
    frame_interp_device.  Stream-ordered."""
    if out_dtype is None:
        out_dtype = torch.float32
    rows, cols = I0.shape[-2:]
    batch = int(np.prod(I0.shape[:-2])) if I0.dim() > 2 else 1
    _check_dense(I0, (rows, cols), "I0")
    _check_dense(I1, (rows, cols), "I1")
    if I1.dtype != I0.dtype or I1.shape != I0.shape:
        raise HsflowError(HSFLOW_ERR_SIZE, "I0/I1 differ in shape or dtype")
    tm = _times_array(times)
    out, flags, trusted = _interp_outputs(I0, len(tm), out, out_dtype, flags, trusted)
    keep, pf = _pf_arg(prefilter)
    keep_sm, sm = _sm_arg(smoothness)
    if workspace is None:
        n = flow_interp_workspace_bytes(rows, cols, batch, levels) + \
            _pf_extra(prefilter, rows, cols, batch)
        workspace = torch.empty(n, dtype=torch.uint8, device=I0.device)
    ptr = (lambda t: t.data_ptr() if t is not None else None)
    with _on(I0.device):
        rc = lib().hsflow_flow_interp_sm_device(
            I0.data_ptr(), I1.data_ptr(), _tensor_dtype(I0), rows, cols, batch, int(levels),
            int(warps), int(median), int(window), int(iters), float(alpha), float(rel),
            float(abs), tm, len(tm), out.data_ptr(), U8 if out.dtype == torch.uint8 else F32,
            ptr(flags), ptr(trusted), pf, sm, workspace.data_ptr(), workspace.numel(),
            _stream_ptr(stream, I0.device))
    _check(rc)
    return out, flags, trusted


def _check_bgr(t, name):
    """A batch of dense interleaved BGR frames: uint8, contiguous, CUDA,
    [B, H, W, 3] or [H, W, 3].  Returns (rows, cols, batch)."""
    if torch is None or not isinstance(t, torch.Tensor) or t.dtype != torch.uint8 or \
            t.dim() not in (3, 4) or t.shape[-1] != 3 or not t.is_cuda or not t.is_contiguous():
        raise HsflowError(HSFLOW_ERR_ARG, f"{name}: need a contiguous uint8 CUDA tensor "
                          "[B, H, W, 3] or [H, W, 3]")
    return t.shape[-3], t.shape[-2], (t.shape[0] if t.dim() == 4 else 1)


def _bgr_interp_outputs(bgr0, nt, out, out_dtype, flags, trusted):
    """out / flags / trusted of a BGR interpolation of `nt` times:
    [B, nt, H, W, 3] ([nt, H, W, 3]), [B, nt, H, W] and [B, nt]."""
    rows, cols, batch = _check_bgr(bgr0, "bgr0")
    lead = tuple(bgr0.shape[:-3])
    if out is None:
        out = torch.empty(lead + (nt, rows, cols, 3), dtype=out_dtype, device=bgr0.device)
    if out.dtype not in (torch.float32, torch.uint8):
        raise HsflowError(HSFLOW_ERR_ARG, "out: need float32 or uint8")
    out = _check_output(out, lead + (nt, rows, cols, 3), out.dtype, bgr0.device, "out")
    flags = _check_output(flags, lead + (nt, rows, cols), torch.uint8, bgr0.device, "flags")
    trusted = _check_output(trusted, (batch, nt), torch.int32, bgr0.device, "trusted")
    return out, flags, trusted


def warp_image_bgr_device(bgr, u, v, out=None, out_dtype=None, oof=None, stream=None):
    """warp_image_device for colour frames: bgr a uint8 CUDA tensor [B, H, W, 3]
    or [H, W, 3], (u, v) float32 [B, H, W] in solver units; out(y, x, c) =
    bgr(.., c) at (y + 8 v, x + 8 u), each channel the bits warp_image_device
    gives its plane (hsflow_warp_image_bgr_device in include/hsflow.h).  out:
    float32 (default) or uint8, like bgr; oof: True / a uint8 tensor [B, H, W].
    Returns out, or (out, oof) when oof was asked for.  Stream-ordered."""
    rows, cols, batch = _check_bgr(bgr, "bgr")
    _check_plane(u, (rows, cols), batch, "u")
    _check_plane(v, (rows, cols), batch, "v")
    if out is None:
        out = torch.empty(bgr.shape, dtype=out_dtype or torch.float32, device=bgr.device)
    if out.dtype not in (torch.float32, torch.uint8):
        raise HsflowError(HSFLOW_ERR_ARG, "out: need float32 or uint8")
    out = _check_output(out, bgr.shape, out.dtype, bgr.device, "out")
    oof = _check_output(oof, bgr.shape[:-1], torch.uint8, bgr.device, "oof")
    with _on(bgr.device):
        rc = lib().hsflow_warp_image_bgr_device(
            bgr.data_ptr(), rows, cols, batch, u.data_ptr(), v.data_ptr(), out.data_ptr(),
            U8 if out.dtype == torch.uint8 else F32, oof.data_ptr() if oof is not None else None,
            _stream_ptr(stream, bgr.device))
    _check(rc)
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
    if out_dtype is None:
        out_dtype = torch.float32
    rows, cols, batch = _check_bgr(bgr0, "bgr0")
    _check_bgr(bgr1, "bgr1")
    if bgr1.shape != bgr0.shape:
        raise HsflowError(HSFLOW_ERR_SIZE, "bgr0/bgr1 differ in shape")
    for t, name in ((uf, "uf"), (vf, "vf"), (ub, "ub"), (vb, "vb")):
        _check_plane(t, (rows, cols), batch, name)
    for t, name in ((mask_f, "mask_f"), (mask_b, "mask_b")):
        if t is not None:
            _check_output(t, bgr0.shape[:-1], torch.uint8, bgr0.device, name)
    tm = _times_array(times)
    out, flags, trusted = _bgr_interp_outputs(bgr0, len(tm), out, out_dtype, flags, trusted)
    ptr = (lambda t: t.data_ptr() if t is not None else None)
    with _on(bgr0.device):
        rc = lib().hsflow_frame_interp_bgr_device(
            bgr0.data_ptr(), bgr1.data_ptr(), rows, cols, batch, uf.data_ptr(), vf.data_ptr(),
            ub.data_ptr(), vb.data_ptr(), ptr(mask_f), ptr(mask_b), tm, len(tm), out.data_ptr(),
            U8 if out.dtype == torch.uint8 else F32, ptr(flags), ptr(trusted),
            _stream_ptr(stream, bgr0.device))
    _check(rc)
    return out, flags, trusted


def flow_interp_bgr_workspace_bytes(rows: int, cols: int, batch: int, levels: int) -> int:
    return int(lib().hsflow_flow_interp_bgr_workspace_bytes(rows, cols, batch, levels))


def flow_interp_bgr_device(bgr0, bgr1, times, levels: int, warps: int, window: int, iters: int,
                           alpha: float, median: int = 0, rel: float = CONSISTENCY_REL,
                           abs: float = CONSISTENCY_ABS, out=None, out_dtype=None, flags=None,
                           trusted=None, workspace=None, stream=None, prefilter=None,
                           smoothness=None):
    """bgr_to_gray_device of both frames, flow_bidir_device(median=...) on the
    grey planes, then frame_interp_bgr_device with both masks: one call, the
    same bits (hsflow_flow_interp_bgr_device in include/hsflow.h).
    `workspace`: flow_interp_bgr_workspace_bytes(rows, cols, batch, levels)
    bytes.  prefilter: a Prefilter run on the grey planes in front of the
    solve (hsflow_flow_interp_bgr_pf_device; prefilter_planes_bytes more
    workspace).  Returns (out, flags, trusted) as frame_interp_bgr_device.
    Stream-ordered."""
    if out_dtype is None:
        out_dtype = torch.float32
    rows, cols, batch = _check_bgr(bgr0, "bgr0")
    _check_bgr(bgr1, "bgr1")
    if bgr1.shape != bgr0.shape:
        raise HsflowError(HSFLOW_ERR_SIZE, "bgr0/bgr1 differ in shape")
    tm = _times_array(times)
    out, flags, trusted = _bgr_interp_outputs(bgr0, len(tm), out, out_dtype, flags, trusted)
    keep, pf = _pf_arg(prefilter)
    keep_sm, sm = _sm_arg(smoothness)
    if workspace is None:
        n = flow_interp_bgr_workspace_bytes(rows, cols, batch, levels) + \
            _pf_extra(prefilter, rows, cols, batch)
        workspace = torch.empty(n, dtype=torch.uint8, device=bgr0.device)
    ptr = (lambda t: t.data_ptr() if t is not None else None)
    with _on(bgr0.device):
        rc = lib().hsflow_flow_interp_bgr_sm_device(
            bgr0.data_ptr(), bgr1.data_ptr(), rows, cols, batch, int(levels), int(warps),
            int(median), int(window), int(iters), float(alpha), float(rel), float(abs), tm,
            len(tm), out.data_ptr(), U8 if out.dtype == torch.uint8 else F32, ptr(flags),
            ptr(trusted), pf, sm, workspace.data_ptr(), workspace.numel(),
            _stream_ptr(stream, bgr0.device))
    _check(rc)
    return out, flags, trusted


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
    rows, cols = I.shape[-2:]
    batch = int(np.prod(I.shape[:-2])) if I.dim() > 2 else 1
    _check_dense(I, (rows, cols), "I")
    if prefilter is None:
        raise HsflowError(HSFLOW_ERR_ARG, "prefilter_device needs a Prefilter")
    if out is None:
        out = torch.empty(I.shape, dtype=torch.float32, device=I.device)
    _check_plane(out, (rows, cols), batch, "out")
    keep, pf = _pf_arg(prefilter)
    with _on(I.device):
        rc = lib().hsflow_prefilter_device(I.data_ptr(), _tensor_dtype(I), rows, cols, batch, pf,
                                           out.data_ptr(), _stream_ptr(stream, I.device))
    _check(rc)
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
    rows, cols = I0.shape[-2:]
    batch = int(np.prod(I0.shape[:-2])) if I0.dim() > 2 else 1
    _check_dense(I0, (rows, cols), "I0")
    _check_dense(I1, (rows, cols), "I1")
    if I1.dtype != I0.dtype or I1.shape != I0.shape:
        raise HsflowError(HSFLOW_ERR_SIZE, "I0/I1 differ in shape or dtype")
    _check_plane(u0, (rows, cols), batch, "u0")
    _check_plane(v0, (rows, cols), batch, "v0")
    for t, name in ((gx, "gx"), (gy, "gy"), (gt, "gt")):
        if t is not None:
            _check_plane(t, (rows, cols), batch, name)
    ptr = (lambda t: t.data_ptr() if t is not None else None)
    with _on(I0.device):
        rc = lib().hsflow_warp_gradients_device(I0.data_ptr(), I1.data_ptr(), _tensor_dtype(I0),
                                                rows, cols, batch, u0.data_ptr(), v0.data_ptr(),
                                                ptr(gx), ptr(gy), ptr(gt), workspace.data_ptr(),
                                                workspace.numel(),
                                                _stream_ptr(stream, I0.device))
    _check(rc)


def pyramid_build_device(I0, I1, levels: int, workspace=None, stream=None):
    """Levels 1..levels-1 of both frames (f32 tensors [B, h_l, w_l]), the
    same planes hsflow_flow_pyramid_device builds internally."""
    rows, cols = I0.shape[-2:]
    batch = int(np.prod(I0.shape[:-2])) if I0.dim() > 2 else 1
    _check_dense(I0, (rows, cols), "I0")
    _check_dense(I1, (rows, cols), "I1")
    lead = tuple(I0.shape[:-2])
    P0, P1 = [], []
    for l in range(1, levels):
        r, c = pyramid_level_size(rows, cols, l)
        P0.append(torch.empty(lead + (r, c), dtype=torch.float32, device=I0.device))
        P1.append(torch.empty(lead + (r, c), dtype=torch.float32, device=I0.device))
    if workspace is None:
        workspace = alloc_workspace(rows, cols, batch, I0.device)
    n = max(1, levels - 1)
    a0 = (_vp * n)(*[t.data_ptr() for t in P0]) if P0 else (_vp * 1)()
    a1 = (_vp * n)(*[t.data_ptr() for t in P1]) if P1 else (_vp * 1)()
    with _on(I0.device):
        _check(lib().hsflow_pyramid_build_device(I0.data_ptr(), I1.data_ptr(), _tensor_dtype(I0),
                                                 rows, cols, batch, int(levels), a0, a1,
                                                 workspace.data_ptr(), workspace.numel(),
                                                 _stream_ptr(stream, I0.device)))
    return P0, P1


def upflow_device(uc, vc, u, v, stream=None):
    """u = 2 uc(y/2, x/2), v likewise (the pyramid's warm start); u, v and
    uc, vc are dense [rows, cols] / [rc, cc] views (row slices allowed)."""
    rc, cc = uc.shape[-2:]
    rows, cols = u.shape[-2:]
    for t, name, shape in ((uc, "uc", (rc, cc)), (vc, "vc", (rc, cc)), (u, "u", (rows, cols)),
                           (v, "v", (rows, cols))):
        _check_plane(t, shape, 1, name)
    with _on(u.device):
        _check(lib().hsflow_upflow_device(uc.data_ptr(), vc.data_ptr(), rc, cc, u.data_ptr(),
                                          v.data_ptr(), rows, cols, 1,
                                          _stream_ptr(stream, u.device)))


def gradients_device(I0, I1, workspace, gx=None, gy=None, gt=None, stream=None):
    rows, cols = I0.shape[-2:]
    batch = int(np.prod(I0.shape[:-2])) if I0.dim() > 2 else 1
    _check_dense(I0, (rows, cols), "I0")
    _check_dense(I1, (rows, cols), "I1")
    ptr = (lambda t: t.data_ptr() if t is not None else None)
    with _on(I0.device):
        rc = lib().hsflow_gradients_device(I0.data_ptr(), I1.data_ptr(), _tensor_dtype(I0),
                                           rows, cols, batch, ptr(gx), ptr(gy), ptr(gt),
                                           workspace.data_ptr(), workspace.numel(),
                                           _stream_ptr(stream, I0.device))
    _check(rc)


def jacobi_device(rows, cols, batch, window, iters, alpha, u, v, workspace,
                  warm_start=False, stream=None):
    _check_plane(u, (rows, cols), batch, "u")
    _check_plane(v, (rows, cols), batch, "v")
    with _on(u.device):
        rc = lib().hsflow_jacobi_device(int(rows), int(cols), int(batch), int(window),
                                        int(iters), float(alpha), int(bool(warm_start)),
                                        u.data_ptr(), v.data_ptr(), workspace.data_ptr(),
                                        workspace.numel(), _stream_ptr(stream, u.device))
    _check(rc)


def diffusivity_device(u, v, lam: float, g=None, stream=None):
    """The flow-driven smoothness weights alone (hsflow_flow_diffusivity_device
    in include/hsflow.h): g = 1 / sqrt(1 + |grad (8u, 8v)|^2 / lam^2) of float32
    CUDA tensors [B, H, W] (or [H, W]) in solver units, central differences,
    border replicated.  g is allocated unless given and must not overlap u or
    v.  Returns g.  Stream-ordered."""
    rows, cols = u.shape[-2:]
    batch = int(np.prod(u.shape[:-2])) if u.dim() > 2 else 1
    if g is None:
        g = torch.empty(u.shape, dtype=torch.float32, device=u.device)
    for t, name in ((u, "u"), (v, "v"), (g, "g")):
        _check_plane(t, (rows, cols), batch, name)
    with _on(u.device):
        rc = lib().hsflow_flow_diffusivity_device(u.data_ptr(), v.data_ptr(), rows, cols, batch,
                                                  float(lam), g.data_ptr(),
                                                  _stream_ptr(stream, u.device))
    _check(rc)
    return g


def jacobi_weighted_device(rows, cols, batch, window, iters, alpha, g, u, v, workspace,
                           stream=None):
    """`iters` g-weighted iterations warm-started from (u, v), in place, from
    the f32 gradient planes warp_gradients_device left in `workspace`
    (hsflow_jacobi_weighted_device in include/hsflow.h); window 3 or 5."""
    for t, name in ((g, "g"), (u, "u"), (v, "v")):
        _check_plane(t, (rows, cols), batch, name)
    with _on(u.device):
        rc = lib().hsflow_jacobi_weighted_device(int(rows), int(cols), int(batch), int(window),
                                                 int(iters), float(alpha), g.data_ptr(),
                                                 u.data_ptr(), v.data_ptr(), workspace.data_ptr(),
                                                 workspace.numel(), _stream_ptr(stream, u.device))
    _check(rc)


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
    bgr = np.ascontiguousarray(bgr, np.uint8)
    if bgr.ndim != 3 or bgr.shape[2] != 3:
        raise HsflowError(HSFLOW_ERR_ARG, "need H x W x 3 BGR uint8")
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
    rows, cols = bgr.shape[-3], bgr.shape[-2]
    batch = int(np.prod(bgr.shape[:-3])) if bgr.dim() > 3 else 1
    if gray is None:
        gray = torch.empty(bgr.shape[:-1], dtype=torch.uint8, device=bgr.device)
    if gray.dtype != torch.uint8 or not gray.is_cuda or not gray.is_contiguous() or \
            gray.numel() < batch * rows * cols or gray.device != bgr.device:
        raise HsflowError(HSFLOW_ERR_ARG, "gray: need a contiguous uint8 CUDA tensor of "
                          f"{batch} x {rows} x {cols} on {bgr.device}")
    with _on(bgr.device):
        _check(lib().hsflow_bgr_to_gray_device(bgr.data_ptr(), rows, cols, batch,
                                               gray.data_ptr(), _stream_ptr(stream, bgr.device)))
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
