"""YUV 4:2:0 frame interpolation (include/hsflow.h, "YUV 4:2:0 frame
interpolation"): I420 and NV12 frames in, the same layout out.

Video arrives as 4:2:0, not as BGR.  The luma plane of such a frame is the grey
frame the solver wants, so it goes through the grey calls as it is -- no colour
conversion either way and half the bytes of BGR -- and the chroma follows the
same flows on its own grid: chroma_interp_device (KIY) is, bit for bit,
temporal.downflow_device on both flow pairs followed by
hsflow.frame_interp_device on the U planes and on the V planes, in one launch.

A packed frame is a uint8 array of rows * cols * 3 // 2 bytes, the luma plane
followed by the chroma (I420: the U plane, then the V plane; NV12: U and V
interleaved); rows and cols are the luma's and even.  On the device luma
[B, rows, cols] and chroma (I420 [B, 2, rows / 2, cols / 2], NV12 [B, rows / 2,
cols / 2, 2]) are separate tensors.

With the flow projection (projection.py) the chroma reads its time-t flow
through the luma's own winners, so that luma and chroma follow the same surface
at a motion boundary: chroma_interp_proj_device (KIYP) is, bit for bit,
temporal.downflow_device on both flow pairs, cells_down_device (KSD) on
projection.project_device's cells of the luma, and
projection.frame_interp_device on the U and on the V planes, in one launch.
flow_interp_yuv_proj_device, interpolate_yuv(projection=) and
frames.interpolate_sequence_yuv(projection=) are the fused, the host and the
clip form.

16-bit samples (include/hsflow.h, "16-bit YUV 4:2:0"): yuv420p10le .. p16le are
the I420 layout and P010 .. P016 the NV12 layout with 2-byte samples.  Every
device call here takes such frames as torch.uint16 tensors -- or torch.int16,
read as the same 16 bits, because torch has few uint16 operators -- and
interpolate_yuv as np.uint16 arrays; they route to the 16-bit entry points and
return uint16 (int16 where an int16 `out` is given) or float32.  A sample is its
value, 0 .. 65535: the results are, bit for bit, those of the same values as
float32 planes in the pieces named above, the pyramid never rounded to integers
(a 16-bit pair is never treated as 8-bit), a uint16 output floor(x + 0.5)
clamped to 0 .. 65535.  A frame scaled by k behaves like alpha divided by k: use
alpha x 4 for 10-bit LSB-aligned content and alpha x 256 for P010, relative to
the 8-bit recommendation of about 100.  A P010 result is a valid P016 frame:
the low six bits of its samples are in general not zero.

Everything here calls the HIP path in libhsflow.so through hsflow's front ends.
"""
from __future__ import annotations

import ctypes

import numpy as np

import hsflow

try:
    import torch
except Exception:  # pragma: no cover
    torch = None


# layouts (HSFLOW_YUV_*)
YUV_I420, YUV_NV12 = 1, 2
# HSFLOW_U16: the dtype code of 16-bit samples, taken by the 16-bit calls only
U16 = hsflow._U16
LAYOUTS = {"i420": YUV_I420, "nv12": YUV_NV12, YUV_I420: YUV_I420, YUV_NV12: YUV_NV12}
# KIY's tile: a block takes 512 consecutive chroma samples of a pair at a time
CHROMA_TILE = 512


def _layout(layout) -> int:
    key = layout.lower() if isinstance(layout, str) else layout
    if key not in LAYOUTS:
        raise hsflow.HsflowError(hsflow.HSFLOW_ERR_ARG,
                                 f"layout {layout!r}: need 'i420' (1) or 'nv12' (2)")
    return LAYOUTS[key]


def _even(rows, cols):
    if rows < 2 or cols < 2 or rows % 2 or cols % 2:
        raise hsflow.HsflowError(hsflow.HSFLOW_ERR_ARG,
                                 f"YUV 4:2:0 needs even rows and cols, not {rows}x{cols}")


def frame_bytes(rows: int, cols: int) -> int:
    """Bytes of a packed 8-bit 4:2:0 frame: its samples, at any depth."""
    _even(rows, cols)
    return rows * cols * 3 // 2


def chroma_shape(rows: int, cols: int, layout=YUV_I420):
    """The shape of one frame's chroma: (2, rows / 2, cols / 2) for I420,
    (rows / 2, cols / 2, 2) for NV12."""
    _even(rows, cols)
    rc, cc = rows // 2, cols // 2
    return (2, rc, cc) if _layout(layout) == YUV_I420 else (rc, cc, 2)


def split(frame, rows: int, cols: int, layout=YUV_I420):
    """(y, u, v) of packed frames [..., rows * cols * 3 / 2] (any dtype): views
    y [..., rows, cols] and u, v [..., rows / 2, cols / 2]."""
    frame = np.asarray(frame)
    n = frame_bytes(rows, cols)
    if frame.shape[-1:] != (n,):
        raise hsflow.HsflowError(hsflow.HSFLOW_ERR_ARG,
                                 f"a packed {rows}x{cols} frame has {n} samples, not "
                                 f"{frame.shape[-1:]}")
    lead = frame.shape[:-1]
    y = frame[..., :rows * cols].reshape(lead + (rows, cols))
    c = frame[..., rows * cols:].reshape(lead + chroma_shape(rows, cols, layout))
    if _layout(layout) == YUV_I420:
        return y, c[..., 0, :, :], c[..., 1, :, :]
    return y, c[..., 0], c[..., 1]


def pack(y, u, v, layout=YUV_I420):
    """The packed frames [..., rows * cols * 3 / 2] of y [..., rows, cols] and
    u, v [..., rows / 2, cols / 2], in y's dtype."""
    y, u, v = np.asarray(y), np.asarray(u), np.asarray(v)
    rows, cols = y.shape[-2:]
    _even(rows, cols)
    lead = y.shape[:-2]
    if u.shape != lead + (rows // 2, cols // 2) or v.shape != u.shape:
        raise hsflow.HsflowError(hsflow.HSFLOW_ERR_SIZE, "u, v: need y's shape halved each way")
    c = np.stack([u, v], axis=-3 if _layout(layout) == YUV_I420 else -1).astype(y.dtype)
    return np.concatenate([y.reshape(lead + (-1,)), c.reshape(lead + (-1,))], axis=-1)


def convert(frame, rows: int, cols: int, src, dst):
    """Packed frames of layout `src` in layout `dst` (a copy)."""
    return pack(*split(frame, rows, cols, src), layout=dst)


def blocks_per_cu() -> int:
    """The cap of KIY's grid in blocks per compute unit
    (hsflow_chroma_interp_blocks_per_cu): a chroma plane of more than
    blocks_per_cu() * CUs * CHROMA_TILE samples makes a single pair's blocks
    stride."""
    return int(hsflow.lib().hsflow_chroma_interp_blocks_per_cu())


def set_nv12_loads(wide: bool) -> bool:
    """How KIY fetches the two adjacent taps of an NV12 row: four byte loads
    (False, the default) or one unaligned 32-bit load; same bits
    (hsflow_set_chroma_nv12_loads).  Returns the previous setting."""
    return bool(hsflow.lib().hsflow_set_chroma_nv12_loads(1 if wide else 0))


def _chroma_pair(c0, c1, layout):
    """(rows, cols, batch) of the luma the uint8 CUDA chroma tensors c0, c1
    belong to: I420 [B, 2, rc, cc] or [2, rc, cc], NV12 [B, rc, cc, 2] or
    [rc, cc, 2]."""
    for t, name in ((c0, "c0"), (c1, "c1")):
        if torch is None or not isinstance(t, torch.Tensor) or \
                not (t.dtype == torch.uint8 or hsflow._is16(t.dtype)) or \
                t.dim() not in (3, 4) or not t.is_cuda or not t.is_contiguous():
            raise hsflow.HsflowError(hsflow.HSFLOW_ERR_ARG, f"{name}: need a contiguous uint8 "
                                     "CUDA tensor, I420 [B, 2, rc, cc] or NV12 [B, rc, cc, 2]")
    if c1.shape != c0.shape:
        raise hsflow.HsflowError(hsflow.HSFLOW_ERR_SIZE, "c0/c1 differ in shape")
    if c1.dtype != c0.dtype:
        raise hsflow.HsflowError(hsflow.HSFLOW_ERR_SIZE, "c0/c1 differ in dtype")
    batch = c0.shape[0] if c0.dim() == 4 else 1
    shape = tuple(c0.shape[-3:])
    two, (rc, cc) = (shape[0], shape[1:]) if layout == YUV_I420 else (shape[2], shape[:2])
    if two != 2:
        raise hsflow.HsflowError(hsflow.HSFLOW_ERR_ARG, f"chroma of shape {shape} is not "
                                 "I420 [2, rc, cc]" if layout == YUV_I420 else
                                 f"chroma of shape {shape} is not NV12 [rc, cc, 2]")
    return 2 * rc, 2 * cc, batch


def _chroma_out(c0, nt, out, out_dtype):
    """out_c of `nt` times: [B, nt] + a chroma frame's shape (no B for a single
    frame's chroma), float32 (default) or uint8; of 16-bit chroma float32 or
    uint16 (int16)."""
    lead = tuple(c0.shape[:-3])
    return hsflow._out_frames(out, lead + (nt,) + tuple(c0.shape[-3:]), out_dtype, c0.device,
                              wide=hsflow._is16(c0.dtype))


def chroma_interp_device(c0, c1, uf, vf, ub, vb, times, layout=YUV_I420, counts_f=None,
                         counts_b=None, fallback=None, out=None, out_dtype=None, stream=None):
    """The chroma of the frames at `times` between the chroma c0 and c1 (uint8
    CUDA tensors, I420 [B, 2, rc, cc] or NV12 [B, rc, cc, 2]) from the
    full-resolution flows of the luma solve, float32 [B, 2 rc, 2 cc]
    (hsflow_chroma_interp_device, KIY): temporal.downflow_device of both flow
    pairs and hsflow.frame_interp_device on the U and on the V planes, bit for
    bit, in one launch.  counts_f, counts_b (int32 [B, 3], the luma's from
    hsflow.consistency_device) and fallback (a fallback.Fallback): a pair that
    fails fallback.min_consistent(2 rc, 2 cc, min_share) gets
    fallback.frame_fallback_device's value.  out: float32 (default) or uint8,
    [B, len(times)] + the chroma's shape.  Returns out.  Stream-ordered.
    16-bit chroma (uint16 or int16 tensors; hsflow_chroma_interp16_device): the
    same on the sample values, out float32 or uint16."""
    lay = _layout(layout)
    dims = _chroma_pair(c0, c1, lay)
    hsflow._check_planes(dims, uf=uf, vf=vf, ub=ub, vb=vb)
    tm = hsflow._times_array(times)
    out = _chroma_out(c0, len(tm), out, out_dtype)
    keep, fb = hsflow._option(hsflow._Fallback, fallback)
    counts = [None, None]
    if fallback is not None:
        import fallback as _fallback
        counts = [_fallback._counts(c, dims[2], c0.device, n)
                  for c, n in ((counts_f, "counts_f"), (counts_b, "counts_b"))]
    if hsflow._is16(c0.dtype):  # cells null: KIY's definition
        counts = [None] + counts
    name = "hsflow_chroma_interp16_device" if hsflow._is16(c0.dtype) else \
        "hsflow_chroma_interp_device"
    hsflow._device_call(name, c0.device, stream, c0.data_ptr(),
                        c1.data_ptr(), lay, *dims, uf.data_ptr(), vf.data_ptr(), ub.data_ptr(),
                        vb.data_ptr(), *counts, fb, tm, len(tm), out.data_ptr(),
                        hsflow._out_code(out))
    return out


def proj_blocks_per_cu() -> int:
    """The cap of KIYP's grid in blocks per compute unit
    (hsflow_chroma_interp_proj_blocks_per_cu); tiles as KIY's."""
    return int(hsflow.lib().hsflow_chroma_interp_proj_blocks_per_cu())


def _luma_cells(cells, dims, nt, device, lead):
    """KS's cells of the luma, int64 [B, nt, rows, cols] (no B for a single
    frame's chroma), checked."""
    rows, cols, _ = dims
    import projection as _projection
    return _projection._cells(cells, lead + (rows, cols), nt, device)


def cells_down_device(cells, cells_c=None, stream=None):
    """projection.project_device's cells of the luma, int64 [B, nt, rows, cols]
    or [nt, rows, cols] (rows, cols even), reduced to the chroma grid
    (hsflow_cells_down_device, KSD): the unsigned 64-bit minimum of each 2 x 2
    block, the winner's source index re-coded to the chroma grid; a chroma cell
    is empty only where all four are.  Returns cells_c, int64 [..., rows / 2,
    cols / 2], for projection.frame_interp_device on a chroma plane.  One
    launch.  Stream-ordered."""
    if torch is None or not isinstance(cells, torch.Tensor) or cells.dtype != torch.int64 or \
            cells.dim() not in (3, 4) or not cells.is_cuda or not cells.is_contiguous():
        raise hsflow.HsflowError(hsflow.HSFLOW_ERR_ARG, "cells: need a contiguous int64 CUDA "
                                 "tensor [B, nt, rows, cols] or [nt, rows, cols]")
    rows, cols = cells.shape[-2:]
    _even(rows, cols)
    batch = cells.shape[0] if cells.dim() == 4 else 1
    nt = cells.shape[-3]
    shape = tuple(cells.shape[:-2]) + (rows // 2, cols // 2)
    cells_c = hsflow._check_output(True if cells_c is None else cells_c, shape, torch.int64,
                                   cells.device, "cells_c")
    hsflow._device_call("hsflow_cells_down_device", cells.device, stream, cells.data_ptr(),
                        int(rows), int(cols), int(batch), int(nt), cells_c.data_ptr())
    return cells_c


def chroma_interp_proj_device(c0, c1, uf, vf, ub, vb, times, cells, layout=YUV_I420,
                              counts_f=None, counts_b=None, fallback=None, out=None,
                              out_dtype=None, stream=None):
    """chroma_interp_device with each sample's time-t flow read through `cells`,
    projection.project_device's tensor of the luma for the same `times`
    (hsflow_chroma_interp_proj_device, KIYP): temporal.downflow_device of both
    flow pairs, cells_down_device and projection.frame_interp_device on the U
    and on the V planes, bit for bit, in one launch; a sample whose four luma
    cells are empty is chroma_interp_device's.  Every other argument as there,
    16-bit chroma included.  Returns out.  Stream-ordered."""
    lay = _layout(layout)
    dims = _chroma_pair(c0, c1, lay)
    hsflow._check_planes(dims, uf=uf, vf=vf, ub=ub, vb=vb)
    tm = hsflow._times_array(times)
    if cells is None:
        raise hsflow.HsflowError(hsflow.HSFLOW_ERR_ARG, "cells: need the luma's cells")
    cells = _luma_cells(cells, dims, len(tm), c0.device, tuple(c0.shape[:-3]))
    out = _chroma_out(c0, len(tm), out, out_dtype)
    keep, fb = hsflow._option(hsflow._Fallback, fallback)
    counts = [None, None]
    if fallback is not None:
        import fallback as _fallback
        counts = [_fallback._counts(c, dims[2], c0.device, n)
                  for c, n in ((counts_f, "counts_f"), (counts_b, "counts_b"))]
    name = "hsflow_chroma_interp16_device" if hsflow._is16(c0.dtype) else \
        "hsflow_chroma_interp_proj_device"
    hsflow._device_call(name, c0.device, stream, c0.data_ptr(),
                        c1.data_ptr(), lay, *dims, uf.data_ptr(), vf.data_ptr(), ub.data_ptr(),
                        vb.data_ptr(), cells.data_ptr(), *counts, fb, tm, len(tm),
                        out.data_ptr(), hsflow._out_code(out))
    return out


def flow_interp_proj_workspace_bytes(rows: int, cols: int, batch: int, levels: int, nt: int,
                                     projection: int = 1, fallback: bool = False) -> int:
    """The workspace of flow_interp_yuv_proj_device
    (hsflow_flow_interp_yuv_pj_workspace_bytes): flow_interp_workspace_bytes
    plus, with projection 1, the cells of nt times; a prefilter's planes come on
    top (hsflow.prefilter_planes_bytes).  0 for a bad shape, nt or projection."""
    return int(hsflow.lib().hsflow_flow_interp_yuv_pj_workspace_bytes(
        rows, cols, batch, levels, nt, projection, 1 if fallback else 0))


def flow_interp_workspace_bytes(rows: int, cols: int, batch: int, levels: int,
                                fallback: bool = False) -> int:
    """The workspace of flow_interp_yuv_device
    (hsflow_flow_interp_yuv_workspace_bytes): the grey fused call's; a
    prefilter's planes come on top (hsflow.prefilter_planes_bytes)."""
    return int(hsflow.lib().hsflow_flow_interp_yuv_workspace_bytes(rows, cols, batch, levels,
                                                                   1 if fallback else 0))


def flow_interp_yuv_device(y0, c0, y1, c1, times, levels: int, warps: int, window: int,
                           iters: int, alpha: float, layout=YUV_I420, median: int = 0,
                           rel: float = hsflow.CONSISTENCY_REL,
                           abs: float = hsflow.CONSISTENCY_ABS, out_y=None, out_c=None,
                           out_dtype=None, flags=None, trusted=None, workspace=None, stream=None,
                           prefilter=None, smoothness=None, finest: int = 0, fallback=None,
                           init=None, cut=None):
    """hsflow.flow_interp_device on the luma planes y0, y1 (uint8 [B, H, W]) and
    chroma_interp_device on the flows and counts it leaves in the workspace: one
    call, the same bits (hsflow_flow_interp_yuv_device).  c0, c1, layout as in
    chroma_interp_device.  out_y [B, len(times), H, W] and out_c [B, len(times)]
    + the chroma's shape share their dtype, float32 (default) or uint8; flags,
    trusted and cut are the luma's.  prefilter, smoothness, finest, fallback,
    init and cut as in hsflow.flow_interp_bgr_device and
    temporal.flow_interp_device; there is no projection.  Returns (out_y, out_c,
    flags, trusted), and cut behind them where it was asked for.
    Stream-ordered.  flow_interp_yuv_proj_device is the form with a projection.
    16-bit frames (uint16 or int16 luma and chroma;
    hsflow_flow_interp_yuv16_device with projection 0): out_y, flags, trusted and
    cut are hsflow.flow_interp_device's on the luma as float32 (any sample above
    255 in the pair), out_y and out_c float32 or uint16."""
    return _flow_interp_yuv(None, y0, c0, y1, c1, times, levels, warps, window, iters, alpha,
                            layout, median, rel, abs, out_y, out_c, out_dtype, flags, trusted,
                            workspace, stream, prefilter, smoothness, finest, fallback, init, cut)


def flow_interp_yuv_proj_device(y0, c0, y1, c1, times, levels: int, warps: int, window: int,
                                iters: int, alpha: float, layout=YUV_I420, median: int = 0,
                                rel: float = hsflow.CONSISTENCY_REL,
                                abs: float = hsflow.CONSISTENCY_ABS, out_y=None, out_c=None,
                                out_dtype=None, flags=None, trusted=None, workspace=None,
                                stream=None, prefilter=None, smoothness=None, finest: int = 0,
                                fallback=None, init=None, cut=None, projection: int = 1):
    """flow_interp_yuv_device with a projection
    (hsflow_flow_interp_yuv_pj_device).  projection = 0: that call's launches
    and bits.  1: hsflow.flow_interp_device(projection=1) on the luma -- out_y,
    flags (FLAG_HOLE included), trusted and cut are its -- and
    chroma_interp_proj_device on the flows, cells and counts it leaves in the
    workspace (flow_interp_proj_workspace_bytes).  Returns as
    flow_interp_yuv_device; 16-bit frames as there.  Stream-ordered."""
    return _flow_interp_yuv(int(projection), y0, c0, y1, c1, times, levels, warps, window, iters,
                            alpha, layout, median, rel, abs, out_y, out_c, out_dtype, flags,
                            trusted, workspace, stream, prefilter, smoothness, finest, fallback,
                            init, cut)


def _flow_interp_yuv(projection, y0, c0, y1, c1, times, levels, warps, window, iters, alpha,
                     layout, median, rel, abs, out_y, out_c, out_dtype, flags, trusted, workspace,
                     stream, prefilter, smoothness, finest, fallback, init, cut):
    """Both fused device calls: projection None is hsflow_flow_interp_yuv_device,
    else hsflow_flow_interp_yuv_pj_device with that projection; 16-bit frames:
    hsflow_flow_interp_yuv16_device (projection None: 0)."""
    lay = _layout(layout)
    dims = hsflow._frame_pair(y0, y1)
    wide = hsflow._is16(y0.dtype)
    if y0.dtype != torch.uint8 and not wide:
        raise hsflow.HsflowError(hsflow.HSFLOW_ERR_ARG, "y0, y1: need uint8 luma planes")
    if _chroma_pair(c0, c1, lay) != dims or c0.device != y0.device:
        raise hsflow.HsflowError(hsflow.HSFLOW_ERR_SIZE,
                                 "the chroma is not that of the luma planes' shape")
    if c0.dtype != y0.dtype:
        raise hsflow.HsflowError(hsflow.HSFLOW_ERR_ARG, "luma and chroma differ in dtype")
    tm = hsflow._times_array(times)
    out_y, flags, trusted = hsflow._interp_outputs(y0, (), len(tm), out_y, out_dtype, flags,
                                                   trusted, wide)
    out_c = _chroma_out(c0, len(tm), out_c, out_y.dtype)
    if out_c.dtype != out_y.dtype:
        raise hsflow.HsflowError(hsflow.HSFLOW_ERR_ARG, "out_y and out_c differ in dtype")
    pf = hsflow._option(hsflow.Prefilter, prefilter)[1]
    sm = hsflow._option(hsflow.Smoothness, smoothness)[1]
    size_fn = hsflow.flow_interp_workspace_bytes
    if projection == 1:
        def size_fn(rows, cols, batch, lv):
            return flow_interp_proj_workspace_bytes(rows, cols, batch, lv, len(tm))
    workspace = hsflow._workspace(workspace, y0.device, size_fn, *dims, levels,
                                  prefilter=prefilter, fallback=fallback)
    _, _, start = hsflow._init_entry("hsflow_flow_interp", init, dims, 1)
    cut = hsflow._check_output(cut, (dims[2],), torch.uint8, y0.device, "cut")
    keep, fb = hsflow._option(hsflow._Fallback, fallback)
    name = "hsflow_flow_interp_yuv_device" if projection is None else \
        "hsflow_flow_interp_yuv_pj_device"
    proj = () if projection is None else (projection,)
    if wide:
        name, proj = "hsflow_flow_interp_yuv16_device", (projection or 0,)
    hsflow._device_call(name, y0.device, stream, y0.data_ptr(),
                        c0.data_ptr(), y1.data_ptr(), c1.data_ptr(), lay, *dims,
                        *hsflow._solve_args(levels, warps, median, window, iters, alpha, finest),
                        float(rel), float(abs), tm, len(tm), *proj, out_y.data_ptr(),
                        out_c.data_ptr(),
                        hsflow._out_code(out_y), hsflow._ptr(flags), hsflow._ptr(trusted),
                        hsflow._ptr(cut), pf, sm, *start, fb, *hsflow._ws_args(workspace))
    res = (out_y, out_c, flags, trusted)
    return res if cut is None else res + (cut,)


def interpolate_yuv(ctx, f0, f1, times, levels: int, warps: int, window: int, iters: int,
                    alpha: float, rows: int, cols: int, layout=YUV_I420, median: int = 0,
                    rel: float = hsflow.CONSISTENCY_REL, abs: float = hsflow.CONSISTENCY_ABS,
                    out_dtype=np.uint8, with_flags: bool = False, prefilter=None,
                    smoothness=None, finest=None, fallback=None, projection=None):
    """The packed frames at `times` between the packed 8-bit 4:2:0 frames f0 and
    f1 (uint8, rows * cols * 3 / 2 bytes each; rows, cols the luma's) on the
    hsflow.Context `ctx` (hsflow_flow_interp_yuv): the luma through
    Context.interpolate's path, the chroma through KIY.  Returns an array
    [len(times), rows * cols * 3 / 2] of out_dtype (uint8 or float32) in the
    same layout, or with_flags: (frames, flags, trusted) -- the luma's, flags
    uint8 [len(times), rows, cols].  prefilter, smoothness, finest and fallback
    as in Context.interpolate_bgr; the context's sequence mode is honoured and
    Context.last_cut set.  projection None: no projection, and a context with
    the projection on is refused; 0 or 1: that, whatever the context's setting
    (hsflow_flow_interp_yuv_pj: the luma through the projected path, the chroma
    through KIYP).
    np.uint16 frames (rows * cols * 3 / 2 16-bit samples each;
    hsflow_flow_interp_yuv16): the same on the sample values, out_dtype uint16
    (what uint8, the default, stands for) or float32; projection None is 0, and
    the context's projection setting is not consulted."""
    lay = _layout(layout)
    n = frame_bytes(rows, cols)
    kinds = {np.asarray(f).dtype for f in (f0, f1)}
    wide = np.dtype(np.uint16) in kinds
    if wide:  # the default stands for the frames' own type
        out_dtype = np.uint16 if np.dtype(out_dtype) == np.uint8 else out_dtype
    frames = []
    for f, name in ((f0, "f0"), (f1, "f1")):
        a = np.ascontiguousarray(f)
        if wide:
            if a.dtype != np.uint16 or a.size != n:
                raise hsflow.HsflowError(hsflow.HSFLOW_ERR_ARG, f"{name}: need a packed uint16 "
                                         f"frame of {n} samples ({rows}x{cols} 4:2:0), as the "
                                         f"other frame is; got {a.dtype} of {a.size}")
            frames.append(a)
            continue
        if a.dtype != np.uint8 or a.size != n:
            raise hsflow.HsflowError(hsflow.HSFLOW_ERR_ARG, f"{name}: need a packed uint8 frame "
                                     f"of {n} bytes ({rows}x{cols} 4:2:0)")
        frames.append(a)
    tm = hsflow._times_array(times)
    nt = len(tm)
    out = np.empty((nt, n), out_dtype)
    if wide and out.dtype not in (np.uint16, np.float32):
        raise hsflow.HsflowError(hsflow.HSFLOW_ERR_ARG, "out_dtype: need uint16 or float32 for "
                                 "uint16 frames")
    if not wide and out.dtype not in (np.uint8, np.float32):
        raise hsflow.HsflowError(hsflow.HSFLOW_ERR_ARG, "out_dtype: need uint8 or float32")
    flags = np.empty((nt, rows, cols), np.uint8) if with_flags else None
    trusted = np.zeros(nt, np.uint32) if with_flags else None
    vp = ctypes.c_void_p
    planes = (vp * nt)(*[out[k].ctypes.data for k in range(nt)])
    fplanes = (vp * nt)(*[flags[k].ctypes.data for k in range(nt)]) if with_flags else None
    name = "hsflow_flow_interp_yuv" if projection is None else "hsflow_flow_interp_yuv_pj"
    proj = () if projection is None else (int(projection),)
    if wide:
        name, proj = "hsflow_flow_interp_yuv16", (int(projection or 0),)
    ctx._call_with(prefilter, smoothness, name, frames[0].ctypes.data,
                   frames[1].ctypes.data, lay, int(rows), int(cols),
                   *hsflow._solve_args(levels, warps, median, window, iters, alpha), float(rel),
                   float(abs), tm, nt, *proj, planes,
                   U16 if out.dtype == np.uint16 else hsflow._dtype_code(out), fplanes,
                   trusted.ctypes.data if with_flags else None, finest=finest, fallback=fallback)
    return (out, flags, trusted) if with_flags else out
