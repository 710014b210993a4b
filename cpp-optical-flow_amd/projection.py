"""Flow projection (include/hsflow.h, "flow projection"): the flows of a
bidirectional solve carried to time t before the frame at t is made.

The interpolation of hsflow.frame_interp_device forms an output pixel's time-t
flow from the four flows at that pixel.  Near a motion boundary the pixel
belongs to whichever surface lands on it at time t, so project_device sends
every pixel of both frames along its flow to where it is at t; per target the
candidate whose brightness matches the other frame best wins (one 64-bit
minimum per candidate, so the result does not depend on the order), and
frame_interp_device here samples both frames with the winner's flow.  A target
nothing lands on keeps hsflow.frame_interp_device's pixel and gets
FLAG_HOLE.

Every interpolating front end of hsflow, temporal and frames takes
`projection=`; on a Context the setting can also stay for a run of host calls:
set_projection / projection_as.

What to expect ("Flow projection"): about a third off the error in
the band around a moving object and off the whole frame's; pure shifts are
unchanged; the narrow ring of real occlusion stays.

Everything here calls the HIP path in libhsflow.so through hsflow's front ends.
"""
from __future__ import annotations

import hsflow

try:
    import torch
except Exception:  # pragma: no cover
    torch = None

FLAG_HOLE = 16          # HSFLOW_INTERP_HOLE: no candidate landed on the pixel
EMPTY_CELL = -1         # an int64 view of a cell nothing landed on (all ones)


def decode_cells(cells):
    """(hole, direction, source index) of a cell tensor or array of int64: hole
    where nothing landed, direction 0 (from I0 by the forward flow) or 1 (from
    I1 by the backward flow), index y * cols + x of the winning source pixel."""
    return cells == EMPTY_CELL, (cells >> 31) & 1, cells & 0x7FFFFFFF


def project_device(G0, G1, uf, vf, ub, vb, times, cells=None, stream=None):
    """The cells of `times` (each in [0, 1]; at most hsflow.MAX_TIMES) from the
    grey frames G0, G1 the flows were solved on -- CUDA tensors [B, H, W] or
    [H, W], uint8 / float16 / float32 / float64 -- and the flows I0 -> I1
    (uf, vf) and I1 -> I0 (ub, vb), float32 in solver units
    (hsflow_flow_project_device).  cells: int64 [B, len(times), H, W]
    (the library's uint64 words: cost << 32 | direction << 31 | source index,
    EMPTY_CELL where nothing landed), allocated unless given.  Returns cells.
    A memset and one launch.  Stream-ordered."""
    dims = hsflow._frame_pair(G0, G1)
    hsflow._check_planes(dims, uf=uf, vf=vf, ub=ub, vb=vb)
    tm = hsflow._times_array(times)
    cells = _cells(cells, G0.shape, len(tm), G0.device)
    hsflow._device_call("hsflow_flow_project_device", G0.device, stream, G0.data_ptr(),
                        G1.data_ptr(), hsflow._tensor_dtype(G0), *dims, uf.data_ptr(),
                        vf.data_ptr(), ub.data_ptr(), vb.data_ptr(), tm, len(tm),
                        cells.data_ptr())
    return cells


def _cells(cells, plane_shape, nt, device):
    """The int64 cell tensor [B, nt, H, W] of frames whose planes are
    `plane_shape` ([B, H, W] or [H, W]): the given one, checked, or a new one."""
    plane = tuple(plane_shape)
    shape = plane[:-2] + (nt,) + plane[-2:]
    return hsflow._check_output(True if cells is None else cells, shape, torch.int64, device,
                                "cells")


def frame_interp_device(I0, I1, uf, vf, ub, vb, times, cells, mask_f=None, mask_b=None, out=None,
                        out_dtype=None, flags=None, trusted=None, stream=None):
    """hsflow.frame_interp_device with each output pixel's time-t flow read at
    the source pixel its cell names (hsflow_frame_interp_proj_device): `cells`
    is project_device's tensor for the same `times`.  flags carry FLAG_HOLE
    where the cell is empty; such a pixel is hsflow.frame_interp_device's.
    Returns (out, flags, trusted) as there.  Stream-ordered."""
    dims = hsflow._frame_pair(I0, I1)
    hsflow._check_planes(dims, uf=uf, vf=vf, ub=ub, vb=vb)
    hsflow._check_masks(I0.shape, I0.device, mask_f, mask_b)
    tm = hsflow._times_array(times)
    cells = _cells(cells, I0.shape, len(tm), I0.device)
    out, flags, trusted = hsflow._interp_outputs(I0, (), len(tm), out, out_dtype, flags, trusted)
    hsflow._device_call("hsflow_frame_interp_proj_device", I0.device, stream, I0.data_ptr(),
                        I1.data_ptr(), hsflow._tensor_dtype(I0), *dims, uf.data_ptr(),
                        vf.data_ptr(), ub.data_ptr(), vb.data_ptr(), hsflow._ptr(mask_f),
                        hsflow._ptr(mask_b), cells.data_ptr(), tm, len(tm), out.data_ptr(),
                        hsflow._out_code(out), hsflow._ptr(flags), hsflow._ptr(trusted))
    return out, flags, trusted


def frame_interp_bgr_device(bgr0, bgr1, uf, vf, ub, vb, times, cells, mask_f=None, mask_b=None,
                            out=None, out_dtype=None, flags=None, trusted=None, stream=None):
    """hsflow.frame_interp_bgr_device through `cells`
    (hsflow_frame_interp_bgr_proj_device): the cells come from project_device on
    hsflow.bgr_to_gray_device of both frames; channel c of the result has the
    bits frame_interp_device here gives the plane bgr[..., c].  Stream-ordered."""
    dims = hsflow._bgr_pair(bgr0, bgr1)
    hsflow._check_planes(dims, uf=uf, vf=vf, ub=ub, vb=vb)
    hsflow._check_masks(bgr0.shape[:-1], bgr0.device, mask_f, mask_b)
    tm = hsflow._times_array(times)
    cells = _cells(cells, bgr0.shape[:-1], len(tm), bgr0.device)
    out, flags, trusted = hsflow._interp_outputs(bgr0, (3,), len(tm), out, out_dtype, flags,
                                                 trusted)
    hsflow._device_call("hsflow_frame_interp_bgr_proj_device", bgr0.device, stream,
                        bgr0.data_ptr(), bgr1.data_ptr(), *dims, uf.data_ptr(), vf.data_ptr(),
                        ub.data_ptr(), vb.data_ptr(), hsflow._ptr(mask_f), hsflow._ptr(mask_b),
                        cells.data_ptr(), tm, len(tm), out.data_ptr(), hsflow._out_code(out),
                        hsflow._ptr(flags), hsflow._ptr(trusted))
    return out, flags, trusted


def flow_interp_workspace_bytes(rows: int, cols: int, batch: int, levels: int, nt: int) -> int:
    """Workspace of hsflow.flow_interp_device(projection=1) at nt times
    (hsflow_flow_interp_pj_workspace_bytes): hsflow.flow_interp_workspace_bytes
    plus the cells; a prefilter's planes come on top, as ever."""
    return int(hsflow.lib().hsflow_flow_interp_pj_workspace_bytes(rows, cols, batch, levels, nt))


def flow_interp_bgr_workspace_bytes(rows: int, cols: int, batch: int, levels: int,
                                    nt: int) -> int:
    """Likewise for hsflow.flow_interp_bgr_device(projection=1)."""
    return int(hsflow.lib().hsflow_flow_interp_bgr_pj_workspace_bytes(rows, cols, batch, levels,
                                                                      nt))


def set_projection(ctx, projection: int = 0):
    """Whether the host calls interpolate and interpolate_bgr of an
    hsflow.Context project the flows first (hsflow_ctx_set_projection): 1 or 0
    (default).  The flow solves ignore it."""
    ctx._set_projection(projection)


def get_projection(ctx) -> int:
    """The context's projection (hsflow_ctx_projection)."""
    return ctx._projection()


def projection_as(ctx, projection):
    """Context manager: `projection` as the context's setting inside the block,
    the previous one after; None leaves the context's own."""
    return ctx._projection_as(projection)
