"""Coarse solve of the warped family (include/hsflow.h, "coarse solve"): the
flow solved down to pyramid level `finest` only, the frames interpolated at
full resolution.

Level 0 holds 76 % of a 3-level solve's pixel x iterations, and interpolation
needs a flow good enough to fetch the right source pixel, not a level-0 solve.
Every warped-family front end of hsflow and temporal takes `finest=`; the flow
of level `finest` reaches the full frame through upflow_bilinear_device, one
call per level, and the flows returned are full resolution in solver units as
ever.  On a Context the setting can also stay for a run of host calls:
set_finest_level / finest_level_as.

What to expect ("Coarse solve"): finest = 1 solves a quarter of the
pixels; pure shifts lose nothing visible; a motion boundary becomes one coarse
pixel wide, which at 4K is the 1080p grid every other figure was measured on.

Everything here calls the HIP path in libhsflow.so through hsflow's front ends.
"""
from __future__ import annotations

import hsflow


def upflow_bilinear_device(uc, vc, u=None, v=None, shape=None, stream=None):
    """(uc, vc) one pyramid level up, bilinearly (hsflow_upflow_bilinear_device):
    float32 CUDA tensors [B, rc, cc] (or [rc, cc]) -> [B, rows, cols] with
    ceil(rows / 2) = rc and ceil(cols / 2) = cc, pixel centres aligned, border
    replicated, values doubled: the step that brings the flow of a coarse solve
    to the full frame, where hsflow.upflow_device is the nearest-neighbour warm
    start.  The fine size comes from u and v where given, else from `shape` =
    (rows, cols), else it is (2 rc, 2 cc); u, v are allocated unless given and
    must not overlap uc or vc.  Returns (u, v).  One launch.  Stream-ordered."""
    rc, cc, batch = hsflow._dims(uc.shape)
    hsflow._check_planes((rc, cc, batch), uc=uc, vc=vc)
    if u is not None:
        shape = tuple(u.shape[-2:])
    elif v is not None:
        shape = tuple(v.shape[-2:])
    elif shape is None:
        shape = (2 * rc, 2 * cc)
    rows, cols = (int(n) for n in shape)
    if u is None:
        u = uc.new_empty(tuple(uc.shape[:-2]) + (rows, cols))
    if v is None:
        v = uc.new_empty(tuple(uc.shape[:-2]) + (rows, cols))
    hsflow._check_planes((rows, cols, batch), u=u, v=v)
    hsflow._device_call("hsflow_upflow_bilinear_device", uc.device, stream, uc.data_ptr(),
                        vc.data_ptr(), rc, cc, u.data_ptr(), v.data_ptr(), rows, cols, batch)
    return u, v


def set_finest_level(ctx, finest: int = 0):
    """The last pyramid level the host calls flow_warped, flow_bidir, interpolate
    and interpolate_bgr of an hsflow.Context solve (hsflow_ctx_set_finest_level);
    it must be below the call's `levels`.  0 = the full frame (default).  flow,
    flow_bgr, flow_pyramid and gradients ignore it."""
    ctx._set_finest_level(finest)


def get_finest_level(ctx) -> int:
    """The context's finest level (hsflow_ctx_finest_level)."""
    return ctx._finest_level()


def finest_level_as(ctx, finest):
    """Context manager: `finest` as the context's finest level inside the block,
    the previous setting after; None leaves the context's own."""
    return ctx._finest_as(finest)
