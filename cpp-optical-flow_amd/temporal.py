"""Temporal warm start of the warped solves (include/hsflow.h, "temporal warm
start"): in video the motion of pair k+1 is almost the motion of pair k.

The backward flow of pair k, (ub, vb) for I1 -> I0, lives on I1's grid, and I1
is the first frame of pair k+1.  predict_device turns it into the start of pair
k+1 -- forward -(ub, vb), backward (ub, vb) read where that motion lands -- and
the four solves below take such a start as `init=`.  On a Context the same runs
by itself between consecutive host calls: set_temporal / sequence.

What to expect ("Temporal warm start"): for steady motion one level
and one warp from the prediction match the cold 3-level, 4-warp solve.  With
the pyramid kept, the warm solve beats the cold solve of the same schedule, and
a wrong prediction is repaired.  Without the pyramid (levels=1) a prediction
that is off by more than about a pixel is NOT repaired.  So keep `levels` and
halve `warps` when motion may change, use levels=1 only for steady motion, and
call reset at a scene cut.

Everything here calls the HIP path in libhsflow.so through hsflow's front ends.
"""
from __future__ import annotations

import collections
import contextlib

import hsflow
from hsflow import CONSISTENCY_ABS, CONSISTENCY_REL

FlowInit = collections.namedtuple("FlowInit", "uf vf ub vb", defaults=(None,) * 4)
FlowInit.__doc__ = """hsflow_flow_init: the start of a solve.  float32 CUDA tensors
like the frames ([B, H, W] or [H, W]), solver units, full resolution; (uf, vf)
starts the forward solve, (ub, vb) the backward one.  A pair of None starts
cold; predict_device returns one."""


def downflow_device(u, v, uc=None, vc=None, stream=None):
    """(u, v) one pyramid level down (hsflow_downflow_device), upflow_device's
    counterpart: float32 CUDA tensors [B, H, W] (or [H, W]) -> [B, ceil(H / 2),
    ceil(W / 2)], uc = ((a + b) + (c + d)) * 0.125 over each 2 x 2 block with the
    border replicated: the mean, in px of the coarser level.  uc, vc are
    allocated unless given and must not overlap u or v.  Returns (uc, vc).
    Stream-ordered."""
    dims = hsflow._dims(u.shape)
    hsflow._check_planes(dims, u=u, v=v)
    rc, cc = hsflow.pyramid_level_size(dims[0], dims[1], 1)
    if uc is None:
        uc = u.new_empty(tuple(u.shape[:-2]) + (rc, cc))
    if vc is None:
        vc = u.new_empty(tuple(u.shape[:-2]) + (rc, cc))
    hsflow._check_planes((rc, cc, dims[2]), uc=uc, vc=vc)
    hsflow._device_call("hsflow_downflow_device", u.device, stream, u.data_ptr(), v.data_ptr(),
                        dims[0], dims[1], uc.data_ptr(), vc.data_ptr(), rc, cc, dims[2])
    return uc, vc


def predict_device(ub, vb, forward=True, backward=True, out=None, stream=None):
    """Pair k's backward flow (ub, vb) -> the FlowInit of pair k+1
    (hsflow_flow_predict_device): uf = -ub, vf = -vb (`forward`), and ub, vb =
    the planes ub, vb sampled at (y + 8 vb, x + 8 ub), warp_image_device's bits
    (`backward`).  A pair not asked for is None; at least one.  `out`: a
    FlowInit of tensors to fill.  The outputs must not overlap the inputs.
    One launch.  Stream-ordered."""
    dims = hsflow._dims(ub.shape)
    hsflow._check_planes(dims, ub=ub, vb=vb)
    given = FlowInit(*out) if out is not None else FlowInit()
    planes = []
    for name, want in (("uf", forward), ("vf", forward), ("ub", backward), ("vb", backward)):
        t = getattr(given, name)
        planes.append(hsflow._plane(t, ub, dims, name + "_next") if want else None)
    hsflow._device_call("hsflow_flow_predict_device", ub.device, stream, ub.data_ptr(),
                        vb.data_ptr(), *dims, *[hsflow._ptr(t) for t in planes])
    return FlowInit(*planes)


def flow_warped_device(I0, I1, levels: int, warps: int, window: int, iters: int, alpha: float,
                       u=None, v=None, workspace=None, stream=None, median: int = 0,
                       prefilter=None, smoothness=None, finest: int = 0, init=None):
    """hsflow.flow_warped_device started from `init` (a FlowInit or a 4-tuple;
    only uf, vf are read): hsflow_flow_warped_init_device.  init=None is that
    call itself.  finest as there: the init stays full resolution."""
    return hsflow._flow_warped_device(I0, I1, levels, warps, window, iters, alpha, u, v, workspace,
                                      stream, median, prefilter, smoothness, init=init,
                                      finest=finest)


def flow_bidir_device(I0, I1, levels: int, warps: int, window: int, iters: int, alpha: float,
                      rel: float = CONSISTENCY_REL, abs: float = CONSISTENCY_ABS,
                      uf=None, vf=None, ub=None, vb=None, err_f=None, mask_f=True,
                      counts_f=None, err_b=None, mask_b=None, counts_b=None, workspace=None,
                      stream=None, median: int = 0, prefilter=None, smoothness=None,
                      finest: int = 0, init=None):
    """hsflow.flow_bidir_device started from `init`: the forward solve from
    (uf, vf), the backward one from (ub, vb) (hsflow_flow_bidir_init_device).
    The init planes must not overlap the outputs or the workspace.  finest as
    in hsflow.flow_bidir_device."""
    return hsflow._flow_bidir_device(I0, I1, levels, warps, window, iters, alpha, rel, abs, uf, vf,
                                     ub, vb, err_f, mask_f, counts_f, err_b, mask_b, counts_b,
                                     workspace, stream, median, prefilter, smoothness, init=init,
                                     finest=finest)


def flow_interp_device(I0, I1, times, levels: int, warps: int, window: int, iters: int,
                       alpha: float, median: int = 0, rel: float = CONSISTENCY_REL,
                       abs: float = CONSISTENCY_ABS, out=None, out_dtype=None, flags=None,
                       trusted=None, workspace=None, stream=None, prefilter=None,
                       smoothness=None, finest: int = 0, projection: int = 0, fallback=None,
                       cut=None, init=None):
    """hsflow.flow_interp_device with its solve started from `init`
    (hsflow_flow_interp_init_device); finest, projection, fallback and cut as
    there."""
    return hsflow._flow_interp_device(I0, I1, times, levels, warps, window, iters, alpha, median,
                                      rel, abs, out, out_dtype, flags, trusted, workspace, stream,
                                      prefilter, smoothness, init=init, finest=finest,
                                      projection=projection, fallback=fallback, cut=cut)


def flow_interp_bgr_device(bgr0, bgr1, times, levels: int, warps: int, window: int, iters: int,
                           alpha: float, median: int = 0, rel: float = CONSISTENCY_REL,
                           abs: float = CONSISTENCY_ABS, out=None, out_dtype=None, flags=None,
                           trusted=None, workspace=None, stream=None, prefilter=None,
                           smoothness=None, finest: int = 0, projection: int = 0, fallback=None,
                           cut=None, init=None):
    """hsflow.flow_interp_bgr_device with its solve started from `init`
    (hsflow_flow_interp_bgr_init_device); finest, projection, fallback and cut as
    there."""
    return hsflow._flow_interp_bgr_device(bgr0, bgr1, times, levels, warps, window, iters, alpha,
                                          median, rel, abs, out, out_dtype, flags, trusted,
                                          workspace, stream, prefilter, smoothness, init=init,
                                          finest=finest, projection=projection,
                                          fallback=fallback, cut=cut)


# ------------------------------------------------------- sequence mode (host)
def set_temporal(ctx, on: bool):
    """Sequence mode of an hsflow.Context (hsflow_ctx_set_temporal): on, flow_bidir,
    interpolate and interpolate_bgr start from the prediction the previous such
    call left (same size) and leave one for the next.  Feed them the
    consecutive pairs of one clip.  Switching drops the stored prediction."""
    hsflow._check(hsflow.lib().hsflow_ctx_set_temporal(ctx.handle, 1 if on else 0), ctx.handle)


def get_temporal(ctx) -> bool:
    """The context's sequence mode (hsflow_ctx_temporal)."""
    rc = hsflow.lib().hsflow_ctx_temporal(ctx.handle)
    if rc < 0:
        hsflow._check(rc, ctx.handle)
    return bool(rc)


def reset(ctx):
    """Drop the stored prediction (hsflow_ctx_temporal_reset): the next call
    solves cold.  Call it at a scene cut."""
    hsflow._check(hsflow.lib().hsflow_ctx_temporal_reset(ctx.handle), ctx.handle)


@contextlib.contextmanager
def sequence(ctx, finest=None):
    """Sequence mode on `ctx` inside the block, starting without a prediction;
    the previous setting is restored afterwards.  finest: the context's finest
    level (coarse.set_finest_level) inside the block, restored likewise; the
    prediction comes from the upsampled backward flow.  None leaves it."""
    was = get_temporal(ctx)
    with ctx._finest_as(finest):
        set_temporal(ctx, True)
        try:
            yield ctx
        finally:
            set_temporal(ctx, was)
