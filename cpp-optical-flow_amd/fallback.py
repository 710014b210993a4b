"""Fallback for a failed pair (include/hsflow.h, "fallback for a failed pair"):
a source frame, or a cross-fade, where a pair's flows fail the check.

A scene cut, a fade the prefilter is not set up for, a motion beyond the
pyramid's reach: the flows of such a pair mean nothing, and the frames made from
them are morphs of two unrelated pictures.  The forward-backward check already
counts the consistent pixels of every pair; their share, both directions
together, is at least 0.55 for related pairs within reach and at most 0.32 for
unrelated ones ("Fallback for a failed pair"), so the default
threshold is 0.4.  frame_fallback_device takes that verdict on the device, with
no host synchronisation, and replaces a failed pair's frames, flags and trusted
counts; a pair that passes keeps its bytes.  A pair that is a cut in half the
picture lands at 0.43 - 0.54: no threshold decides that case.

Every interpolating front end of hsflow, temporal and frames takes `fallback=`;
on a Context the setting can also stay for a run of host calls: set_fallback /
fallback_as, and last_cut tells what the last call found.

Everything here calls the HIP path in libhsflow.so through hsflow's front ends.
"""
from __future__ import annotations

import hsflow

try:
    import torch
except Exception:  # pragma: no cover
    torch = None


# modes (HSFLOW_FALLBACK_*), the default threshold and the flag of a replaced
# pixel (HSFLOW_INTERP_FALLBACK)
FALLBACK_OFF, FALLBACK_NEAREST, FALLBACK_BLEND = 0, 1, 2
FALLBACK_MIN_SHARE = 0.4
FLAG_FALLBACK = 32
# Fallback(mode=FALLBACK_NEAREST, min_share=FALLBACK_MIN_SHARE): hsflow_fallback
Fallback = hsflow._Fallback


def min_consistent(rows: int, cols: int, min_share: float = FALLBACK_MIN_SHARE) -> int:
    """The count below which a pair fails (hsflow_fallback_min_consistent): the
    smallest integer >= float32(min_share) * 2 * rows * cols; 0 for a bad size or
    share."""
    return int(hsflow.lib().hsflow_fallback_min_consistent(int(rows), int(cols),
                                                           float(min_share)))


def counts_bytes(batch: int) -> int:
    """What the workspace of a fused call grows by with a fallback on
    (hsflow_fallback_counts_bytes)."""
    return int(hsflow.lib().hsflow_fallback_counts_bytes(int(batch)))


def _counts(counts, batch, device, name):
    if torch is None or not isinstance(counts, torch.Tensor) or not counts.is_cuda or \
            counts.device != device or counts.dtype != torch.int32 or \
            not counts.is_contiguous() or counts.numel() != batch * 3:
        raise hsflow.HsflowError(hsflow.HSFLOW_ERR_ARG, f"{name}: need a contiguous int32 CUDA "
                                 f"tensor [{batch}, 3] (flow_consistency_device's counts)")
    return counts.data_ptr()


def _fallback_call(name, frames, lead, dims, channels, counts_f, counts_b, fallback, times, out,
                   out_dtype, flags, trusted, cut, stream):
    if out is None:
        raise hsflow.HsflowError(hsflow.HSFLOW_ERR_ARG, "out: the interpolation's frames are "
                                 "required (a pair that passes keeps them)")
    tm = hsflow._times_array(times)
    out, flags, trusted = hsflow._interp_outputs(frames, channels, len(tm), out, out_dtype, flags,
                                                 trusted)
    cut = hsflow._check_output(cut, (dims[2],), torch.uint8, frames.device, "cut")
    keep, fb = hsflow._option(Fallback, fallback)
    hsflow._device_call(name, frames.device, stream, *lead, *dims,
                        _counts(counts_f, dims[2], frames.device, "counts_f"),
                        _counts(counts_b, dims[2], frames.device, "counts_b"), fb, tm, len(tm),
                        out.data_ptr(), hsflow._out_code(out), hsflow._ptr(flags),
                        hsflow._ptr(trusted), hsflow._ptr(cut))
    return out, flags, trusted, cut


def frame_fallback_device(I0, I1, counts_f, counts_b, fallback, times, out, flags=None,
                          trusted=None, cut=True, stream=None):
    """The verdict of every pair and the replacement of the failed ones
    (hsflow_frame_fallback_device), over the outputs hsflow.frame_interp_device
    gave for the same frames and times: `out` (float32 or uint8 [B, len(times),
    H, W]; required), `flags` and `trusted` as there.  counts_f, counts_b: the
    int32 [B, 3] counts of hsflow.flow_consistency_device each way.  fallback:
    a Fallback with mode FALLBACK_NEAREST or FALLBACK_BLEND.  cut: True or a
    uint8 tensor [B]; None for none.  A failed pair's frames are I0 / I1 or
    their cross-fade, its flags FLAG_FALLBACK, its trusted counts 0; a pair
    that passes keeps its bytes.  Returns (out, flags, trusted, cut).  One
    launch.  Stream-ordered."""
    dims = hsflow._frame_pair(I0, I1)
    return _fallback_call("hsflow_frame_fallback_device", I0,
                          (I0.data_ptr(), I1.data_ptr(), hsflow._tensor_dtype(I0)), dims, (),
                          counts_f, counts_b, fallback, times, out, None, flags, trusted, cut,
                          stream)


def frame_fallback_bgr_device(bgr0, bgr1, counts_f, counts_b, fallback, times, out, flags=None,
                              trusted=None, cut=True, stream=None):
    """frame_fallback_device for colour frames, uint8 [B, H, W, 3]
    (hsflow_frame_fallback_bgr_device): the same per channel; flags, trusted
    and cut are per pixel and per pair as there."""
    dims = hsflow._bgr_pair(bgr0, bgr1)
    return _fallback_call("hsflow_frame_fallback_bgr_device", bgr0,
                          (bgr0.data_ptr(), bgr1.data_ptr()), dims, (3,), counts_f, counts_b,
                          fallback, times, out, None, flags, trusted, cut, stream)


def set_fallback(ctx, fallback=None):
    """What the host calls interpolate and interpolate_bgr of an hsflow.Context
    do with a pair that fails the check (hsflow_ctx_set_fallback): a Fallback;
    None or mode FALLBACK_OFF = nothing (default).  The flow solves ignore it."""
    ctx._set(Fallback, fallback)


def get_fallback(ctx):
    """The context's Fallback (hsflow_ctx_fallback), None when off."""
    return ctx._get(Fallback)


def fallback_as(ctx, fallback):
    """Context manager: `fallback` as the context's setting inside the block,
    the previous one after; None leaves the context's own."""
    return ctx._setting_as(Fallback, fallback)


def last_cut(ctx):
    """The verdict of the context's last interpolate / interpolate_bgr
    (hsflow_ctx_last_cut): True for a cut, False for a pair that passed, None
    where there was no such call or the fallback was off."""
    return ctx.last_cut
