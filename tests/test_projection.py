"""Flow projection (include/hsflow.h, "flow projection"; DESIGN.md, "Flow
projection"): KS carries both flows of a bidirectional solve to time t, KIP
interpolates the frame there with the flow that landed on each pixel.

The float64 reference below restates the rule on test_interp's _sample_np:
project_np makes the cells of one pair and one time and says which targets are
"in doubt" -- where a rounding of the f32 arithmetic may legitimately decide
otherwise -- and frame_interp_proj_np resolves and blends given cells.  The GPU
comparisons upload nothing the reference did not make: KS is compared cell by
cell outside the doubt, KIP on the reference's own cells under
test_interp_kernel_against_reference's tolerance and bands.

CPU tests: the reference's quality on the moving square and on pure shifts, its
identities, the share of doubtful targets of every GPU case, argument errors,
the Python surface, the C++ adapter.  GPU tests are marked gpu.
"""
import ctypes
import functools
import inspect
import os
import shutil
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from synth_ref import synth_pair as np_synth
from test_consistency import HOSTILE
from test_interp import (ABS, BAND, QUALITY, REL, SOLVE, TOL, _assert_shift_quality, _cuda,
                         _e2e_ref, _flows, _guards_intact, _interior, _masks, _mean_err,
                         _pair_frames, _placed, _same_bits, _sample_np, _solve_ref, _textures,
                         _truth, frame_interp_np)
from test_smoothness import LAM, OCCLUDER, WARPS4, _middle_ref, _ref, band_error

GAIN = 8.0
EMPTY = np.uint64(0xFFFFFFFFFFFFFFFF)
HOLE = 16
CODE_CAP = float(1 << 30)
# the doubt of a candidate (the issue's three conditions)
DOUBT_CODE, DOUBT_POS, DOUBT_HALF = 8e-3, 1e-3, 1e-3
DOUBT_CAP = 0.15  # of a case's targets

KS_SHAPES = [(3, 37, 131), (1, 67, 64), (1, 96, 128)]
TINY_SHAPES = [(2, 5, 3), (1, 1, 1)]
KINDS = ["u8", "f16", "f32", "f64"]
TIMES = {1: (0.3,), 3: (0.0, 0.5, 1.0)}
SHAPE_IDS = dict(ids=lambda s: "x".join(map(str, s)))
RING = [(slice(44, 84), slice(50, 53)), (slice(44, 84), slice(93, 96))]


# ------------------------------------------------------------ f64 reference
def _candidates(own, other, u, v, tau, direction):
    """One direction's candidates of one pair at one time: per source pixel
    the key, the target (flat index, -1 for none), its doubt, and the targets it
    could reach across a rounding boundary (a list of flat-index arrays)."""
    rows, cols = own.shape
    with np.errstate(invalid="ignore", over="ignore"):
        w, _, _, _, half = _sample_np(other, u, v)
        c8 = np.abs(w - np.asarray(own, np.float64)) * 8.0
        c8 = np.where(c8 < CODE_CAP, c8, CODE_CAP)  # NaN -> the cap
        code = np.floor(c8).astype(np.uint64)
        dx = np.fmin(np.fmax(GAIN * np.asarray(u, np.float64), -float(cols)), float(cols))
        dy = np.fmin(np.fmax(GAIN * np.asarray(v, np.float64), -float(rows)), float(rows))
        xs, ys = np.arange(cols)[None, :], np.arange(rows)[:, None]
        tx, ty = xs + tau * dx + 0.5, ys + tau * dy + 0.5
    src = (ys * cols + xs).astype(np.uint64)
    key = (code << np.uint64(32)) | np.uint64(direction << 31) | src

    def flat(qx, qy):
        ok = (qx >= 0) & (qx < cols) & (qy >= 0) & (qy < rows)
        return np.where(ok, qy.astype(np.int64) * cols + qx.astype(np.int64), -1)

    target = flat(np.floor(tx), np.floor(ty))
    near_code = (c8 != 0.0) & (np.abs(c8 - np.rint(c8)) <= DOUBT_CODE)
    near_pos = (np.abs(tx - np.rint(tx)) <= DOUBT_POS) | (np.abs(ty - np.rint(ty)) <= DOUBT_POS)
    doubt = near_code | near_pos | (half <= DOUBT_HALF)
    reach = [flat(np.floor(tx + ex), np.floor(ty + ey))
             for ex in (-DOUBT_POS, DOUBT_POS) for ey in (-DOUBT_POS, DOUBT_POS)]
    return key, target, doubt, reach


def project_np(G0, G1, uf, vf, ub, vb, t):
    """The cells (uint64 [rows, cols]) of one pair at time t, and the targets in
    doubt: those that receive a doubtful candidate, or could across a rounding
    boundary.  t and 1 - t as the f32 values the kernel multiplies by."""
    rows, cols = np.asarray(G0).shape
    t32 = np.float32(t)
    tau = (float(t32), float(np.float32(1.0) - t32))
    cells = np.full(rows * cols, EMPTY, np.uint64)
    taint = np.zeros(rows * cols, bool)
    for direction, (own, other, u, v) in enumerate(((G0, G1, uf, vf), (G1, G0, ub, vb))):
        key, target, doubt, reach = _candidates(own, other, u, v, tau[direction], direction)
        hit = target >= 0
        np.minimum.at(cells, target[hit], key[hit])
        for q in [target] + reach:
            sel = doubt & (q >= 0)
            taint[q[sel]] = True
    return cells.reshape(rows, cols), taint.reshape(rows, cols)


def _blend_np(I0, I1, u0, v0, u1, v1, t, mask_f, mask_b):
    """frame_interp_np from the two time-t flows on: out, flags, rim, half."""
    with np.errstate(invalid="ignore", over="ignore"):
        s0, in0, n0, rim0, half0 = _sample_np(I0, u0, v0)
        s1, in1, n1, rim1, half1 = _sample_np(I1, u1, v1)
        wt = np.where(in0 == in1, t, np.where(in0, 0.0, 1.0))
        out = np.where(wt == 0.0, s0, np.where(wt == 1.0, s1, (1.0 - wt) * s0 + wt * s1))
    flags = (~in0).astype(np.uint8) | ((~in1).astype(np.uint8) << 1)
    if mask_f is not None:
        flags |= (np.asarray(mask_f).ravel()[n0] != 0).astype(np.uint8) << 2
    if mask_b is not None:
        flags |= (np.asarray(mask_b).ravel()[n1] != 0).astype(np.uint8) << 3
    return out, flags, np.minimum(rim0, rim1), np.minimum(half0, half1)


def frame_interp_proj_np(I0, I1, uf, vf, ub, vb, t, cells, mask_f=None, mask_b=None):
    """The projected frame of one pair at time t given its cells: out, flags
    (HOLE included), and frame_interp_np's two distances."""
    uf, vf, ub, vb = (np.asarray(a, np.float64) for a in (uf, vf, ub, vb))
    cells = np.asarray(cells, np.uint64)
    t = float(np.float32(t))
    s = 1.0 - t
    a, b, c = s * t, t * t, s * s
    hole = cells == EMPTY
    back = ((cells >> np.uint64(31)) & np.uint64(1)) != 0
    p = np.where(hole, 0, cells & np.uint64(0x7FFFFFFF)).astype(np.int64)
    assert p.max() < uf.size
    with np.errstate(invalid="ignore", over="ignore"):
        ut = np.where(back, -ub.ravel()[p], uf.ravel()[p])
        vt = np.where(back, -vb.ravel()[p], vf.ravel()[p])
        u0 = np.where(hole, b * ub - a * uf, -t * ut)
        v0 = np.where(hole, b * vb - a * vf, -t * vt)
        u1 = np.where(hole, c * uf - a * ub, s * ut)
        v1 = np.where(hole, c * vf - a * vb, s * vt)
    out, flags, rim, half = _blend_np(I0, I1, u0, v0, u1, v1, t, mask_f, mask_b)
    return out, flags | (hole.astype(np.uint8) * HOLE), rim, half


def projected_np(I0, I1, uf, vf, ub, vb, t, mask_f=None, mask_b=None):
    """project_np then frame_interp_proj_np on the same frames: out, flags."""
    cells, _ = project_np(I0, I1, uf, vf, ub, vb, t)
    return frame_interp_proj_np(I0, I1, uf, vf, ub, vb, t, cells, mask_f, mask_b)[:2]


# ------------------------------------------------------------ shared inputs
@functools.lru_cache(maxsize=None)
def _cells_ref(shape, kind, times):
    """project_np of a shape's textures and smooth flows: cells and doubt,
    [B, nt, H, W]."""
    G0, G1 = _textures(shape, kind)
    flows = _flows(shape)
    batch, rows, cols = shape
    cells = np.empty((batch, len(times), rows, cols), np.uint64)
    doubt = np.empty(cells.shape, bool)
    for k in range(batch):
        for j, t in enumerate(times):
            cells[k, j], doubt[k, j] = project_np(G0[k], G1[k], *(a[k] for a in flows), t)
    cells.setflags(write=False)
    doubt.setflags(write=False)
    return cells, doubt


@functools.lru_cache(maxsize=None)
def _proj_ref(shape, kind, times, masks=True):
    """frame_interp_proj_np on the reference's own cells: out, flags and the
    pixels left out of the comparisons, [B, nt, H, W]."""
    I0, I1 = _textures(shape, kind)
    flows = _flows(shape)
    mf, mb = _masks(shape) if masks else (None, None)
    cells, _ = _cells_ref(shape, kind, times)
    batch, rows, cols = shape
    out = np.empty(cells.shape)
    flags = np.empty(cells.shape, np.uint8)
    rim, half = np.empty(cells.shape, bool), np.empty(cells.shape, bool)
    for k in range(batch):
        for j, t in enumerate(times):
            o, f, r, h = frame_interp_proj_np(
                I0[k], I1[k], *(a[k] for a in flows), t, cells[k, j],
                None if mf is None else mf[k], None if mb is None else mb[k])
            out[k, j], flags[k, j], rim[k, j], half[k, j] = o, f, r <= BAND, h <= BAND
    for a in (out, flags, rim, half):
        a.setflags(write=False)
    return out, flags, rim, half


def _square_flows():
    """The moving square's flows both ways: lam 0.3, 4 warps, alpha 100, 5 x 5
    median (test_smoothness' shared reference)."""
    return (*_ref(OCCLUDER, WARPS4, LAM), *_ref(OCCLUDER, WARPS4, LAM, backward=True))


def _ring_error(frame):
    e = np.abs(np.asarray(frame, np.float64) - _truth(OCCLUDER, 0.5))
    return float(np.concatenate([e[r].ravel() for r in RING]).mean())


def _assert_square_gain(plain, projected, holes, who):
    """The issue's two ratio conditions; the ring is printed, not asserted."""
    (bp, wp), (bj, wj) = band_error(plain), band_error(projected)
    print(f"{who} moving square, lam {LAM}, 4 warps, t 0.5: band {bp:.3f} -> {bj:.3f} "
          f"({bj / bp:.3f}), whole frame {wp:.4f} -> {wj:.4f} ({wj / wp:.3f}) grey levels; ring "
          f"{_ring_error(plain):.2f} -> {_ring_error(projected):.2f}; empty targets {holes} px")
    assert bj <= 0.8 * bp
    assert wj <= 0.8 * wp


# ------------------------------------------------------------------ CPU tests
def test_reference_projection_improves_the_moving_square():
    """Reference: band 4.30 -> 2.84, whole frame 0.608 -> 0.402 (0.66 both)."""
    I0, I1 = _pair_frames(OCCLUDER)
    out, flags = projected_np(I0, I1, *_square_flows(), 0.5)
    _assert_square_gain(_middle_ref(LAM), out, int((flags & HOLE != 0).sum()), "reference")


@pytest.mark.parametrize("pair,alpha,k,t", QUALITY)
def test_reference_projection_keeps_a_pure_shift(pair, alpha, k, t):
    """_assert_shift_quality holds for the projected frame, and its interior
    mean error is at most 1.02 x the unprojected one (reference: 1.000, 1.000,
    0.981)."""
    flows, _, _ = _solve_ref(pair, alpha, k)
    I0, I1 = _pair_frames(pair)
    out, flags = projected_np(I0, I1, *flows, t)
    _assert_shift_quality(out, pair, t, "reference, projected")
    truth = _truth(pair, t)
    got = _mean_err(_interior(out), _interior(truth))
    plain = _mean_err(_interior(_e2e_ref(pair, alpha, k, t)[0]), _interior(truth))
    print(f"reference {pair} t {t}: interior mean error {plain:.5f} -> {got:.5f} "
          f"({got / plain:.3f}); empty targets {np.mean(flags & HOLE != 0):.4f} of the frame")
    assert got <= 1.02 * plain


def test_reference_zero_flows_give_the_plain_blend():
    rng = np.random.default_rng(21)
    I0, I1 = rng.random((7, 9)) * 255, rng.random((7, 9)) * 255
    z = np.zeros((7, 9))
    for t in (0.0, 0.25, 0.5, 1.0):
        cells, _ = project_np(I0, I1, z, z, z, z, t)
        assert not (cells == EMPTY).any()  # every pixel lands on itself, twice
        out, flags, _, _ = frame_interp_proj_np(I0, I1, z, z, z, z, t, cells)
        assert np.abs(out - ((1.0 - t) * I0 + t * I1)).max() <= 1e-4
        assert not flags.any()


def test_reference_end_times_return_the_frames():
    rng = np.random.default_rng(22)
    I0, I1 = rng.random((9, 12)) * 255, rng.random((9, 12)) * 255
    uf, vf, ub, vb = (rng.normal(size=(9, 12)) for _ in range(4))
    assert np.array_equal(projected_np(I0, I1, uf, vf, ub, vb, 0.0)[0], I0)
    assert np.array_equal(projected_np(I0, I1, uf, vf, ub, vb, 1.0)[0], I1)


def test_reference_keys_order_by_cost_then_direction_then_index():
    """Two candidates on one target: the lower cost wins; on a tie direction 0,
    then the lower source index.  A 1 x 4 pair whose flows send pixels 0 and 1
    of I0 and pixel 3 of I1 to target 2 at t = 1 / 0."""
    z = np.zeros((1, 4))
    I0 = np.array([[10.0, 10.0, 0.0, 0.0]])
    I1 = np.array([[0.0, 0.0, 10.0, 10.0]])
    uf = np.array([[2.0, 1.0, 0.0, 0.0]]) / GAIN  # pixels 0 and 1 land on 2 at t = 1
    cells, _ = project_np(I0, I1, uf, z, z, z, 1.0)
    # costs: pixel 0 |I1[2] - 10| = 0, pixel 1 |I1[2] - 10| = 0, pixel 2 of I0
    # stays (cost |I1[2] - 0| = 10, code 80); I1's own pixel 2 at tau = 0: cost
    # |I0[2] - 10| = 10.  Tie between pixels 0 and 1 of direction 0: index 0.
    assert int(cells[0, 2]) == 0
    cells, _ = project_np(I0, I1, np.array([[0.0, 1.0, 0.0, 0.0]]) / GAIN, z, z, z, 1.0)
    assert int(cells[0, 2]) == 1
    # direction 1 with the same cost loses to direction 0
    I0b, I1b = np.array([[5.0, 5.0]]), np.array([[5.0, 5.0]])
    z2 = np.zeros((1, 2))
    cells, _ = project_np(I0b, I1b, z2, z2, z2, z2, 0.5)
    assert cells.tolist() == [[0, 1]]
    # NaN cost lands on the cap and still names its source
    cells, _ = project_np(np.array([[np.nan]]), np.array([[1.0]]), z[:, :1], z[:, :1], z[:, :1],
                          z[:, :1], 0.0)
    assert int(cells[0, 0]) == (1 << 62) | 0


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("shape", KS_SHAPES, **SHAPE_IDS)
def test_reference_doubt_is_under_the_cap(shape, kind):
    """Condition on the inputs of the GPU comparison of the cells: at most 15 %
    of a case's targets are in doubt, and the cases have holes and both
    directions among their winners."""
    for nt, times in TIMES.items():
        cells, doubt = _cells_ref(shape, kind, times)
        share = [float(doubt[:, j].mean()) for j in range(nt)]
        back = ((cells >> np.uint64(31)) & np.uint64(1) != 0) & (cells != EMPTY)
        print(f"{shape} {kind} nt {nt}: in doubt " + " ".join(f"{s:.4f}" for s in share)
              + f"; holes {np.mean(cells == EMPTY):.4f}, direction 1 wins {back.mean():.3f}")
        assert max(share) <= DOUBT_CAP
        assert back.any() and (~back & (cells != EMPTY)).any()
    assert (_cells_ref(shape, kind, TIMES[1])[0] == EMPTY).any()


def _times(*t):
    return (ctypes.c_float * len(t))(*t)


def test_argument_errors_without_a_gpu():
    import hsflow
    L = hsflow.lib()
    E = hsflow.HSFLOW_ERR_ARG
    nan = float("nan")
    half = _times(0.5)
    # never dereferenced: every call fails its checks first.  16 x 16 f32 planes
    # are 1024 bytes, a cell plane 2048; the addresses below are 4096 apart
    A = [4096 * k for k in range(1, 20)]

    def err():
        return L.hsflow_last_error(None).decode()

    def ks(G0=A[0], G1=A[1], uf=A[2], vf=A[3], ub=A[4], vb=A[5], times=half, nt=1, cells=A[6],
           dtype=hsflow.F32, rows=16, cols=16):
        return L.hsflow_flow_project_device(G0, G1, dtype, rows, cols, 1, uf, vf, ub, vb, times,
                                            nt, cells, None)

    for null in ("G0", "G1", "uf", "vf", "ub", "vb", "times", "cells"):
        assert ks(**{null: None}) == E, null
    for nt in (0, -1, 17):
        assert ks(times=_times(*([0.5] * 17)), nt=nt) == E and "nt" in err()
    for bad in (-0.01, 1.01, nan, float("inf")):
        assert ks(times=_times(bad)) == E and "time" in err()
    assert ks(dtype=7) == E and ks(rows=0) == E
    for off in (1, 2, 4, 7):
        assert ks(cells=A[6] + off) == E and "aligned" in err(), off
    for over in (dict(cells=A[0]), dict(cells=A[1] - 2040), dict(cells=A[5] + 1016),
                 dict(cells=A[2] - 8, times=_times(0.2, 0.4), nt=2),
                 dict(cells=A[3] - 4096 + 8, times=_times(0.2, 0.4), nt=2)):
        assert ks(**over) == E and "overlap" in err(), over
    # rows * cols > 2^31, and the largest legal-looking rows at that width
    assert ks(rows=65536, cols=32769) == E and "size" in err()
    assert ks(rows=1 << 16, cols=1 << 16) == E and "size" in err()

    def kip(bgr, I0=A[0], I1=A[1], uf=A[2], vf=A[3], ub=A[4], vb=A[5], mf=A[6], mb=A[7],
            cells=A[8], times=half, nt=1, out=A[10], dtype_out=hsflow.F32, flags=A[12],
            trusted=A[13], rows=16):
        if bgr:
            return L.hsflow_frame_interp_bgr_proj_device(I0, I1, rows, 16, 1, uf, vf, ub, vb, mf,
                                                         mb, cells, times, nt, out, dtype_out,
                                                         flags, trusted, None)
        return L.hsflow_frame_interp_proj_device(I0, I1, hsflow.F32, rows, 16, 1, uf, vf, ub, vb,
                                                 mf, mb, cells, times, nt, out, dtype_out, flags,
                                                 trusted, None)

    for bgr in (False, True):
        for null in ("I0", "I1", "uf", "vf", "ub", "vb", "out", "times", "cells"):
            assert kip(bgr, **{null: None}) == E, (bgr, null)
        assert kip(bgr, cells=A[8] + 4) == E and "aligned" in err()
        assert kip(bgr, nt=0) == E and kip(bgr, times=_times(nan)) == E and kip(bgr, rows=0) == E
        assert kip(bgr, dtype_out=hsflow.F64) == E
        for over in (dict(out=A[8]), dict(out=A[8] + 2044), dict(flags=A[8] + 2047),
                     dict(trusted=A[8] + 8), dict(out=A[0]), dict(flags=A[10] + 16)):
            assert kip(bgr, **over) == E and "overlap" in err(), (bgr, over)

    ws, big = 1 << 20, 1 << 30

    def fused(bgr, projection=1, levels=3, finest=0, wsb=big, times=half, nt=1, out=A[2],
              flags=A[5], trusted=A[6], rows=16, cols=16):
        tail = (levels, finest, 1, 0, 5, 10, 1.0, REL, ABS, times, nt, projection, out, hsflow.F32,
                flags, trusted, None, None, None, ws, wsb, None)
        if bgr:
            return L.hsflow_flow_interp_bgr_pj_device(A[0], A[1], rows, cols, 1, *tail)
        return L.hsflow_flow_interp_pj_device(A[0], A[1], hsflow.F32, rows, cols, 1, *tail)

    for bgr in (False, True):
        size_lv = (hsflow.flow_interp_bgr_workspace_bytes if bgr
                   else hsflow.flow_interp_workspace_bytes)(16, 16, 1, 3)
        size_pj = (L.hsflow_flow_interp_bgr_pj_workspace_bytes if bgr
                   else L.hsflow_flow_interp_pj_workspace_bytes)
        for bad in (-1, 2, 3, 1 << 30):
            assert fused(bgr, projection=bad) == E and "projection" in err(), (bgr, bad)
        # the workspace: the *_lv call's for projection 0, the cell planes more for 1
        assert size_pj(16, 16, 1, 3, 1) == size_lv + 2048
        assert size_pj(16, 16, 1, 3, 3) == size_lv + 3 * 2048
        assert size_pj(16, 16, 1, 3, 0) == 0 and size_pj(16, 16, 1, 3, 17) == 0
        assert size_pj(0, 16, 1, 3, 1) == 0 and size_pj(16, 16, 1, 9, 1) == 0
        assert fused(bgr, projection=0, wsb=size_lv - 1) == E and "workspace" in err()
        assert fused(bgr, projection=1, wsb=size_lv) == E and "workspace" in err()
        assert fused(bgr, projection=1, wsb=size_lv + 2047) == E and "workspace" in err()
        two = _times(0.25, 0.5)
        assert fused(bgr, times=two, nt=2, wsb=size_lv + 2048) == E and "workspace" in err()
        # an output inside the cells at the workspace's end
        assert fused(bgr, out=ws + size_lv + 1024, wsb=size_lv + 2048) == E and "overlap" in err()
        assert fused(bgr, finest=3) == E and "finest" in err()
        assert fused(bgr, levels=0) == E and fused(bgr, nt=0) == E
        assert fused(bgr, rows=65536, cols=32769) == E and "size" in err()

    # the context's setting: no context can be made here without a device
    assert L.hsflow_ctx_set_projection(None, 1) == E and "context" in err()
    assert L.hsflow_ctx_set_projection(None, 2) == E
    assert L.hsflow_ctx_projection(None) == E and "context" in err()


def test_exports_and_python_surface():
    import frames
    import hsflow
    import projection
    import temporal
    new = ("hsflow_flow_project_device", "hsflow_frame_interp_proj_device",
           "hsflow_frame_interp_bgr_proj_device", "hsflow_flow_interp_pj_device",
           "hsflow_flow_interp_bgr_pj_device", "hsflow_flow_interp_pj_workspace_bytes",
           "hsflow_flow_interp_bgr_pj_workspace_bytes", "hsflow_ctx_set_projection",
           "hsflow_ctx_projection")
    with open(os.path.join(ROOT, "include", "hsflow.h")) as f:
        header = f.read()
    for name in new:
        assert name in hsflow.EXPORTS and hasattr(hsflow.lib(), name)
        assert name + "(" in header
    assert "#define HSFLOW_HAS_PROJECTION 1" in header
    assert "#define HSFLOW_INTERP_HOLE 16" in header and projection.FLAG_HOLE == HOLE
    assert hsflow.lib().hsflow_version() == 20000
    for name in ("flow_interp_device", "flow_interp_bgr_device"):
        for mod in (hsflow, temporal):
            assert inspect.signature(getattr(mod, name)).parameters["projection"].default == 0
    for name in ("interpolate", "interpolate_bgr"):
        # None: the context's own setting, which is 0 unless set
        assert inspect.signature(getattr(hsflow.Context, name)).parameters["projection"].default \
            is None
    assert inspect.signature(hsflow.compute).parameters["projection"].default == 0
    assert inspect.signature(frames.interpolate_sequence).parameters["projection"].default is None
    for name in ("project_device", "frame_interp_device", "frame_interp_bgr_device",
                 "set_projection", "get_projection", "projection_as"):
        assert callable(getattr(projection, name))
    assert projection.flow_interp_workspace_bytes(16, 16, 1, 3, 2) == \
        hsflow.flow_interp_workspace_bytes(16, 16, 1, 3) + 2 * 2048
    assert projection.flow_interp_bgr_workspace_bytes(16, 16, 1, 3, 1) == \
        hsflow.flow_interp_bgr_workspace_bytes(16, 16, 1, 3) + 2048
    z = np.zeros((8, 8), np.uint8)
    with pytest.raises(hsflow.HsflowError, match="projection"):
        hsflow.compute(z, z, 1.0, 5, warps=1, projection=1)
    hole, back, src = projection.decode_cells(np.array([-1, 5, (7 << 32) | (1 << 31) | 9],
                                                       np.int64))
    assert hole.tolist() == [True, False, False]
    assert back.tolist()[1:] == [0, 1] and src.tolist()[1:] == [5, 9]


def test_setprojection_compiles_and_links(tmp_path):
    """A caller of the cv::Mat adapter's setProjection / projection (and of
    hsflow::Context's and hsflow::HornSchunck's) builds against
    include/hornSchunck.hpp, the cv::Mat test double and libhsflow.so; without
    a device the calls throw (never a crash)."""
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("no C++ compiler")
    src = tmp_path / "projection_main.cpp"
    src.write_text(r'''
#include <cstdio>
#include "hornSchunck.hpp"
#if !defined(HSFLOW_HAS_PROJECTION) || HSFLOW_HAS_PROJECTION != 1 || HSFLOW_INTERP_HOLE != 16
#error "hsflow.h lacks the flow projection"
#endif
int main() {
    hornSchunck hs(5, 10, 100.0);
    int thrown = 0, set = -1, back = -1, bad = 0;
    try {
        hs.setProjection(1);
        set = hs.projection();
        try { hs.setProjection(2); } catch (const cv::Exception &) { bad = 1; }
        if (hs.projection() != 1) return 4;  // a bad value leaves the old one
        hs.setProjection(0);
        back = hs.projection();
    } catch (const cv::Exception &) { ++thrown; }
    try {
        hsflow::Context c(0);
        c.setProjection(1);
        if (c.projection() != 1) return 3;
        hsflow::HornSchunck h(5, 10, 100.0);
        h.setProjection(1);
        if (h.projection() != 1) return 5;
    } catch (const hsflow::Error &) { ++thrown; }
    int (*ks)(const void *, const void *, int, int, int, int, const float *, const float *,
              const float *, const float *, const float *, int, uint64_t *, void *) =
        hsflow_flow_project_device;
    std::printf("%d %d %d %d %d %d %d\n", thrown, set, back, bad,
                hsflow_ctx_set_projection(nullptr, 1), hsflow_ctx_projection(nullptr),
                ks(nullptr, nullptr, 1, 16, 16, 1, nullptr, nullptr, nullptr, nullptr, nullptr, 1,
                   nullptr, nullptr));
    return 0;
}
''')
    lib_dir = os.path.join(ROOT, "cpp-optical-flow_amd")
    exe = str(tmp_path / "projection_main")
    subprocess.check_call([gxx, "-std=c++17", "-Wall", "-Werror",
                           "-I", os.path.join(ROOT, "tests", "cpp", "cvstub"),
                           "-I", os.path.join(ROOT, "include"), str(src), "-o", exe, "-L", lib_dir,
                           "-lhsflow", "-Wl,-rpath," + lib_dir])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    thrown, set_, back, bad, rc0, rc1, rc2 = (int(x) for x in out.stdout.split())
    # 2 thrown where no gfx950 device is present
    assert (thrown, set_, back, bad) in ((0, 1, 0, 1), (2, -1, -1, 0))
    assert (rc0, rc1, rc2) == (-1, -1, -1)


# ------------------------------------------------------------------ GPU tests
GUARD_F, GUARD_B, GUARD_C = -7.25, 0xA5, 0x0123456789ABCDEF


def _u64(t):
    """A cell tensor (int64) as numpy uint64."""
    return t.cpu().numpy().view(np.uint64)


def _cells_cuda(cells):
    return _cuda(np.asarray(cells).view(np.int64))


def _run_ks(shape, kind, times):
    import projection
    import torch
    G0, G1 = _textures(shape, kind)
    cells = projection.project_device(_cuda(G0), _cuda(G1), *(_cuda(a) for a in _flows(shape)),
                                      times)
    torch.cuda.synchronize()
    return cells


def _decodable(cells, plane):
    c = np.asarray(cells, np.uint64)
    full = c != EMPTY
    return bool(np.all((c[full] & np.uint64(0x7FFFFFFF)) < np.uint64(plane)))


@pytest.mark.gpu
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("shape", KS_SHAPES, **SHAPE_IDS)
def test_cells_against_reference(hs, shape, kind):
    """KS's cells equal project_np's word for word outside the targets in
    doubt (test_reference_doubt_is_under_the_cap bounds their share)."""
    for nt, times in TIMES.items():
        ref, doubt = _cells_ref(shape, kind, times)
        cells = _run_ks(shape, kind, times)
        assert tuple(cells.shape) == (shape[0], nt, *shape[1:])
        got = _u64(cells)
        differ = got != ref
        print(f"{shape} {kind} nt {nt}: in doubt {doubt.mean():.4f}, cells that differ "
              f"{differ.mean():.5f}, of them outside the doubt {int((differ & ~doubt).sum())}")
        assert doubt.mean() <= DOUBT_CAP
        assert not (differ & ~doubt).any()
        assert _decodable(got, shape[1] * shape[2])


@pytest.mark.gpu
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("shape", TINY_SHAPES, **SHAPE_IDS)
def test_cells_of_tiny_planes_are_decodable(hs, shape, kind):
    """One pixel is 3 % or more of these planes: no cap, only the guards and
    cells that decode to a source in the plane (and, for one pixel at t = 0,
    the pixel itself)."""
    import projection
    import torch
    G0, G1 = _textures(shape, kind)
    flows = [_cuda(a) for a in _flows(shape)]
    for nt, times in TIMES.items():
        fc, cells, (c0, c1) = _placed(None, 1, torch.int64, GUARD_C, (shape[0], nt, *shape[1:]))
        projection.project_device(_cuda(G0), _cuda(G1), *flows, times, cells=cells)
        torch.cuda.synchronize()
        assert _guards_intact(fc, c0, c1, GUARD_C)
        assert _decodable(_u64(cells), shape[1] * shape[2])
    if shape == (1, 1, 1):
        got = _u64(projection.project_device(_cuda(G0), _cuda(G1), *flows, (0.0,)))
        assert got.ravel()[0] != EMPTY and int(got.ravel()[0] & np.uint64(0x7FFFFFFF)) == 0


def _bgr_frames(shape):
    """Two BGR uint8 frames [B, H, W, 3] made of the shape's grey textures."""
    I0, I1 = _textures(shape, "u8")
    bgr0 = np.stack([I0, 255 - I1, I0[:, ::-1, :]], axis=-1)
    bgr1 = np.stack([I1, 255 - I0, I1[:, ::-1, :]], axis=-1)
    return np.ascontiguousarray(bgr0), np.ascontiguousarray(bgr1)


@pytest.mark.gpu
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("shape", KS_SHAPES[:2], **SHAPE_IDS)
def test_projected_interp_kernel_against_reference(hs, shape, kind):
    """KIP on the reference's own cells: |out - ref| <= 1e-4 max|ref| outside the
    rim band, flags (HOLE included) equal outside both bands, trusted the count
    of the device's own flags == 0; the u8 output is the rounded f32 one."""
    import projection
    import torch
    I0, I1 = (_cuda(a) for a in _textures(shape, kind))
    flows = [_cuda(a) for a in _flows(shape)]
    mf, mb = (_cuda(m) for m in _masks(shape))
    for nt, times in TIMES.items():
        ref, ref_flags, rim, half = _proj_ref(shape, kind, times)
        cells = _cells_cuda(_cells_ref(shape, kind, times)[0])
        out, flags, trusted = projection.frame_interp_device(
            I0, I1, *flows, times, cells, mask_f=mf, mask_b=mb, flags=True, trusted=True)
        u8 = projection.frame_interp_device(I0, I1, *flows, times, cells,
                                            out_dtype=torch.uint8)[0]
        torch.cuda.synchronize()
        out, flags, trusted = out.cpu().numpy(), flags.cpu().numpy(), trusted.cpu().numpy()
        assert out.shape == (shape[0], nt, *shape[1:]) and out.dtype == np.float32
        d = np.abs(out.astype(np.float64) - ref)[~rim]
        bound = TOL * float(np.abs(ref).max())
        print(f"{shape} {kind} nt {nt}: worst |out - ref| {d.max():.3e} (bound {bound:.3e}), "
              f"excluded {(rim | half).mean():.4f}, holes {np.mean(ref_flags & HOLE != 0):.4f}")
        assert np.all(d <= bound)
        keep = ~(rim | half)
        assert np.array_equal(flags[keep], ref_flags[keep])
        assert np.array_equal(flags & HOLE, ref_flags & HOLE)  # the cells alone decide
        assert (flags & HOLE).any()
        assert np.array_equal(trusted.astype(np.int64), (flags == 0).sum(axis=(2, 3)))
        want8 = np.clip(np.floor(out + np.float32(0.5)), 0.0, 255.0).astype(np.uint8)
        assert np.array_equal(u8.cpu().numpy(), want8)


@pytest.mark.gpu
@pytest.mark.parametrize("out_dtype", ["f32", "u8"])
def test_projected_bgr_kernel_equals_the_grey_kernel_per_channel(hs, out_dtype):
    """Each channel of KIP on BGR frames has the bits of KIP on that channel's
    plane with the same cells (here the reference's, made from grey textures);
    flags and trusted are the grey call's.  Both load forms.  Channel 0 is the
    u8 grey texture pair itself, so it meets frame_interp_proj_np's frame under
    the grey test's tolerance (u8 output: half a grey level more for the
    rounding) and its flags outside the bands."""
    import projection
    import torch
    shape, times = (3, 37, 131), TIMES[3]
    odt = torch.float32 if out_dtype == "f32" else torch.uint8
    bgr0, bgr1 = (_cuda(a) for a in _bgr_frames(shape))
    flows = [_cuda(a) for a in _flows(shape)]
    mf, mb = (_cuda(m) for m in _masks(shape))
    cells = _cells_cuda(_cells_ref(shape, "u8", times)[0])
    was = hs.set_interp_bgr_loads(False)
    try:
        outs = []
        for wide in (False, True):
            hs.set_interp_bgr_loads(wide)
            outs.append(projection.frame_interp_bgr_device(
                bgr0, bgr1, *flows, times, cells, mask_f=mf, mask_b=mb, out_dtype=odt,
                flags=True, trusted=True))
    finally:
        hs.set_interp_bgr_loads(was)
    (out, flags, trusted), (out_w, flags_w, trusted_w) = outs
    assert _same_bits(out, out_w) and torch.equal(flags, flags_w)
    assert torch.equal(trusted, trusted_w)
    for ch in range(3):
        o, f, c = projection.frame_interp_device(
            bgr0[..., ch].contiguous(), bgr1[..., ch].contiguous(), *flows, times, cells,
            mask_f=mf, mask_b=mb, out_dtype=odt, flags=True, trusted=True)
        assert _same_bits(out[..., ch].contiguous(), o)
        assert torch.equal(flags, f) and torch.equal(trusted, c)
    torch.cuda.synchronize()
    assert int((flags & HOLE != 0).sum()) > 0
    ref, ref_flags, rim, half = _proj_ref(shape, "u8", times)
    d = np.abs(out[..., 0].cpu().numpy().astype(np.float64) - ref)[~rim]
    bound = TOL * float(np.abs(ref).max()) + (0.5 if out_dtype == "u8" else 0.0)
    print(f"BGR {out_dtype} channel 0: worst |out - ref| {d.max():.3e} (bound {bound:.3e})")
    assert np.all(d <= bound)
    keep = ~(rim | half)
    assert np.array_equal(flags.cpu().numpy()[keep], ref_flags[keep])


@pytest.mark.gpu
def test_runs_batches_and_times_are_bitwise_the_same(hs):
    """Two runs of KS give identical cells (the minimum does not depend on the
    order of arrival); a batch equals single calls; nt = 3 equals three calls;
    likewise KIP on those cells; t = 0 and t = 1 return the frames."""
    import projection
    import torch
    shape, times = (3, 37, 131), (0.0, 0.5, 1.0)
    I0, I1 = (_cuda(a) for a in _textures(shape, "f32"))
    flows = [_cuda(a) for a in _flows(shape)]
    mf, mb = (_cuda(m) for m in _masks(shape))
    cells = projection.project_device(I0, I1, *flows, times)
    again = projection.project_device(I0, I1, *flows, times)
    assert torch.equal(cells, again)
    out, flags, trusted = projection.frame_interp_device(
        I0, I1, *flows, times, cells, mask_f=mf, mask_b=mb, flags=True, trusted=True)
    for j, t in enumerate(times):
        cj = projection.project_device(I0, I1, *flows, (t,))
        assert torch.equal(cells[:, j], cj[:, 0])
        o, f, c = projection.frame_interp_device(I0, I1, *flows, (t,), cj, mask_f=mf, mask_b=mb,
                                                 flags=True, trusted=True)
        assert _same_bits(out[:, j], o[:, 0]) and torch.equal(flags[:, j], f[:, 0])
        assert torch.equal(trusted[:, j], c[:, 0])
    for k in range(shape[0]):
        one = [a[k].contiguous() for a in (I0, I1, *flows)]
        ck = projection.project_device(*one, times)
        assert torch.equal(cells[k], ck)
        o, f, c = projection.frame_interp_device(*one, times, ck, mask_f=mf[k].contiguous(),
                                                 mask_b=mb[k].contiguous(), flags=True,
                                                 trusted=True)
        assert _same_bits(out[k], o) and torch.equal(flags[k], f)
        assert torch.equal(trusted[k], c[0])
    torch.cuda.synchronize()
    assert _same_bits(out[:, 0], I0) and _same_bits(out[:, 2], I1)


def _solve_pair(batch):
    I0, I1 = np_synth(2030, 90, 140, -6, 9)
    if batch == 1:
        return I0, I1
    J0, J1 = np_synth(2130, 90, 140, 5, -7)
    return np.stack([I0, J0]), np.stack([I1, J1])


@pytest.mark.gpu
@pytest.mark.parametrize("finest", [0, 1])
@pytest.mark.parametrize("batch", [1, 2])
def test_fused_call_equals_the_public_pieces_bitwise(hs, batch, finest):
    """flow_interp_device(projection=1) = flow_bidir_device, project_device on
    the frames, the projected interpolation; projection=0 = the call without
    it.  With a prefilter the cells come from the prefiltered planes."""
    import projection
    import torch
    I0, I1 = (_cuda(a) for a in _solve_pair(batch))
    times = (0.25, 0.5, 1.0)
    args = (3, 2, 5, 20, 100.0)
    r = hs.flow_bidir_device(I0, I1, *args, mask_f=True, mask_b=True, median=5, finest=finest)
    cells = projection.project_device(I0, I1, r.uf, r.vf, r.ub, r.vb, times)
    want, want_f, want_c = projection.frame_interp_device(
        I0, I1, r.uf, r.vf, r.ub, r.vb, times, cells, mask_f=r.mask_f, mask_b=r.mask_b,
        flags=True, trusted=True)
    out, flags, trusted = hs.flow_interp_device(I0, I1, times, *args, median=5, flags=True,
                                                trusted=True, finest=finest, projection=1)
    frames_only = hs.flow_interp_device(I0, I1, times, *args, median=5, finest=finest,
                                        projection=1)[0]
    torch.cuda.synchronize()
    assert _same_bits(out, want) and torch.equal(flags, want_f) and torch.equal(trusted, want_c)
    assert _same_bits(frames_only, want)
    assert int((flags & HOLE != 0).sum()) > 0 and int(trusted.sum()) > 0
    # projection = 0 through the new entry point: the *_lv call's bits
    plain = hs.flow_interp_device(I0, I1, times, *args, median=5, flags=True, trusted=True,
                                  finest=finest)
    L = hs.lib()
    o0 = torch.empty_like(out)
    f0, c0 = torch.empty_like(flags), torch.empty_like(trusted)
    ws = torch.empty(hs.flow_interp_workspace_bytes(90, 140, batch, 3), dtype=torch.uint8,
                     device="cuda")
    tm = _times(*times)
    rc = L.hsflow_flow_interp_pj_device(
        I0.data_ptr(), I1.data_ptr(), hs.F32, 90, 140, batch, 3, finest, 2, 5, 5, 20, 100.0,
        hs.CONSISTENCY_REL, hs.CONSISTENCY_ABS, tm, 3, 0, o0.data_ptr(), hs.F32, f0.data_ptr(),
        c0.data_ptr(), None, None, None, ws.data_ptr(), ws.numel(),
        torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert rc == 0
    assert _same_bits(o0, plain[0]) and torch.equal(f0, plain[1]) and torch.equal(c0, plain[2])
    assert int((f0 & HOLE != 0).sum()) == 0
    if batch == 1 and finest == 0:
        pf = hs.Prefilter(hs.PREFILTER_NORMALIZE, 2.0, 1.0, 32.0)
        p0, p1 = hs.prefilter_device(I0, pf), hs.prefilter_device(I1, pf)
        r = hs.flow_bidir_device(I0, I1, *args, mask_f=True, mask_b=True, prefilter=pf)
        cells = projection.project_device(p0, p1, r.uf, r.vf, r.ub, r.vb, times)
        want = projection.frame_interp_device(I0, I1, r.uf, r.vf, r.ub, r.vb, times, cells,
                                              mask_f=r.mask_f, mask_b=r.mask_b, flags=True)
        got = hs.flow_interp_device(I0, I1, times, *args, flags=True, prefilter=pf, projection=1)
        torch.cuda.synchronize()
        assert _same_bits(got[0], want[0]) and torch.equal(got[1], want[1])


@pytest.mark.gpu
def test_fused_bgr_call_equals_the_public_pieces_bitwise(hs):
    """The cells come from bgr_to_gray_device of both frames; uint8 output."""
    import projection
    import torch
    shape = (2, 37, 131)
    bgr0, bgr1 = (_cuda(a) for a in _bgr_frames(shape))
    times = (0.5, 0.75)
    args = (2, 2, 5, 10, 100.0)
    g0, g1 = hs.bgr_to_gray_device(bgr0), hs.bgr_to_gray_device(bgr1)
    r = hs.flow_bidir_device(g0, g1, *args, mask_f=True, mask_b=True)
    cells = projection.project_device(g0, g1, r.uf, r.vf, r.ub, r.vb, times)
    want = projection.frame_interp_bgr_device(bgr0, bgr1, r.uf, r.vf, r.ub, r.vb, times, cells,
                                              mask_f=r.mask_f, mask_b=r.mask_b,
                                              out_dtype=torch.uint8, flags=True, trusted=True)
    got = hs.flow_interp_bgr_device(bgr0, bgr1, times, *args, out_dtype=torch.uint8, flags=True,
                                    trusted=True, projection=1)
    plain = hs.flow_interp_bgr_device(bgr0, bgr1, times, *args, out_dtype=torch.uint8, flags=True)
    torch.cuda.synchronize()
    for a, b in zip(got, want):
        assert torch.equal(a, b)
    assert int((plain[1] & HOLE != 0).sum()) == 0 and not torch.equal(plain[0], got[0])


@pytest.mark.gpu
def test_host_calls_equal_device_calls_bitwise(hs):
    """Context.interpolate / interpolate_bgr with projection: the keyword, and
    the context's own setting, restored after a call that overrides it; a bad
    value is rejected and leaves the old one."""
    import projection
    import torch
    I0, I1 = _solve_pair(1)
    times = (0.0, 0.5, 1.0)
    args = (3, 2, 5, 20, 100.0)
    out, flags, trusted = hs.flow_interp_device(_cuda(I0), _cuda(I1), times, *args, median=5,
                                                flags=True, trusted=True, projection=1)
    plain = hs.flow_interp_device(_cuda(I0), _cuda(I1), times, *args, median=5)[0]
    bgr0, bgr1 = (a[0] for a in _bgr_frames((1, 37, 131)))
    dev_bgr = hs.flow_interp_bgr_device(_cuda(bgr0), _cuda(bgr1), (0.5,), 2, 2, 5, 10, 100.0,
                                        out_dtype=torch.uint8, projection=1)[0]
    torch.cuda.synchronize()
    with hs.Context(0) as ctx:
        assert projection.get_projection(ctx) == 0
        h, hf, hc = ctx.interpolate(I0, I1, times, *args, median=5, with_flags=True, projection=1)
        assert projection.get_projection(ctx) == 0
        assert np.array_equal(h, out.cpu().numpy()) and np.array_equal(hf, flags.cpu().numpy())
        assert np.array_equal(hc.astype(np.int64), trusted.cpu().numpy()[0].astype(np.int64))
        assert np.array_equal(h[0], I0) and np.array_equal(h[2], I1)
        assert np.array_equal(ctx.interpolate(I0, I1, times, *args, median=5), plain.cpu().numpy())
        projection.set_projection(ctx, 1)
        assert projection.get_projection(ctx) == 1
        assert np.array_equal(ctx.interpolate(I0, I1, times, *args, median=5), h)
        assert np.array_equal(ctx.interpolate(I0, I1, times, *args, median=5, projection=0),
                              plain.cpu().numpy())
        assert projection.get_projection(ctx) == 1
        hb = ctx.interpolate_bgr(bgr0, bgr1, (0.5,), 2, 2, 5, 10, 100.0)
        assert np.array_equal(hb, dev_bgr.cpu().numpy())
        with pytest.raises(hs.HsflowError, match="projection"):
            projection.set_projection(ctx, 2)
        assert projection.get_projection(ctx) == 1
        with projection.projection_as(ctx, 0):
            assert projection.get_projection(ctx) == 0
        assert projection.get_projection(ctx) == 1


@pytest.mark.gpu
def test_graph_capture_replays_the_eager_result(hs):
    """One capture and replay of flow_interp_device(projection=1) on the origin
    stream, an eager call on a side stream first: the memset of the cells, KS
    and KIP are stream-ordered and allocate nothing."""
    import projection
    import torch
    rows, cols, levels = 64, 96, 2
    I0, I1 = np_synth(2080, rows, cols, -6, 9)
    t0, t1 = _cuda(I0), _cuda(I1)
    times = (0.25, 0.5, 0.75)
    out = torch.empty((len(times), rows, cols), dtype=torch.float32, device="cuda")
    flags = torch.empty(out.shape, dtype=torch.uint8, device="cuda")
    trusted = torch.empty((1, len(times)), dtype=torch.int32, device="cuda")
    ws = torch.empty(projection.flow_interp_workspace_bytes(rows, cols, 1, levels, len(times)),
                     dtype=torch.uint8, device="cuda")

    def solve(s):
        hs.flow_interp_device(t0, t1, times, levels, 2, 5, 20, 100.0, median=5, out=out,
                              flags=flags, trusted=trusted, workspace=ws, stream=s, projection=1)

    stream = torch.cuda.current_stream()
    cap = torch.cuda.Stream()
    cap.wait_stream(stream)
    with torch.cuda.stream(cap):
        solve(cap)
    stream.wait_stream(cap)
    torch.cuda.synchronize()
    ref = [t.clone() for t in (out, flags, trusted)]
    assert int(trusted.sum()) > 0
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, capture_error_mode="thread_local"):
        solve(torch.cuda.current_stream())
    torch.cuda.synchronize()
    for t in (out, flags, trusted):
        t.fill_(1)
    ws.fill_(0)  # stale cells of all zeros would win every minimum
    graph.replay()
    torch.cuda.synchronize()
    for t, want in zip((out, flags, trusted), ref):
        assert _same_bits(t, want)


@pytest.mark.gpu
@pytest.mark.parametrize("plane", range(4), ids=["uf", "vf", "ub", "vb"])
def test_hostile_flows_stay_inside_the_pair(hs, plane):
    """NaN, +-inf and +-1e30 at scattered pixels (corners included) of one flow
    plane; cells and outputs between guard planes at element-aligned, otherwise
    odd bases: the calls complete, the guards keep their bytes, every non-empty
    cell names a source pixel of the plane, and KIP on those cells counts its
    own flags."""
    import projection
    import torch
    shape = (2, 37, 131)
    times = (0.0, 0.5, 1.0)
    flows = [np.array(a) for a in _flows(shape)]
    rng = np.random.default_rng(291 + plane)
    _, rows, cols = shape
    spots = [(0, 0), (0, cols - 1), (rows - 1, 0), (rows - 1, cols - 1)]
    spots += [(int(rng.integers(rows)), int(rng.integers(cols))) for _ in range(26)]
    for b in range(shape[0]):
        for k, (y, x) in enumerate(spots):
            flows[plane][b, y, x] = HOSTILE[(k + b) % len(HOSTILE)]
    I0, I1 = _textures(shape, "f32")
    oshape = (shape[0], len(times), rows, cols)
    ins = [_placed(a, 1 + k % 3, torch.float32, 0.0)[1] for k, a in enumerate((I0, I1, *flows))]
    # a guard plane and one or two elements in front: 8 bytes past 16-byte alignment
    fc, cells, (c0, c1) = _placed(None, 1 + rows * cols % 2, torch.int64, GUARD_C, oshape)
    assert cells.data_ptr() % 16 == 8
    projection.project_device(*ins, times, cells=cells)  # raises unless the call returns 0
    torch.cuda.synchronize()
    assert _guards_intact(fc, c0, c1, GUARD_C)
    got = _u64(cells)
    assert _decodable(got, rows * cols) and (got != EMPTY).mean() > 0.9
    fo, o, (o0, o1) = _placed(None, 3, torch.float32, GUARD_F, oshape)
    ff, f, (f0, f1) = _placed(None, 1, torch.uint8, GUARD_B, oshape)
    c = torch.full((shape[0] + 2, len(times)), -12345, dtype=torch.int32, device="cuda")
    projection.frame_interp_device(*ins, times, cells, out=o, flags=f, trusted=c[1:-1])
    torch.cuda.synchronize()
    assert _guards_intact(fo, o0, o1, GUARD_F) and _guards_intact(ff, f0, f1, GUARD_B)
    assert _guards_intact(fc, c0, c1, GUARD_C)
    assert bool((c[0] == -12345).all()) and bool((c[-1] == -12345).all())
    fl = f.cpu().numpy()
    assert np.array_equal(fl & HOLE != 0, got == EMPTY)
    assert np.array_equal(c[1:-1].cpu().numpy().astype(np.int64), (fl == 0).sum(axis=(2, 3)))
    # a foreign cell plane (every source index past the plane) stays inside too
    junk = torch.full(oshape, 0x7FFFFFFF, dtype=torch.int64, device="cuda")
    projection.frame_interp_device(*ins, times, junk, out=o, flags=f, trusted=c[1:-1])
    torch.cuda.synchronize()
    assert _guards_intact(fo, o0, o1, GUARD_F) and _guards_intact(ff, f0, f1, GUARD_B)


@pytest.mark.gpu
def test_end_to_end_on_the_moving_square(hs):
    """The CPU test's two ratio conditions for the GPU's projected frame against
    the GPU's own unprojected one, next to the reference's figures."""
    import torch
    I0, I1 = _pair_frames(OCCLUDER)
    sm = hs.Smoothness(hs.SMOOTH_FLOW_DRIVEN, LAM)
    t0, t1 = _cuda(I0), _cuda(I1)
    plain = hs.flow_interp_device(t0, t1, (0.5,), *WARPS4, 100.0, median=5, smoothness=sm)[0]
    proj, flags, _ = hs.flow_interp_device(t0, t1, (0.5,), *WARPS4, 100.0, median=5,
                                           smoothness=sm, flags=True, projection=1)
    torch.cuda.synchronize()
    ref, ref_flags = projected_np(I0, I1, *_square_flows(), 0.5)
    _assert_square_gain(_middle_ref(LAM), ref, int((ref_flags & HOLE != 0).sum()), "reference")
    holes = int((flags[0].cpu().numpy() & HOLE != 0).sum())
    _assert_square_gain(plain[0].cpu().numpy(), proj[0].cpu().numpy(), holes, "GPU")
