"""Flow-driven (edge-preserving) smoothness of the warped solves
(hsflow_flow_diffusivity_device, hsflow_jacobi_weighted_device,
hsflow_flow_*_sm_device, hsflow_ctx_set_smoothness, the smoothness= arguments
of the bindings).

The quadratic smoothness term replaces (u, v) by its plain window mean, which
averages across a motion boundary: the flow crosses a moving object's edge as
a ramp about ten pixels wide.  The flow-driven term weights each tap by a
diffusivity of the flow the warp linearises around (lagged diffusivity).  Per
level and per warp, U = 8 u, V = 8 v in px:

    Ux = 0.5 (U[y][min(x+1, cols-1)] - U[y][max(x-1, 0)]),  Uy, Vx, Vy likewise
    s  = Ux^2 + Uy^2 + Vx^2 + Vy^2
    g  = 1 / sqrt(1 + s / lambda^2)                              in (0, 1]

and the getFlow loop with the two means replaced; S = the w x w window sum over
the taps inside the plane, m = the number of taps outside (u = 0, weight 1):

    ubar = S(g u) / (S(g) + m);   vbar = S(g v) / (S(g) + m)
    c = (Ix ubar + Iy vbar + It') / (alpha^2 + Ix^2 + Iy^2)
    u = ubar - Ix c;   v = vbar - Iy c

diffusivity_np, jacobi_weighted_np and warped_smooth_np below are that
definition in float64 (the window sums run over a plane padded with g = 1,
u = 0).  The kernels are held to them within the module's tolerance, the fused
solves to their public pieces bit for bit, the host calls to the device calls
bit for bit, and the whole to warped_smooth_np.
"""
import ctypes
import functools
import os
import shutil
import subprocess

import numpy as np
import pytest

import oracle
from conftest import ROOT, norm_rel_err
from test_consistency import _smooth_flows
from test_interp import (ABS, REL, _guards_intact, _placed, _same_bits, _truth, frame_interp_np)
from test_median import (KM_SHAPES, OCCLUDER, SHIFT_BOUNDS, SOLVE, _cuda, _occluder, median_np,
                         shift_epe, square_epe, warped_median_np)
from test_warped import PAIR_A, PAIR_B, _inputs, _pair, warp_gradients_np

TOL = 1e-4  # the module's flow tolerance, max|d| / max|ref|
GAIN = 8.0
ALPHA, MEDIAN = 100.0, 5
LAM = 0.3  # the recommended setting (include/hsflow.h)
FLOW_DRIVEN = 1
WARPS4 = (SOLVE[0], 4, SOLVE[2], SOLVE[3])  # SOLVE with 4 warps
# the band around the moving square's border in the middle frame
BAND_OUTER = (slice(36, 92), slice(42, 104))
BAND_INNER = (slice(52, 76), slice(61, 85))
SHAPE_IDS = dict(ids=lambda s: "x".join(map(str, s)))
GUARD = -7.25


# ------------------------------------------------------------ f64 reference
def diffusivity_np(u, v, lam):
    """g of one 2-D plane pair in solver units (float64); lam as the f32 it
    travels as."""
    lam = float(np.float32(lam))
    s = 0.0
    for a in (u, v):
        p = np.pad(GAIN * np.asarray(a, np.float64), 1, mode="edge")
        ax = 0.5 * (p[1:-1, 2:] - p[1:-1, :-2])
        ay = 0.5 * (p[2:, 1:-1] - p[:-2, 1:-1])
        s = s + ax * ax + ay * ay
    return 1.0 / np.sqrt(1.0 + s / (lam * lam))


def _window_sum(a, w, fill):
    """w x w window sum (centred anchor) of a plane padded with `fill`."""
    h = w // 2
    p = np.pad(np.asarray(a, np.float64), h, mode="constant", constant_values=fill)
    rows, cols = a.shape
    return sum(p[j:j + rows, i:i + cols] for j in range(w) for i in range(w))


def jacobi_weighted_np(gx, gy, gt, g, u, v, w, n, alpha):
    """n weighted iterations from (u, v), float64."""
    gx, gy, gt, g = (np.asarray(a, np.float64) for a in (gx, gy, gt, g))
    u, v = np.asarray(u, np.float64).copy(), np.asarray(v, np.float64).copy()
    den = _window_sum(g, w, 1.0)  # S(g) + m
    D = float(alpha) ** 2 + gx * gx + gy * gy
    for _ in range(n):
        ub = _window_sum(g * u, w, 0.0) / den
        vb = _window_sum(g * v, w, 0.0) / den
        c = (gx * ub + gy * vb + gt) / D
        u, v = ub - gx * c, vb - gy * c
    return u, v


def warped_smooth_np(I0, I1, levels, warps, w, n, alpha, k, lam, ones=False):
    """warped_median_np's loop with the two new steps: g from the warp's
    (u, v), then the weighted iterations.  ones=True sets g = 1 (the plain
    iteration, through this module's window sums)."""
    a, b = np.asarray(I0, np.float64), np.asarray(I1, np.float64)
    rnd = oracle.integer_pair(a, b)
    P = [(a, b)]
    for _ in range(1, levels):
        P.append((oracle.pyrdown(P[-1][0], rnd), oracle.pyrdown(P[-1][1], rnd)))
    u = v = None
    for lv in range(levels - 1, -1, -1):
        p0, p1 = P[lv]
        if u is None:
            u, v = np.zeros_like(p0), np.zeros_like(p0)
        else:
            u = 2.0 * np.repeat(np.repeat(u, 2, 0), 2, 1)[:p0.shape[0], :p0.shape[1]]
            v = 2.0 * np.repeat(np.repeat(v, 2, 0), 2, 1)[:p0.shape[0], :p0.shape[1]]
        for _ in range(warps):
            gx, gy, gt = warp_gradients_np(p0, p1, u, v)
            g = np.ones_like(u) if ones else diffusivity_np(u, v, lam)
            u, v = jacobi_weighted_np(gx, gy, gt, g, u, v, w, n, alpha)
            if k:
                u, v = median_np(u, k), median_np(v, k)
    return u, v


# ------------------------------------------------------------ shared inputs
def _frames(pair, kind="f32"):
    if pair[0] == "occluder":
        return _occluder(pair[1])
    return _inputs(pair, kind)


@functools.lru_cache(maxsize=None)
def _ref(pair, solve, lam, kind="f32", backward=False):
    """The float64 solve of a case at alpha 100 with the 5 x 5 median, computed
    once and shared: lam = None is the plain reference (warped_median_np)."""
    I0, I1 = _frames(pair, kind)
    if backward:
        I0, I1 = I1, I0
    if lam is None:
        u, v = warped_median_np(I0, I1, *solve, ALPHA, MEDIAN)
    else:
        u, v = warped_smooth_np(I0, I1, *solve, ALPHA, MEDIAN, lam)
    u.setflags(write=False)
    v.setflags(write=False)
    return u, v


def visible_epe(u, v, d):
    """Mean end-point error (px) of the moving square's pair over the pixels
    visible in both frames: everything but the strip of background that the
    square covers in the second frame."""
    tu = np.zeros((128, 160))
    tu[44:84, 50:90] = d
    e = np.hypot(GAIN * np.asarray(u, np.float64) - tu, GAIN * np.asarray(v, np.float64))
    seen = np.ones(e.shape, bool)
    seen[44:84, 90:90 + d] = False
    return float(e[seen].mean())


def band_error(frame):
    """Mean error (grey levels) of a middle frame of the moving square over
    the band around the square's border, and over the whole frame."""
    e = np.abs(np.asarray(frame, np.float64) - _truth(OCCLUDER, 0.5))
    band = np.zeros(e.shape, bool)
    band[BAND_OUTER] = True
    band[BAND_INNER] = False
    return float(e[band].mean()), float(e.mean())


def _middle_ref(lam):
    I0, I1 = _occluder(OCCLUDER[1])
    uf, vf = _ref(OCCLUDER, WARPS4, lam)
    ub, vb = _ref(OCCLUDER, WARPS4, lam, backward=True)
    return frame_interp_np(I0, I1, uf, vf, ub, vb, 0.5)[0]


def _assert_square_quality(plain, smooth, mid_plain, mid_smooth, who):
    """The issue's three conditions on the moving square (4 warps, lam 0.3)."""
    d = OCCLUDER[1]
    sp, ss = square_epe(*plain, d), square_epe(*smooth, d)
    vp, vs = visible_epe(*plain, d), visible_epe(*smooth, d)
    (bp, wp), (bs, ws) = band_error(mid_plain), band_error(mid_smooth)
    print(f"{who} moving square, 4 warps: inner-square EPE plain {sp:.3f}, lam {LAM} {ss:.3f} px "
          f"({ss / sp:.2f}); visible-pixel EPE {vp:.3f} -> {vs:.3f} px; middle frame band "
          f"{bp:.2f} -> {bs:.2f} ({bs / bp:.2f}), whole frame {wp:.3f} -> {ws:.3f} grey levels")
    assert ss <= 0.5 * sp
    assert vs < vp
    assert bs <= 0.9 * bp


# ------------------------------------------------------------------ CPU tests
@pytest.mark.parametrize("pair,solve", [(PAIR_B, (3, 2, 5, 20)), (OCCLUDER, (2, 2, 3, 15))],
                         ids=["97x131-w5", "square-w3"])
def test_reference_with_unit_weights_is_the_plain_reference(pair, solve):
    I0, I1 = _frames(pair)
    u, v = warped_smooth_np(I0, I1, *solve, ALPHA, MEDIAN, LAM, ones=True)
    ur, vr = warped_median_np(I0, I1, *solve, ALPHA, MEDIAN)
    eu, ev = norm_rel_err(u, ur), norm_rel_err(v, vr)
    print(f"{pair} {solve} g = 1 against warped_median_np: {eu:.2e} {ev:.2e}")
    assert eu <= 1e-10 and ev <= 1e-10


def test_reference_diffusivity_of_a_step_and_a_ramp():
    z = np.zeros((6, 9))
    assert np.array_equal(diffusivity_np(z, z, 0.3), np.ones_like(z))
    ramp = np.tile(np.arange(9.0) / GAIN * 0.3, (6, 1))  # 0.3 px per px along x
    g = diffusivity_np(ramp, z, 0.3)
    assert np.allclose(g[:, 1:-1], 1.0 / np.sqrt(2.0), atol=1e-6)  # lam's definition (lam as f32)
    assert np.allclose(g[:, 0], 1.0 / np.sqrt(1.25), atol=1e-6)    # the border halves the slope
    step = np.where(np.arange(9) >= 5, 6.0 / GAIN, 0.0) * np.ones((6, 1))
    g = diffusivity_np(z, step, 0.3)
    assert np.all(g[:, [4, 5]] < 0.1) and np.all(g[:, :4] == 1.0) and np.all(g[:, 6:] == 1.0)


def test_reference_sharpens_the_moving_square():
    plain = _ref(OCCLUDER, WARPS4, None)
    smooth = _ref(OCCLUDER, WARPS4, LAM)
    _assert_square_quality(plain, smooth, _middle_ref(None), _middle_ref(LAM), "reference")
    row = GAIN * smooth[0][64, 44:56]
    print("reference 8 uf along row 64, cols 44:56: " + " ".join(f"{x:.1f}" for x in row))


@pytest.mark.parametrize("pair", [PAIR_A, PAIR_B])
def test_reference_keeps_a_pure_shift(pair):
    mean, worst = shift_epe(*_ref(pair, SOLVE, LAM), pair)
    pm, pw = shift_epe(*_ref(pair, SOLVE, None), pair)
    print(f"reference {pair} alpha 100, 5x5, 2 warps: interior EPE mean/max plain {pm:.4f}/"
          f"{pw:.4f}, lam {LAM} {mean:.4f}/{worst:.4f} px")
    assert mean <= SHIFT_BOUNDS[pair][0] and worst <= SHIFT_BOUNDS[pair][1]


def _csm(mode=FLOW_DRIVEN, lam=LAM):
    import hsflow
    return hsflow._CSmoothness(mode, lam)


def test_argument_errors_without_a_gpu():
    import hsflow
    L = hsflow.lib()
    E = hsflow.HSFLOW_ERR_ARG
    nan, inf = float("nan"), float("inf")
    # never dereferenced: every call fails its checks first.  16 x 16 f32 planes
    # are 1024 bytes; the addresses below are 4096 apart, the workspace far off
    A = [4096 * k for k in range(1, 16)]
    ws, big = 1 << 20, 1 << 30

    def err():
        return L.hsflow_last_error(None).decode()

    def kg(u=A[0], v=A[1], lam=LAM, g=A[2], rows=16):
        return L.hsflow_flow_diffusivity_device(u, v, rows, 16, 1, lam, g, None)

    for lam in (0.0, -0.3, nan, inf, -inf):
        assert kg(lam=lam) == E and "lambda" in err()
    for null in ("u", "v", "g"):
        assert kg(**{null: None}) == E
    assert kg(rows=0) == E
    for over in (dict(g=A[0]), dict(g=A[1]), dict(g=A[0] + 1020), dict(g=A[1] - 1020)):
        assert kg(**over) == E and "overlap" in err()

    need = hsflow.workspace_bytes(16, 16, 1)

    def kj(window=5, iters=3, g=A[0], u=A[1], v=A[2], w=ws, wsb=big, rows=16):
        return L.hsflow_jacobi_weighted_device(rows, 16, 1, window, iters, 1.0, g, u, v, w, wsb,
                                               None)

    for window in (1, 2, 4, 7, 9, 0, -5):
        assert kj(window=window) == E and "windowSize" in err()
    assert kj(iters=-1) == E
    assert kj(rows=0) == E
    for null in ("g", "u", "v", "w"):
        assert kj(**{null: None}) == E
    assert kj(wsb=need - 1) == E and "workspace" in err()
    for over in (dict(g=A[1]), dict(g=A[2] + 4), dict(v=A[1] + 1020), dict(u=ws + need - 4),
                 dict(g=ws), dict(v=ws - 1020)):
        assert kj(**over) == E and "overlap" in err()

    half = (ctypes.c_float * 1)(0.5)

    def warped(sm=_csm(), window=5, wsb=big, warps=1):
        return L.hsflow_flow_warped_sm_device(A[0], A[1], hsflow.F32, 16, 16, 1, 3, warps, 5,
                                              window, 10, 1.0, A[2], A[3], None, sm, ws, wsb, None)

    def bidir(sm=_csm(), window=5, wsb=big):
        return L.hsflow_flow_bidir_sm_device(A[0], A[1], hsflow.F32, 16, 16, 1, 3, 1, 5, window, 10,
                                             1.0, REL, ABS, A[2], A[3], A[4], A[5], None, A[6],
                                             None, None, None, None, None, sm, ws, wsb, None)

    def interp(sm=_csm(), window=5, wsb=big):
        return L.hsflow_flow_interp_sm_device(A[0], A[1], hsflow.F32, 16, 16, 1, 3, 1, 5, window,
                                              10, 1.0, REL, ABS, half, 1, A[2], hsflow.F32, None,
                                              None, None, sm, ws, wsb, None)

    def interp_bgr(sm=_csm(), window=5, wsb=big):
        return L.hsflow_flow_interp_bgr_sm_device(A[0], A[1], 16, 16, 1, 3, 1, 5, window, 10, 1.0,
                                                  REL, ABS, half, 1, A[2], hsflow.F32, None, None,
                                                  None, sm, ws, wsb, None)

    own = {warped: hsflow.pyramid_workspace_bytes(16, 16, 1, 3),
           bidir: hsflow.bidir_workspace_bytes(16, 16, 1, 3),
           interp: hsflow.flow_interp_workspace_bytes(16, 16, 1, 3),
           interp_bgr: hsflow.flow_interp_bgr_workspace_bytes(16, 16, 1, 3)}
    for call, size in own.items():
        for lam in (0.0, -1.0, nan, inf):
            assert call(sm=_csm(lam=lam)) == E and "lambda" in err(), call.__name__
        for mode in (-1, 2, 7):
            assert call(sm=_csm(mode=mode)) == E and "mode" in err(), call.__name__
        for window in (4, 7):
            assert call(window=window) == E and "windowSize" in err(), call.__name__
            # off: the window is the plain solve's business (the next check fails)
            for off in (None, _csm(mode=0, lam=nan)):
                assert call(sm=off, window=window, wsb=size - 1) == E and "workspace" in err()
        # the mode needs no workspace beyond the call's own
        assert call(wsb=size - 1) == E and "workspace" in err(), call.__name__
    assert warped(warps=0) == E and "warps" in err()

    # the context's setting: a null context, and a null struct to read into
    assert L.hsflow_ctx_set_smoothness(None, _csm()) == E and "context" in err()
    assert L.hsflow_ctx_smoothness(None, _csm()) == E
    z = np.zeros((8, 8), np.float32)
    with pytest.raises(hsflow.HsflowError) as info:
        hsflow.compute(z, z, 100.0, 1, levels=2, warps=0, smoothness=hsflow.Smoothness())
    assert info.value.status == E


def test_python_surface():
    import hsflow
    import inspect
    import frames
    for name in ("hsflow_flow_diffusivity_device", "hsflow_jacobi_weighted_device",
                 "hsflow_flow_warped_sm_device", "hsflow_flow_bidir_sm_device",
                 "hsflow_flow_interp_sm_device", "hsflow_flow_interp_bgr_sm_device",
                 "hsflow_ctx_set_smoothness", "hsflow_ctx_smoothness"):
        assert name in hsflow.EXPORTS and hasattr(hsflow.lib(), name)
    assert (hsflow.SMOOTH_QUADRATIC, hsflow.SMOOTH_FLOW_DRIVEN) == (0, FLOW_DRIVEN)
    assert hsflow.Smoothness(FLOW_DRIVEN, 0.25) == (FLOW_DRIVEN, 0.25)
    assert hsflow.Smoothness._fields == ("mode", "lam")
    assert callable(hsflow.diffusivity_device) and callable(hsflow.jacobi_weighted_device)
    assert callable(hsflow.Context.set_smoothness) and callable(hsflow.Context.smoothness)
    for f in (hsflow.flow_warped_device, hsflow.flow_bidir_device, hsflow.flow_interp_device,
              hsflow.flow_interp_bgr_device, hsflow.Context.flow_warped, hsflow.Context.flow_bidir,
              hsflow.Context.interpolate, hsflow.Context.interpolate_bgr, hsflow.compute,
              frames.interpolate_sequence):
        assert inspect.signature(f).parameters["smoothness"].default is None
    assert "smoothness" not in inspect.signature(hsflow.Context.flow).parameters
    assert "smoothness" not in inspect.signature(hsflow.Context.flow_pyramid).parameters


def test_setsmoothness_compiles_and_links(tmp_path):
    """A C++ caller of setSmoothness builds against include/hsflow.hpp and
    libhsflow.so; without a device the calls throw hsflow::Error (never a
    crash), and the C entry points' argument errors need no device."""
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("no C++ compiler")
    src = tmp_path / "smoothness_main.cpp"
    src.write_text(r'''
#include <cstdint>
#include <cstdio>
#include <vector>
#include "hsflow.hpp"
#if !defined(HSFLOW_HAS_SMOOTHNESS) || HSFLOW_HAS_SMOOTHNESS != 1
#error "hsflow.h lacks the flow-driven smoothness"
#endif
int main() {
    const int rows = 24, cols = 40;
    std::vector<float> a(rows * cols, 1.f), b(rows * cols, 2.f), g(rows * cols);
    std::vector<double> u, v;
    hsflow::HornSchunck hs(5, 10, 100.0);
    const auto A = hsflow::view(a.data(), rows, cols), B = hsflow::view(b.data(), rows, cols);
    const hsflow_smoothness sm{HSFLOW_SMOOTH_FLOW_DRIVEN, 0.3f};
    int thrown = 0;
    try { hs.setSmoothness(&sm); } catch (const hsflow::Error &) { ++thrown; }
    try { hs.getFlowWarped(A, B, 3, 2, u, v, 5); } catch (const hsflow::Error &) { ++thrown; }
    try { hs.setSmoothness(nullptr); } catch (const hsflow::Error &) { ++thrown; }
    const int rc0 = hsflow_flow_diffusivity_device(a.data(), b.data(), rows, cols, 1, 0.0f,
                                                   g.data(), nullptr);
    const int rc1 = hsflow_ctx_set_smoothness(nullptr, &sm);
    const int rc2 = hsflow_jacobi_weighted_device(rows, cols, 1, 4, 1, 1.0f, g.data(), a.data(),
                                                  b.data(), g.data(), 1, nullptr);
    std::printf("%d %d %d %d %d\n", thrown, rc0, rc1, rc2, HSFLOW_SMOOTH_QUADRATIC);
    return 0;
}
''')
    lib_dir = os.path.join(ROOT, "cpp-optical-flow_amd")
    exe = str(tmp_path / "smoothness_main")
    subprocess.check_call([gxx, "-std=c++17", "-Wall", "-Werror", "-I",
                           os.path.join(ROOT, "include"), str(src), "-o", exe, "-L", lib_dir,
                           "-lhsflow", "-Wl,-rpath," + lib_dir])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    thrown, rc0, rc1, rc2, quad = (int(x) for x in out.stdout.split())
    assert thrown in (0, 3)  # 3 where no gfx950 device is present
    assert (rc0, rc1, rc2, quad) == (-1, -1, -1, 0)


# ------------------------------------------------------------------ GPU tests
def _sm(hs, lam=LAM):
    return hs.Smoothness(FLOW_DRIVEN, lam)


@pytest.mark.gpu
def test_context_setting_round_trips(hs):
    ctx = hs.Context(0)
    assert ctx.smoothness() is None
    ctx.set_smoothness(_sm(hs, 0.125))
    assert ctx.smoothness() == (FLOW_DRIVEN, 0.125)
    for bad in (hs.Smoothness(FLOW_DRIVEN, 0.0), hs.Smoothness(FLOW_DRIVEN, float("nan")),
                hs.Smoothness(3, 0.3)):
        with pytest.raises(hs.HsflowError):
            ctx.set_smoothness(bad)
        assert ctx.smoothness() == (FLOW_DRIVEN, 0.125)  # a bad setting changes nothing
    ctx.set_smoothness(None)
    assert ctx.smoothness() is None
    ctx.set_smoothness(_sm(hs))
    ctx.set_smoothness(hs.Smoothness(0, 0.0))
    assert ctx.smoothness() is None
    ctx.close()


@functools.lru_cache(maxsize=None)
def _kg_flows(shape):
    """test_consistency's smooth flows plus a step edge of 6 px in u down the
    middle column and of -3 px in v across the middle row."""
    uf, vf = (a.copy() for a in _smooth_flows(*shape)[:2])
    uf[:, :, shape[2] // 2:] += np.float32(6.0 / GAIN)
    vf[:, shape[1] // 2:, :] -= np.float32(3.0 / GAIN)
    uf.setflags(write=False)
    vf.setflags(write=False)
    return uf, vf


@pytest.mark.gpu
@pytest.mark.parametrize("shape", KM_SHAPES, **SHAPE_IDS)
def test_diffusivity_kernel_against_reference(hs, shape):
    """max|g - ref| <= 1e-5: g <= 1 and each value takes a handful of f32
    roundings (four differences, the fused sum of squares, one rsq)."""
    import torch
    u, v = _kg_flows(shape)
    for lam in (0.1, 1.0):
        g = hs.diffusivity_device(_cuda(u), _cuda(v), lam)
        torch.cuda.synchronize()
        got = g.cpu().numpy().astype(np.float64)
        ref = np.stack([diffusivity_np(u[k], v[k], lam) for k in range(shape[0])])
        worst = float(np.abs(got - ref).max())
        print(f"{shape} lam {lam}: worst |g - ref| {worst:.3e}, g in [{got.min():.3e}, "
              f"{got.max():.3e}]")
        assert tuple(g.shape) == shape and g.dtype == torch.float32
        assert worst <= 1e-5
        assert got.min() > 0.0 and got.max() <= 1.0


@functools.lru_cache(maxsize=None)
def _kj_inputs(shape):
    """Frames, a linearisation point, flows and weights in (0, 1] for KJ."""
    batch, rows, cols = shape
    rng = np.random.default_rng(900 + 1000 * batch + 10 * rows + cols)
    I0 = rng.uniform(0.0, 255.0, shape).astype(np.float32)
    I1 = rng.uniform(0.0, 255.0, shape).astype(np.float32)
    u0, v0 = (rng.normal(scale=0.2, size=shape).astype(np.float32) for _ in range(2))
    u, v = (rng.normal(scale=0.5, size=shape).astype(np.float32) for _ in range(2))
    g = (1.0 - rng.uniform(0.0, 1.0, shape) ** 3 * 0.999).astype(np.float32)
    out = (I0, I1, u0, v0, u, v, g)
    for a in out:
        a.setflags(write=False)
    return out


def _kj_setup(hs, shape):
    """The workspace after warp_gradients_device, and the planes it holds."""
    import torch
    I0, I1, u0, v0 = (_cuda(a) for a in _kj_inputs(shape)[:4])
    ws = hs.alloc_workspace(shape[1], shape[2], shape[0])
    gx, gy, gt = (torch.empty(shape, dtype=torch.float32, device="cuda") for _ in range(3))
    hs.warp_gradients_device(I0, I1, u0, v0, ws, gx, gy, gt)
    torch.cuda.synchronize()
    return ws, tuple(t.cpu().numpy() for t in (gx, gy, gt))


def _kj_run(hs, shape, ws, w, iters, g, u, v, alpha=ALPHA):
    import torch
    tu, tv = _cuda(u), _cuda(v)
    for n in iters:
        hs.jacobi_weighted_device(shape[1], shape[2], shape[0], w, n, alpha, g, tu, tv, ws)
    torch.cuda.synchronize()
    return tu, tv


@pytest.mark.gpu
@pytest.mark.parametrize("shape", KM_SHAPES, **SHAPE_IDS)
@pytest.mark.parametrize("w", [3, 5])
def test_weighted_kernel_against_reference(hs, shape, w):
    """1, 7 and 13 iterations (a launch shorter than the depth, whole launches
    and a remainder) against jacobi_weighted_np on the planes the workspace
    holds; with g = 1 the kernel equals jacobi_device on the same planes within
    the tolerance, which is the border rule m."""
    import torch
    _, _, _, _, u, v, g = _kj_inputs(shape)
    ws, (gx, gy, gt) = _kj_setup(hs, shape)
    tg = _cuda(g)
    for n in (1, 7, 13):
        tu, tv = _kj_run(hs, shape, ws, w, (n,), tg, u, v)
        ref = [jacobi_weighted_np(gx[k], gy[k], gt[k], g[k], u[k], v[k], w, n, ALPHA)
               for k in range(shape[0])]
        eu = norm_rel_err(tu.cpu().numpy(), np.stack([r[0] for r in ref]))
        ev = norm_rel_err(tv.cpu().numpy(), np.stack([r[1] for r in ref]))
        print(f"{shape} w {w} n {n}: {eu:.2e} {ev:.2e}")
        assert eu <= TOL and ev <= TOL
    ones = torch.ones(shape, dtype=torch.float32, device="cuda")
    tu, tv = _kj_run(hs, shape, ws, w, (7,), ones, u, v)
    pu, pv = _cuda(u), _cuda(v)
    hs.jacobi_device(shape[1], shape[2], shape[0], w, 7, ALPHA, pu, pv, ws, warm_start=True)
    torch.cuda.synchronize()
    eu = norm_rel_err(tu.cpu().numpy(), pu.cpu().numpy().astype(np.float64))
    ev = norm_rel_err(tv.cpu().numpy(), pv.cpu().numpy().astype(np.float64))
    print(f"{shape} w {w} g = 1 against jacobi_device: {eu:.2e} {ev:.2e}")
    assert eu <= TOL and ev <= TOL


@pytest.mark.gpu
@pytest.mark.parametrize("w", [3, 5])
def test_weighted_kernel_is_bitwise_reproducible(hs, w):
    """13 iterations in one call equal 13 calls of 1 and 6 + 7, whatever depth
    a launch fuses; a batch equals its single calls; a second run the first;
    planes at unaligned offsets between guard planes leave the guards intact."""
    import torch
    for shape in ((3, 37, 131), (2, 4, 256), (1, 67, 64)):
        _, _, _, _, u, v, g = _kj_inputs(shape)
        ws, _ = _kj_setup(hs, shape)
        tg = _cuda(g)
        want = _kj_run(hs, shape, ws, w, (13,), tg, u, v)
        for split in ((1,) * 13, (6, 7), (13,)):
            got = _kj_run(hs, shape, ws, w, split, tg, u, v)
            assert _same_bits(got[0], want[0]) and _same_bits(got[1], want[1]), split
        try:
            for depth in (2, 3, 4, 6):  # those the kernel is not built for keep the default
                hs.set_iters_per_launch(depth)
                got = _kj_run(hs, shape, ws, w, (13,), tg, u, v)
                assert _same_bits(got[0], want[0]) and _same_bits(got[1], want[1]), depth
        finally:
            hs.set_iters_per_launch(0)
        for n in (1, 2):
            with hs.max_streams_as(n):
                got = _kj_run(hs, shape, ws, w, (13,), tg, u, v)
            assert _same_bits(got[0], want[0]) and _same_bits(got[1], want[1]), n
        for k in range(shape[0]):
            one = (1,) + shape[1:]
            I0, I1, u0, v0 = (_cuda(a[k:k + 1]) for a in _kj_inputs(shape)[:4])
            ws1 = hs.alloc_workspace(shape[1], shape[2], 1)
            hs.warp_gradients_device(I0, I1, u0, v0, ws1)
            got = _kj_run(hs, one, ws1, w, (13,), _cuda(g[k:k + 1]), u[k:k + 1], v[k:k + 1])
            assert _same_bits(got[0][0], want[0][k]) and _same_bits(got[1][0], want[1][k])
        for off in (1, 2, 3):
            _, pg, _ = _placed(g, off, torch.float32, 7777.0)
            fu, pu, (a0, a1) = _placed(u, (off + 1) % 4, torch.float32, GUARD)
            fv, pv, (b0, b1) = _placed(v, (off + 2) % 4, torch.float32, GUARD)
            hs.jacobi_weighted_device(shape[1], shape[2], shape[0], w, 13, ALPHA, pg, pu, pv, ws)
            torch.cuda.synchronize()
            assert _same_bits(pu, want[0]) and _same_bits(pv, want[1])
            assert _guards_intact(fu, a0, a1, GUARD) and _guards_intact(fv, b0, b1, GUARD)
    with pytest.raises(hs.HsflowError):
        hs.jacobi_weighted_device(shape[1], shape[2], shape[0], w, 1, ALPHA, want[0], want[0],
                                  want[1], ws)  # g is u: rejected, not run


def _small_pair(batch=1):
    frames = [_pair(2004 + 7 * k, 97, 131, 10, -18) for k in range(batch)]
    I0, I1 = (np.stack([f[j] for f in frames]) for j in range(2))
    return (I0, I1) if batch > 1 else (I0[0], I1[0])


def _bgr_pair(I0, I1):
    import torch
    B0 = torch.stack([I0.to(torch.uint8), (I0 * 0.5).to(torch.uint8), I1.to(torch.uint8)], -1)
    B1 = torch.stack([I1.to(torch.uint8), (I1 * 0.5).to(torch.uint8), I0.to(torch.uint8)], -1)
    return B0.contiguous(), B1.contiguous()


@pytest.mark.gpu
def test_no_smoothness_gives_the_bits_of_the_pf_calls(hs):
    """smoothness=None and mode 0 run the launches of the *_pf_device entry
    points (called here through the library as before this argument existed),
    with and without a prefilter, for all four fused calls."""
    import torch
    L = hs.lib()
    I0, I1 = (_cuda(a) for a in _small_pair())
    B0, B1 = _bgr_pair(I0, I1)
    rows, cols = I0.shape
    s = torch.cuda.current_stream().cuda_stream
    extra = hs.prefilter_planes_bytes(rows, cols, 1)
    ws = torch.empty(hs.flow_interp_bgr_workspace_bytes(rows, cols, 1, 3) + extra,
                     dtype=torch.uint8, device="cuda")
    half = (ctypes.c_float * 1)(0.5)
    offs = (None, hs.Smoothness(0, 0.0), hs.Smoothness(0, float("nan")))
    for pf in (None, hs.Prefilter(2, 4.0, 4.0, 32.0)):
        keep = pf._c() if pf else None
        p = ctypes.byref(keep) if pf else None
        old = [torch.empty_like(I0) for _ in range(4)]
        assert L.hsflow_flow_warped_pf_device(
            I0.data_ptr(), I1.data_ptr(), hs.F32, rows, cols, 1, 3, 2, 5, 5, 20, ALPHA,
            old[0].data_ptr(), old[1].data_ptr(), p, ws.data_ptr(), ws.numel(), s) == 0
        for sm in offs:
            u, v = hs.flow_warped_device(I0, I1, 3, 2, 5, 20, ALPHA, median=5, prefilter=pf,
                                         smoothness=sm)
            assert _same_bits(u, old[0]) and _same_bits(v, old[1])
        on = hs.flow_warped_device(I0, I1, 3, 2, 5, 20, ALPHA, median=5, prefilter=pf,
                                   smoothness=_sm(hs))
        assert not _same_bits(on[0], old[0])  # the mode does run
        mask = torch.empty(I0.shape, dtype=torch.uint8, device="cuda")
        assert L.hsflow_flow_bidir_pf_device(
            I0.data_ptr(), I1.data_ptr(), hs.F32, rows, cols, 1, 3, 2, 5, 5, 20, ALPHA, REL, ABS,
            *[t.data_ptr() for t in old], None, mask.data_ptr(), None, None, None, None, p,
            ws.data_ptr(), ws.numel(), s) == 0
        for sm in offs:
            r = hs.flow_bidir_device(I0, I1, 3, 2, 5, 20, ALPHA, median=5, mask_f=True,
                                     prefilter=pf, smoothness=sm)
            for got, want in zip((r.uf, r.vf, r.ub, r.vb), old):
                assert _same_bits(got, want)
            assert torch.equal(r.mask_f, mask)
        frame = torch.empty((1, rows, cols), dtype=torch.float32, device="cuda")
        assert L.hsflow_flow_interp_pf_device(
            I0.data_ptr(), I1.data_ptr(), hs.F32, rows, cols, 1, 3, 2, 5, 5, 20, ALPHA, REL, ABS,
            half, 1, frame.data_ptr(), hs.F32, None, None, p, ws.data_ptr(), ws.numel(), s) == 0
        for sm in offs:
            o, _, _ = hs.flow_interp_device(I0, I1, 0.5, 3, 2, 5, 20, ALPHA, median=5,
                                            prefilter=pf, smoothness=sm)
            assert _same_bits(o, frame)
        cframe = torch.empty((1, rows, cols, 3), dtype=torch.float32, device="cuda")
        assert L.hsflow_flow_interp_bgr_pf_device(
            B0.data_ptr(), B1.data_ptr(), rows, cols, 1, 3, 2, 5, 5, 20, ALPHA, REL, ABS, half, 1,
            cframe.data_ptr(), hs.F32, None, None, p, ws.data_ptr(), ws.numel(), s) == 0
        for sm in offs:
            o, _, _ = hs.flow_interp_bgr_device(B0, B1, 0.5, 3, 2, 5, 20, ALPHA, median=5,
                                                prefilter=pf, smoothness=sm)
            assert _same_bits(o, cframe)
    torch.cuda.synchronize()


def _pieces_warped(hs, t0, t1, levels, warps, w, n, alpha, k, lam):
    """The schedule as a loop over the public pieces (one pair)."""
    import torch
    P0, P1 = hs.pyramid_build_device(t0, t1, levels)
    frames = [(t0, t1)] + list(zip(P0, P1))
    u = v = None
    for lv in range(levels - 1, -1, -1):
        a, b = frames[lv]
        r, c = a.shape
        if u is None:
            u = torch.zeros((r, c), dtype=torch.float32, device="cuda")
            v = torch.zeros_like(u)
        else:
            nu, nv = (torch.empty((r, c), dtype=torch.float32, device="cuda") for _ in range(2))
            hs.upflow_device(u, v, nu, nv)
            u, v = nu, nv
        ws = hs.alloc_workspace(r, c, 1)
        for _ in range(warps):
            hs.warp_gradients_device(a, b, u, v, ws)
            g = hs.diffusivity_device(u, v, lam)
            hs.jacobi_weighted_device(r, c, 1, w, n, alpha, g, u, v, ws)
            if k:
                u, v = hs.median_device(u, v, k)
    return u, v


@pytest.mark.gpu
@pytest.mark.parametrize("levels,warps", [(1, 1), (1, 2), (3, 1), (3, 2)])
@pytest.mark.parametrize("k", [0, 5])
def test_schedule_equals_a_loop_over_the_public_pieces(hs, levels, warps, k):
    """Per level, coarsest first: warm start, then `warps` times KW, KG, the
    weighted iterations and KM.  Window 5 with 25 iterations (whole launches
    and a remainder), and window 3."""
    import torch
    I0, I1 = _pair(*PAIR_B)
    t0, t1 = _cuda(I0), _cuda(I1)
    for w, n in ((5, 25), (3, 10)):
        u, v = _pieces_warped(hs, t0, t1, levels, warps, w, n, ALPHA, k, LAM)
        gu, gv = hs.flow_warped_device(t0, t1, levels, warps, w, n, ALPHA, median=k,
                                       smoothness=_sm(hs))
        torch.cuda.synchronize()
        assert _same_bits(gu, u) and _same_bits(gv, v), (w, n)
    if (levels, warps) == (1, 1):
        # zero flow, so g = 1: the mode changes nothing but rounding
        pu, pv = hs.flow_warped_device(t0, t1, 1, 1, 3, 10, ALPHA, median=k)
        eu = norm_rel_err(gu.cpu().numpy(), pu.cpu().numpy().astype(np.float64))
        ev = norm_rel_err(gv.cpu().numpy(), pv.cpu().numpy().astype(np.float64))
        print(f"levels 1, warps 1, median {k}: against the plain solve {eu:.2e} {ev:.2e}")
        assert eu <= TOL and ev <= TOL


@pytest.mark.gpu
@pytest.mark.parametrize("levels,median", [(1, 0), (3, 5)])
def test_fused_calls_equal_their_public_pieces_bitwise(hs, levels, median):
    """The bidirectional call: the two warped calls and the check.  The two
    fused interpolations: the bidirectional call (with a prefilter: on the
    prefiltered planes), then the frame-interpolation kernel on the frames.
    97 x 131, batch 2."""
    import torch
    sm, pf = _sm(hs), hs.Prefilter(2, 4.0, 4.0, 32.0)
    args = (levels, 2, 5, 20, ALPHA)
    times = (0.25, 0.5)
    I0, I1 = (_cuda(a) for a in _small_pair(2))
    uf, vf = hs.flow_warped_device(I0, I1, *args, median=median, smoothness=sm)
    ub, vb = hs.flow_warped_device(I1, I0, *args, median=median, smoothness=sm)
    r = hs.flow_bidir_device(I0, I1, *args, median=median, err_f=True, mask_f=True, counts_f=True,
                             err_b=True, mask_b=True, counts_b=True, smoothness=sm)
    for got, want in ((r.uf, uf), (r.vf, vf), (r.ub, ub), (r.vb, vb)):
        assert _same_bits(got, want)
    ef, mf, cf = hs.consistency_device(uf, vf, ub, vb, err=True, mask=True, counts=True)
    eb, mb, cb = hs.consistency_device(ub, vb, uf, vf, err=True, mask=True, counts=True)
    assert _same_bits(r.err_f, ef) and _same_bits(r.err_b, eb)
    for got, want in ((r.mask_f, mf), (r.mask_b, mb), (r.counts_f, cf), (r.counts_b, cb)):
        assert torch.equal(got, want)
    plain = hs.flow_warped_device(I0, I1, *args, median=median)
    assert not _same_bits(plain[0], uf)  # the mode did run
    # grey interpolation, without and with a prefilter
    wo, wf, wc = hs.frame_interp_device(I0, I1, r.uf, r.vf, r.ub, r.vb, times, mask_f=r.mask_f,
                                        mask_b=r.mask_b, flags=True, trusted=True)
    go, gf, gc = hs.flow_interp_device(I0, I1, times, *args, median=median, flags=True,
                                       trusted=True, smoothness=sm)
    assert _same_bits(go, wo) and torch.equal(gf, wf) and torch.equal(gc, wc)
    P0, P1 = hs.prefilter_device(I0, pf), hs.prefilter_device(I1, pf)
    q = hs.flow_bidir_device(P0, P1, *args, median=median, mask_f=True, mask_b=True,
                             smoothness=sm)
    q2 = hs.flow_bidir_device(I0, I1, *args, median=median, mask_f=True, mask_b=True,
                              prefilter=pf, smoothness=sm)
    for got, want in zip(q2[:4], q[:4]):
        assert _same_bits(got, want)
    wo, wf, wc = hs.frame_interp_device(I0, I1, q.uf, q.vf, q.ub, q.vb, times, mask_f=q.mask_f,
                                        mask_b=q.mask_b, flags=True, trusted=True)
    go, gf, gc = hs.flow_interp_device(I0, I1, times, *args, median=median, flags=True,
                                       trusted=True, prefilter=pf, smoothness=sm)
    assert _same_bits(go, wo) and torch.equal(gf, wf) and torch.equal(gc, wc)
    # colour
    B0, B1 = _bgr_pair(I0, I1)
    G0, G1 = hs.bgr_to_gray_device(B0), hs.bgr_to_gray_device(B1)
    c = hs.flow_bidir_device(G0, G1, *args, median=median, mask_f=True, mask_b=True,
                             smoothness=sm)
    wo, wf, wc = hs.frame_interp_bgr_device(B0, B1, c.uf, c.vf, c.ub, c.vb, times,
                                            mask_f=c.mask_f, mask_b=c.mask_b, flags=True,
                                            trusted=True)
    go, gf, gc = hs.flow_interp_bgr_device(B0, B1, times, *args, median=median, flags=True,
                                           trusted=True, smoothness=sm)
    torch.cuda.synchronize()
    assert _same_bits(go, wo) and torch.equal(gf, wf) and torch.equal(gc, wc)


@pytest.mark.gpu
def test_host_calls_equal_device_calls_bitwise(hs):
    """With the context's smoothness set (by set_smoothness, or for one call by
    smoothness=) every host call equals its *_sm_device form; afterwards the
    setting is off again; flow and flow_pyramid keep their bits while it is
    set."""
    import torch
    sm = _sm(hs)
    args = (3, 2, 5, 20, ALPHA)
    times = (0.0, 0.5, 1.0)
    I0, I1 = _small_pair()
    t0, t1 = _cuda(I0), _cuda(I1)
    du, dv = hs.flow_warped_device(t0, t1, *args, median=5, smoothness=sm)
    dr = hs.flow_bidir_device(t0, t1, *args, median=5, mask_f=True, mask_b=True, smoothness=sm)
    do, dfl, dtr = hs.flow_interp_device(t0, t1, times, *args, median=5, flags=True, trusted=True,
                                         smoothness=sm)
    B0 = np.stack([I0, 0.5 * I0, I1], -1).astype(np.uint8)
    B1 = np.stack([I1, 0.5 * I1, I0], -1).astype(np.uint8)
    co, cfl, ctr = hs.flow_interp_bgr_device(_cuda(B0), _cuda(B1), times, *args, median=5,
                                             out_dtype=torch.uint8, flags=True, trusted=True,
                                             smoothness=sm)
    torch.cuda.synchronize()
    ctx = hs.Context(0)
    before = ctx.flow(I0, I1, 5, 20, ALPHA)
    pyr = ctx.flow_pyramid(I0, I1, 3, 5, 20, ALPHA)
    plain = ctx.flow_warped(I0, I1, *args, out_dtype=np.float32, median=5)
    for how in ("set", "call"):
        kw = {}
        if how == "set":
            ctx.set_smoothness(sm)
        else:
            kw = dict(smoothness=sm)
        hu, hv = ctx.flow_warped(I0, I1, *args, out_dtype=np.float32, median=5, **kw)
        hb = ctx.flow_bidir(I0, I1, *args, out_dtype=np.float32, median=5, **kw)
        ho, hfl, htr = ctx.interpolate(I0, I1, times, *args, median=5, with_flags=True, **kw)
        hc, hcf, hct = ctx.interpolate_bgr(B0, B1, times, *args, median=5, with_flags=True, **kw)
        if how == "set":
            # the reference-semantics calls ignore the setting
            for got, want in zip(ctx.flow(I0, I1, 5, 20, ALPHA), before):
                assert np.array_equal(got, want)
            for got, want in zip(ctx.flow_pyramid(I0, I1, 3, 5, 20, ALPHA), pyr):
                assert np.array_equal(got, want)
            assert ctx.smoothness() == (FLOW_DRIVEN, float(np.float32(LAM)))  # lambda is an f32
            with pytest.raises(hs.HsflowError):  # the window is checked by the call
                ctx.flow_warped(I0, I1, 3, 2, 7, 20, ALPHA)
            ctx.set_smoothness(None)
        assert ctx.smoothness() is None  # off again afterwards
        assert np.array_equal(hu, du.cpu().numpy()) and np.array_equal(hv, dv.cpu().numpy())
        assert not np.array_equal(hu, plain[0])
        for got, want in zip(hb[:4], (dr.uf, dr.vf, dr.ub, dr.vb)):
            assert np.array_equal(got, want.cpu().numpy())
        assert np.array_equal(hb.mask_f, dr.mask_f.cpu().numpy())
        assert np.array_equal(hb.mask_b, dr.mask_b.cpu().numpy())
        assert np.array_equal(ho, do.cpu().numpy()) and np.array_equal(hfl, dfl.cpu().numpy())
        assert np.array_equal(htr.astype(np.int64), dtr.cpu().numpy()[0].astype(np.int64))
        assert np.array_equal(hc, co.cpu().numpy()) and np.array_equal(hcf, cfl.cpu().numpy())
        assert np.array_equal(hct.astype(np.int64), ctr.cpu().numpy()[0].astype(np.int64))
    again = ctx.flow_warped(I0, I1, *args, out_dtype=np.float32, median=5)
    ctx.close()
    assert np.array_equal(again[0], plain[0]) and np.array_equal(again[1], plain[1])


def _dev_flow(hs, frames, solve, lam):
    import torch
    u, v = hs.flow_warped_device(_cuda(frames[0]), _cuda(frames[1]), *solve, ALPHA, median=MEDIAN,
                                 smoothness=None if lam is None else _sm(hs, lam))
    torch.cuda.synchronize()
    return u.cpu().numpy(), v.cpu().numpy()


PARITY = [(OCCLUDER, WARPS4, 0.3, "f32"), (OCCLUDER, WARPS4, 0.1, "f32"),
          (PAIR_A, SOLVE, 0.3, "f32"), (PAIR_B, SOLVE, 0.3, "f32"),
          (PAIR_B, SOLVE, 0.3, "u8"), (PAIR_B, SOLVE, 0.3, "f16"),
          (PAIR_B, SOLVE, 0.3, "f32_nonint"), (PAIR_B, SOLVE, 0.3, "f64")]


@pytest.mark.gpu
@pytest.mark.parametrize("pair,solve,lam,kind", PARITY,
                         ids=lambda p: "x".join(map(str, p)) if isinstance(p, tuple) else str(p))
def test_whole_solve_against_reference(hs, pair, solve, lam, kind):
    """max|d| / max|ref| against warped_smooth_np within the module's
    tolerance (an f32 emulation of the scheme predicts 1e-6 to 3e-6)."""
    u, v = _dev_flow(hs, _frames(pair, kind), solve, lam)
    ur, vr = _ref(pair, solve, lam, kind)
    eu, ev = norm_rel_err(u, ur), norm_rel_err(v, vr)
    print(f"{pair} {solve} lam {lam} {kind}: {eu:.2e} {ev:.2e}")
    assert eu <= TOL and ev <= TOL


@pytest.mark.gpu
def test_gpu_sharpens_the_moving_square(hs):
    """The reference's quality conditions on the GPU's flows and on its
    interpolated middle frame."""
    import torch
    frames = _occluder(OCCLUDER[1])
    t0, t1 = _cuda(frames[0]), _cuda(frames[1])
    flows, mids = {}, {}
    for name, lam in (("plain", None), ("smooth", LAM)):
        flows[name] = _dev_flow(hs, frames, WARPS4, lam)
        out, _, _ = hs.flow_interp_device(t0, t1, 0.5, *WARPS4, ALPHA, median=MEDIAN,
                                          smoothness=None if lam is None else _sm(hs, lam))
        torch.cuda.synchronize()
        mids[name] = out[0].cpu().numpy()
    _assert_square_quality(flows["plain"], flows["smooth"], mids["plain"], mids["smooth"], "GPU")


@pytest.mark.gpu
@pytest.mark.parametrize("pair", [PAIR_A, PAIR_B])
def test_gpu_keeps_a_pure_shift(hs, pair):
    mean, worst = shift_epe(*_dev_flow(hs, _pair(*pair), SOLVE, LAM), pair)
    print(f"GPU {pair} alpha 100, 5x5, lam {LAM}: interior EPE mean {mean:.4f} max {worst:.4f} px")
    assert mean <= SHIFT_BOUNDS[pair][0] and worst <= SHIFT_BOUNDS[pair][1]


@pytest.mark.gpu
def test_side_streams_give_the_same_bits(hs):
    """A batch of 3 on one stream, split over 2 side streams, and as single
    calls."""
    I0, I1 = (_cuda(a) for a in _small_pair(3))
    args = (3, 2, 5, 15, ALPHA)
    got = {}
    for n in (1, 2):
        with hs.max_streams_as(n):
            got[n] = hs.flow_warped_device(I0, I1, *args, median=5, smoothness=_sm(hs))
    assert _same_bits(got[1][0], got[2][0]) and _same_bits(got[1][1], got[2][1])
    for k in range(3):
        us, vs = hs.flow_warped_device(I0[k].contiguous(), I1[k].contiguous(), *args, median=5,
                                       smoothness=_sm(hs))
        assert _same_bits(got[1][0][k], us) and _same_bits(got[1][1][k], vs)


@pytest.mark.gpu
def test_graph_capture_replays_the_eager_result(hs):
    """One capture and replay of flow_bidir_device(smoothness=) on the origin
    stream (no side streams: batch 1), an eager call on a side stream first."""
    import torch
    rows, cols, levels = 64, 96, 2
    I0, I1 = _pair(2080, rows, cols, -6, 9)
    t0, t1 = _cuda(I0), _cuda(I1)
    flows = [torch.empty_like(t0) for _ in range(4)]
    mask = torch.empty(t0.shape, dtype=torch.uint8, device="cuda")
    ws = torch.empty(hs.bidir_workspace_bytes(rows, cols, 1, levels), dtype=torch.uint8,
                     device="cuda")

    def solve(s):
        hs.flow_bidir_device(t0, t1, levels, 2, 5, 20, ALPHA, uf=flows[0], vf=flows[1],
                             ub=flows[2], vb=flows[3], mask_f=mask, workspace=ws, stream=s,
                             median=5, smoothness=_sm(hs))

    stream = torch.cuda.current_stream()
    cap = torch.cuda.Stream()
    cap.wait_stream(stream)
    with torch.cuda.stream(cap):
        solve(cap)
    stream.wait_stream(cap)
    torch.cuda.synchronize()
    ref = [t.clone() for t in flows + [mask]]
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, capture_error_mode="thread_local"):
        solve(torch.cuda.current_stream())
    torch.cuda.synchronize()
    for t in flows + [mask]:
        t.fill_(1)
    graph.replay()
    torch.cuda.synchronize()
    for t, want in zip(flows + [mask], ref):
        assert _same_bits(t, want)
