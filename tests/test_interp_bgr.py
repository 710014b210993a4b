"""Frame warp and frame interpolation of colour frames
(hsflow_warp_image_bgr_device, hsflow_frame_interp_bgr_device,
hsflow_flow_interp_bgr*, Context.interpolate_bgr, frames.interpolate_sequence).

Frames are dense 8-bit interleaved BGR [..., H, W, 3].  The flow is a grey-level
quantity: per pixel the colour kernel computes what the grey one does (targets,
taps, fractions, in0, in1, n0, n1, wt, flags) once and runs its lerps and blend
on each channel.  So the float64 reference is test_interp.frame_interp_np on
each channel plane, and the kernel is held to the grey kernel per channel bit
for bit, to that reference within the module's tolerance, the fused call to its
public pieces bit for bit, and the whole to the float64 solve of the grey
frames run both ways.
"""
import ctypes
import functools
import os
import shutil
import subprocess

import numpy as np
import pytest

import oracle
from conftest import ROOT
from synth_ref import synth_pair as np_synth
from synth_ref import texture
from test_consistency import HOSTILE, KC_SHAPES, consistency_np
from test_interp import (BAND, GAIN, MARGIN, REL, ABS, SOLVE, TIMES, TOL, _cuda, _flows,
                         _guards_intact, _interior, _masks, _placed, _same_bits, frame_interp_np,
                         warp_image_np)
from test_median import warped_median_np

GUARD_F, GUARD_B = -7.25, 0xA5
SHAPE_IDS = dict(ids=lambda s: "x".join(map(str, s)))
# the colour pair of the end-to-end test: channel c is synth_pair(seed + 100 c)
E2E_PAIR = (2001, 96, 128, -12, 20)
E2E_CASES = [(100.0, 5, 0.5), (100.0, 5, 0.25), (400.0, 0, 0.5)]  # alpha, median, t


# ------------------------------------------------------------ shared inputs
@functools.lru_cache(maxsize=None)
def _bgr_textures(shape):
    """Two BGR frames per pair, three different u8 textures per frame."""
    batch, rows, cols = shape
    out = []
    for base in (4000, 5000):
        out.append(np.stack([np.stack([texture(base + 10 * c + k, 0, rows, 0, cols)
                                       for c in range(3)], axis=-1)
                             for k in range(batch)]).astype(np.uint8))
    for a in out:
        a.setflags(write=False)
    return tuple(out)


def _channel(bgr, c):
    return np.ascontiguousarray(bgr[..., c])


@functools.lru_cache(maxsize=None)
def _bgr_ref(shape, times):
    """frame_interp_np per channel: out [B, nt, H, W, 3], flags [B, nt, H, W]
    and the pixels left out of the comparisons (they depend on the flows only)."""
    I0, I1 = _bgr_textures(shape)
    flows, (mf, mb) = _flows(shape), _masks(shape)
    batch, rows, cols = shape
    out = np.empty((batch, len(times), rows, cols, 3))
    flags = np.empty(out.shape[:-1], np.uint8)
    rim = np.empty(flags.shape, bool)
    half = np.empty(flags.shape, bool)
    for k in range(batch):
        for j, t in enumerate(times):
            for c in range(3):
                o, f, r, h = frame_interp_np(I0[k, ..., c], I1[k, ..., c],
                                             *(a[k] for a in flows), t, mf[k], mb[k])
                out[k, j, ..., c] = o
            flags[k, j], rim[k, j], half[k, j] = f, r <= BAND, h <= BAND
    for a in (out, flags, rim, half):
        a.setflags(write=False)
    return out, flags, rim, half


def _colour_pair(seed, rows, cols, qdy, qdx):
    """Channel c = synth_pair(seed + 100 c): all channels share the shift."""
    chans = [np_synth(seed + 100 * c, rows, cols, qdy, qdx) for c in range(3)]
    return tuple(np.stack([ch[k] for ch in chans], axis=-1).astype(np.uint8) for k in range(2))


@functools.lru_cache(maxsize=None)
def _e2e_solve(alpha, k):
    """Float64 solve of the grey frames (the oracle's 15-bit formula) both ways,
    the check both ways and the flows' own band (test_interp._solve_ref)."""
    B0, B1 = _colour_pair(*E2E_PAIR)
    G0, G1 = oracle.bgr_to_gray(B0), oracle.bgr_to_gray(B1)
    levels, warps, w, n = SOLVE
    uf, vf = warped_median_np(G0, G1, levels, warps, w, n, alpha, k)
    ub, vb = warped_median_np(G1, G0, levels, warps, w, n, alpha, k)
    mf = consistency_np(uf, vf, ub, vb, REL, ABS)[1]
    mb = consistency_np(ub, vb, uf, vf, REL, ABS)[1]
    band = 4.0 * GAIN * TOL * max(float(np.abs(a).max()) for a in (uf, vf, ub, vb))
    return (uf, vf, ub, vb), (mf, mb), band


@functools.lru_cache(maxsize=None)
def _e2e_ref(alpha, k, t):
    flows, (mf, mb), band = _e2e_solve(alpha, k)
    B0, B1 = _colour_pair(*E2E_PAIR)
    outs = [frame_interp_np(B0[..., c], B1[..., c], *flows, t, mf, mb) for c in range(3)]
    return np.stack([o[0] for o in outs], axis=-1), outs[0][1], outs[0][2], band


def _e2e_quality(frame, t, who):
    """Per channel: interior mean error at most a quarter of the plain blend's."""
    seed, rows, cols, qdy, qdx = E2E_PAIR
    B0, B1 = _colour_pair(*E2E_PAIR)
    assert qdy * t == int(qdy * t) and qdx * t == int(qdx * t)
    for c in range(3):
        truth = np_synth(seed + 100 * c, rows, cols, int(qdy * t), int(qdx * t))[1]
        inner = (slice(MARGIN, -MARGIN), slice(MARGIN, -MARGIN))
        got = float(np.abs(frame[..., c].astype(np.float64) - truth)[inner].mean())
        plain = (1.0 - t) * B0[..., c].astype(np.float64) + t * B1[..., c]
        blend = float(np.abs(plain - truth)[inner].mean())
        print(f"{who} channel {c} t {t}: interior mean error {got:.3f}, plain blend {blend:.3f} "
              f"({got / blend:.4f})")
        assert got <= 0.25 * blend


# ------------------------------------------------------------------ CPU tests
def test_reference_on_a_grey_frame_gives_three_equal_channels():
    shape = (3, 37, 131)
    flows, (mf, mb) = _flows(shape), _masks(shape)
    g0, g1 = (_channel(a, 1)[0].astype(np.float64) for a in _bgr_textures(shape))
    b0, b1 = (np.repeat(g[..., None], 3, axis=-1) for g in (g0, g1))
    for t in (0.0, 0.3, 1.0):
        grey, gf, _, _ = frame_interp_np(g0, g1, *(a[0] for a in flows), t, mf[0], mb[0])
        for c in range(3):
            o, f, _, _ = frame_interp_np(b0[..., c], b1[..., c], *(a[0] for a in flows), t,
                                         mf[0], mb[0])
            assert np.array_equal(o, grey) and np.array_equal(f, gf)


@pytest.mark.parametrize("alpha,k,t", E2E_CASES)
def test_reference_interpolates_the_colour_pair(alpha, k, t):
    """The inputs of the GPU end-to-end test are in a regime where the float64
    reference alone passes both of its conditions with a wide margin."""
    ref, _, rim, band = _e2e_ref(alpha, k, t)
    assert (rim <= band).mean() <= 0.02
    _e2e_quality(ref, t, "reference")


def _times(*t):
    return (ctypes.c_float * len(t))(*t)


def test_argument_errors_without_a_gpu():
    import hsflow
    L = hsflow.lib()
    E = hsflow.HSFLOW_ERR_ARG
    nan = float("nan")
    half = _times(0.5)
    # never dereferenced: every call fails its checks first.  16 x 16: a BGR u8
    # frame is 768 bytes, an f32 BGR frame 3072, an f32 plane 1024; the
    # addresses below are 4096 apart
    A = [4096 * k for k in range(1, 16)]

    def err():
        return L.hsflow_last_error(None).decode()

    def krc(I=A[0], u=A[1], v=A[2], out=A[3], oof=A[4], dtype_out=hsflow.F32, rows=16):
        return L.hsflow_warp_image_bgr_device(I, rows, 16, 1, u, v, out, dtype_out, oof, None)

    for null in ("I", "u", "v", "out"):
        assert krc(**{null: None}) == E
    assert krc(rows=0) == E
    for bad in (hsflow.F64, hsflow.F16, 9):
        assert krc(dtype_out=bad) == E
    for over in (dict(out=A[0]), dict(out=A[0] + 767), dict(out=A[1] - 3071), dict(oof=A[0]),
                 dict(oof=A[3] + 3071), dict(out=A[4] - 3071)):
        assert krc(**over) == E
        assert "overlap" in err()

    def kic(I0=A[0], I1=A[1], uf=A[2], vf=A[3], ub=A[4], vb=A[5], mf=A[6], mb=A[7], times=half,
            nt=1, out=A[8], dtype_out=hsflow.F32, flags=A[10], trusted=A[12], rows=16):
        return L.hsflow_frame_interp_bgr_device(I0, I1, rows, 16, 1, uf, vf, ub, vb, mf, mb,
                                                times, nt, out, dtype_out, flags, trusted, None)

    for null in ("I0", "I1", "uf", "vf", "ub", "vb", "out", "times"):
        assert kic(**{null: None}) == E
    for nt in (0, -1, 17):
        assert kic(times=_times(*([0.5] * 17)), nt=nt) == E
        assert "nt" in err()
    for bad in (-0.01, 1.01, nan, float("inf")):
        assert kic(times=_times(bad)) == E
        assert kic(times=_times(0.5, bad), nt=2) == E
        assert "time" in err()
    assert kic(rows=0) == E
    for bad in (hsflow.F64, hsflow.F16, 9):
        assert kic(dtype_out=bad) == E
    for over in (dict(out=A[0]), dict(out=A[0] + 767), dict(out=A[7] + 255), dict(flags=A[1]),
                 dict(flags=A[8] + 3071), dict(trusted=A[4] + 1020), dict(trusted=A[10] + 252),
                 dict(out=A[10] - 3071),  # an f32 BGR frame is three planes long
                 # two times: the second output frame reaches the flags
                 dict(times=_times(0.25, 0.5), nt=2, flags=A[8] + 3072)):
        assert kic(**over) == E
        assert "overlap" in err()

    big = 1 << 30

    def fused(I0=A[0], I1=A[1], levels=3, warps=1, median=0, rel=REL, abs_=ABS, times=half, nt=1,
              out=A[2], dtype_out=hsflow.F32, flags=A[3], trusted=A[4], ws=1 << 20, wsb=big,
              rows=16):
        return L.hsflow_flow_interp_bgr_device(I0, I1, rows, 16, 1, levels, warps, median, 5, 10,
                                               1.0, rel, abs_, times, nt, out, dtype_out, flags,
                                               trusted, ws, wsb, None)

    need = hsflow.flow_interp_bgr_workspace_bytes(16, 16, 1, 3)
    for null in ("I0", "I1", "out", "ws", "times"):
        assert fused(**{null: None}) == E
    for kw in (dict(warps=0), dict(warps=17), dict(median=4), dict(levels=0), dict(levels=9),
               dict(rel=nan), dict(abs_=-1.0), dict(nt=0), dict(nt=17), dict(times=_times(1.5)),
               dict(times=_times(nan)), dict(dtype_out=hsflow.F64), dict(dtype_out=9),
               dict(rows=0)):
        assert fused(**kw) == E, kw
    assert fused(wsb=need - 1) == E
    assert "workspace" in err()
    for over in (dict(out=A[0]), dict(flags=A[1] + 700), dict(out=(1 << 20) + need - 4),
                 dict(trusted=(1 << 20) + 64), dict(flags=A[2] + 512),
                 dict(I0=(1 << 20) + need - 1)):
        assert fused(**over, wsb=need) == E
        assert "overlap" in err()

    # the host form: its arguments are checked before the context
    planes = (ctypes.c_void_p * 1)(A[2])

    def host(ctx=None, b0=A[0], b1=A[1], step0=48, step1=48, levels=3, times=half, nt=1,
             out=planes, dtype_out=hsflow.U8, out_step=48, flags=None, flags_step=16):
        return L.hsflow_flow_interp_bgr(ctx, b0, b1, 16, 16, step0, step1, levels, 1, 0, 5, 10,
                                        1.0, REL, ABS, times, nt, out, dtype_out, out_step, flags,
                                        flags_step, None)

    assert host() == E and "context" in err()
    for kw, word in ((dict(b0=None), "null"), (dict(b1=None), "null"), (dict(out=None), "null"),
                     (dict(step0=47), "steps"), (dict(step1=47), "steps"),
                     (dict(out_step=47), "output step"),
                     (dict(dtype_out=hsflow.F32, out_step=191), "output step"),
                     (dict(dtype_out=hsflow.F64, out_step=1024), "dtype"),
                     (dict(nt=0), "nt"), (dict(nt=17, times=_times(*([0.5] * 17))), "nt"),
                     (dict(times=_times(nan)), "time"), (dict(times=_times(1.5)), "time"),
                     (dict(levels=0), "levels"),
                     (dict(flags=(ctypes.c_void_p * 1)(A[5]), flags_step=15), "flags step")):
        assert host(**kw) == E, kw
        assert word in err(), (kw, err())
    z = np.zeros((8, 8, 3), np.uint8)
    with pytest.raises(hsflow.HsflowError):
        hsflow.Context.interpolate_bgr(None, z, z[:4], [0.5], 3, 2, 5, 10, 100.0)
    with pytest.raises(hsflow.HsflowError):
        hsflow.Context.interpolate_bgr(None, z[..., 0], z[..., 0], [0.5], 3, 2, 5, 10, 100.0)


def test_workspace_size_is_monotone_and_holds_the_grey_interpolation():
    import hsflow
    assert hsflow.flow_interp_bgr_workspace_bytes(0, 16, 1, 3) == 0
    assert hsflow.flow_interp_bgr_workspace_bytes(16, 16, 1, 0) == 0
    prev = 0
    for rows, cols, batch, levels in ((16, 16, 1, 1), (16, 16, 1, 3), (48, 64, 1, 3), (48, 64, 2, 3),
                                      (97, 131, 2, 3), (97, 131, 3, 4)):
        n = hsflow.flow_interp_bgr_workspace_bytes(rows, cols, batch, levels)
        px = rows * cols * batch
        assert n >= hsflow.flow_interp_workspace_bytes(rows, cols, batch, levels) + 2 * px
        assert n % 256 == 0 and n > prev
        prev = n


def test_python_surface():
    import hsflow
    import inspect
    for name in ("hsflow_warp_image_bgr_device", "hsflow_frame_interp_bgr_device",
                 "hsflow_flow_interp_bgr_workspace_bytes", "hsflow_flow_interp_bgr_device",
                 "hsflow_flow_interp_bgr", "hsflow_set_interp_bgr_loads"):
        assert name in hsflow.EXPORTS and hasattr(hsflow.lib(), name)
    for f in ("warp_image_bgr_device", "frame_interp_bgr_device",
              "flow_interp_bgr_workspace_bytes", "flow_interp_bgr_device"):
        assert callable(getattr(hsflow, f))
    sig = inspect.signature(hsflow.Context.interpolate_bgr).parameters
    assert sig["median"].default == 0 and sig["with_flags"].default is False
    assert sig["out_dtype"].default is np.uint8
    import torch
    grey = torch.zeros((8, 8), dtype=torch.uint8)
    real = torch.zeros((8, 8, 3), dtype=torch.float32)
    uv = torch.zeros((8, 8), dtype=torch.float32)
    for bad in (grey, real):
        with pytest.raises(hsflow.HsflowError):
            hsflow.warp_image_bgr_device(bad, uv, uv)
        with pytest.raises(hsflow.HsflowError):
            hsflow.frame_interp_bgr_device(bad, bad, uv, uv, uv, uv, (0.5,))
        with pytest.raises(hsflow.HsflowError):
            hsflow.flow_interp_bgr_device(bad, bad, (0.5,), 3, 2, 5, 10, 100.0)


def test_getframeinterpbgr_compiles_and_links(tmp_path):
    """A C++ caller of HornSchunck::getFrameInterpBgr builds against
    include/hsflow.hpp and libhsflow.so; without a device the call throws
    hsflow::Error (never a crash), bad times are rejected with or without one."""
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("no C++ compiler")
    src = tmp_path / "interp_bgr_main.cpp"
    src.write_text(r'''
#include <cstdint>
#include <cstdio>
#include <vector>
#include "hsflow.hpp"
#if !defined(HSFLOW_HAS_INTERP_BGR) || HSFLOW_HAS_INTERP_BGR != 1
#error "hsflow.h lacks the colour frame interpolation"
#endif
int main() {
    const int rows = 24, cols = 40;
    std::vector<uint8_t> a(rows * cols * 3, 10), b(rows * cols * 3, 20);
    std::vector<std::vector<uint8_t>> frames, flags;
    hsflow::HornSchunck hs(5, 10, 100.0);
    const hsflow::BgrView A{a.data(), rows, cols, 0}, B{b.data(), rows, cols, (size_t)cols * 3};
    int thrown = 0, rejected = 0;
    try { hs.getFrameInterpBgr(A, B, {0.25f, 0.5f, 0.75f}, 3, 2, 5, frames); }
    catch (const hsflow::Error &) { ++thrown; }
    try { hs.getFrameInterpBgr(A, B, {0.5f}, 3, 2, 0, frames, &flags); }
    catch (const hsflow::Error &) { ++thrown; }
    try { hs.getFrameInterpBgr(A, B, {1.5f}, 3, 2, 0, frames); }
    catch (const hsflow::Error &) { ++rejected; }
    try { hs.getFrameInterpBgr(A, B, {}, 3, 2, 0, frames); }
    catch (const hsflow::Error &) { ++rejected; }
    int (*fn)(const uint8_t *, int, int, int, const float *, const float *, void *, int, uint8_t *,
              void *) = &hsflow_warp_image_bgr_device;
    std::printf("%d %d %zu %zu %zu %d\n", thrown, rejected, flags.size(),
                flags.empty() ? 0 : flags[0].size(), frames.empty() ? 0 : frames[0].size(),
                fn != nullptr);
    return 0;
}
''')
    lib_dir = os.path.join(ROOT, "cpp-optical-flow_amd")
    exe = str(tmp_path / "interp_bgr_main")
    subprocess.check_call([gxx, "-std=c++17", "-Wall", "-Werror", "-I",
                           os.path.join(ROOT, "include"), str(src), "-o", exe, "-L", lib_dir,
                           "-lhsflow", "-Wl,-rpath," + lib_dir])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    thrown, rejected, nf, npx, nbytes, linked = (int(x) for x in out.stdout.split())
    assert nf == 1 and npx == 24 * 40 and linked == 1
    assert thrown in (0, 2)  # 2 where no gfx950 device is present
    assert rejected == 2     # argument errors with or without a device
    if thrown == 0:
        assert nbytes == 24 * 40 * 3


def test_interpolate_sequence_refuses_a_grey_source(tmp_path):
    import frames
    path = tmp_path / "grey.gray"
    np.zeros((3, 48, 64), np.uint8).tofile(path)
    src = frames.RawVideo(str(path), 48, 64, "gray8")
    with pytest.raises(frames.FrameError, match="Context.interpolate"):
        next(frames.interpolate_sequence(src, 2, 3, 2, 5, 20, 100.0))


# ------------------------------------------------------------------ GPU tests
def _run_kic(hs, shape, times, flows=None, masks=True, out_dtype=None):
    """KIC on a shape's BGR textures and smooth flows: numpy out, flags, trusted."""
    import torch
    B0, B1 = _bgr_textures(shape)
    flows = _flows(shape) if flows is None else flows
    mf, mb = (_cuda(m) for m in _masks(shape)) if masks else (None, None)
    out, flags, trusted = hs.frame_interp_bgr_device(
        _cuda(B0), _cuda(B1), *(_cuda(a) for a in flows), times, mask_f=mf, mask_b=mb,
        out_dtype=out_dtype, flags=True, trusted=True)
    torch.cuda.synchronize()
    return out.cpu().numpy(), flags.cpu().numpy(), trusted.cpu().numpy()


@pytest.mark.gpu
@pytest.mark.parametrize("shape", KC_SHAPES, **SHAPE_IDS)
def test_colour_kernel_equals_the_grey_kernel_per_channel_bitwise(hs, shape):
    import torch
    B0, B1 = _bgr_textures(shape)
    flows = [_cuda(a) for a in _flows(shape)]
    mf, mb = (_cuda(m) for m in _masks(shape))
    for nt, times in TIMES.items():
        out, flags, trusted = hs.frame_interp_bgr_device(
            _cuda(B0), _cuda(B1), *flows, times, mask_f=mf, mask_b=mb, flags=True, trusted=True)
        assert tuple(out.shape) == (shape[0], nt, *shape[1:], 3) and out.dtype == torch.float32
        assert tuple(flags.shape) == (shape[0], nt, *shape[1:])
        for c in range(3):
            want, want_f, want_c = hs.frame_interp_device(
                _cuda(_channel(B0, c)), _cuda(_channel(B1, c)), *flows, times, mask_f=mf,
                mask_b=mb, flags=True, trusted=True)
            assert _same_bits(out[..., c].contiguous(), want)
            assert torch.equal(flags, want_f) and torch.equal(trusted, want_c)
        # both forms of the tap loads (wide, single bytes) give the same bits
        for wide in (True, False):
            was = hs.set_interp_bgr_loads(wide)
            try:
                o2, f2, c2 = hs.frame_interp_bgr_device(
                    _cuda(B0), _cuda(B1), *flows, times, mask_f=mf, mask_b=mb, flags=True,
                    trusted=True)
            finally:
                hs.set_interp_bgr_loads(was)
            assert _same_bits(o2, out) and torch.equal(f2, flags) and torch.equal(c2, trusted)
    torch.cuda.synchronize()


@pytest.mark.gpu
@pytest.mark.parametrize("shape", KC_SHAPES, **SHAPE_IDS)
def test_colour_kernel_against_reference(hs, shape):
    """|out - ref| <= 1e-4 max|ref| outside the rim band; flags equal outside
    the rim and half bands; trusted the count of the device's own flags == 0
    (test_interp.test_interp_kernel_against_reference, per channel)."""
    for nt, times in TIMES.items():
        ref, ref_flags, rim, half = _bgr_ref(shape, times)
        out, flags, trusted = _run_kic(hs, shape, times)
        d = np.abs(out.astype(np.float64) - ref)[~rim]
        bound = TOL * float(np.abs(ref).max())
        print(f"{shape} nt {nt}: worst |out - ref| {d.max() if d.size else 0.0:.3e} "
              f"(bound {bound:.3e}), excluded {(rim | half).mean():.4f}")
        assert np.all(d <= bound)
        keep = ~(rim | half)
        assert np.array_equal(flags[keep], ref_flags[keep])
        assert np.array_equal(trusted.astype(np.int64), (flags == 0).sum(axis=(2, 3)))


@pytest.mark.gpu
@pytest.mark.parametrize("shape", [(3, 37, 131), (2, 4, 256)], **SHAPE_IDS)
def test_u8_output_is_the_rounded_f32_output(hs, shape):
    """floor(x + 0.5) in float32 numpy on the f32 output of the same inputs."""
    import torch
    B0, B1 = (_cuda(a) for a in _bgr_textures(shape))
    flows = [_cuda(a) for a in _flows(shape)]
    times = (0.0, 0.4, 1.0)
    f32, fl32, _ = hs.frame_interp_bgr_device(B0, B1, *flows, times, flags=True)
    u8, fl8, _ = hs.frame_interp_bgr_device(B0, B1, *flows, times, out_dtype=torch.uint8,
                                            flags=True)
    torch.cuda.synchronize()
    x = f32.cpu().numpy()
    want = np.clip(np.floor(x + np.float32(0.5)), 0.0, 255.0).astype(np.uint8)
    assert u8.dtype == torch.uint8 and np.array_equal(u8.cpu().numpy(), want)
    assert torch.equal(fl8, fl32)


@pytest.mark.gpu
def test_end_times_return_the_frames_bytewise(hs):
    import torch
    shape = (3, 37, 131)
    B0, B1 = (_cuda(a) for a in _bgr_textures(shape))
    flows = [_cuda(a) for a in _flows(shape)]
    out, _, _ = hs.frame_interp_bgr_device(B0, B1, *flows, (0.0, 1.0), out_dtype=torch.uint8)
    torch.cuda.synchronize()
    assert torch.equal(out[:, 0], B0) and torch.equal(out[:, 1], B1)


@pytest.mark.gpu
def test_three_times_equal_three_calls_and_a_batch_single_calls_bitwise(hs):
    import torch
    shape = (3, 37, 131)
    B0, B1 = (_cuda(a) for a in _bgr_textures(shape))
    flows = [_cuda(a) for a in _flows(shape)]
    mf, mb = (_cuda(m) for m in _masks(shape))
    times = (0.25, 0.5, 0.9)
    out, flags, trusted = hs.frame_interp_bgr_device(B0, B1, *flows, times, mask_f=mf, mask_b=mb,
                                                     flags=True, trusted=True)
    for j, t in enumerate(times):
        o, f, c = hs.frame_interp_bgr_device(B0, B1, *flows, (t,), mask_f=mf, mask_b=mb,
                                             flags=True, trusted=True)
        assert _same_bits(out[:, j].contiguous(), o[:, 0].contiguous())
        assert torch.equal(flags[:, j], f[:, 0]) and torch.equal(trusted[:, j], c[:, 0])
    for k in range(shape[0]):
        o, f, c = hs.frame_interp_bgr_device(
            B0[k].contiguous(), B1[k].contiguous(), *(a[k].contiguous() for a in flows), times,
            mask_f=mf[k].contiguous(), mask_b=mb[k].contiguous(), flags=True, trusted=True)
        assert _same_bits(out[k], o) and torch.equal(flags[k], f)
        assert torch.equal(trusted[k], c[0])
    torch.cuda.synchronize()


def _placed_bgr(a, offset, dtype, fill, shape=None):
    """test_interp._placed for a [..., H, W, 3] array: the guards are one
    frame's bytes (or elements) long.  Returns (flat, view, (lo, hi))."""
    shape = tuple(a.shape) if shape is None else tuple(shape)
    flat_shape = shape[:-2] + (shape[-2] * 3,)  # rows of 3 W elements
    src = None if a is None else np.ascontiguousarray(a).reshape(flat_shape)
    flat, view, span = _placed(src, offset, dtype, fill, None if a is not None else flat_shape)
    return flat, view.view(shape), span


@pytest.mark.gpu
@pytest.mark.parametrize("out_dtype", ["f32", "u8"])
def test_unaligned_bases_null_masks_and_single_outputs(hs, out_dtype):
    """Every input and output at byte (u8) or element (f32) offsets 1, 2 and 3 of
    an allocation of its own, between guards: the guards keep their bytes and
    the results equal the aligned call's.  37 x 131 x 3 is odd, so the three
    pairs' frames take the dword stores and the byte stores in turn; 4 x 256
    takes the dwords where the base allows."""
    import torch
    odt = torch.float32 if out_dtype == "f32" else torch.uint8
    gfill = GUARD_F if out_dtype == "f32" else GUARD_B
    times = (0.25, 0.5, 0.9)
    for shape in ((3, 37, 131), (2, 4, 256)):
        B0, B1 = _bgr_textures(shape)
        flows, (mf, mb) = _flows(shape), _masks(shape)
        oshape = (shape[0], len(times), *shape[1:], 3)
        fshape = oshape[:-1]
        ins = [_cuda(a) for a in (B0, B1, *flows)]
        want, want_f, want_c = hs.frame_interp_bgr_device(
            *ins, times, mask_f=_cuda(mf), mask_b=_cuda(mb), out_dtype=odt, flags=True,
            trusted=True)
        for off in (1, 2, 3):
            pb = [_placed_bgr(a, (off + k) % 4, torch.uint8, 7)[1] for k, a in enumerate((B0, B1))]
            pf = [_placed(a, (off + k) % 4, torch.float32, 0.0)[1] for k, a in enumerate(flows)]
            pmf = _placed(mf, off, torch.uint8, 1)[1]
            pmb = _placed(mb, (off + 1) % 4, torch.uint8, 1)[1]
            fo, o, (o0, o1) = _placed_bgr(None, off, odt, gfill, oshape)
            ff, f, (f0, f1) = _placed(None, (off + 2) % 4, torch.uint8, GUARD_B, fshape)
            c = torch.full((shape[0] + 2, len(times)), -12345, dtype=torch.int32, device="cuda")
            hs.frame_interp_bgr_device(*pb, *pf, times, mask_f=pmf, mask_b=pmb, out=o, flags=f,
                                       trusted=c[1:-1])
            torch.cuda.synchronize()
            assert _same_bits(o, want) and torch.equal(f, want_f)
            assert torch.equal(c[1:-1], want_c)
            assert _guards_intact(fo, o0, o1, gfill) and _guards_intact(ff, f0, f1, GUARD_B)
            assert bool((c[0] == -12345).all()) and bool((c[-1] == -12345).all())
        # each optional output alone, and none
        o, f, c = hs.frame_interp_bgr_device(*ins, times, mask_f=_cuda(mf), mask_b=_cuda(mb),
                                             out_dtype=odt)
        assert f is None and c is None and _same_bits(o, want)
        o, f, _ = hs.frame_interp_bgr_device(*ins, times, mask_f=_cuda(mf), mask_b=_cuda(mb),
                                             out_dtype=odt, flags=True)
        assert _same_bits(o, want) and torch.equal(f, want_f)
        o, _, c = hs.frame_interp_bgr_device(*ins, times, mask_f=_cuda(mf), mask_b=_cuda(mb),
                                             out_dtype=odt, trusted=True)
        assert _same_bits(o, want) and torch.equal(c, want_c)
        # NULL masks: the frames are the same, the two mask bits never set
        o, f, c = hs.frame_interp_bgr_device(*ins, times, out_dtype=odt, flags=True, trusted=True)
        assert _same_bits(o, want)
        assert torch.equal(f, want_f & 3) and int((f & 12).sum()) == 0
        assert torch.equal(c.to(torch.int64), (f == 0).sum(dim=(2, 3)))
        torch.cuda.synchronize()


@pytest.mark.gpu
@pytest.mark.parametrize("plane", range(4), ids=["uf", "vf", "ub", "vb"])
def test_hostile_flows_stay_inside_the_pair(hs, plane):
    """NaN, +-inf and +-1e30 at scattered pixels (corners included) of one flow
    plane of the middle pair of three, everything between guards: the call
    completes, the guards keep their bytes, the other pairs' outputs equal a
    clean run bit for bit, the hostile pair's pixels with finite flows too, and
    every output is finite."""
    import torch
    shape = (3, 37, 131)
    times = (0.0, 0.5, 1.0)
    flows = [np.array(a) for a in _flows(shape)]
    rng = np.random.default_rng(291 + plane)
    _, rows, cols = shape
    spots = [(0, 0), (0, cols - 1), (rows - 1, 0), (rows - 1, cols - 1)]
    spots += [(int(rng.integers(rows)), int(rng.integers(cols))) for _ in range(26)]
    for k, (y, x) in enumerate(spots):
        flows[plane][1, y, x] = HOSTILE[k % len(HOSTILE)]
    B0, B1 = _bgr_textures(shape)
    mf, mb = _masks(shape)
    oshape = (shape[0], len(times), rows, cols, 3)
    want, want_f, want_c = _run_kic(hs, shape, times)
    ins = [_placed_bgr(a, 0, torch.uint8, 7)[1] for a in (B0, B1)]
    ins += [_placed(a, 0, torch.float32, 0.0)[1] for a in flows]
    fo, o, (o0, o1) = _placed_bgr(None, 0, torch.float32, GUARD_F, oshape)
    ff, f, (f0, f1) = _placed(None, 0, torch.uint8, GUARD_B, oshape[:-1])
    c = torch.full((shape[0] + 2, len(times)), -12345, dtype=torch.int32, device="cuda")
    hs.frame_interp_bgr_device(*ins, times, mask_f=_placed(mf, 0, torch.uint8, 1)[1],
                               mask_b=_placed(mb, 0, torch.uint8, 1)[1], out=o, flags=f,
                               trusted=c[1:-1])  # raises unless the call returns 0
    torch.cuda.synchronize()
    assert _guards_intact(fo, o0, o1, GUARD_F) and _guards_intact(ff, f0, f1, GUARD_B)
    assert bool((c[0] == -12345).all()) and bool((c[-1] == -12345).all())
    out, fl, cnt = o.cpu().numpy(), f.cpu().numpy(), c[1:-1].cpu().numpy()
    assert np.isfinite(out).all()
    for k in (0, 2):
        assert out[k].tobytes() == want[k].tobytes() and np.array_equal(fl[k], want_f[k])
        assert np.array_equal(cnt[k], want_c[k])
    finite = np.isfinite(flows[plane][1]) & (np.abs(flows[plane][1]) < 1e29)
    assert (~finite).sum() >= 20
    for j in range(len(times)):
        assert out[1, j][finite].tobytes() == want[1, j][finite].tobytes()
        assert np.array_equal(fl[1, j][finite], want_f[1, j][finite])
    assert np.array_equal(cnt.astype(np.int64), (fl == 0).sum(axis=(2, 3)))


@pytest.mark.gpu
@pytest.mark.parametrize("shape", KC_SHAPES, **SHAPE_IDS)
def test_colour_warp_equals_the_grey_warp_per_channel_bitwise(hs, shape):
    import torch
    B1 = _bgr_textures(shape)[1]
    uf, vf, _, _ = _flows(shape)
    t1, u, v = _cuda(B1), _cuda(uf), _cuda(vf)
    out, oof = hs.warp_image_bgr_device(t1, u, v, oof=True)
    alone = hs.warp_image_bgr_device(t1, u, v)
    u8 = hs.warp_image_bgr_device(t1, u, v, out_dtype=torch.uint8)
    forms = []  # both forms of the tap loads: wide, single bytes
    for wide in (True, False):
        was = hs.set_interp_bgr_loads(wide)
        try:
            forms.append(hs.warp_image_bgr_device(t1, u, v))
        finally:
            hs.set_interp_bgr_loads(was)
    torch.cuda.synchronize()
    assert tuple(out.shape) == (*shape, 3) and tuple(oof.shape) == shape
    assert _same_bits(alone, out) and all(_same_bits(f, out) for f in forms)
    for c in range(3):
        want, want_oof = hs.warp_image_device(_cuda(_channel(B1, c)), u, v, oof=True)
        assert _same_bits(out[..., c].contiguous(), want) and torch.equal(oof, want_oof)
    x = out.cpu().numpy()
    assert np.array_equal(u8.cpu().numpy(),
                          np.clip(np.floor(x + np.float32(0.5)), 0.0, 255.0).astype(np.uint8))
    # and against the float64 reference, which makes the test stand alone
    for k in range(shape[0]):
        for c in range(3):
            ref, _, rim = warp_image_np(B1[k, ..., c], uf[k], vf[k])
            assert np.abs(x[k, ..., c] - ref).max() <= TOL * max(float(np.abs(ref).max()), 1.0)


def _solve_bgr(which):
    B0, B1 = _colour_pair(*E2E_PAIR)  # 96 x 128
    if which == "batch2":
        C0, C1 = _colour_pair(E2E_PAIR[0] + 7, *E2E_PAIR[1:])
        return np.stack([B0, C0]), np.stack([B1, C1])
    return B0, B1


@pytest.mark.gpu
@pytest.mark.parametrize("which", ["single", "batch2"])
@pytest.mark.parametrize("median", [0, 5])
@pytest.mark.parametrize("levels", [1, 3])
def test_fused_call_equals_the_three_public_calls_bitwise(hs, levels, median, which):
    import torch
    B0, B1 = (_cuda(a) for a in _solve_bgr(which))
    times = (0.25, 0.5, 0.75)
    args = (levels, 2, 5, 20, 100.0)
    G0, G1 = hs.bgr_to_gray_device(B0), hs.bgr_to_gray_device(B1)
    r = hs.flow_bidir_device(G0, G1, *args, mask_f=True, mask_b=True, median=median)
    want, want_f, want_c = hs.frame_interp_bgr_device(B0, B1, r.uf, r.vf, r.ub, r.vb, times,
                                                      mask_f=r.mask_f, mask_b=r.mask_b,
                                                      flags=True, trusted=True)
    out, flags, trusted = hs.flow_interp_bgr_device(B0, B1, times, *args, median=median,
                                                    flags=True, trusted=True)
    frames_only, f, c = hs.flow_interp_bgr_device(B0, B1, times, *args, median=median)
    u8 = hs.flow_interp_bgr_device(B0, B1, times, *args, median=median, out_dtype=torch.uint8)[0]
    want8 = hs.frame_interp_bgr_device(B0, B1, r.uf, r.vf, r.ub, r.vb, times,
                                       out_dtype=torch.uint8)[0]
    torch.cuda.synchronize()
    assert _same_bits(out, want) and torch.equal(flags, want_f) and torch.equal(trusted, want_c)
    assert f is None and c is None and _same_bits(frames_only, want)
    assert torch.equal(u8, want8)
    assert int((flags != 0).sum()) > 0 and int(trusted.sum()) > 0


@pytest.mark.gpu
@pytest.mark.parametrize("out_dtype", [np.uint8, np.float32])
def test_host_call_equals_device_call_bitwise(hs, out_dtype):
    import torch
    B0, B1 = _colour_pair(2030, 90, 140, -6, 9)
    times = (0.0, 0.5, 0.75, 1.0)
    args = (3, 2, 5, 20, 100.0)
    odt = torch.uint8 if out_dtype == np.uint8 else torch.float32
    out, flags, trusted = hs.flow_interp_bgr_device(_cuda(B0), _cuda(B1), times, *args, median=5,
                                                    out_dtype=odt, flags=True, trusted=True)
    torch.cuda.synchronize()
    ctx = hs.Context(0)
    h, hf, hc = ctx.interpolate_bgr(B0, B1, times, *args, median=5, out_dtype=out_dtype,
                                    with_flags=True)
    # strided input rows: a window of wider frames
    wide0 = np.zeros((90, 150, 3), np.uint8)
    wide1 = np.zeros((90, 150, 3), np.uint8)
    wide0[:, 4:144], wide1[:, 4:144] = B0, B1
    strided = ctx.interpolate_bgr(wide0[:, 4:144], wide1[:, 4:144], times, *args, median=5,
                                  out_dtype=out_dtype)
    # a padded out_step, through the C ABI
    nt, es = len(times), np.dtype(out_dtype).itemsize
    step = 140 * 3 * es + 8 * es
    padded = np.full((nt, 90, step // es), 77, out_dtype)
    planes = (ctypes.c_void_p * nt)(*[padded[k].ctypes.data for k in range(nt)])
    rc = hs.lib().hsflow_flow_interp_bgr(
        ctx.handle, B0.ctypes.data, B1.ctypes.data, 90, 140, 420, 420, 3, 2, 5, 5, 20, 100.0,
        REL, ABS, _times(*times), nt, planes, hs.U8 if out_dtype == np.uint8 else hs.F32, step,
        None, 0, None)
    ctx.close()
    assert rc == 0
    assert h.dtype == out_dtype and h.shape == (4, 90, 140, 3)
    assert np.array_equal(h, out.cpu().numpy())
    assert np.array_equal(hf, flags.cpu().numpy())
    assert np.array_equal(hc.astype(np.int64), trusted.cpu().numpy()[0].astype(np.int64))
    assert np.array_equal(strided, h)
    assert np.array_equal(padded[:, :, :420].reshape(h.shape), h)
    assert np.all(padded[:, :, 420:] == 77)
    assert np.array_equal(h[0], B0) and np.array_equal(h[3], B1)


@pytest.mark.gpu
@pytest.mark.parametrize("alpha,k,t", E2E_CASES)
def test_end_to_end_against_reference(hs, alpha, k, t):
    """|out - ref| <= band G + 1e-4 x 255 over the interior, per channel
    (test_interp.test_end_to_end_against_reference's bound: band the flows' own
    tolerance in px, G the steepest slope of the channel's two frames), pixels
    with a target within `band` of a rim left out (at most 2 %); per channel the
    interior mean error is at most a quarter of the plain blend's."""
    import torch
    ref, _, rim, band = _e2e_ref(alpha, k, t)
    B0, B1 = _colour_pair(*E2E_PAIR)
    out, _, _ = hs.flow_interp_bgr_device(_cuda(B0), _cuda(B1), (t,), *SOLVE, alpha, median=k,
                                          flags=True, trusted=True)
    torch.cuda.synchronize()
    out = out[0].cpu().numpy()
    near = rim <= band
    assert near.mean() <= 0.02
    for c in range(3):
        G = max(float(np.abs(np.diff(a[..., c].astype(np.float64), axis=ax)).max())
                for a in (B0, B1) for ax in (0, 1))
        bound = band * G + TOL * 255.0
        d = np.abs(out[..., c].astype(np.float64) - ref[..., c])
        worst = float(_interior(np.where(near, 0.0, d)).max())
        print(f"alpha {alpha} median {k} t {t} channel {c}: worst interior |out - ref| "
              f"{worst:.3e} (bound {bound:.3e}: band {band:.2e} px, G {G:.0f}), near a rim "
              f"{near.mean():.4f}")
        assert worst <= bound
    _e2e_quality(out, t, "GPU")


@pytest.mark.gpu
def test_graph_capture_replays_the_eager_result(hs):
    """One capture and one replay of flow_interp_bgr_device at batch 1 on the
    capturing stream alone (no side streams, no parallel branches)."""
    import torch
    rows, cols, levels = 64, 96, 2
    B0, B1 = (_cuda(a) for a in _colour_pair(2080, rows, cols, -6, 9))
    times = (0.25, 0.5, 0.75)
    out = torch.empty((len(times), rows, cols, 3), dtype=torch.uint8, device="cuda")
    flags = torch.empty(out.shape[:-1], dtype=torch.uint8, device="cuda")
    trusted = torch.empty((1, len(times)), dtype=torch.int32, device="cuda")
    ws = torch.empty(hs.flow_interp_bgr_workspace_bytes(rows, cols, 1, levels), dtype=torch.uint8,
                     device="cuda")

    def solve(s):
        hs.flow_interp_bgr_device(B0, B1, times, levels, 2, 5, 20, 100.0, median=5, out=out,
                                  flags=flags, trusted=trusted, workspace=ws, stream=s)

    solve(torch.cuda.current_stream())
    torch.cuda.synchronize()
    ref = [t.clone() for t in (out, flags, trusted)]
    assert int(trusted.sum()) > 0
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, capture_error_mode="thread_local"):
        solve(torch.cuda.current_stream())
    torch.cuda.synchronize()
    for t in (out, flags, trusted):
        t.fill_(1)
    graph.replay()
    torch.cuda.synchronize()
    for t, want in zip((out, flags, trusted), ref):
        assert _same_bits(t, want)


@pytest.mark.gpu
def test_interpolate_sequence_doubles_the_frame_rate(hs, tmp_path):
    import frames
    rows, cols = 48, 64
    vid = np.stack([np.stack([texture(6000 + c, 0, rows, 2 * i, cols + 2 * i) for c in range(3)],
                             axis=-1) for i in range(3)]).astype(np.uint8)
    path = tmp_path / "clip.bgr"
    vid.tofile(path)
    src = frames.RawVideo(str(path), rows, cols)
    args = (3, 2, 5, 20, 100.0)
    ctx = hs.Context(0)
    got = list(frames.interpolate_sequence(src, 2, *args, median=5, context=ctx))
    mids = [ctx.interpolate_bgr(vid[i], vid[i + 1], 0.5, *args, median=5)[0] for i in range(2)]
    ctx.close()
    assert len(got) == 5
    for f in got:
        assert f.dtype == np.uint8 and f.shape == (rows, cols, 3)
    for i in range(3):
        assert np.array_equal(got[2 * i], vid[i])
    assert np.array_equal(got[1], mids[0]) and np.array_equal(got[3], mids[1])
    assert not np.array_equal(got[1], vid[0])
