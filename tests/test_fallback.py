"""Fallback for a failed pair (include/hsflow.h, "fallback for a failed pair";
DESIGN.md, "Fallback for a failed pair"): the verdict per pair from the
forward-backward check's counts, KF replacing a failed pair's frames, flags and
trusted counts, and the verdict carried through the fused calls, the context,
sequence mode and frames.interpolate_sequence.

fallback_np below restates the rule in integers and float32: the verdict is an
integer comparison, the values are selects of the source pixels or one fused
multiply-add, done here exactly (the product in float64, the sum rounded to
odd, one rounding to float32).  KF is held to it bit for bit, and to
hsflow_frame_interp_device at zero flow, which is where the rule comes from.

CPU tests: the threshold against exact arithmetic, argument errors (none of
which reaches the device), the surface, the C++ adapter, and the separation of
related from unrelated pairs in the float64 reference that lets the GPU tests
compare verdicts at all.  GPU tests are marked gpu.
"""
import ctypes
import fractions
import functools
import inspect
import math
import os
import shutil
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from synth_ref import synth_pair as np_synth
from test_consistency import _smooth_flows, consistency_np
from test_interp import (GUARD_B, GUARD_F, _cuda, _guards_intact, _placed, _same_bits, _textures,
                         _times)
from test_median import _occluder, warped_median_np

NEAREST, BLEND, FLAG = 1, 2, 32
MIN_SHARE = 0.4
# the cheap schedule of the verdict tests: levels, warps, window, iterations,
# alpha, median
CHEAP = (2, 1, 3, 20, 100.0, 3)
RELATED = {"square": ("occluder", 6), "40x56": (2001, 40, 56, -4, 8), "24x40": (21, 24, 40, 0, 4)}
UNRELATED = {"96x128": (2001, 2777, 96, 128), "40x56": (11, 12, 40, 56), "24x40": (21, 22, 24, 40)}
KINDS = ["u8", "f16", "f32", "f64", "bgr"]
BELOW_HALF = float(np.nextafter(np.float32(0.5), np.float32(0)))
TIMES = {1: (0.5,), 3: (0.0, BELOW_HALF, 1.0),
         16: (0.0, 0.5, 1.0, BELOW_HALF, 1 / 3, 0.25, 0.75, 0.1, 0.9, 2 / 3, 0.49, 0.51, 1e-3,
              0.999, 0.3, 0.7)}
# shape -> the number of times it runs with
KF_SHAPES = {(3, 1, 1): 16, (3, 3, 5): 3, (3, 37, 53): 16, (3, 64, 128): 1}
BIG_PLANE = (2044, 262657)  # 2^29 - 4 pixels, the library's cap


# ------------------------------------------------------------ the reference
def min_consistent_exact(rows, cols, min_share):
    share = fractions.Fraction(float(np.float32(min_share)))
    return math.ceil(share * 2 * rows * cols)


def _fma32(x, y, z):
    """fma(x, y, z) of float32 arrays, exactly: the product is exact in float64,
    the sum is rounded to odd there (TwoSum's error says which way), and the
    one rounding to float32 that follows is then the fused operation's."""
    p = x.astype(np.float64) * y.astype(np.float64)
    z = z.astype(np.float64)
    s = p + z
    b = s - p
    err = (p - (s - b)) + (z - b)
    bits = s.view(np.int64).copy()
    away = (err != 0) & ((err > 0) == (s > 0))
    back = (err != 0) & ~away
    bits[away] |= 1
    bits[back] = (bits[back] - 1) | 1
    return bits.view(np.float64).astype(np.float32)


def _round_u8(x):
    with np.errstate(invalid="ignore"):
        r = np.floor((x + np.float32(0.5)).astype(np.float32))
        return np.where(np.isnan(r), 0, np.clip(r, 0, 255)).astype(np.uint8)


def fallback_np(I0, I1, counts_f, counts_b, mode, min_share, times, dtype_out):
    """(out, cut) of frames [B, H, W] or [B, H, W, 3]: out [B, nt, H, W(, 3)] of
    dtype_out holds the fallback's pixels for every pair (the caller keeps them
    where cut[b] == 1); flags there are FLAG and trusted 0."""
    rows, cols = I0.shape[1:3]
    m = min_consistent_exact(rows, cols, min_share)
    cut = np.array([int(counts_f[b][0]) + int(counts_b[b][0]) < m for b in range(len(I0))],
                   np.uint8)
    a, c = np.asarray(I0).astype(np.float32), np.asarray(I1).astype(np.float32)
    planes = []
    for t in np.asarray(times, np.float32):
        if mode == NEAREST:
            o = a if t < np.float32(0.5) else c
        elif t == 0:
            o = a
        elif t == 1:
            o = c
        else:
            s = np.float32(1) - t
            o = _fma32(np.full(a.shape, s, np.float32), a, (t * c).astype(np.float32))
        planes.append(_round_u8(o) if dtype_out == np.uint8 else o)
    return np.stack(planes, axis=1), cut


def _unrelated(key):
    s0, s1, rows, cols = UNRELATED[key]
    return np_synth(s0, rows, cols, 0, 0)[0], np_synth(s1, rows, cols, 0, 0)[0]


def _related(key):
    pair = RELATED[key]
    return _occluder(pair[1]) if pair[0] == "occluder" else np_synth(*pair)


@functools.lru_cache(maxsize=None)
def _share_ref(kind, key):
    """The share of consistent pixels of a pair in the float64 reference, the
    cheap schedule, forward and backward together."""
    I0, I1 = _related(key) if kind == "related" else _unrelated(key)
    levels, warps, w, n, alpha, k = CHEAP
    uf, vf = warped_median_np(I0, I1, levels, warps, w, n, alpha, k)
    ub, vb = warped_median_np(I1, I0, levels, warps, w, n, alpha, k)
    good = int((consistency_np(uf, vf, ub, vb)[1] == 0).sum())
    good += int((consistency_np(ub, vb, uf, vf)[1] == 0).sum())
    return good / (2.0 * I0.size)


# ---------------------------------------------------------------- CPU tests
@pytest.mark.parametrize("share", [0.0, 1.0, 0.4, 0.5])
def test_min_consistent_is_the_exact_ceiling(share):
    import fallback
    for rows, cols in ((1, 1), (3, 5), (262140, 5), BIG_PLANE):
        assert fallback.min_consistent(rows, cols, share) == \
            min_consistent_exact(rows, cols, share), (rows, cols)
    assert BIG_PLANE[0] * BIG_PLANE[1] == (1 << 29) - 4
    assert fallback.min_consistent(*BIG_PLANE, 1.0) == (1 << 30) - 8
    assert fallback.min_consistent(7, 9, 0.0) == 0
    for rows, cols in ((0, 5), (5, 0), (262141, 1), (BIG_PLANE[0], BIG_PLANE[1] + 1)):
        assert fallback.min_consistent(rows, cols, share) == 0  # a bad size


def test_separation_in_the_reference():
    """What lets the GPU tests compare verdicts: in the float64 reference every
    related pair's share is at least 0.55 and every unrelated pair's at most
    0.25 under the cheap schedule, so each lies 0.15 or more from the default
    threshold -- far beyond the few pixels whose decision lies on a threshold
    of the check."""
    for key in RELATED:
        share = _share_ref("related", key)
        print("related", key, round(share, 3))
        assert share >= 0.55, (key, share)
        assert abs(share - MIN_SHARE) >= 0.15
    for key in UNRELATED:
        share = _share_ref("unrelated", key)
        print("unrelated", key, round(share, 3))
        assert share <= 0.25, (key, share)
        assert abs(share - MIN_SHARE) >= 0.15


def test_argument_errors_reach_no_device():
    """Every bad argument is HSFLOW_ERR_ARG with its text before any device
    work: the pointers below are made-up addresses."""
    import hsflow
    L = hsflow.lib()
    E = hsflow.HSFLOW_ERR_ARG
    A = [(k + 1) << 20 for k in range(10)]  # 1 MiB apart
    half = _times(0.5)
    nan = float("nan")

    def err():
        return L.hsflow_last_error(None).decode()

    def fb(mode=NEAREST, share=MIN_SHARE):
        return ctypes.byref(hsflow._CFallback(mode, share))

    def kf(I0=A[0], I1=A[1], cf=A[2], cb=A[3], f=None, times=half, nt=1, out=A[4],
           dtype_out=hsflow.F32, flags=A[5], trusted=A[6], cut=A[7], rows=16, dtype=hsflow.F32,
           bgr=False):
        f = fb() if f is None else f
        if bgr:
            return L.hsflow_frame_fallback_bgr_device(I0, I1, rows, 16, 1, cf, cb, f, times, nt, out,
                                                      dtype_out, flags, trusted, cut, None)
        return L.hsflow_frame_fallback_device(I0, I1, dtype, rows, 16, 1, cf, cb, f, times, nt,
                                              out, dtype_out, flags, trusted, cut, None)

    for bgr in (False, True):
        for null in ("I0", "I1", "cf", "cb", "out"):
            assert kf(**{null: None}, bgr=bgr) == E and "null" in err(), null
        assert kf(times=None, bgr=bgr) == E
        assert kf(f=fb(3), bgr=bgr) == E and "mode" in err()
        assert kf(f=fb(-1), bgr=bgr) == E and "mode" in err()
        # off is an error for KF alone, as mode 0 is for hsflow_prefilter_device
        assert kf(f=fb(0), bgr=bgr) == E and "fallback" in err()
        assert L.hsflow_frame_fallback_device(A[0], A[1], hsflow.F32, 16, 16, 1, A[2], A[3], None,
                                              half, 1, A[4], hsflow.F32, None, None, None,
                                              None) == E
        for bad in (nan, -0.1, 1.5, float("inf")):
            assert kf(f=fb(BLEND, bad), bgr=bgr) == E and "min_share" in err(), bad
        for nt in (0, 17):
            assert kf(times=_times(*([0.5] * 17)), nt=nt, bgr=bgr) == E and "nt" in err()
        assert kf(times=_times(1.5), bgr=bgr) == E and "time" in err()
        assert kf(rows=0, bgr=bgr) == E and kf(dtype_out=hsflow.F64, bgr=bgr) == E
        for over in (dict(out=A[0]), dict(out=A[1] + 100), dict(flags=A[4] + 1023),
                     dict(trusted=A[2] + 8), dict(cut=A[3] + 11), dict(cut=A[4]),
                     dict(flags=A[6]), dict(cut=A[6] + 3), dict(out=A[2] - 4)):
            assert kf(**over, bgr=bgr) == E and "overlap" in err(), over
    assert kf(dtype=7) == E

    big = 1 << 30

    def fused(bgr, f=None, cut=A[5], projection=0, wsb=big, out=A[2], nt=1, times=half,
              flags=A[3], trusted=A[4]):
        tail = (levels, 0, 1, 0, 5, 10, 1.0, 0.01, 0.5, times, nt, projection, out, hsflow.F32,
                flags, trusted, cut, None, None, None, f, 1 << 24, wsb, None)
        if bgr:
            return L.hsflow_flow_interp_bgr_fb_device(A[0], A[1], 16, 16, 1, *tail)
        return L.hsflow_flow_interp_fb_device(A[0], A[1], hsflow.F32, 16, 16, 1, *tail)

    levels = 3
    assert L.hsflow_fallback_counts_bytes(1) == 512 == L.hsflow_fallback_counts_bytes(21)
    assert L.hsflow_fallback_counts_bytes(22) == 1024
    assert L.hsflow_fallback_counts_bytes(0) == 0 == L.hsflow_fallback_counts_bytes(65536)
    for bgr in (False, True):
        stem = "hsflow_flow_interp_bgr" if bgr else "hsflow_flow_interp"
        plain = getattr(L, stem + "_workspace_bytes")(16, 16, 1, levels)
        proj = getattr(L, stem + "_pj_workspace_bytes")(16, 16, 1, levels, 1)
        assert fused(bgr, f=fb(3)) == E and "mode" in err()
        for bad in (nan, -0.1, 1.5):
            assert fused(bgr, f=fb(NEAREST, bad)) == E and "min_share" in err()
        # off needs the *_pj_ call's workspace only; on, the counts on top
        assert fused(bgr, wsb=plain - 1) == E and "workspace" in err()
        assert fused(bgr, f=fb(0), wsb=plain - 1) == E and "workspace" in err()
        assert fused(bgr, f=fb(), wsb=plain + 511) == E and "workspace" in err()
        assert fused(bgr, f=fb(), projection=1, wsb=proj + 511) == E and "workspace" in err()
        assert fused(bgr, f=fb(), out=None) == E
        assert fused(bgr, f=fb(), nt=0) == E and fused(bgr, f=fb(), nt=17) == E
        assert fused(bgr, f=fb(), cut=A[2] + 8) == E and "overlap" in err()
        assert fused(bgr, f=fb(), cut=(1 << 24) + plain + 100, wsb=plain + 512) == E
        assert "overlap" in err()
    assert L.hsflow_ctx_set_fallback(None, fb()) == E
    assert L.hsflow_ctx_fallback(None, fb()) == E
    assert L.hsflow_ctx_last_cut(None) == -1


def test_exports_and_python_surface():
    import fallback
    import frames
    import hsflow
    import temporal
    new = ("hsflow_fallback_min_consistent", "hsflow_frame_fallback_device",
           "hsflow_frame_fallback_bgr_device", "hsflow_fallback_counts_bytes",
           "hsflow_flow_interp_fb_device", "hsflow_flow_interp_bgr_fb_device",
           "hsflow_ctx_set_fallback", "hsflow_ctx_fallback", "hsflow_ctx_last_cut")
    with open(os.path.join(ROOT, "include", "hsflow.h")) as f:
        header = f.read()
    for name in new:
        assert name in hsflow.EXPORTS and hasattr(hsflow.lib(), name)
        assert name + "(" in header
    for line in ("#define HSFLOW_HAS_FALLBACK 1", "#define HSFLOW_FALLBACK_OFF 0",
                 "#define HSFLOW_FALLBACK_NEAREST 1", "#define HSFLOW_FALLBACK_BLEND 2",
                 "#define HSFLOW_FALLBACK_MIN_SHARE 0.4f", "#define HSFLOW_INTERP_FALLBACK 32",
                 "typedef struct hsflow_fallback { int mode; float min_share; } hsflow_fallback;"):
        assert line in header, line
    assert (fallback.FALLBACK_OFF, fallback.FALLBACK_NEAREST, fallback.FALLBACK_BLEND) == (0, 1, 2)
    assert fallback.FALLBACK_MIN_SHARE == MIN_SHARE and fallback.FLAG_FALLBACK == FLAG
    assert fallback.Fallback(BLEND) == (BLEND, MIN_SHARE)
    assert fallback.Fallback(NEAREST, 0.25) == (1, 0.25)
    for name in ("frame_fallback_device", "frame_fallback_bgr_device", "min_consistent",
                 "set_fallback", "get_fallback", "fallback_as", "last_cut", "counts_bytes"):
        assert callable(getattr(fallback, name))
    for name in ("flow_interp_device", "flow_interp_bgr_device"):
        for mod in (hsflow, temporal):
            sig = inspect.signature(getattr(mod, name)).parameters
            assert sig["fallback"].default is None and sig["cut"].default is None
    for name in ("interpolate", "interpolate_bgr"):
        assert inspect.signature(getattr(hsflow.Context, name)).parameters["fallback"].default \
            is None
    assert isinstance(hsflow.Context.last_cut, property)
    sig = inspect.signature(frames.interpolate_sequence).parameters
    assert sig["fallback"].default is None and sig["cuts"].default is None
    assert fallback.counts_bytes(3) == 512
    with open(os.path.join(ROOT, "cpp-optical-flow_amd", "frames.py")) as f:
        assert "scene cut is\n    two calls" not in f.read()


def test_setfallback_compiles_and_links(tmp_path):
    """A caller of the cv::Mat adapter's setFallback / fallback / lastCut (and of
    hsflow::Context's and hsflow::HornSchunck's) builds against
    include/hornSchunck.hpp, the cv::Mat test double and libhsflow.so; without a
    device the calls throw (never a crash)."""
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("no C++ compiler")
    src = tmp_path / "fallback_main.cpp"
    src.write_text(r'''
#include <cstdio>
#include "hornSchunck.hpp"
#if !defined(HSFLOW_HAS_FALLBACK) || HSFLOW_HAS_FALLBACK != 1 || HSFLOW_INTERP_FALLBACK != 32
#error "hsflow.h lacks the fallback"
#endif
int main() {
    hornSchunck hs(5, 10, 100.0);
    int thrown = 0, set = -1, back = -1, bad = 0, cut = -2;
    try {
        const hsflow::Fallback blend(HSFLOW_FALLBACK_BLEND, 0.5f);
        hs.setFallback(&blend);
        set = hs.fallback().mode;
        const hsflow::Fallback wrong(3);
        try { hs.setFallback(&wrong); } catch (const cv::Exception &) { bad = 1; }
        // a bad value leaves the old one
        if (hs.fallback().mode != HSFLOW_FALLBACK_BLEND || hs.fallback().min_share != 0.5f) return 4;
        hs.setFallback(nullptr);
        back = hs.fallback().mode;
        cut = hs.lastCut();
    } catch (const cv::Exception &) { ++thrown; }
    try {
        hsflow::Context c(0);
        const hsflow::Fallback nearest;
        c.setFallback(&nearest);
        if (c.fallback().mode != HSFLOW_FALLBACK_NEAREST || c.lastCut() != -1) return 3;
        if (c.fallback().min_share != HSFLOW_FALLBACK_MIN_SHARE) return 6;
        hsflow::HornSchunck h(5, 10, 100.0);
        h.setFallback(&nearest);
        if (h.fallback().mode != HSFLOW_FALLBACK_NEAREST || h.lastCut() != -1) return 5;
    } catch (const hsflow::Error &) { ++thrown; }
    int (*kf)(const void *, const void *, int, int, int, int, const uint32_t *, const uint32_t *,
              const hsflow_fallback *, const float *, int, void *, int, uint8_t *, uint32_t *,
              uint8_t *, void *) = hsflow_frame_fallback_device;
    std::printf("%d %d %d %d %d %d %d %zu\n", thrown, set, back, bad, cut,
                hsflow_ctx_set_fallback(nullptr, nullptr),
                kf(nullptr, nullptr, 1, 16, 16, 1, nullptr, nullptr, nullptr, nullptr, 1, nullptr,
                   1, nullptr, nullptr, nullptr, nullptr),
                (size_t)hsflow_fallback_min_consistent(3, 5, 0.5f));
    return 0;
}
''')
    lib_dir = os.path.join(ROOT, "cpp-optical-flow_amd")
    exe = str(tmp_path / "fallback_main")
    subprocess.check_call([gxx, "-std=c++17", "-Wall", "-Werror",
                           "-I", os.path.join(ROOT, "tests", "cpp", "cvstub"),
                           "-I", os.path.join(ROOT, "include"), str(src), "-o", exe, "-L", lib_dir,
                           "-lhsflow", "-Wl,-rpath," + lib_dir])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    thrown, set_, back, bad, cut, rc0, rc1, m = (int(x) for x in out.stdout.split())
    # 2 thrown where no gfx950 device is present
    assert (thrown, set_, back, bad, cut) in ((0, 2, 0, 1, -1), (2, -1, -1, 0, -2))
    assert (rc0, rc1, m) == (-1, -1, 15)


# ------------------------------------------------------------------ GPU tests
@functools.lru_cache(maxsize=None)
def _frames_of(shape, kind):
    """A shape's two batches of frames as the kind's arrays; bgr: [B, H, W, 3]."""
    if kind != "bgr":
        return _textures(shape, kind)
    I0, I1 = _textures(shape, "u8")
    bgr0 = np.ascontiguousarray(np.stack([I0, 255 - I1, I0[:, ::-1, :]], axis=-1))
    bgr1 = np.ascontiguousarray(np.stack([I1, 255 - I0, I1[:, ::-1, :]], axis=-1))
    return bgr0, bgr1


def _counts(rows, cols, verdicts, min_share=MIN_SHARE):
    """int32 [B, 3] counts each way whose sums say `verdicts` (1: cut) exactly
    at the threshold: m - 1 fails, m passes."""
    m = min_consistent_exact(rows, cols, min_share)
    cf = np.zeros((len(verdicts), 3), np.int32)
    cb = np.zeros((len(verdicts), 3), np.int32)
    for b, cut in enumerate(verdicts):
        total = m - 1 if cut else m
        cf[b] = (total // 2, 7, 3)
        cb[b] = (total - total // 2, 1, 9)
    return cf, cb


def _ki(hs, kind, t0, t1, flows, times, **kw):
    fn = hs.frame_interp_bgr_device if kind == "bgr" else hs.frame_interp_device
    return fn(t0, t1, *flows, times, **kw)


def _kf(kind, *args, **kw):
    import fallback
    fn = fallback.frame_fallback_bgr_device if kind == "bgr" else fallback.frame_fallback_device
    return fn(*args, **kw)


@pytest.mark.gpu
@pytest.mark.parametrize("mode", [NEAREST, BLEND], ids=["nearest", "blend"])
@pytest.mark.parametrize("u8_out", [False, True], ids=["f32out", "u8out"])
@pytest.mark.parametrize("kind", KINDS)
def test_kernel_against_reference_bitwise(hs, kind, u8_out, mode):
    """KF over KI's own result for smooth flows, batch 3 with verdicts (cut,
    pass, cut) at the boundary (m - 1 fails, m passes): the failed pairs equal
    fallback_np bit for bit with flags 32 and trusted 0, the passing pair keeps
    KI's bytes, cut is written for all, the guards around out and flags and the
    counts next to trusted and cut stay."""
    import fallback
    import torch
    ch = (3,) if kind == "bgr" else ()
    for shape, nt in KF_SHAPES.items():
        batch, rows, cols = shape
        times = TIMES[nt]
        I0, I1 = _frames_of(shape, kind)
        t0, t1 = _cuda(I0), _cuda(I1)
        flows = [_cuda(a) for a in _smooth_flows(batch, rows, cols)]
        odt = torch.uint8 if u8_out else torch.float32
        oshape = (batch, nt, rows, cols)
        fo, out, (o0, o1) = _placed(None, 4, odt, GUARD_B if u8_out else GUARD_F, oshape + ch)
        ff, flags, (f0, f1) = _placed(None, 4, torch.uint8, GUARD_B, oshape)
        trusted = torch.full((batch + 2, nt), -12345, dtype=torch.int32, device="cuda")
        cut = torch.full((batch + 2,), 77, dtype=torch.uint8, device="cuda")
        _ki(hs, kind, t0, t1, flows, times, out=out, flags=flags, trusted=trusted[1:-1])
        ki = [t.clone() for t in (out, flags, trusted)]
        cf, cb = _counts(rows, cols, (1, 0, 1))
        _kf(kind, t0, t1, _cuda(cf), _cuda(cb), fallback.Fallback(mode), times, out, flags=flags,
            trusted=trusted[1:-1], cut=cut[1:-1])
        torch.cuda.synchronize()
        want, want_cut = fallback_np(I0, I1, cf, cb, mode, MIN_SHARE, times,
                                     np.uint8 if u8_out else np.float32)
        assert want_cut.tolist() == [1, 0, 1] == cut[1:-1].tolist(), shape
        assert cut[0] == 77 and cut[-1] == 77
        got = out.cpu().numpy()
        view = np.uint8 if u8_out else np.uint32
        for b in (0, 2):
            assert np.array_equal(got[b].view(view), want[b].view(view)), (shape, b)
            assert bool((flags[b] == FLAG).all()) and bool((trusted[1 + b] == 0).all())
        assert _same_bits(out[1], ki[0][1]) and torch.equal(flags[1], ki[1][1])
        assert torch.equal(trusted[2], ki[2][2])
        assert bool((trusted[0] == -12345).all()) and bool((trusted[-1] == -12345).all())
        assert _guards_intact(fo, o0, o1, GUARD_B if u8_out else GUARD_F), shape
        assert _guards_intact(ff, f0, f1, GUARD_B), shape


@pytest.mark.gpu
def test_threshold_zero_never_fails_and_optional_outputs(hs):
    """min_share = 0 gives m = 0: counts of zero pass.  flags, trusted and cut
    may each be None; with all three None only out is written."""
    import fallback
    import torch
    shape = (2, 37, 53)
    I0, I1 = (_cuda(a) for a in _frames_of(shape, "u8"))
    zero = torch.zeros((2, 3), dtype=torch.int32, device="cuda")
    out = torch.full((2, 2, 37, 53), 9, dtype=torch.uint8, device="cuda")
    got = fallback.frame_fallback_device(I0, I1, zero, zero, fallback.Fallback(BLEND, 0.0),
                                         (0.25, 0.5), out, flags=True, trusted=True)
    torch.cuda.synchronize()
    assert bool((out == 9).all()) and got[3].tolist() == [0, 0]
    got = fallback.frame_fallback_device(I0, I1, zero, zero, fallback.Fallback(NEAREST, 1e-6),
                                         (0.25, 0.5), out, cut=None)
    torch.cuda.synchronize()
    assert got[1] is None and got[2] is None and got[3] is None
    assert torch.equal(out[:, 0], I0) and torch.equal(out[:, 1], I1)
    with pytest.raises(hs.HsflowError):
        fallback.frame_fallback_device(I0, I1, zero, zero, fallback.Fallback(NEAREST),
                                       (0.5,), None)


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["u8", "bgr"])
def test_unaligned_planes_give_the_same_bits(hs, kind):
    """u8 frames, output and flags 1 and 4 bytes past an aligned base (the quad
    stores take the byte path or the dword path): the bits of the aligned run."""
    import fallback
    import torch
    shape = (2, 37, 53)
    batch, rows, cols = shape
    ch = 3 if kind == "bgr" else 1
    I0, I1 = _frames_of(shape, kind)
    times = TIMES[3]
    cf, cb = (_cuda(a) for a in _counts(rows, cols, (1, 1)))
    n = batch * len(times) * rows * cols
    runs = []
    for off in (0, 1, 4):
        ins = []
        for a in (I0, I1):
            flat = torch.zeros(a.size + 64, dtype=torch.uint8, device="cuda")
            v = flat[off:off + a.size].view(a.shape)
            v.copy_(_cuda(a))
            ins.append(v)
        fo = torch.full((n * ch + 64,), GUARD_B, dtype=torch.uint8, device="cuda")
        ff = torch.full((n + 64,), GUARD_B, dtype=torch.uint8, device="cuda")
        out = fo[32 + off:32 + off + n * ch].view((batch, len(times), rows, cols) + (3,) * (ch == 3))
        flags = ff[32 + off:32 + off + n].view(batch, len(times), rows, cols)
        assert out.data_ptr() % 4 == off % 4
        _kf(kind, *ins, cf, cb, fallback.Fallback(BLEND), times, out, flags=flags)
        torch.cuda.synchronize()
        assert bool((fo[:32 + off] == GUARD_B).all()) and bool((fo[32 + off + n * ch:] == GUARD_B).all())
        assert bool((ff[:32 + off] == GUARD_B).all()) and bool((ff[32 + off + n:] == GUARD_B).all())
        runs.append((out.clone(), flags.clone()))
    want = fallback_np(I0, I1, [(0,)] * 2, [(0,)] * 2, BLEND, MIN_SHARE, times, np.uint8)[0]
    for out, flags in runs:
        assert np.array_equal(out.cpu().numpy(), want) and bool((flags == FLAG).all())


@pytest.mark.gpu
@pytest.mark.parametrize("kind", KINDS)
def test_failed_pair_equals_the_interpolation_at_zero_flow(hs, kind):
    """The yardstick: BLEND equals frame_interp_device on four all-zero flow
    planes with no masks at the same times, NEAREST equals that call at t = 0
    and t = 1, bit for bit, f32 and u8 output."""
    import fallback
    import torch
    shape = (3, 37, 53)
    batch, rows, cols = shape
    I0, I1 = _frames_of(shape, kind)
    t0, t1 = _cuda(I0), _cuda(I1)
    zero = [torch.zeros(shape, dtype=torch.float32, device="cuda")] * 4
    cf, cb = (_cuda(a) for a in _counts(rows, cols, (1, 1, 1)))
    times = TIMES[16]
    for odt in (torch.float32, torch.uint8):
        want = _ki(hs, kind, t0, t1, zero, times, out_dtype=odt)[0]
        ends = _ki(hs, kind, t0, t1, zero, (0.0, 1.0), out_dtype=odt)[0]
        got = _kf(kind, t0, t1, cf, cb, fallback.Fallback(BLEND), times, torch.empty_like(want))[0]
        near = _kf(kind, t0, t1, cf, cb, fallback.Fallback(NEAREST), times,
                   torch.empty_like(want))[0]
        torch.cuda.synchronize()
        assert _same_bits(got, want), odt
        for k, t in enumerate(np.asarray(times, np.float32)):
            assert _same_bits(near[:, k], ends[:, 0 if t < np.float32(0.5) else 1]), (odt, t)


def _verdict_batch(key):
    """A related and an unrelated pair of one size as a batch of two (f32)."""
    r0, r1 = _related(key)
    u0, u1 = _unrelated(key)
    return (np.stack([r0, u0]).astype(np.float32), np.stack([r1, u1]).astype(np.float32))


def _fused_args():
    levels, warps, w, n, alpha, k = CHEAP
    return (levels, warps, w, n, alpha), k


@pytest.mark.gpu
@pytest.mark.parametrize("projection", [0, 1])
@pytest.mark.parametrize("key", ["24x40", "40x56"])
def test_fused_call_equals_the_public_pieces_bitwise(hs, key, projection):
    """flow_interp_device(fallback=...) on a batch of a related and an unrelated
    pair = flow_bidir_device with counts, the interpolation, then
    frame_fallback_device: the related pair passes, the unrelated one fails.
    fallback None through the new entry point = the call without it, and cut
    is zeroed."""
    import fallback
    import projection as pj
    import torch
    I0, I1 = (_cuda(a) for a in _verdict_batch(key))
    args, k = _fused_args()
    times = (0.25, 0.5, 1.0)
    fb = fallback.Fallback(BLEND)
    r = hs.flow_bidir_device(I0, I1, *args, mask_f=True, mask_b=True, counts_f=True,
                             counts_b=True, median=k)
    if projection:
        cells = pj.project_device(I0, I1, r.uf, r.vf, r.ub, r.vb, times)
        want = pj.frame_interp_device(I0, I1, r.uf, r.vf, r.ub, r.vb, times, cells,
                                      mask_f=r.mask_f, mask_b=r.mask_b, flags=True, trusted=True)
    else:
        want = hs.frame_interp_device(I0, I1, r.uf, r.vf, r.ub, r.vb, times, mask_f=r.mask_f,
                                      mask_b=r.mask_b, flags=True, trusted=True)
    plain = [t.clone() for t in want]
    want = fallback.frame_fallback_device(I0, I1, r.counts_f, r.counts_b, fb, times, *want)
    got = hs.flow_interp_device(I0, I1, times, *args, median=k, flags=True, trusted=True,
                                projection=projection, fallback=fb, cut=True)
    bare = hs.flow_interp_device(I0, I1, times, *args, median=k, projection=projection,
                                 fallback=fb)
    torch.cuda.synchronize()
    rows, cols = I0.shape[1:]
    shares = (r.counts_f[:, 0] + r.counts_b[:, 0]).cpu().numpy() / (2.0 * rows * cols)
    print(key, "GPU shares", shares, "reference", _share_ref("related", key),
          _share_ref("unrelated", key))
    assert got[3].tolist() == [0, 1] == want[3].tolist()
    assert _same_bits(got[0], want[0]) and torch.equal(got[1], want[1])
    assert torch.equal(got[2], want[2]) and len(bare) == 3 and _same_bits(bare[0], want[0])
    assert bool((got[1][1] == FLAG).all()) and got[2][1].tolist() == [0, 0, 0]
    assert _same_bits(got[0][0], plain[0][0]) and int(got[2][0].sum()) > 0
    # off: the *_pj_ call's launches and bits, cut zeroed
    cut = torch.full((2,), 5, dtype=torch.uint8, device="cuda")
    off = hs.flow_interp_device(I0, I1, times, *args, median=k, flags=True, trusted=True,
                                projection=projection, cut=cut)
    old = hs.flow_interp_device(I0, I1, times, *args, median=k, flags=True, trusted=True,
                                projection=projection)
    torch.cuda.synchronize()
    assert cut.tolist() == [0, 0] and off[3] is cut
    for a, b, c in zip(off, old, plain):
        assert _same_bits(a, b) and _same_bits(a, c)


@pytest.mark.gpu
def test_fused_bgr_call_equals_the_public_pieces_bitwise(hs):
    import fallback
    import torch
    g0, g1 = _verdict_batch("24x40")
    bgr0, bgr1 = (_cuda(np.ascontiguousarray(np.stack([g, 255 - g, g[:, ::-1]], axis=-1)
                                             .astype(np.uint8))) for g in (g0, g1))
    args, k = _fused_args()
    times = (BELOW_HALF, 0.5)
    fb = fallback.Fallback(NEAREST)
    y0, y1 = hs.bgr_to_gray_device(bgr0), hs.bgr_to_gray_device(bgr1)
    r = hs.flow_bidir_device(y0, y1, *args, mask_f=True, mask_b=True, counts_f=True,
                             counts_b=True, median=k)
    want = hs.frame_interp_bgr_device(bgr0, bgr1, r.uf, r.vf, r.ub, r.vb, times, mask_f=r.mask_f,
                                      mask_b=r.mask_b, out_dtype=torch.uint8, flags=True,
                                      trusted=True)
    want = fallback.frame_fallback_bgr_device(bgr0, bgr1, r.counts_f, r.counts_b, fb, times, *want)
    got = hs.flow_interp_bgr_device(bgr0, bgr1, times, *args, median=k, out_dtype=torch.uint8,
                                    flags=True, trusted=True, fallback=fb, cut=True)
    torch.cuda.synchronize()
    assert got[3].tolist() == [0, 1]
    for a, b in zip(got, want):
        assert torch.equal(a, b)
    assert torch.equal(got[0][1, 0], bgr0[1]) and torch.equal(got[0][1, 1], bgr1[1])


@pytest.mark.gpu
def test_host_calls_equal_device_calls_and_report_the_verdict(hs):
    """Context.interpolate / interpolate_bgr with the fallback: the device
    call's bits, last_cut True for an unrelated pair and then False for a
    related one, None with the fallback off; the setting round-trips, a bad one
    keeps the old."""
    import fallback
    import torch
    args, k = _fused_args()
    times = (0.25, 0.75)
    fb = fallback.Fallback(BLEND)
    pairs = {"cut": _unrelated("24x40"), "ok": _related("24x40")}
    dev = {}
    for name, (I0, I1) in pairs.items():
        dev[name] = hs.flow_interp_device(_cuda(I0), _cuda(I1), times, *args, median=k,
                                          flags=True, trusted=True, fallback=fb, cut=True)
    torch.cuda.synchronize()
    assert dev["cut"][3].tolist() == [1] and dev["ok"][3].tolist() == [0]
    with hs.Context(0) as ctx:
        assert fallback.get_fallback(ctx) is None and ctx.last_cut is None
        for name, want in (("cut", True), ("ok", False)):
            I0, I1 = pairs[name]
            h, hf, hc = ctx.interpolate(I0, I1, times, *args, median=k, with_flags=True,
                                        fallback=fb)
            assert ctx.last_cut is want and fallback.last_cut(ctx) is want
            assert fallback.get_fallback(ctx) is None  # restored
            out, flags, trusted, _ = dev[name]
            assert np.array_equal(h, out.cpu().numpy()) and np.array_equal(hf, flags.cpu().numpy())
            assert np.array_equal(hc.astype(np.int64), trusted.cpu().numpy()[0].astype(np.int64))
        assert bool((hf == 0).any())
        ctx.interpolate(*pairs["cut"], times, *args, median=k)
        assert ctx.last_cut is None  # the fallback is off
        fallback.set_fallback(ctx, fb)
        got = fallback.get_fallback(ctx)
        assert got == (BLEND, float(np.float32(MIN_SHARE)))
        for bad in ((3, 0.4), (NEAREST, float("nan")), (NEAREST, -0.1), (BLEND, 1.5)):
            with pytest.raises(hs.HsflowError, match="fallback"):
                fallback.set_fallback(ctx, bad)
            assert fallback.get_fallback(ctx) == got
        g = pairs["cut"]
        bgr = [np.ascontiguousarray(np.stack([a, 255 - a, a[::-1]], axis=-1).astype(np.uint8))
               for a in g]
        hb = ctx.interpolate_bgr(*bgr, (0.25, 0.5), *args, median=k)
        assert ctx.last_cut is True
        assert np.array_equal(hb[0], _round_u8(_fma32(
            np.full(bgr[0].shape, 0.75, np.float32), bgr[0].astype(np.float32),
            (np.float32(0.25) * bgr[1].astype(np.float32)))))
        with fallback.fallback_as(ctx, None):
            assert fallback.get_fallback(ctx) == got
        with fallback.fallback_as(ctx, (NEAREST, 0.0)):
            assert fallback.get_fallback(ctx) == (NEAREST, 0.0)
        fallback.set_fallback(ctx, None)
        assert fallback.get_fallback(ctx) is None


@pytest.mark.gpu
def test_graph_capture_and_side_streams(hs):
    """One capture and replay of flow_interp_device(fallback=...) on the origin
    stream, an eager call on a side stream first: the counts, KF and the
    verdict are stream-ordered and allocate nothing."""
    import fallback
    import torch
    I0, I1 = (_cuda(a) for a in _verdict_batch("24x40"))
    args, k = _fused_args()
    times = (0.25, 0.5, 0.75)
    fb = fallback.Fallback(NEAREST)
    out = torch.empty((2, 3, 24, 40), dtype=torch.float32, device="cuda")
    flags = torch.empty(out.shape, dtype=torch.uint8, device="cuda")
    trusted = torch.empty((2, 3), dtype=torch.int32, device="cuda")
    cut = torch.empty((2,), dtype=torch.uint8, device="cuda")
    ws = torch.empty(hs.flow_interp_workspace_bytes(24, 40, 2, args[0]) + fallback.counts_bytes(2),
                     dtype=torch.uint8, device="cuda")

    def solve(s):
        hs.flow_interp_device(I0, I1, times, *args, median=k, out=out, flags=flags,
                              trusted=trusted, workspace=ws, stream=s, fallback=fb, cut=cut)

    stream = torch.cuda.current_stream()
    side = torch.cuda.Stream()
    side.wait_stream(stream)
    with torch.cuda.stream(side):
        solve(side)
    stream.wait_stream(side)
    torch.cuda.synchronize()
    ref = [t.clone() for t in (out, flags, trusted, cut)]
    assert cut.tolist() == [0, 1]
    solve(None)  # the null stream: the same bits
    torch.cuda.synchronize()
    for t, want in zip((out, flags, trusted, cut), ref):
        assert _same_bits(t, want)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, capture_error_mode="thread_local"):
        solve(torch.cuda.current_stream())
    torch.cuda.synchronize()
    for t in (out, flags, trusted, cut):
        t.fill_(3)
    ws.fill_(0xFF)  # stale counts of all ones would pass every pair
    graph.replay()
    torch.cuda.synchronize()
    for t, want in zip((out, flags, trusted, cut), ref):
        assert _same_bits(t, want)


def _clip_pairs():
    """Two related pairs, a cut pair, a related pair: five frames of 24 x 40."""
    a = [np_synth(21, 24, 40, 0, 4 * j)[1] for j in range(3)]   # one texture shifting
    b = [np_synth(22, 24, 40, 0, 4 * j)[1] for j in range(2)]   # another
    return a + b


@pytest.mark.gpu
def test_sequence_mode_drops_the_prediction_at_a_cut(hs):
    """In sequence mode with the fallback the call after a cut pair is the cold
    call bit for bit; without the fallback it is the warm call, as before."""
    import fallback
    import temporal
    frames = _clip_pairs()
    args, k = _fused_args()
    times = (0.5,)
    fb = fallback.Fallback(NEAREST)
    with hs.Context(0) as ctx:
        cold = ctx.interpolate(frames[3], frames[4], times, *args, median=k, with_flags=True)
        for setting, verdicts in ((fb, [False, False, True, False]), (None, [None] * 4)):
            got = []
            with temporal.sequence(ctx):
                for i in range(4):
                    got.append(ctx.interpolate(frames[i], frames[i + 1], times, *args, median=k,
                                               with_flags=True, fallback=setting))
                    assert ctx.last_cut is verdicts[i], (i, setting)
            if setting is not None:
                assert np.array_equal(got[2][0][0], frames[3]) and bool((got[2][1] == FLAG).all())
                for a, b in zip(got[3], cold):
                    assert np.array_equal(a, b)
                with_fb = got
            else:
                # the prediction crosses the cut: the fourth call starts warm
                assert not np.array_equal(got[3][0], cold[0])
                # ... and up to the cut the fallback changes nothing
                for i in range(2):
                    for a, b in zip(got[i], with_fb[i]):
                        assert np.array_equal(a, b)


class _Clip:
    def __init__(self, frames):
        self.frames = frames

    def __len__(self):
        return len(self.frames)

    def read(self, i):
        return self.frames[i]


@pytest.mark.gpu
def test_interpolate_sequence_emits_source_frames_across_a_cut(hs):
    """Six BGR frames, three of one texture shifting and three of another, at
    three times the rate with NEAREST: the two frames inside the cut pair are
    frames 2 and 3, cuts == [3], every other frame is the run without."""
    import fallback
    import frames as fr
    grey = [np_synth(21, 24, 40, 0, 4 * j)[1] for j in range(3)]
    grey += [np_synth(22, 24, 40, 0, 4 * j)[1] for j in range(3)]
    clip = _Clip([np.ascontiguousarray(np.stack([g, 255 - g, g[::-1]], axis=-1).astype(np.uint8))
                  for g in grey])
    levels, warps, w, n, alpha, k = CHEAP
    with hs.Context(0) as ctx:
        plain = list(fr.interpolate_sequence(clip, 3, levels, warps, w, n, alpha, median=k,
                                             context=ctx))
        cuts = []
        got = list(fr.interpolate_sequence(clip, 3, levels, warps, w, n, alpha, median=k,
                                           context=ctx, fallback=fallback.Fallback(NEAREST),
                                           cuts=cuts))
        assert fallback.get_fallback(ctx) is None
    assert cuts == [3] and len(got) == len(plain) == 16
    assert np.array_equal(got[7], clip.read(2)) and np.array_equal(got[8], clip.read(3))
    assert not np.array_equal(plain[7], clip.read(2))
    for j in range(16):
        if j not in (7, 8):
            assert np.array_equal(got[j], plain[j]), j
