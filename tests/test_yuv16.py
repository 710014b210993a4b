"""16-bit-sample YUV 4:2:0 frame interpolation (include/hsflow.h, "16-bit YUV
4:2:0"; yuv.py, frames.Y4MVideo16): yuv420p10le .. p16le and P010 .. P016.

A 16-bit sample is its value, 0 .. 65535.  Every kernel converts a frame element
to float on load, so a U16 plane gives, bit for bit, what the same values give
as a float32 plane in the existing calls -- the pyramid included, because every
pair here holds a sample above 255 (a U16 pair is never treated as 8-bit, and a
float32 pair with such a sample is not either).  A U16 output is floor(x + 0.5)
clamped to 0 .. 65535, NaN -> 0, of the float32 output x.  So every GPU test is
a bit equality against the existing public pieces on float32 planes, with no
tolerance and no excluded pixel.

Sample values are drawn over the whole of 0 .. 65535 and 0, 255, 256, 32768 and
65535 are planted: a byte truncation or a sign extension cannot pass.

Quality (float64 reference, printed by the test): the quality pair of test_yuv
times 4 plus a 2-bit dither is 10-bit content; at QUALITY_SOLVE with alpha x 4
the middle frame's interior chroma error is 1.20 (U), 1.25 (V) 10-bit levels
against 53.1 and 44.6 for the plain blend, 0.023 and 0.028 of it -- the 8-bit
figure is 0.02; the bound is 0.1.
"""
import ctypes
import functools
import os
import shutil
import subprocess

import numpy as np
import pytest

import yuv  # noqa: F401  (the module under test)
from conftest import ROOT
from test_consistency import _smooth_flows
from test_fallback import BLEND, CHEAP, MIN_SHARE, NEAREST
from test_interp import _cuda, _guards_intact, _placed, _times
from test_temporal import HOSTILE, _init_for
from test_yuv import (I420, LAYOUT_IDS, LAYOUTS, NV12, QUALITY, QUALITY_SOLVE, SHAPE_IDS, SHAPES,
                      TIMES, _as_layout, _chroma_errors, _luma_batch, _quality_pair, _third_frame,
                      chroma_interp_np)
from test_yuv import _flows_ref  # noqa: F401  (the float64 solve of the quality test)

SPECIAL = (0, 255, 256, 32768, 65535)
GUARD_I16, GUARD_F32 = 0x6B6B, -7.25
# the fused tests' schedule: test_fallback's cheap one on three levels, so that
# the unrounded pyramid is exercised; the luma is scaled by LUMA_GAIN, and so is
# alpha (a frame scaled by k behaves like alpha / k)
LUMA_GAIN = 200
LEVELS3 = (3,) + CHEAP[1:4] + (CHEAP[4] * LUMA_GAIN, CHEAP[5])


# ------------------------------------------------------------------ helpers
@functools.lru_cache(maxsize=None)
def _chroma16_np(shape, which):
    """A shape's chroma as I420 uint16 [B, 2, rc, cc]: values over the whole
    range with SPECIAL planted, and 65535 in every pair."""
    batch, rows, cols = shape
    rng = np.random.default_rng(1600 + which + 1000 * batch + 10 * rows + cols)
    a = rng.integers(0, 65536, (batch, 2, rows // 2, cols // 2)).astype(np.uint16)
    flat = a.reshape(batch, -1)
    if flat.shape[1] >= 4 * len(SPECIAL):
        at = rng.choice(flat.shape[1], len(SPECIAL), replace=False)
        flat[:, at] = SPECIAL
    flat[:, 0] = 65535 if which == 0 else 256
    a.setflags(write=False)
    return a


def _t16(a):
    """A numpy uint16 array as a CUDA uint16 tensor."""
    import torch
    return torch.from_numpy(np.array(a, np.uint16, order="C")).cuda()


def _f32(a):
    return _cuda(np.asarray(a).astype(np.float32))


def _np16(t):
    """The 16 bits of a uint16 / int16 tensor as numpy uint16."""
    import torch
    return t.contiguous().view(torch.int16).cpu().numpy().view(np.uint16)


def _round16(x):
    """floor(x + 0.5) clamped to 0 .. 65535, NaN -> 0, of a float32 CUDA tensor:
    numpy uint16."""
    import torch
    assert x.dtype == torch.float32
    r = torch.floor(x + np.float32(0.5))
    r = torch.where(torch.isnan(r), torch.zeros_like(r), r).clamp(0.0, 65535.0)
    return r.cpu().numpy().astype(np.int64).astype(np.uint16)


def _bits32(t):
    import torch
    return t.contiguous().view(torch.int32).cpu().numpy()


def _matches(got, want_f32, u16):
    """got (the 16-bit call's output) against the float32 pieces' output."""
    if u16:
        return np.array_equal(_np16(got), _round16(want_f32))
    return np.array_equal(_bits32(got), _bits32(want_f32))


def _out_dtype(u16):
    import torch
    return torch.uint16 if u16 else torch.float32


def _pieces(hs, c0, c1, flows, times, cells=None, fb=None, counts=None):
    """The definition on the GPU, on float32 planes with float32 out:
    downflow_device of both flow pairs, then frame_interp_device (with `cells`:
    cells_down_device and projection.frame_interp_device) on the U and on the V
    planes, and where `fb` is given frame_fallback_device over each plane's
    result.  c0, c1: numpy I420 uint16 [B, 2, rc, cc]; returns float32 I420
    [B, nt, 2, rc, cc]."""
    import fallback
    import projection
    import temporal
    import torch
    uf, vf, ub, vb = flows
    df = temporal.downflow_device(uf, vf) + temporal.downflow_device(ub, vb)
    cc = yuv.cells_down_device(cells) if cells is not None else None
    planes = []
    for ch in range(2):
        p0, p1 = _f32(c0[:, ch]), _f32(c1[:, ch])
        if cc is None:
            out = hs.frame_interp_device(p0, p1, *df, times, out_dtype=torch.float32)[0]
        else:
            out = projection.frame_interp_device(p0, p1, *df, times, cc,
                                                 out_dtype=torch.float32)[0]
        if fb is not None:
            out = fallback.frame_fallback_device(p0, p1, counts[0], counts[1], fb, times, out,
                                                 cut=None)[0]
        planes.append(out)
    return torch.stack(planes, dim=2)


def _inputs(shape):
    flows = [_cuda(a) for a in _smooth_flows(*shape)]
    return _chroma16_np(shape, 0), _chroma16_np(shape, 1), flows


def _luma16_batch():
    """test_yuv's related and unrelated luma pair times LUMA_GAIN with a dither,
    65535 planted in every frame, and 16-bit chroma for them: numpy uint16."""
    y0, y1, _, _ = _luma_batch()
    rng = np.random.default_rng(77)
    out = []
    for y in (y0, y1):
        a = y.astype(np.int64) * LUMA_GAIN + rng.integers(0, LUMA_GAIN, y.shape)
        a[:, 0, 0] = 65535
        assert a.max() == 65535 and a.min() >= 0
        out.append(a.astype(np.uint16))
    return out[0], out[1], _chroma16_np((2, 24, 40), 0), _chroma16_np((2, 24, 40), 1)


# ------------------------------------------------------------------ CPU tests
def test_exports_and_python_surface():
    import inspect

    import frames
    import hsflow
    new = ("hsflow_chroma_interp16_device", "hsflow_flow_interp_yuv16_device",
           "hsflow_flow_interp_yuv16")
    with open(os.path.join(ROOT, "include", "hsflow.h")) as f:
        header = f.read()
    for name in new:
        assert name in hsflow.EXPORTS and hasattr(hsflow.lib(), name)
        assert name + "(" in header
    assert "#define HSFLOW_HAS_YUV16 1" in header and "HSFLOW_U16 = 4" in header
    assert "never treated as 8-bit" in header and "P016" in header
    assert yuv.U16 == 4
    assert callable(frames.Y4MVideo16)
    assert "depth" in inspect.signature(frames.write_y4m_420).parameters
    assert inspect.signature(frames.write_y4m_420).parameters["depth"].default == 8
    for fn in (yuv.chroma_interp_device, yuv.chroma_interp_proj_device, yuv.flow_interp_yuv_device,
               yuv.flow_interp_yuv_proj_device, yuv.interpolate_yuv,
               frames.interpolate_sequence_yuv):
        assert "16" in fn.__doc__
    assert "alpha" in frames.interpolate_sequence_yuv.__doc__


def test_argument_errors_reach_no_device():
    """Every bad argument of the three 16-bit calls is HSFLOW_ERR_ARG with its
    text before any device work: the pointers below are made-up addresses."""
    import hsflow
    L = hsflow.lib()
    E = hsflow.HSFLOW_ERR_ARG
    A = [(k + 1) << 20 for k in range(16)]  # 1 MiB apart
    half = _times(0.5)

    def err():
        return L.hsflow_last_error(None).decode()

    def fb(mode=NEAREST, share=MIN_SHARE):
        return ctypes.byref(hsflow._CFallback(mode, share))

    def kiy(c0=A[0], c1=A[1], layout=I420, rows=16, cols=16, batch=1, uf=A[2], vf=A[3], ub=A[4],
            vb=A[5], cells=None, cf=None, cb=None, f=None, times=half, nt=1, out=A[6],
            dtype_out=yuv.U16):
        return L.hsflow_chroma_interp16_device(c0, c1, layout, rows, cols, batch, uf, vf, ub, vb,
                                               cells, cf, cb, f, times, nt, out, dtype_out, None)

    for null in ("c0", "c1", "uf", "vf", "ub", "vb", "out"):
        assert kiy(**{null: None}) == E and "null" in err(), null
    assert kiy(times=None) == E
    for odd in (dict(rows=15), dict(cols=17), dict(rows=1, cols=2)):
        assert kiy(**odd) == E and "even" in err(), odd
    assert kiy(rows=0) == E and kiy(batch=0) == E
    for lay in (0, 3, -1):
        assert kiy(layout=lay) == E and "layout" in err(), lay
    for nt in (0, 17):
        assert kiy(times=_times(*([0.5] * 17)), nt=nt) == E and "nt" in err()
    for t in (1.5, -0.1, float("nan")):
        assert kiy(times=_times(t)) == E and "time" in err()
    for code in (hsflow.U8, hsflow.F64, hsflow.F16, 9):
        assert kiy(dtype_out=code) == E and "U16 or F32" in err(), code
    assert kiy(cells=A[9] + 4) == E and "8-byte" in err()
    assert kiy(f=fb(3), cf=A[7], cb=A[8]) == E and "mode" in err()
    assert kiy(f=fb(BLEND, 1.5), cf=A[7], cb=A[8]) == E and "min_share" in err()
    assert kiy(f=fb(), cf=None, cb=A[8]) == E and "null" in err()
    # 16 x 16: chroma 256 bytes per frame, flows 1024, the output 256 (u16),
    # cells 2048
    for over in (dict(out=A[0]), dict(out=A[0] + 255), dict(out=A[1] - 255), dict(out=A[2] + 1023),
                 dict(out=A[5] - 200), dict(out=A[3]), dict(out=A[9] + 2047, cells=A[9])):
        assert kiy(**over) == E and "overlap" in err(), over
    assert kiy(out=A[7] + 11, f=fb(), cf=A[7], cb=A[8]) == E and "overlap" in err()
    # f32 output: 512 bytes
    assert kiy(out=A[1] - 511, dtype_out=hsflow.F32) == E and "overlap" in err()

    ws, big, levels = 1 << 28, 1 << 30, 3

    def fused(y0=A[0], c0=A[1], y1=A[2], c1=A[3], layout=NV12, rows=16, cols=16, times=half, nt=1,
              proj=0, out_y=A[4], out_c=A[5], dtype_out=yuv.U16, flags=A[6], trusted=A[7],
              cut=A[8], f=None, wsb=big, levels=levels, finest=0, init=None):
        return L.hsflow_flow_interp_yuv16_device(y0, c0, y1, c1, layout, rows, cols, 1, levels,
                                                 finest, 1, 0, 5, 10, 1.0, 0.01, 0.5, times, nt,
                                                 proj, out_y, out_c, dtype_out, flags, trusted,
                                                 cut, None, None, init, f, ws, wsb, None)

    for null in ("y0", "c0", "y1", "c1", "out_y", "out_c"):
        assert fused(**{null: None}) == E and "null" in err(), null
    assert fused(rows=15) == E and "even" in err()
    assert fused(cols=7) == E and "even" in err()
    for lay in (0, 3):
        assert fused(layout=lay) == E and "layout" in err()
    assert fused(nt=0) == E and fused(nt=17, times=_times(*([0.5] * 17))) == E and "nt" in err()
    assert fused(times=_times(2.0)) == E and "time" in err()
    for p in (2, -1):
        assert fused(proj=p) == E and "projection" in err()
    for code in (hsflow.U8, hsflow.F64, 9):
        assert fused(dtype_out=code) == E and "U16 or F32" in err()
    assert fused(f=fb(3)) == E and "mode" in err()
    assert fused(levels=0) == E and "levels" in err()
    assert fused(finest=3) == E and "finest" in err()
    plain = L.hsflow_flow_interp_yuv_pj_workspace_bytes(16, 16, 1, levels, 1, 0, 0)
    with_cells = L.hsflow_flow_interp_yuv_pj_workspace_bytes(16, 16, 1, levels, 1, 1, 0)
    assert 0 < plain < with_cells
    assert fused(wsb=plain - 1) == E and "workspace" in err()
    assert fused(proj=1, wsb=with_cells - 1) == E and "workspace" in err()
    assert fused(f=fb(), wsb=plain + 511) == E and "workspace" in err()
    # luma 512 bytes, chroma 256, out_y 512, out_c 256
    for over in (dict(out_c=A[0] + 511), dict(out_c=A[1]), dict(out_c=A[3] + 255),
                 dict(out_c=A[4] + 511), dict(out_y=A[5] - 511), dict(out_y=A[1] + 200),
                 dict(out_y=A[3] - 400), dict(flags=A[5] + 128), dict(trusted=A[5] + 252),
                 dict(cut=A[5] + 255), dict(out_c=ws + 100), dict(out_c=ws + plain - 1),
                 dict(flags=A[1] + 1), dict(cut=A[3])):
        assert fused(**over) == E and "overlap" in err(), over
    start = hsflow._CFlowInit(A[5] - 1000, A[10], None, None)
    assert fused(init=ctypes.byref(start)) == E and "init" in err()

    # the host call: its own checks come before the context
    def host(f0=A[0], f1=A[1], layout=I420, rows=16, cols=16, times=half, nt=1, proj=0, out=None,
             dtype_out=yuv.U16, levels=levels):
        planes = (ctypes.c_void_p * 1)(A[2]) if out is None else out
        return L.hsflow_flow_interp_yuv16(None, f0, f1, layout, rows, cols, levels, 1, 0, 5, 10,
                                          1.0, 0.01, 0.5, times, nt, proj, planes, dtype_out, None,
                                          None)

    assert host(f0=None) == E and host(f1=None) == E
    assert host(rows=15) == E and "even" in err()
    assert host(layout=0) == E and "layout" in err()
    assert host(nt=0) == E and host(times=_times(1.5)) == E
    for code in (hsflow.U8, hsflow.F64):
        assert host(dtype_out=code) == E and "U16 or F32" in err()
    assert host(proj=2) == E and "projection" in err()
    assert host(proj=-1) == E and "projection" in err()
    assert host(out=(ctypes.c_void_p * 1)(None)) == E and "plane" in err()
    assert host(levels=9) == E and "levels" in err()
    assert host() == E and "context" in err()


def test_existing_entry_points_still_refuse_u16():
    """Code 4 enters through the 16-bit calls only: the grey calls refuse it as
    input and as output with the text they have for any unknown code."""
    import hsflow
    L = hsflow.lib()
    E = hsflow.HSFLOW_ERR_ARG
    A = [(k + 1) << 20 for k in range(16)]
    half = _times(0.5)

    def err():
        return L.hsflow_last_error(None).decode()

    def ki(dtype_in=hsflow.U8, dtype_out=hsflow.U8):
        return L.hsflow_frame_interp_device(A[0], A[1], dtype_in, 16, 16, 1, A[2], A[3], A[4], A[5],
                                            None, None, half, 1, A[6], dtype_out, None, None, None)

    def fused(dtype_in=hsflow.U8, dtype_out=hsflow.U8):
        return L.hsflow_flow_interp_fb_device(A[0], A[1], dtype_in, 16, 16, 1, 2, 0, 1, 0, 5, 10,
                                              1.0, 0.01, 0.5, half, 1, 0, A[6], dtype_out, None,
                                              None, None, None, None, None, None, 1 << 28, 1 << 30,
                                              None)

    for call in (ki, fused):
        assert call(dtype_in=9) == E
        text9 = err()
        assert "dtype" in text9
        assert call(dtype_in=yuv.U16) == E and err() == text9
        assert call(dtype_out=9) == E
        out9 = err()
        assert call(dtype_out=yuv.U16) == E and err() == out9 and "U8 or F32" in out9
    # the 8-bit YUV calls too, and a host solve
    assert L.hsflow_chroma_interp_device(A[0], A[1], I420, 16, 16, 1, A[2], A[3], A[4], A[5], None,
                                         None, None, half, 1, A[6], yuv.U16, None) == E
    assert "U8 or F32" in err()
    with pytest.raises(hsflow.HsflowError):
        hsflow._dtype_code(np.zeros((4, 4), np.uint16))


def test_y4m16_round_trip(tmp_path):
    import frames
    rng = np.random.default_rng(16)
    rows, cols = 6, 10
    n = yuv.frame_bytes(rows, cols)
    clip = [rng.integers(0, 1024, n).astype(np.uint16) for _ in range(3)]
    clip[0][:5] = (0, 255, 256, 512, 1023)
    path = str(tmp_path / "clip10.y4m")
    frames.write_y4m_420(path, clip, rows, cols, depth=10)
    with open(path, "rb") as f:
        assert b" C420p10" in f.readline()
    src = frames.Y4MVideo16(path)
    assert len(src) == 3 and (src.rows, src.cols, src.bit_depth) == (rows, cols, 10)
    for k, fr in enumerate(clip):
        got = src.read_yuv(k)
        assert got.dtype == np.uint16 and np.array_equal(got, fr)
    with pytest.raises(frames.FrameError):
        src.read_yuv(3)
    # little-endian 2-byte samples behind the frame header
    raw = open(path, "rb").read()
    first = raw.index(b"FRAME\n") + 6
    assert raw[first:first + 10] == clip[0][:5].astype("<u2").tobytes()
    for depth in (12, 14, 16):
        p = str(tmp_path / f"clip{depth}.y4m")
        wide = [(c.astype(np.uint32) << (depth - 10)).astype(np.uint16) for c in clip]
        frames.write_y4m_420(p, wide, rows, cols, depth=depth, full_range=True)
        s = frames.Y4MVideo16(p)
        assert s.bit_depth == depth and s.full_range and np.array_equal(s.read_yuv(2), wide[2])
    # the 8-bit readers keep refusing the high-bit-depth tags, and the other way
    with pytest.raises(frames.FrameError):
        frames.Y4MVideo(path)
    with pytest.raises(frames.FrameError):
        frames.open_source(path)
    clip8 = [rng.integers(0, 256, n).astype(np.uint8) for _ in range(2)]
    p8, p8d = str(tmp_path / "a.y4m"), str(tmp_path / "b.y4m")
    frames.write_y4m_420(p8, clip8, rows, cols)
    frames.write_y4m_420(p8d, clip8, rows, cols, depth=8)
    head = b"YUV4MPEG2 W10 H6 F25:1 Ip A1:1 C420jpeg\n"
    want = head + b"".join(b"FRAME\n" + c.tobytes() for c in clip8)
    assert open(p8, "rb").read() == want == open(p8d, "rb").read()
    with pytest.raises(frames.FrameError):
        frames.Y4MVideo16(p8)
    with pytest.raises(frames.FrameError):
        frames.write_y4m_420(str(tmp_path / "c.y4m"), clip, rows, cols, depth=9)
    with pytest.raises(frames.FrameError):
        frames.write_y4m_420(str(tmp_path / "d.y4m"), [clip[0][:-1]], rows, cols, depth=10)
    with pytest.raises(frames.FrameError, match="does not fit"):
        frames.write_y4m_420(str(tmp_path / "e.y4m"), [clip[0] + 1024], rows, cols, depth=10)


def test_misuse_of_uint16_frames_has_its_own_text():
    """A uint16 frame of the wrong size, or next to a uint8 one, is refused before
    the context is reached, in words about 16-bit frames."""
    import hsflow
    good = np.zeros(yuv.frame_bytes(6, 10), np.uint16)
    for f0, f1 in ((good, good[:-1]), (good, good.astype(np.uint8)), (good.astype(np.uint8), good)):
        with pytest.raises(hsflow.HsflowError, match="uint16"):
            yuv.interpolate_yuv(None, f0, f1, 0.5, 2, 1, 3, 10, 400.0, 6, 10)
    with pytest.raises(hsflow.HsflowError, match="uint8"):
        yuv.interpolate_yuv(None, good.astype(np.uint8)[:-1], good.astype(np.uint8), 0.5, 2, 1, 3,
                            10, 100.0, 6, 10)


def test_pack_split_convert_on_uint16():
    rng = np.random.default_rng(61)
    y = rng.integers(0, 65536, (3, 6, 10)).astype(np.uint16)
    u, v = (rng.integers(0, 65536, (3, 3, 5)).astype(np.uint16) for _ in range(2))
    y[0, 0, :5], u[0, 0, :5] = SPECIAL, SPECIAL[::-1]
    for lay in (I420, NV12):
        p = yuv.pack(y, u, v, lay)
        assert p.shape == (3, 90) and p.dtype == np.uint16
        for a, b in zip(yuv.split(p, 6, 10, lay), (y, u, v)):
            assert a.dtype == np.uint16 and np.array_equal(a, b)
    p = yuv.pack(y[0], u[0], v[0], I420)
    q = yuv.pack(y[0], u[0], v[0], NV12)
    assert np.array_equal(q[60::2], u[0].ravel()) and np.array_equal(q[61::2], v[0].ravel())
    assert np.array_equal(yuv.convert(p, 6, 10, I420, NV12), q)
    assert np.array_equal(yuv.convert(q, 6, 10, NV12, I420), p)


@functools.lru_cache(maxsize=None)
def _quality10():
    """test_yuv's quality pair as 10-bit content: every plane times 4 plus a
    2-bit dither; the true middle chroma times 4 plus the dither's mean."""
    (y0, u0, v0), (y1, u1, v1), (um, vm) = _quality_pair()
    rng = np.random.default_rng(10)

    def ten(p):
        a = p.astype(np.int64) * 4 + rng.integers(0, 4, p.shape)
        assert a.min() >= 0 and a.max() <= 1023
        return a.astype(np.uint16)

    f0, f1 = [ten(p) for p in (y0, u0, v0)], [ten(p) for p in (y1, u1, v1)]
    assert max(int(p.max()) for p in f0 + f1) > 255
    return f0, f1, (um.astype(np.float64) * 4 + 1.5, vm.astype(np.float64) * 4 + 1.5)


def _errors10(got_u, got_v):
    """Mean absolute interior error (10-bit levels) of a middle frame's chroma
    against the truth, and the plain blend's."""
    from test_yuv import _interior
    (_, u0, v0), (_, u1, v1), (um, vm) = _quality10()
    mc = [float(np.abs(_interior(g) - _interior(m)).mean()) for g, m in ((got_u, um), (got_v, vm))]
    blend = [float(np.abs(_interior((a.astype(np.float64) + b) / 2) - _interior(m)).mean())
             for a, b, m in ((u0, u1, um), (v0, v1, vm))]
    return mc, blend


def test_reference_quality_on_10_bit_content():
    """The float64 reference on 10-bit content with alpha x 4: the middle frame's
    interior chroma error is at most 0.1 of the plain blend's (the 8-bit figure
    is 0.02)."""
    (y0, u0, v0), (y1, u1, v1), _ = _quality10()
    levels, warps, w, n, alpha, k = QUALITY_SOLVE
    from test_median import warped_median_np
    a0, a1 = y0.astype(np.float64), y1.astype(np.float64)
    uf, vf = warped_median_np(a0, a1, levels, warps, w, n, alpha * 4, k)
    ub, vb = warped_median_np(a1, a0, levels, warps, w, n, alpha * 4, k)
    cu, cv = chroma_interp_np(*(p.astype(np.float64) for p in (u0, v0, u1, v1)), uf, vf, ub, vb,
                              0.5)
    mc, blend = _errors10(cu, cv)
    print("reference, 10-bit: motion-compensated chroma error (U, V)", mc, "plain blend", blend,
          "ratios", [m / b for m, b in zip(mc, blend)])
    assert mc[0] <= 0.1 * blend[0] and mc[1] <= 0.1 * blend[1]


def test_getframeinterpyuv16_compiles_and_links(tmp_path):
    """A caller of the uint16_t overloads of hsflow::Context::getFrameInterpYuv
    and hsflow::HornSchunck's, and of the cv::Mat adapter on CV_16UC1 frames,
    builds against include/hornSchunck.hpp, the cv::Mat test double and
    libhsflow.so; without a device the calls throw (never a crash), and a
    malformed cv::Mat is refused before the library is reached."""
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("no C++ compiler")
    src = tmp_path / "yuv16_main.cpp"
    src.write_text(r'''
#include <cstdio>
#include "hornSchunck.hpp"
#if !defined(HSFLOW_HAS_YUV16) || HSFLOW_HAS_YUV16 != 1
#error "hsflow.h lacks the 16-bit YUV 4:2:0 interpolation"
#endif
static_assert(HSFLOW_U16 == 4, "HSFLOW_U16");
int main() {
    const int rows = 16, cols = 24;
    cv::Mat a(rows * 3 / 2, cols, CV_16UC1), b(rows * 3 / 2, cols, CV_16UC1);
    for (int i = 0; i < rows * 3 / 2 * cols; ++i)
        ((uint16_t *)a.data)[i] = (uint16_t)(i * 977), ((uint16_t *)b.data)[i] = ((uint16_t *)a.data)[i];
    std::vector<float> times{0.5f};
    std::vector<cv::Mat> frames;
    hornSchunck hs(3, 10, 400.0);
    int thrown = 0, made = 0, bad = 0;
    try {
        hs.getFrameInterpYuv(a, b, times, 2, 1, 0, frames, HSFLOW_YUV_NV12);
        made = (int)frames.size() == 1 && frames[0].rows == rows * 3 / 2 && frames[0].cols == cols &&
               frames[0].type() == CV_16UC1;
    } catch (const cv::Exception &) { ++thrown; }
    cv::Mat odd(rows + 1, cols, CV_16UC1), u8(rows * 3 / 2, cols, CV_8UC1);
    try { hs.getFrameInterpYuv(odd, odd, times, 2, 1, 0, frames); } catch (const cv::Exception &) { ++bad; }
    try { hs.getFrameInterpYuv(a, u8, times, 2, 1, 0, frames); } catch (const cv::Exception &) { ++bad; }
    try { hs.getFrameInterpYuv(a, odd, times, 2, 1, 0, frames); } catch (const cv::Exception &) { ++bad; }
    try {
        hsflow::Context c(0);
        std::vector<std::vector<uint16_t>> out;
        std::vector<std::vector<uint8_t>> flags;
        c.getFrameInterpYuv((const uint16_t *)a.data, (const uint16_t *)b.data, HSFLOW_YUV_I420, rows,
                            cols, times, 2, 1, 0, 3, 10, 400.0, out, &flags, 1);
        if (out.size() != 1 || out[0].size() != (size_t)rows * cols * 3 / 2) return 3;
        if (flags[0].size() != (size_t)rows * cols) return 4;
        hsflow::HornSchunck h(3, 10, 400.0);
        h.getFrameInterpYuv((const uint16_t *)a.data, (const uint16_t *)b.data, HSFLOW_YUV_NV12, rows,
                            cols, times, 2, 1, 0, out);
        if (out[0].size() != (size_t)rows * cols * 3 / 2) return 5;
    } catch (const hsflow::Error &) { ++thrown; }
    std::printf("%d %d %d %d\n", thrown, made, bad,
                hsflow_flow_interp_yuv16(nullptr, (const uint16_t *)a.data, (const uint16_t *)b.data, 1,
                                         rows, cols, 2, 1, 0, 3, 10, 400.0, 0.01f, 0.5f, times.data(),
                                         1, 0, nullptr, HSFLOW_U16, nullptr, nullptr));
    return 0;
}
''')
    lib_dir = os.path.join(ROOT, "cpp-optical-flow_amd")
    exe = str(tmp_path / "yuv16_main")
    subprocess.check_call([gxx, "-std=c++17", "-Wall", "-Werror",
                           "-I", os.path.join(ROOT, "tests", "cpp", "cvstub"),
                           "-I", os.path.join(ROOT, "include"), str(src), "-o", exe, "-L", lib_dir,
                           "-lhsflow", "-Wl,-rpath," + lib_dir])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    thrown, made, bad, rc0 = (int(x) for x in out.stdout.split())
    # 2 thrown where no gfx950 device is present
    assert (thrown, made) in ((0, 1), (2, 0))
    assert (bad, rc0) == (3, -1)


# ------------------------------------------------------------------ GPU tests
@pytest.mark.gpu
@pytest.mark.parametrize("nt", [1, 3])
@pytest.mark.parametrize("u16", [False, True], ids=["f32out", "u16out"])
@pytest.mark.parametrize("layout", LAYOUTS, **LAYOUT_IDS)
@pytest.mark.parametrize("shape", SHAPES, **SHAPE_IDS)
def test_kernel_equals_the_public_pieces_bitwise(hs, shape, layout, u16, nt):
    import torch
    c0, c1, flows = _inputs(shape)
    want = _as_layout(_pieces(hs, c0, c1, flows, TIMES[nt]), layout)
    l0, l1 = _t16(_as_layout(c0, layout)), _t16(_as_layout(c1, layout))
    got = yuv.chroma_interp_device(l0, l1, *flows, TIMES[nt], layout, out_dtype=_out_dtype(u16))
    torch.cuda.synchronize()
    assert got.shape == want.shape and got.dtype == _out_dtype(u16)
    assert _matches(got, want, u16)
    if u16 and nt == 3:  # times 0 and 1 are the source chroma itself
        assert np.array_equal(_np16(got[:, 0]), _as_layout(c0, layout))
        assert np.array_equal(_np16(got[:, 2]), _as_layout(c1, layout))
    # int16 tensors are read as the same 16 bits, and give int16
    i0, i1 = l0.view(torch.int16), l1.view(torch.int16)
    same = yuv.chroma_interp_device(i0, i1, *flows, TIMES[nt], layout,
                                    out_dtype=torch.int16 if u16 else torch.float32)
    torch.cuda.synchronize()
    assert same.dtype == (torch.int16 if u16 else torch.float32) and _matches(same, want, u16)
    if layout == NV12:  # one 8-byte load per row's two taps: the same bits
        assert yuv.set_nv12_loads(True) is False
        try:
            wide = yuv.chroma_interp_device(l0, l1, *flows, TIMES[nt], layout,
                                            out_dtype=_out_dtype(u16))
            torch.cuda.synchronize()
        finally:
            yuv.set_nv12_loads(False)
        assert _matches(wide, want, u16)


@pytest.mark.gpu
@pytest.mark.parametrize("nt", [1, 3])
@pytest.mark.parametrize("u16", [False, True], ids=["f32out", "u16out"])
@pytest.mark.parametrize("layout", LAYOUTS, **LAYOUT_IDS)
@pytest.mark.parametrize("shape", SHAPES, **SHAPE_IDS)
def test_projected_kernel_equals_the_public_pieces_bitwise(hs, shape, layout, u16, nt):
    import torch
    from test_yuv_projection import _luma_cells
    c0, c1, flows = _inputs(shape)
    cells = _luma_cells(shape, TIMES[nt])
    if nt == 3:
        cells[:, 0] = -1  # a time plane that is all holes: KIY's value
    want = _as_layout(_pieces(hs, c0, c1, flows, TIMES[nt], cells=cells), layout)
    l0, l1 = _t16(_as_layout(c0, layout)), _t16(_as_layout(c1, layout))
    got = yuv.chroma_interp_proj_device(l0, l1, *flows, TIMES[nt], cells, layout,
                                        out_dtype=_out_dtype(u16))
    plain = yuv.chroma_interp_device(l0, l1, *flows, TIMES[nt], layout, out_dtype=_out_dtype(u16))
    torch.cuda.synchronize()
    assert got.shape == want.shape and _matches(got, want, u16)
    if nt == 3:
        view = _np16 if u16 else _bits32
        assert np.array_equal(view(got[:, 0]), view(plain[:, 0]))
        if shape[1] >= 34:  # ... and at t = 0.5 the projection does change the result
            assert not np.array_equal(view(got[:, 1]), view(plain[:, 1]))
    if layout == NV12:
        assert yuv.set_nv12_loads(True) is False
        try:
            wide = yuv.chroma_interp_proj_device(l0, l1, *flows, TIMES[nt], cells, layout,
                                                 out_dtype=_out_dtype(u16))
            torch.cuda.synchronize()
        finally:
            yuv.set_nv12_loads(False)
        assert _matches(wide, want, u16)


def _placed16(a, odd, shape=None):
    """`a` (numpy uint16; or an uninitialised tensor of `shape`) in a flat int16
    allocation between guards, at a base that is 2-byte but not 4-byte aligned
    when `odd`.  Returns (flat, view, (lo, hi))."""
    import torch
    shape = tuple(a.shape) if shape is None else tuple(shape)
    n, guard = int(np.prod(shape)), 64
    flat = torch.full((n + 2 * guard + 1,), GUARD_I16, dtype=torch.int16, device="cuda")
    lo = guard + (1 if (flat.data_ptr() // 2 + guard) % 2 == (0 if odd else 1) else 0)
    view = flat[lo:lo + n].view(shape)
    assert view.data_ptr() % 4 == (2 if odd else 0)
    if a is not None:
        view.copy_(_t16(a).view(torch.int16))
    return flat, view, (lo, lo + n)


@pytest.mark.gpu
@pytest.mark.parametrize("proj", [False, True], ids=["kiy", "kiyp"])
@pytest.mark.parametrize("layout", LAYOUTS, **LAYOUT_IDS)
def test_two_byte_aligned_planes_give_the_same_bits(hs, layout, proj):
    """Inputs and output at a base that is 2-byte but not 4-byte aligned: the
    unaligned dword loads and stores of NV12 and the two-byte stores of I420;
    the same bits, and the guards around the output are intact."""
    import torch
    from test_yuv_projection import _luma_cells
    shape = (3, 34, 130)
    c0, c1, flows = _inputs(shape)
    cells = _luma_cells(shape, TIMES[3]) if proj else None

    def run(l0, l1, **kw):
        if proj:
            return yuv.chroma_interp_proj_device(l0, l1, *flows, TIMES[3], cells, layout, **kw)
        return yuv.chroma_interp_device(l0, l1, *flows, TIMES[3], layout, **kw)

    a0, a1 = _as_layout(c0, layout), _as_layout(c1, layout)
    aligned = run(_t16(a0), _t16(a1), out_dtype=torch.uint16)
    want = _as_layout(_pieces(hs, c0, c1, flows, TIMES[3], cells=cells), layout)
    torch.cuda.synchronize()
    assert aligned.data_ptr() % 4 == 0 and _matches(aligned, want, True)
    for odd_in, odd_out in ((True, True), (False, True), (True, False)):
        f0, v0, _ = _placed16(a0, odd_in)
        f1, v1, _ = _placed16(a1, odd_in)
        flat, out, (lo, hi) = _placed16(None, odd_out, tuple(aligned.shape))
        got = run(v0, v1, out=out)
        torch.cuda.synchronize()
        assert got is out and np.array_equal(_np16(got), _np16(aligned)), (odd_in, odd_out)
        assert _guards_intact(flat, lo, hi, GUARD_I16)
        assert np.array_equal(_np16(v0), a0) and np.array_equal(_np16(v1), a1)


@pytest.mark.gpu
@pytest.mark.parametrize("layout", LAYOUTS, **LAYOUT_IDS)
def test_hostile_flow_values_stay_in_their_block(hs, layout):
    """NaN, +-inf and +-1e30 in each flow plane: the bits are the pieces', the
    guards around the output stay, and only the chroma samples whose 2 x 2 block
    holds one differ from the clean run."""
    import torch
    shape = (2, 34, 130)
    c0, c1, flows = _inputs(shape)
    rng = np.random.default_rng(12)
    hit = np.zeros((shape[0], shape[1] // 2, shape[2] // 2), bool)
    dirty = []
    for a in _smooth_flows(*shape):
        a = a.copy()
        for val in HOSTILE:
            b, y, x = (int(rng.integers(n)) for n in shape)
            a[b, y, x] = val
            hit[b, y // 2, x // 2] = True
        dirty.append(_cuda(a))
    l0, l1 = _t16(_as_layout(c0, layout)), _t16(_as_layout(c1, layout))
    want = _as_layout(_pieces(hs, c0, c1, dirty, TIMES[3]), layout)
    for u16 in (False, True):
        clean = yuv.chroma_interp_device(l0, l1, *flows, TIMES[3], layout,
                                         out_dtype=_out_dtype(u16))
        if u16:
            flat, out, (lo, hi) = _placed16(None, True, tuple(clean.shape))
            fill = GUARD_I16
        else:
            flat, out, (lo, hi) = _placed(None, 0, torch.float32, GUARD_F32, tuple(clean.shape))
            fill = GUARD_F32
        yuv.chroma_interp_device(l0, l1, *dirty, TIMES[3], layout, out=out)
        torch.cuda.synchronize()
        assert _matches(out, want, u16) and _guards_intact(flat, lo, hi, fill)
        view = _np16 if u16 else _bits32
        same = view(out) == view(clean)  # [B, nt, 2, rc, cc] or [B, nt, rc, cc, 2]
        same = same.all(axis=2 if layout == I420 else 4).all(axis=1)
        assert same[~hit].all()


@pytest.mark.gpu
@pytest.mark.parametrize("mode", [NEAREST, BLEND], ids=["nearest", "blend"])
@pytest.mark.parametrize("layout", LAYOUTS, **LAYOUT_IDS)
def test_fallback_is_per_pair_and_equals_the_public_piece(hs, layout, mode):
    import fallback
    import torch
    from test_yuv_projection import _luma_cells
    shape = (2, 34, 130)
    batch, rows, cols = shape
    c0, c1, flows = _inputs(shape)
    a0, a1 = _as_layout(c0, layout), _as_layout(c1, layout)
    l0, l1 = _t16(a0), _t16(a1)
    fb = fallback.Fallback(mode)
    cells = _luma_cells(shape, TIMES[3])

    def counts(verdicts):  # 1: fails under the luma's and the chroma's threshold
        c = np.array([[0 if v else rows * cols, 5, 6] for v in verdicts], np.int32)
        return _cuda(c), _cuda(c.copy())

    for u16 in (False, True):
        dt = _out_dtype(u16)
        view = _np16 if u16 else _bits32
        plain = yuv.chroma_interp_device(l0, l1, *flows, TIMES[3], layout, out_dtype=dt)
        for verdicts in ((1, 1), (0, 0), (1, 0), (0, 1)):
            cf, cb = counts(verdicts)
            got = yuv.chroma_interp_device(l0, l1, *flows, TIMES[3], layout, counts_f=cf,
                                           counts_b=cb, fallback=fb, out_dtype=dt)
            want = _as_layout(_pieces(hs, c0, c1, flows, TIMES[3], fb=fb, counts=(cf, cb)), layout)
            torch.cuda.synchronize()
            assert _matches(got, want, u16), (u16, verdicts)
            for b, v in enumerate(verdicts):
                assert np.array_equal(view(got[b]), view(plain[b])) is (not v), (u16, verdicts, b)
        # the projected kernel takes the same verdict
        cf, cb = counts((1, 0))
        got = yuv.chroma_interp_proj_device(l0, l1, *flows, TIMES[3], cells, layout, counts_f=cf,
                                            counts_b=cb, fallback=fb, out_dtype=dt)
        want = _as_layout(_pieces(hs, c0, c1, flows, TIMES[3], cells=cells, fb=fb,
                                  counts=(cf, cb)), layout)
        torch.cuda.synchronize()
        assert _matches(got, want, u16)
    # a failed pair at t = 0 and 1 is the source chroma itself
    cf, cb = counts((1, 1))
    ends = yuv.chroma_interp_device(l0, l1, *flows, (0.0, 1.0), layout, counts_f=cf, counts_b=cb,
                                    fallback=fb, out_dtype=torch.uint16)
    torch.cuda.synchronize()
    assert np.array_equal(_np16(ends[:, 0]), a0) and np.array_equal(_np16(ends[:, 1]), a1)


@pytest.mark.gpu
@pytest.mark.parametrize("proj", [0, 1])
@pytest.mark.parametrize("warm", [False, True], ids=["cold", "init"])
@pytest.mark.parametrize("finest", [0, 1])
@pytest.mark.parametrize("loaded", [False, True], ids=["plain", "pf-sm"])
def test_fused_call_equals_its_pieces_bitwise(hs, loaded, finest, warm, proj):
    """The fused 16-bit call: out_y, flags, trusted and cut are
    flow_interp_device's on the luma as float32 (float32 out, then rounded);
    out_c is the 16-bit chroma call on the flows, cells and counts of
    flow_bidir_device and project_device on those float32 planes.  Three levels:
    the pyramid is the unrounded one on both sides."""
    import fallback
    import projection
    import temporal
    import torch
    y0n, y1n, c0, c1 = _luma16_batch()
    y0, y1 = _t16(y0n), _t16(y1n)
    g0, g1 = _f32(y0n), _f32(y1n)
    levels, warps, w, n, alpha, k = LEVELS3
    args, times = (levels, warps, w, n, alpha), (0.25, 0.5)
    fb = fallback.Fallback(BLEND)
    pf = hs.Prefilter(2) if loaded else None
    kw = dict(median=k, finest=finest, init=_init_for(y0.shape) if warm else None,
              prefilter=pf, smoothness=hs.Smoothness(1, 0.3) if loaded else None)
    r = temporal.flow_bidir_device(g0, g1, *args, mask_f=True, mask_b=True, counts_f=True,
                                   counts_b=True, **kw)
    cells = None
    if proj:
        s0, s1 = (hs.prefilter_device(g0, pf), hs.prefilter_device(g1, pf)) if loaded else (g0, g1)
        cells = projection.project_device(s0, s1, r.uf, r.vf, r.ub, r.vb, times)
    want_y = temporal.flow_interp_device(g0, g1, times, *args, out_dtype=torch.float32, flags=True,
                                         trusted=True, fallback=fb, cut=True, projection=proj,
                                         **kw)
    outs = {}
    for lay in LAYOUTS:
        l0, l1 = _t16(_as_layout(c0, lay)), _t16(_as_layout(c1, lay))
        for u16 in (True, False):
            dt = _out_dtype(u16)
            if proj:
                want_c = yuv.chroma_interp_proj_device(
                    l0, l1, r.uf, r.vf, r.ub, r.vb, times, cells, lay, counts_f=r.counts_f,
                    counts_b=r.counts_b, fallback=fb, out_dtype=dt)
            else:
                want_c = yuv.chroma_interp_device(
                    l0, l1, r.uf, r.vf, r.ub, r.vb, times, lay, counts_f=r.counts_f,
                    counts_b=r.counts_b, fallback=fb, out_dtype=dt)
            got = yuv.flow_interp_yuv_proj_device(y0, l0, y1, l1, times, *args, layout=lay,
                                                  out_dtype=dt, flags=True, trusted=True,
                                                  fallback=fb, cut=True, projection=proj, **kw)
            torch.cuda.synchronize()
            out_y, out_c, flags, trusted, cut = got
            assert out_y.dtype == dt and out_c.dtype == dt
            assert _matches(out_y, want_y[0], u16)
            assert torch.equal(flags, want_y[1]) and torch.equal(trusted, want_y[2])
            assert torch.equal(cut, want_y[3])
            view = _np16 if u16 else _bits32
            assert np.array_equal(view(out_c), view(want_c))
            if u16:
                outs[lay] = _np16(out_c)
        if not proj:  # the form without a projection argument is projection 0
            old = yuv.flow_interp_yuv_device(y0, l0, y1, l1, times, *args, layout=lay,
                                             out_dtype=torch.uint16, flags=True, trusted=True,
                                             fallback=fb, cut=True, **kw)
            torch.cuda.synchronize()
            assert np.array_equal(_np16(old[1]), outs[lay]) and torch.equal(old[2], want_y[1])
    assert np.array_equal(_as_layout(outs[I420], NV12), outs[NV12])
    if not loaded and not warm and finest == 0:
        assert cut.tolist() == [0, 1]
        assert int(_np16(out_y).max()) > 255


@pytest.mark.gpu
def test_host_call_equals_the_device_call(hs):
    """interpolate_yuv on uint16 frames against the device call, with the
    context's fallback honoured and last_cut set; sequence mode is honoured: the
    second call of a sequence starts from the first one's prediction."""
    import fallback
    import projection
    import temporal
    import torch
    y0, y1, c0, c1 = _luma16_batch()
    levels, warps, w, n, alpha, k = LEVELS3
    args, times = (levels, warps, w, n, alpha), (0.25, 0.75)
    fb = fallback.Fallback(NEAREST)
    with hs.Context(0) as ctx:
        for lay, proj, ctx_proj in ((I420, 1, 0), (NV12, 0, 1)):
            projection.set_projection(ctx, ctx_proj)
            for b, verdict in ((0, False), (1, True)):
                f0 = yuv.pack(y0[b], c0[b, 0], c0[b, 1], lay)
                f1 = yuv.pack(y1[b], c1[b, 0], c1[b, 1], lay)
                assert f0.dtype == np.uint16
                for dt, u16 in ((np.uint16, True), (np.float32, False)):
                    got, flags, trusted = yuv.interpolate_yuv(
                        ctx, f0, f1, times, *args, 24, 40, layout=lay, median=k, out_dtype=dt,
                        with_flags=True, fallback=fb, finest=1, projection=proj)
                    assert ctx.last_cut is verdict
                    dev = yuv.flow_interp_yuv_proj_device(
                        _t16(y0[b:b + 1]), _t16(_as_layout(c0[b:b + 1], lay)),
                        _t16(y1[b:b + 1]), _t16(_as_layout(c1[b:b + 1], lay)), times, *args,
                        layout=lay, median=k, out_dtype=_out_dtype(u16), flags=True, trusted=True,
                        fallback=fb, finest=1, cut=True, projection=proj)
                    torch.cuda.synchronize()
                    assert got.shape == (2, 24 * 40 * 3 // 2) and got.dtype == dt
                    view = _np16 if u16 else _bits32
                    raw = got.view(np.uint16 if u16 else np.int32)
                    for j in range(2):
                        assert np.array_equal(raw[j, :960], view(dev[0][0, j]).ravel())
                        assert np.array_equal(raw[j, 960:], view(dev[1][0, j]).ravel())
                    assert np.array_equal(flags, dev[2][0].cpu().numpy())
                    assert trusted.tolist() == dev[3][0].tolist()
                    assert dev[4].tolist() == [int(verdict)]
        projection.set_projection(ctx, 0)
        assert fallback.get_fallback(ctx) is None and ctx.last_cut is True
        # the related pair, no fallback: the default out_dtype is the frames' own
        f0, f1 = (yuv.pack(y[0], c[0, 0], c[0, 1]) for y, c in ((y0, c0), (y1, c1)))
        cold = yuv.interpolate_yuv(ctx, f0, f1, 0.5, *args, 24, 40, median=k)
        assert cold.shape == (1, 1440) and cold.dtype == np.uint16 and ctx.last_cut is None
        with temporal.sequence(ctx):
            first = yuv.interpolate_yuv(ctx, f0, f1, 0.5, *args, 24, 40, median=k)
            second = yuv.interpolate_yuv(ctx, f0, f1, 0.5, *args, 24, 40, median=k)
        assert np.array_equal(first, cold) and not np.array_equal(second, cold)
        with pytest.raises(hs.HsflowError, match="even"):
            yuv.interpolate_yuv(ctx, f0[:-40], f1[:-40], 0.5, *args, 23, 40)
        with pytest.raises(hs.HsflowError):
            yuv.interpolate_yuv(ctx, f0, f1, 0.5, *args, 24, 40, out_dtype=np.float64)


@pytest.mark.gpu
def test_cpp_overload_runs(hs, tmp_path):
    """The uint16_t overload of hsflow::Context::getFrameInterpYuv once on the
    device, against interpolate_yuv on the same frames."""
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("no C++ compiler")
    y0, y1, c0, c1 = _luma16_batch()
    f0, f1 = (yuv.pack(y[0], c[0, 0], c[0, 1], NV12) for y, c in ((y0, c0), (y1, c1)))
    levels, warps, w, n, alpha, k = LEVELS3
    f0.astype("<u2").tofile(str(tmp_path / "f0.bin"))
    f1.astype("<u2").tofile(str(tmp_path / "f1.bin"))
    src = tmp_path / "run16.cpp"
    src.write_text(r'''
#include <cstdio>
#include <cstdlib>
#include "hsflow.hpp"
static std::vector<uint16_t> load(const char *p, size_t n) {
    std::vector<uint16_t> v(n);
    FILE *f = std::fopen(p, "rb");
    if (!f || std::fread(v.data(), 2, n, f) != n) std::exit(2);
    std::fclose(f);
    return v;
}
int main(int argc, char **argv) {
    const int rows = 24, cols = 40;
    const size_t n = (size_t)rows * cols * 3 / 2;
    std::vector<uint16_t> a = load(argv[1], n), b = load(argv[2], n);
    std::vector<float> times{0.5f};
    std::vector<std::vector<uint16_t>> out;
    hsflow::Context c(0);
    c.getFrameInterpYuv(a.data(), b.data(), HSFLOW_YUV_NV12, rows, cols, times, std::atoi(argv[4]),
                        std::atoi(argv[5]), std::atoi(argv[6]), std::atoi(argv[7]),
                        std::atoi(argv[8]), std::atof(argv[9]), out, nullptr, 1);
    FILE *f = std::fopen(argv[3], "wb");
    if (!f || std::fwrite(out[0].data(), 2, n, f) != n) return 3;
    std::fclose(f);
    return 0;
}
''')
    lib_dir = os.path.join(ROOT, "cpp-optical-flow_amd")
    exe = str(tmp_path / "run16")
    subprocess.check_call([gxx, "-std=c++17", "-Wall", "-Werror", "-I",
                           os.path.join(ROOT, "include"), str(src), "-o", exe, "-L", lib_dir,
                           "-lhsflow", "-Wl,-rpath," + lib_dir])
    res = str(tmp_path / "out.bin")
    subprocess.run([exe, str(tmp_path / "f0.bin"), str(tmp_path / "f1.bin"), res, str(levels),
                    str(warps), str(k), str(w), str(n), repr(alpha)], check=True, timeout=120)
    with hs.Context(0) as ctx:
        want = yuv.interpolate_yuv(ctx, f0, f1, 0.5, levels, warps, w, n, alpha, 24, 40,
                                   layout=NV12, median=k, projection=1)
    assert np.array_equal(np.fromfile(res, "<u2"), want[0])


@pytest.mark.gpu
def test_interpolate_sequence_yuv_on_a_y4m16_clip(hs, tmp_path):
    """Three 10-bit frames through Y4MVideo16 at twice the rate, alpha x 4:
    source frames pass through sample for sample, the middle frame of the related
    pair beats the plain blend in chroma by the reference's factor, never
    leaves 0 .. 1023, and with a fallback the unrelated pair is a cut."""
    import fallback
    import frames as fr
    f0, f1, _ = _quality10()
    seed, rows, cols = QUALITY[:3]
    third = [(p.astype(np.uint16) * 4) for p in _third_frame()]
    path = str(tmp_path / "clip10.y4m")
    fr.write_y4m_420(path, [yuv.pack(*f) for f in (f0, f1, third)], rows, cols, depth=10)
    clip = fr.Y4MVideo16(path)
    assert len(clip) == 3 and clip.bit_depth == 10
    levels, warps, w, n, alpha, k = QUALITY_SOLVE
    with hs.Context(0) as ctx:
        cuts = []
        got = list(fr.interpolate_sequence_yuv(clip, 2, levels, warps, w, n, alpha * 4, median=k,
                                               context=ctx, fallback=fallback.Fallback(NEAREST),
                                               cuts=cuts))
    assert len(got) == 5 and cuts == [2]
    for j in range(3):
        assert got[2 * j].dtype == np.uint16 and np.array_equal(got[2 * j], clip.read_yuv(j))
    assert got[1].dtype == np.uint16 and int(got[1].max()) <= 1023
    assert np.array_equal(got[3], clip.read_yuv(2))
    _, mu, mv = yuv.split(got[1], rows, cols)
    mc, blend = _errors10(mu, mv)
    print("GPU, 10-bit: motion-compensated chroma error (U, V)", mc, "plain blend", blend)
    assert mc[0] <= 0.1 * blend[0] and mc[1] <= 0.1 * blend[1]


@pytest.mark.gpu
def test_side_stream_and_graph_capture(hs):
    """The fused 16-bit call on a side stream, and torch.cuda.graph of it
    replaying the eager result: nothing allocates or synchronises.  KIY-16 and
    KIYP-16 alone, one launch each, are replayed three times.  The fused call's
    graph is replayed once: from the second replay on, graphs of the fused YUV
    calls -- the 8-bit ones on the parent commit's library included -- have
    been seen to judge a passing pair a cut ("16-bit YUV 4:2:0",
    Capture), which include/hsflow.h states as a limitation."""
    import fallback
    import torch
    y0n, y1n, c0, c1 = _luma16_batch()
    y0, y1 = _t16(y0n), _t16(y1n)
    l0, l1 = _t16(_as_layout(c0, NV12)), _t16(_as_layout(c1, NV12))
    batch, rows, cols = y0.shape
    levels, warps, w, n, alpha, k = LEVELS3
    args, times = (levels, warps, w, n, alpha), (0.25, 0.75)
    fb = fallback.Fallback(NEAREST)
    ws = torch.empty(yuv.flow_interp_proj_workspace_bytes(rows, cols, batch, levels, 2, 1, True),
                     dtype=torch.uint8, device="cuda")
    out_y = torch.zeros((batch, 2, rows, cols), dtype=torch.int16, device="cuda")
    out_c = torch.zeros((batch, 2, rows // 2, cols // 2, 2), dtype=torch.int16, device="cuda")
    cut = torch.zeros((batch,), dtype=torch.uint8, device="cuda")

    def solve(s):
        yuv.flow_interp_yuv_proj_device(y0, l0, y1, l1, times, *args, layout=NV12, median=k,
                                        out_y=out_y, out_c=out_c, cut=cut, fallback=fb,
                                        workspace=ws, stream=s, projection=1)

    eager = yuv.flow_interp_yuv_proj_device(y0, l0, y1, l1, times, *args, layout=NV12, median=k,
                                            out_dtype=torch.uint16, cut=True, fallback=fb,
                                            projection=1)
    torch.cuda.synchronize()
    want_y, want_c = _np16(eager[0]), _np16(eager[1])
    stream = torch.cuda.current_stream()
    side = torch.cuda.Stream()
    side.wait_stream(stream)
    with torch.cuda.stream(side):
        solve(side)
    stream.wait_stream(side)
    torch.cuda.synchronize()
    assert np.array_equal(_np16(out_y), want_y) and np.array_equal(_np16(out_c), want_c)
    assert torch.equal(cut, eager[4]) and cut.tolist() == [0, 1]
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, capture_error_mode="thread_local"):
        solve(torch.cuda.current_stream())
    torch.cuda.synchronize()
    out_y.zero_(), out_c.zero_(), cut.fill_(7)
    graph.replay()
    torch.cuda.synchronize()
    assert np.array_equal(_np16(out_y), want_y) and np.array_equal(_np16(out_c), want_c)
    assert cut.tolist() == [0, 1]
    # the chroma kernels alone: one launch each, no memset, any number of replays
    from test_yuv_projection import _luma_cells
    flows = [_cuda(a) for a in _smooth_flows(batch, rows, cols)]
    cells = _luma_cells((batch, rows, cols), times)
    kiy, kiyp = torch.zeros_like(out_c), torch.zeros_like(out_c)
    want_k = _np16(yuv.chroma_interp_device(l0, l1, *flows, times, NV12, out_dtype=torch.uint16))
    want_p = _np16(yuv.chroma_interp_proj_device(l0, l1, *flows, times, cells, NV12,
                                                 out_dtype=torch.uint16))
    torch.cuda.synchronize()
    both = torch.cuda.CUDAGraph()
    with torch.cuda.graph(both, capture_error_mode="thread_local"):
        s = torch.cuda.current_stream()
        yuv.chroma_interp_device(l0, l1, *flows, times, NV12, out=kiy, stream=s)
        yuv.chroma_interp_proj_device(l0, l1, *flows, times, cells, NV12, out=kiyp, stream=s)
    torch.cuda.synchronize()
    for _ in range(3):
        kiy.zero_(), kiyp.zero_()
        both.replay()
        torch.cuda.synchronize()
        assert np.array_equal(_np16(kiy), want_k) and np.array_equal(_np16(kiyp), want_p)
    assert not np.array_equal(want_k, want_p)
