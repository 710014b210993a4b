"""The device API's memory contract (include/hsflow.h, "Memory contract of the
device calls"): where a call may read and write, and what it may assume.

1.  Caller planes at every 4-byte alignment.  (u, v), the frames and the
    gradient outputs of the Jacobi core -- hsflow_flow_device, K1 and a
    warm-started hsflow_jacobi_device, hsflow_flow_pyramid_device,
    hsflow_gradients_device -- sit at element offsets 0..3 of flat allocations
    between guard planes.  K2 and K4's X2 bodies move a column pair as one 8-byte
    word, and between two full-depth K4 passes the interleaved state is written
    into the caller's (u, v) with 16-byte stores; the header asks of a float
    plane no more than its element's alignment, so each plane here sees all four
    4-byte classes of a 16-byte line.  The words must be those of the same call
    on private exact-size tensors, the guards and the inputs keep their bits, and
    the launch counters tell that the interleaved and the fused kernels really
    ran on the offset planes.  One private-tensor baseline per window is held to
    the float64 oracle, so the equalities hang on the reference.

2.  Workspaces.  Every entry point that takes one gets exactly its size
    function's bytes, 256-byte aligned, between two 64 KiB guards, three times:
    filled with 0x00, with 0xFF (every float a NaN, every flag set) and holding
    the finished workspace of the same call on other frames.  The guards keep
    their bytes and every output has the same bits in all runs; the 0x00 run is
    held to the float64 references of the modules that own them, with their
    bounds.  The context's sequence mode, whose buffers the context owns, must
    forget a clip at reset.

3.  Without a GPU: the size functions (256-byte multiples, monotone) and the
    size check of the core entry points.
"""
import contextlib
import ctypes
import functools

import numpy as np
import pytest

import oracle
from conftest import norm_rel_err
from test_first_pass import _frames, _planes
from test_interp import GAIN, _guards_intact, _interior, _placed, _same_bits, frame_interp_np
from test_median import warped_median_np
from test_prefilter import PF, prefilter_np
from test_smoothness import LAM, diffusivity_np, jacobi_weighted_np
from test_strips import TOL
from test_strips_uv import KB, _interleave, _k4, _launches, _planned
from test_temporal import predict_np, warped_temporal_np
from test_warped import _pair, warp_gradients_np
import test_consistency
import test_interp
import test_prefilter
import test_smoothness
import test_temporal
import test_warped

gpu = pytest.mark.gpu

GUARD = -7.25
BATCH, NONINT = 3, (1,)  # pair 1 non-integral: the packed and the f32-gradient body in one launch
ROWS, COLS = 100, 130    # even x even: interleaved under forced K4
SEG = 12                 # K4 rows per segment: several segments, both stream directions
LEVELS = 3
# (u, v) at these element offsets: each plane sees all four 4-byte classes of a
# 16-byte line and the two never share one
OFFSETS = [(1, 2), (2, 3), (3, 0), (0, 1)]
PASSES = {"1": 0, "2": 1, "3": 2, "3+1": 2}  # interleaved passes of a K4 solve of n KB iterations


def _iters(w, n):
    return 3 * KB[w] + 1 if n == "3+1" else int(n) * KB[w]


def _words(t):
    import torch
    return t.contiguous().view(torch.int32)


@contextlib.contextmanager
def _plan(hs, kernel, fuse=True, il=True, streams=1, kb=0):
    with hs.max_streams_as(streams), _k4(hs, SEG if kernel == 4 else 0, kb, kernel), \
            hs.first_pass_fusion_as(fuse), _interleave(hs, il):
        yield


def _warm(shape):
    import torch
    g = torch.Generator(device="cuda").manual_seed(5)
    return (torch.randn(shape, device="cuda", generator=g) * 0.1,
            torch.randn(shape, device="cuda", generator=g) * 0.1)


# ------------------------------------------------- 1. caller planes, the core
def _core_call(hs, mode, I0, I1, w, iters, u, v, warm):
    """cold: hsflow_flow_device; warm: K1, then the passes from `warm`; pyramid:
    hsflow_flow_pyramid_device.  The workspace is a poisoned private tensor."""
    import torch
    batch, rows, cols = I0.shape
    size = (hs.pyramid_workspace_bytes(rows, cols, batch, LEVELS) if mode == "pyramid"
            else hs.workspace_bytes(rows, cols, batch))
    ws = torch.full((size,), 0xA5, dtype=torch.uint8, device="cuda")
    if mode == "pyramid":
        hs.flow_pyramid_device(I0, I1, LEVELS, w, iters, 1.0, u, v, ws)
    elif mode == "cold":
        hs.flow_device(I0, I1, w, iters, 1.0, u, v, ws)
    else:
        u.copy_(warm[0])
        v.copy_(warm[1])
        hs.gradients_device(I0, I1, ws)
        hs.jacobi_device(rows, cols, batch, w, iters, 1.0, u, v, ws, warm_start=True)
    torch.cuda.synchronize()


def _private(hs, mode, I0, I1, w, iters, warm=None):
    """(u, v) as words, of fresh exact-size tensors that start as NaN."""
    import torch
    u = torch.full(I0.shape, float("nan"), device="cuda")
    v = torch.full(I0.shape, float("nan"), device="cuda")
    _core_call(hs, mode, I0, I1, w, iters, u, v, warm)
    return _words(u), _words(v)


def _place_frames(frames, offsets):
    """The frames at element offsets (u8: byte offsets 1..3) between guard planes
    of NaN (u8: 255).  Returns (views, flats)."""
    import torch
    views, flats = [], []
    for t, off in zip(frames, offsets):
        if t.dtype == torch.uint8:
            flat, view, _ = _placed(None, 1 + off % 3, torch.uint8, 255, t.shape)
        else:
            flat, view, _ = _placed(None, off, t.dtype, float("nan"), t.shape)
        view.copy_(t)
        views.append(view)
        flats.append(flat)
    return views, flats


def _at_offsets(hs, mode, I0, I1, w, iters, a, b, warm=None, place_frames=True):
    """The call with u at element offset a and v at b of guarded allocations
    (NaN inside, so a cold solve must write every word), the frames placed
    likewise; the guards and the inputs must keep their bits."""
    import torch
    fu, u, (ulo, uhi) = _placed(None, a, torch.float32, GUARD, I0.shape)
    fv, v, (vlo, vhi) = _placed(None, b, torch.float32, GUARD, I0.shape)
    u.fill_(float("nan"))
    v.fill_(float("nan"))
    frames, flats = _place_frames((I0, I1), (b, a)) if place_frames else ((I0, I1), (I0, I1))
    before = [f.clone() for f in flats]
    _core_call(hs, mode, frames[0], frames[1], w, iters, u, v, warm)
    assert _guards_intact(fu, ulo, uhi, GUARD), f"u at offset {a}: a guard was written"
    assert _guards_intact(fv, vlo, vhi, GUARD), f"v at offset {b}: a guard was written"
    for f, was in zip(flats, before):
        assert _same_bits(f, was), "a frame or its guards changed"
    return _words(u), _words(v)


def _assert_same(got, want, what):
    import torch
    for name, g, r in zip("uv", got, want):
        assert torch.equal(g, r), f"{name}: {what}"
        assert torch.isfinite(g.view(torch.float32)).all(), f"{name} not finite: {what}"


@functools.lru_cache(maxsize=None)
def _oracle_flow(mode, rows, cols, w, iters):
    """The float64 reference of the core cases' frames (test_first_pass._frames
    is seeded by the shape; the values are exact in float32)."""
    rng = np.random.default_rng(7 + 1000 * rows + cols)
    a = rng.integers(0, 256, (BATCH, rows, cols)).astype(np.float64)
    b = rng.integers(0, 256, (BATCH, rows, cols)).astype(np.float64)
    for i in NONINT:
        a[i] = a[i] * 0.73 + 0.21
        b[i] = b[i] * 0.61 + 3.3
    a, b = a.astype(np.float32), b.astype(np.float32)
    if mode == "pyramid":
        uv = [oracle.flow_pyramid(a[k], b[k], LEVELS, w, iters, 1.0) for k in range(BATCH)]
    else:
        uv = [oracle.flow(a[k], b[k], w, iters, 1.0) for k in range(BATCH)]
    return a, b, np.stack([p[0] for p in uv]), np.stack([p[1] for p in uv])


def _anchor(mode, I0, I1, w, iters, words):
    """The private-tensor baseline against the float64 oracle, within the
    project's 1e-4 (test_strips.TOL, norm_rel_err)."""
    import torch
    a, b, ur, vr = _oracle_flow(mode, I0.shape[1], I0.shape[2], w, iters)
    assert np.array_equal(a, I0.cpu().numpy()) and np.array_equal(b, I1.cpu().numpy())
    eu = norm_rel_err(words[0].view(torch.float32).cpu().numpy(), ur)
    ev = norm_rel_err(words[1].view(torch.float32).cpu().numpy(), vr)
    print(f"{mode} w {w} iters {iters}: against the oracle u {eu:.2e} v {ev:.2e}")
    assert eu <= TOL and ev <= TOL


def _core_cases():
    out = []
    for w in (5, 3):
        for n in PASSES:
            # K2 has neither the fusion nor the interleave; a warm start never fuses
            out.append(("cold", 2, w, n, False, False))
            out.append(("warm", 2, w, n, False, False))
            for il in (True, False):
                out.append(("warm", 4, w, n, False, il))
                for fuse in (True, False):
                    out.append(("cold", 4, w, n, fuse, il))
    return out


def _core_id(c):
    mode, kernel, w, n, fuse, il = c
    return f"{mode}-K{kernel}-w{w}-{n}KB" + ("-fused" if fuse else "") + ("-il" if il else "")


@gpu
@pytest.mark.parametrize("case", _core_cases(), ids=_core_id)
def test_core_solve_with_planes_at_every_alignment(hs, case):
    """100 x 130, batch 3, one and two side streams.  iters = KB: no interleaved
    pass; 2 KB: the interleaved state lives in the workspace; 3 KB: in the
    caller's (u, v) as well; 3 KB + 1: handed to a short K2 pass as planes.  The
    frames of a fused first pass stay where they are (test_first_pass places
    them); all others move with (u, v)."""
    mode, kernel, w, n, fuse, il = case
    I0, I1 = _frames("f32", BATCH, ROWS, COLS, nonint=NONINT)
    iters = _iters(w, n)
    warm = _warm(I0.shape) if mode == "warm" else None
    fused = mode == "cold" and kernel == 4 and fuse
    for streams in (1, 2):
        chains = min(streams, BATCH)
        with _plan(hs, kernel, fuse, il, streams):
            planned = _planned(hs, ROWS, COLS, BATCH, w, iters)
            assert planned == (PASSES[n] if kernel == 4 and il else 0)
            want = _private(hs, mode, I0, I1, w, iters, warm)
            for a, b in OFFSETS:
                il0, fp0 = _launches(hs), hs.first_pass_launches()
                got = _at_offsets(hs, mode, I0, I1, w, iters, a, b, warm, place_frames=not fused)
                # the 16-byte stores and the fused pass did run on these planes
                assert _launches(hs) - il0 == planned * chains
                assert hs.first_pass_launches() - fp0 == (chains if fused else 0)
                _assert_same(got, want, f"offsets ({a}, {b}), {streams} stream(s)")
    if case[:2] == ("cold", 4) and n == "3" and fuse and il:
        _anchor(mode, I0, I1, w, iters, want)


@gpu
@pytest.mark.parametrize("kb", [4, 5])
def test_shallow_depths_with_planes_at_every_alignment(hs, kb):
    """w 5 at KB 4 and 5: K4 passes that stay planar."""
    I0, I1 = _frames("f32", BATCH, ROWS, COLS, nonint=NONINT)
    with _plan(hs, 4, kb=kb):
        assert _planned(hs, ROWS, COLS, BATCH, 5, 3 * kb) == 0
        want = _private(hs, "cold", I0, I1, 5, 3 * kb)
        for a, b in OFFSETS:
            got = _at_offsets(hs, "cold", I0, I1, 5, 3 * kb, a, b, place_frames=False)
            _assert_same(got, want, f"KB {kb}, offsets ({a}, {b})")


# 100 x 129, 61 x 130: planar (the dword path, an odd height); 2 x 2, 1 x 7: the
# degenerate ones; 100 x 260: a third strip, interleaved
@gpu
@pytest.mark.parametrize("mode", ["cold", "warm"])
@pytest.mark.parametrize("kernel", [4, 2])
@pytest.mark.parametrize("rows,cols", [(100, 129), (61, 130), (2, 2), (1, 7), (100, 260)])
def test_other_shapes_with_planes_at_every_alignment(hs, rows, cols, kernel, mode):
    I0, I1 = _frames("f32", BATCH, rows, cols, nonint=NONINT)
    iters = 3 * KB[5]
    warm = _warm(I0.shape) if mode == "warm" else None
    fused = mode == "cold" and kernel == 4
    for streams in (1, 2):
        with _plan(hs, kernel, streams=streams):
            planned = _planned(hs, rows, cols, BATCH, 5, iters)
            assert planned == (2 if kernel == 4 and rows % 2 == 0 and cols % 2 == 0 else 0)
            want = _private(hs, mode, I0, I1, 5, iters, warm)
            for a, b in OFFSETS:
                il0 = _launches(hs)
                got = _at_offsets(hs, mode, I0, I1, 5, iters, a, b, warm, place_frames=not fused)
                assert _launches(hs) - il0 == planned * min(streams, BATCH)
                _assert_same(got, want, f"{rows}x{cols} offsets ({a}, {b}), {streams} stream(s)")


@gpu
@pytest.mark.parametrize("kernel", [4, 2])
@pytest.mark.parametrize("rows,cols", [(100, 130), (61, 129)])
def test_cold_solve_from_u8_frames_at_byte_offsets(hs, rows, cols, kernel):
    """K1 in front of the passes (the fusion off) reads 8-bit frames at byte
    offsets 1..3 between guards of 255."""
    I0, I1 = _frames("u8", BATCH, rows, cols)
    iters = 2 * KB[5]
    for streams in (1, 2):
        with _plan(hs, kernel, fuse=False, streams=streams):
            want = _private(hs, "cold", I0, I1, 5, iters)
            for a, b in OFFSETS:
                got = _at_offsets(hs, "cold", I0, I1, 5, iters, a, b)
                _assert_same(got, want, f"offsets ({a}, {b}), {streams} stream(s)")


@gpu
@pytest.mark.parametrize("kind", ["f32", "u8"])
@pytest.mark.parametrize("kernel,il", [(4, True), (4, False), (2, False)])
@pytest.mark.parametrize("rows,cols", [(100, 130), (61, 129)])
def test_pyramid_with_planes_at_every_alignment(hs, rows, cols, kernel, il, kind):
    """Three levels: pyrdown reads the placed frames, upflow writes the placed
    (u, v), level 0 is a warm solve in them (interleaved at 100 x 130; the levels
    50 x 65 and 25 x 33 stay planar).  u8 frames sit at byte offsets 1..3."""
    I0, I1 = _frames(kind, BATCH, rows, cols, nonint=NONINT if kind == "f32" else None)
    iters = 3 * KB[5]
    for streams in (1, 2):
        with _plan(hs, kernel, il=il, streams=streams):
            planned = _planned(hs, rows, cols, BATCH, 5, iters)
            assert planned == (2 if il and rows % 2 == 0 else 0)
            want = _private(hs, "pyramid", I0, I1, 5, iters)
            for a, b in OFFSETS:
                il0 = _launches(hs)
                got = _at_offsets(hs, "pyramid", I0, I1, 5, iters, a, b)
                assert _launches(hs) - il0 == planned * min(streams, BATCH)
                _assert_same(got, want, f"offsets ({a}, {b}), {streams} stream(s)")
    if (rows, kernel, il, kind) == (100, 4, True, "f32"):
        _anchor("pyramid", I0, I1, 5, iters, want)


@gpu
@pytest.mark.parametrize("kind", ["f32", "u8"])
@pytest.mark.parametrize("rows,cols", [(100, 130), (61, 129), (2, 2), (1, 7)])
def test_gradient_outputs_at_every_alignment(hs, rows, cols, kind):
    """hsflow_gradients_device with gx, gy, gt: three placed outputs, placed
    frames, against private tensors and (exactly representable or not, within
    1e-4) the float64 gradients."""
    import torch
    I0, I1 = _frames(kind, BATCH, rows, cols, nonint=NONINT if kind == "f32" else None)
    size = hs.workspace_bytes(rows, cols, BATCH)
    want = [torch.full(I0.shape, float("nan"), device="cuda") for _ in range(3)]
    hs.gradients_device(I0, I1, torch.full((size,), 0xA5, dtype=torch.uint8, device="cuda"), *want)
    torch.cuda.synchronize()
    for a, b in OFFSETS:
        placed = [_placed(None, off, torch.float32, GUARD, I0.shape) for off in (a, b, (b + 2) % 4)]
        frames, flats = _place_frames((I0, I1), (b, a))
        before = [f.clone() for f in flats]
        hs.gradients_device(frames[0], frames[1],
                            torch.full((size,), 0xA5, dtype=torch.uint8, device="cuda"),
                            *[p[1] for p in placed])
        torch.cuda.synchronize()
        for (flat, view, (lo, hi)), ref, name in zip(placed, want, ("gx", "gy", "gt")):
            assert _same_bits(view, ref), f"{name} at offsets ({a}, {b})"
            assert _guards_intact(flat, lo, hi, GUARD), f"{name}: a guard was written"
        for f, was in zip(flats, before):
            assert _same_bits(f, was)
    a64, b64 = I0.cpu().numpy().astype(np.float64), I1.cpu().numpy().astype(np.float64)
    for k in range(BATCH):
        for got, ref in zip(want, oracle.gradients(a64[k], b64[k])):
            assert norm_rel_err(got[k].cpu().numpy(), ref) <= TOL


# ------------------------------------------------------------ 2. workspaces
GUARD_BYTES, GUARD_BYTE = 64 * 1024, 0xA5
ALPHA, WINDOW, WARPS = 100.0, 5, 2
ITERS = 3 * KB[WINDOW]
TIMES = (0.25, 0.5, 0.75)
# entry point -> the variants it has: "plain", and "loaded" (normalize prefilter,
# flow-driven smoothness, 5 x 5 median, an init) where it takes those
ENTRIES = {"flow": ("plain",), "jacobi": ("plain",), "weighted": ("plain",), "pyramid": ("plain",),
           "warped": ("plain", "loaded"), "bidir": ("plain", "loaded"),
           "interp": ("plain", "loaded"), "interp_bgr": ("plain", "loaded")}


def _np_frames(which):
    """Three textured pairs with a shift of a few px (test_warped._pair), pair 1
    scaled off the integers; `which`: "A", or "B" for the solve whose finished
    workspace the stale run starts from."""
    base, shift = (2101, (-6, 10)) if which == "A" else (2301, (8, -6))
    pairs = [_pair(base + 7 * k, ROWS, COLS, *shift) for k in range(BATCH)]
    I0 = np.stack([p[0] for p in pairs]).astype(np.float32)
    I1 = np.stack([p[1] for p in pairs]).astype(np.float32)
    for k in NONINT:
        I0[k] = I0[k] * np.float32(0.9) + np.float32(0.3)
        I1[k] = I1[k] * np.float32(0.9) + np.float32(0.3)
    return I0, I1


def _np_bgr(which):
    """8-bit BGR frames with three different channels, and their grey planes."""
    I0, I1 = (np.clip(a, 0, 255).astype(np.uint8) for a in _np_frames(which))
    B0 = np.stack([I0, 255 - I0, I0 // 2 + 17], -1)
    B1 = np.stack([I1, 255 - I1, I1 // 2 + 17], -1)
    grey = [np.stack([oracle.bgr_to_gray(b[k]) for k in range(BATCH)]) for b in (B0, B1)]
    return B0, B1, grey[0], grey[1]


@functools.lru_cache(maxsize=None)
def _np_init():
    """The start of the loaded solves: the prediction (test_temporal.predict_np)
    from a smooth backward flow, as the float32 planes the device receives."""
    _, _, ub, vb = test_consistency._smooth_flows(BATCH, ROWS, COLS)
    planes = [np.stack(p) for p in zip(*[predict_np(0.25 * ub[k], 0.25 * vb[k])
                                         for k in range(BATCH)])]
    return tuple(p.astype(np.float32) for p in planes)


@functools.lru_cache(maxsize=None)
def _ref_flows(variant, source):
    """(uf, vf, ub, vb) of frames A in float64, [B, H, W]: warped_median_np, or
    for "loaded" warped_temporal_np on prefilter_np's frames from _np_init."""
    if source == "bgr":
        I0, I1 = _np_bgr("A")[2:]
    else:
        I0, I1 = _np_frames("A")
    out = []
    for k in range(BATCH):
        a, b = I0[k].astype(np.float64), I1[k].astype(np.float64)
        if variant == "plain":
            f = warped_median_np(a, b, LEVELS, WARPS, WINDOW, ITERS, ALPHA, 0)
            r = warped_median_np(b, a, LEVELS, WARPS, WINDOW, ITERS, ALPHA, 0)
        else:
            a, b = prefilter_np(a, *PF), prefilter_np(b, *PF)
            iu, iv, ibu, ibv = (p[k] for p in _np_init())
            f = warped_temporal_np(a, b, LEVELS, WARPS, WINDOW, ITERS, ALPHA, 5, iu, iv, LAM)
            r = warped_temporal_np(b, a, LEVELS, WARPS, WINDOW, ITERS, ALPHA, 5, ibu, ibv, LAM)
        out.append((*f, *r))
    return tuple(np.stack(p) for p in zip(*out))


def _cuda(a):
    import torch
    return torch.from_numpy(np.array(a, order="C")).cuda()


def _filled(shape, dtype):
    """An output that starts as NaN / 0xEE bytes / -12345."""
    import torch
    fill = {torch.float32: float("nan"), torch.uint8: 0xEE, torch.int32: -12345}[dtype]
    return torch.full(tuple(shape), fill, dtype=dtype, device="cuda")


def _need(hs, entry, variant):
    extra = hs.prefilter_planes_bytes(ROWS, COLS, BATCH) if variant == "loaded" else 0
    fn = {"flow": None, "jacobi": None, "weighted": None, "pyramid": hs.pyramid_workspace_bytes,
          "warped": hs.pyramid_workspace_bytes, "bidir": hs.bidir_workspace_bytes,
          "interp": hs.flow_interp_workspace_bytes,
          "interp_bgr": hs.flow_interp_bgr_workspace_bytes}[entry]
    if fn is None:
        return hs.workspace_bytes(ROWS, COLS, BATCH)
    return fn(ROWS, COLS, BATCH, LEVELS) + extra


def _guarded_workspace(nbytes, fill):
    """Exactly `nbytes` at a 256-byte multiple between two 64 KiB guards;
    `fill`: a byte, or a tensor of its contents.  Returns (allocation, slice, lo)."""
    import torch
    big = torch.full((nbytes + 2 * GUARD_BYTES + 256,), GUARD_BYTE, dtype=torch.uint8,
                     device="cuda")
    lo = GUARD_BYTES + (-(big.data_ptr() + GUARD_BYTES)) % 256
    ws = big[lo:lo + nbytes]
    assert ws.data_ptr() % 256 == 0 and ws.numel() == nbytes
    if isinstance(fill, int):
        ws.fill_(fill)
    else:
        ws.copy_(fill)
    return big, ws, lo


def _workspace_guards_intact(big, lo, nbytes):
    return bool((big[:lo] == GUARD_BYTE).all()) and bool((big[lo + nbytes:] == GUARD_BYTE).all())


def _run_entry(hs, entry, variant, which, ws):
    """One call on frames `which` with the workspace `ws`; every output starts
    poisoned.  Returns name -> tensor."""
    import temporal
    import torch
    f32, u8, i32 = torch.float32, torch.uint8, torch.int32
    shape = (BATCH, ROWS, COLS)
    kw = dict(median=0)
    if variant == "loaded":
        kw = dict(median=5, prefilter=hs.Prefilter(*PF), smoothness=hs.Smoothness(1, LAM),
                  init=temporal.FlowInit(*[_cuda(p) for p in _np_init()]))
    out = {}
    if entry in ("flow", "jacobi", "weighted", "pyramid", "warped"):
        out["u"], out["v"] = _filled(shape, f32), _filled(shape, f32)
    I0, I1 = (_cuda(a) for a in _np_frames(which))
    solve = (LEVELS, WARPS, WINDOW, ITERS, ALPHA)
    if entry == "flow":
        hs.flow_device(I0, I1, WINDOW, ITERS, ALPHA, out["u"], out["v"], ws)
        torch.cuda.synchronize()
        # K1's outputs, which the call leaves in the workspace for a Jacobi call
        out["packed"], out["flags"] = _planes(ws, BATCH, ROWS, COLS)
    elif entry == "jacobi":
        for t, p in zip((out["u"], out["v"]), _np_init()):
            t.copy_(_cuda(p))
        hs.gradients_device(I0, I1, ws)
        hs.jacobi_device(ROWS, COLS, BATCH, WINDOW, ITERS, ALPHA, out["u"], out["v"], ws,
                         warm_start=True)
    elif entry == "weighted":
        u0, v0 = (_cuda(p) for p in _np_init()[:2])
        out["u"].copy_(u0)
        out["v"].copy_(v0)
        hs.warp_gradients_device(I0, I1, u0, v0, ws)
        g = hs.diffusivity_device(u0, v0, LAM)
        hs.jacobi_weighted_device(ROWS, COLS, BATCH, WINDOW, ITERS, ALPHA, g, out["u"], out["v"],
                                  ws)
    elif entry == "pyramid":
        hs.flow_pyramid_device(I0, I1, LEVELS, WINDOW, ITERS, ALPHA, out["u"], out["v"], ws)
    elif entry == "warped":
        temporal.flow_warped_device(I0, I1, *solve, u=out["u"], v=out["v"], workspace=ws, **kw)
    elif entry == "bidir":
        for name in ("uf", "vf", "ub", "vb", "err_f", "err_b"):
            out[name] = _filled(shape, f32)
        out["mask_f"], out["mask_b"] = _filled(shape, u8), _filled(shape, u8)
        out["counts_f"], out["counts_b"] = _filled((BATCH, 3), i32), _filled((BATCH, 3), i32)
        temporal.flow_bidir_device(I0, I1, *solve, workspace=ws, **out, **kw)
    else:
        # the loaded spec writes 8-bit frames
        odt = u8 if variant == "loaded" else f32
        nt = len(TIMES)
        out["flags"] = _filled((BATCH, nt, ROWS, COLS), u8)
        out["trusted"] = _filled((BATCH, nt), i32)
        if entry == "interp":
            out["out"] = _filled((BATCH, nt, ROWS, COLS), odt)
            temporal.flow_interp_device(I0, I1, TIMES, *solve, workspace=ws, **out, **kw)
        else:
            B0, B1 = (_cuda(b) for b in _np_bgr(which)[:2])
            out["out"] = _filled((BATCH, nt, ROWS, COLS, 3), odt)
            temporal.flow_interp_bgr_device(B0, B1, TIMES, *solve, workspace=ws, **out, **kw)
    torch.cuda.synchronize()
    return out


def _flow_errors(out, names, refs):
    errs = {n: norm_rel_err(out[n].cpu().numpy(), r) for n, r in zip(names, refs)}
    print("against the float64 reference: " + " ".join(f"{n} {e:.2e}" for n, e in errs.items()))
    return max(errs.values())


def _anchor_interp(out, variant, frames0, frames1, flows, who):
    """test_interp's end-to-end bound: |out - ref| <= band G + 1e-4 x 255 over
    the interior, band = 4 x 8 x 1e-4 x max|flow| px the flows' own tolerance, G
    the steepest step between adjacent pixels, pixels with a target within
    `band` of a rim left out.  An 8-bit output ("loaded") is floor(x + 0.5)
    clamped to 0..255: it equals the reference rounded the same way wherever the
    reference is further than the bound from a rounding step, and is one grey
    level off at most elsewhere."""
    got = out.cpu().numpy().astype(np.float64)
    band = 4.0 * GAIN * test_interp.TOL * max(float(np.abs(a).max()) for a in flows)
    for k in range(BATCH):
        a, b = frames0[k].astype(np.float64), frames1[k].astype(np.float64)
        G = max(float(np.abs(np.diff(x, axis=ax)).max()) for x in (a, b) for ax in (0, 1))
        bound = band * G + test_interp.TOL * 255.0
        for j, t in enumerate(TIMES):
            ref, _, rim, _ = frame_interp_np(a, b, *(f[k] for f in flows), t)
            assert (rim <= band).mean() <= 0.02
            if variant == "loaded":
                ref = np.clip(ref, 0.0, 255.0)
                rounded = np.floor(ref + 0.5)
                step = np.abs(ref + 0.5 - np.round(ref + 0.5)) <= bound  # near a rounding step
                d = np.where(rim <= band, 0.0, np.abs(got[k, j] - rounded))
                clear = float(_interior(np.where(step, 0.0, d)).max())
                worst = float(_interior(d).max())
                print(f"{who} pair {k} t {t}: 8-bit, off the rounded reference by {clear:.0f} "
                      f"away from a rounding step ({_interior(step).mean():.3f} of the pixels "
                      f"are near one), by {worst:.0f} anywhere")
                assert clear == 0.0 and worst <= 1.0
                continue
            d = np.where(rim <= band, 0.0, np.abs(got[k, j] - ref))
            worst = float(_interior(d).max())
            print(f"{who} pair {k} t {t}: worst interior |out - ref| {worst:.3e} (bound "
                  f"{bound:.3e})")
            assert worst <= bound


def _anchor_entry(entry, variant, out):
    """The 0x00 run against the float64 reference of the module that owns the
    entry point, with that module's bound."""
    I0, I1 = _np_frames("A")
    if entry in ("flow", "pyramid"):
        fn = (lambda a, b: oracle.flow(a, b, WINDOW, ITERS, ALPHA)) if entry == "flow" else \
            (lambda a, b: oracle.flow_pyramid(a, b, LEVELS, WINDOW, ITERS, ALPHA))
        uv = [fn(I0[k], I1[k]) for k in range(BATCH)]
        refs = [np.stack([p[j] for p in uv]) for j in range(2)]
        assert _flow_errors(out, "uv", refs) <= TOL
        if entry == "flow":  # one flag word per pair: 1 where the frames are not integral
            assert out["flags"].tolist() == [1 if k in NONINT else 0 for k in range(BATCH)]
    elif entry == "jacobi":
        u0, v0 = _np_init()[:2]
        uv = [oracle.jacobi(*oracle.gradients(I0[k], I1[k]), u0[k], v0[k], WINDOW, ITERS, ALPHA)
              for k in range(BATCH)]
        refs = [np.stack([p[j] for p in uv]) for j in range(2)]
        assert _flow_errors(out, "uv", refs) <= TOL
    elif entry == "weighted":
        u0, v0 = (p.astype(np.float64) for p in _np_init()[:2])
        uv = [jacobi_weighted_np(*warp_gradients_np(I0[k], I1[k], u0[k], v0[k]),
                                 diffusivity_np(u0[k], v0[k], LAM), u0[k], v0[k], WINDOW, ITERS,
                                 ALPHA) for k in range(BATCH)]
        refs = [np.stack([p[j] for p in uv]) for j in range(2)]
        assert _flow_errors(out, "uv", refs) <= test_smoothness.TOL
    elif entry == "warped":
        tol = test_warped.TOL if variant == "plain" else min(test_temporal.TOL, test_prefilter.TOL,
                                                             test_smoothness.TOL)
        assert _flow_errors(out, "uv", _ref_flows(variant, "grey")[:2]) <= tol
    elif entry == "bidir":
        flows = _ref_flows(variant, "grey")
        assert _flow_errors(out, ("uf", "vf", "ub", "vb"), flows) <= test_consistency.TOL
        for d in "fb":  # the counts are those of the mask
            mask, counts = out["mask_" + d].cpu().numpy(), out["counts_" + d].cpu().numpy()
            for k in range(BATCH):
                assert np.array_equal(counts[k], np.bincount(mask[k].ravel(), minlength=3)[:3])
    else:
        flags, trusted = out["flags"].cpu().numpy(), out["trusted"].cpu().numpy()
        assert np.array_equal(trusted.astype(np.int64), (flags == 0).sum(axis=(2, 3)))
        if entry == "interp":
            _anchor_interp(out["out"], variant, I0, I1, _ref_flows(variant, "grey"), entry)
        else:
            B0, B1 = _np_bgr("A")[:2]
            for c in range(3):
                _anchor_interp(out["out"][..., c], variant, B0[..., c], B1[..., c],
                               _ref_flows(variant, "bgr"), f"{entry} channel {c}")


def _workspace_cases():
    out = []
    for entry, variants in ENTRIES.items():
        for variant in variants:
            out.append((entry, variant, "k4"))
        out.append((entry, variants[-1], "auto"))
    return out


@gpu
@pytest.mark.parametrize("entry,variant,plan", _workspace_cases(),
                         ids=lambda x: x if isinstance(x, str) else None)
def test_workspace_guards_and_prior_contents(hs, entry, variant, plan):
    """The workspace is exactly the size function's bytes (with the prefilter's
    planes where one is on) between two 64 KiB guards, and starts as 0x00, as
    0xFF and as the finished workspace of the same call on other frames (what
    torch.empty hands a suite that runs one solve after another), under forced K4
    with 12-row segments ("k4": the quadratic solves' level 0 runs the warm
    f32-gradient interleaved body) or the automatic plan, over two side streams,
    and once over one.  The guards keep their bytes; every output has one set of
    bits; the flows are finite; the 0x00 run meets the float64 reference."""
    import torch
    need = _need(hs, entry, variant)
    assert need % 256 == 0
    forced = _k4(hs, SEG) if plan == "k4" else contextlib.nullcontext()
    with forced:
        with hs.max_streams_as(2):
            big, ws, lo = _guarded_workspace(need, 0x00)
            _run_entry(hs, entry, variant, "B", ws)
            assert _workspace_guards_intact(big, lo, need), "frames B"
            stale = ws.clone()
        runs = []
        for name, fill, streams in (("0x00", 0x00, 2), ("0xFF", 0xFF, 2), ("stale", stale, 2),
                                    ("0xFF, one stream", 0xFF, 1)):
            with hs.max_streams_as(streams):
                big, ws, lo = _guarded_workspace(need, fill)
                before = _launches(hs)
                runs.append((name, _run_entry(hs, entry, variant, "A", ws)))
                assert _workspace_guards_intact(big, lo, need), f"workspace {name}: a guard changed"
                if plan == "k4" and variant == "plain" and entry != "weighted":
                    assert _launches(hs) - before > 0  # the interleaved kernels ran
    first = runs[0][1]
    for name, out in runs[1:]:
        for key, t in out.items():
            assert _same_bits(t, first[key]), f"{key}: workspace {name} against 0x00"
    for key, t in first.items():
        if t.dtype == torch.float32 and not key.startswith("err"):
            assert torch.isfinite(t).all(), key
    _anchor_entry(entry, variant, first)


@gpu
@pytest.mark.parametrize("call", ["flow_bidir", "interpolate"])
def test_sequence_mode_forgets_a_clip_at_reset(hs, call):
    """The context owns the prediction planes and its workspace: clip A, reset,
    then clip B on one context gives the bits of clip B on a fresh one."""
    import temporal
    A = [test_temporal._square_at(x) for x in (50, 56, 64)]
    B = [np.ascontiguousarray(a[::-1, ::-1]) for a in A]
    args = (2, 1, 5, 20, ALPHA)

    def clip(ctx, frames):
        out = []
        for a, b in zip(frames, frames[1:]):
            if call == "flow_bidir":
                r = ctx.flow_bidir(a, b, *args, out_dtype=np.float32, median=5)
                out += [r.u, r.v, r.ub, r.vb, r.mask_f, r.mask_b, r.counts]
            else:
                out += list(ctx.interpolate(a, b, TIMES, *args, median=5, with_flags=True))
        return out

    with hs.Context(0) as used, hs.Context(0) as fresh:
        temporal.set_temporal(used, True)
        temporal.set_temporal(fresh, True)
        clip(used, A)
        temporal.reset(used)
        got, want = clip(used, B), clip(fresh, B)
    assert len(got) == len(want)
    for g, w in zip(got, want):
        assert g.tobytes() == w.tobytes()


# ------------------------------------------------------------- 3. without a GPU
SIZE_SHAPES = [(1, 7), (2, 2), (61, 130), (100, 129), (100, 130), (100, 260)]


def _size_functions(hs):
    """name -> f(rows, cols, batch, levels)."""
    return {"workspace_bytes": lambda r, c, b, l: hs.workspace_bytes(r, c, b),
            "prefilter_planes_bytes": lambda r, c, b, l: hs.prefilter_planes_bytes(r, c, b),
            "pyramid_workspace_bytes": hs.pyramid_workspace_bytes,
            "bidir_workspace_bytes": hs.bidir_workspace_bytes,
            "flow_interp_workspace_bytes": hs.flow_interp_workspace_bytes,
            "flow_interp_bgr_workspace_bytes": hs.flow_interp_bgr_workspace_bytes}


def test_size_functions_return_whole_256_byte_planes(hs):
    """The header aligns every plane of a workspace to 256 bytes; a size that is
    no multiple of it would leave the prefilter's planes, which follow the
    workspace's own layout, unaligned."""
    for name, fn in _size_functions(hs).items():
        for rows, cols in SIZE_SHAPES:
            for batch in (1, 3):
                for levels in (1, 3):
                    n = fn(rows, cols, batch, levels)
                    assert n > 0 and n % 256 == 0, (name, rows, cols, batch, levels)


def _a256(x):
    return (x + 255) // 256 * 256


def test_size_functions_hold_the_planes_their_calls_use(hs):
    """The layouts restated plane by plane, every plane rounded up to 256 bytes:
    the Jacobi workspace is the packed gradients, gx, gy, gt, the second (u, v)
    and one flag word per pair; a pyramid adds the pairs' saved flags and per
    coarser level two frames and (u, v); the bidirectional solve runs both ways
    in that; an interpolation adds four flows and two masks, and for BGR frames
    two grey planes; a prefilter two f32 frames.  A size function that loses a
    plane, or 256 bytes of one, fails here."""
    fns = _size_functions(hs)
    for rows, cols in SIZE_SHAPES:
        for batch in (1, 3):
            for levels in (1, 2, 3):
                n = rows * cols * batch
                jac = 6 * _a256(4 * n) + _a256(4 * batch)
                pyr, r, c = _a256(jac + 4 * batch), rows, cols
                for _ in range(1, levels):
                    r, c = (r + 1) // 2, (c + 1) // 2
                    pyr += 4 * _a256(4 * r * c * batch)
                interp = pyr + 4 * _a256(4 * n) + 2 * _a256(n)
                want = {"workspace_bytes": jac, "prefilter_planes_bytes": 2 * _a256(4 * n),
                        "pyramid_workspace_bytes": pyr, "bidir_workspace_bytes": pyr,
                        "flow_interp_workspace_bytes": interp,
                        "flow_interp_bgr_workspace_bytes": interp + 2 * _a256(n)}
                for name, size in want.items():
                    assert fns[name](rows, cols, batch, levels) == size, (name, rows, cols, batch,
                                                                          levels)


def test_size_functions_are_monotone(hs):
    """Non-decreasing in rows, cols, batch and levels over the module's shapes."""
    for name, fn in _size_functions(hs).items():
        for rows, cols in SIZE_SHAPES:
            for batch in (1, 2, 3):
                for levels in (1, 2, 3):
                    n = fn(rows, cols, batch, levels)
                    for more in ((rows + 1, cols, batch, levels), (rows, cols + 1, batch, levels),
                                 (rows, cols, batch + 1, levels), (rows, cols, batch, levels + 1)):
                        assert fn(*more) >= n, (name, rows, cols, batch, levels, more)


def test_core_entry_points_refuse_a_short_workspace_without_a_gpu(hs):
    """hsflow_flow_device, hsflow_gradients_device, hsflow_jacobi_device,
    hsflow_flow_pyramid_device and hsflow_pyramid_build_device (the warped family
    is in tests/golden/arg_errors.json and its modules): one byte less than the
    size function is HSFLOW_ERR_ARG before any device work -- the pointers are
    never dereferenced.  The size check is the last one, so that the exact size
    passes it shows without a GPU only where the call then has nothing to launch
    (a warm start of 0 iterations); the GPU tests above pass exactly that size to
    every entry point."""
    L, E = hs.lib(), hs.HSFLOW_ERR_ARG
    A = [k << 20 for k in range(1, 8)]  # 1 MiB apart: no two planes share a byte
    ws = 1 << 26
    levels = (ctypes.c_void_p * 2)(A[4], A[5])
    for rows, cols, batch in ((16, 16, 1), (100, 130, 3), (1, 7, 1)):
        jac = hs.workspace_bytes(rows, cols, batch)
        pyr = hs.pyramid_workspace_bytes(rows, cols, batch, 3)
        calls = {
            "flow": lambda n: L.hsflow_flow_device(A[0], A[1], hs.F32, rows, cols, batch, 5, 10,
                                                   1.0, A[2], A[3], ws, n, None),
            "gradients": lambda n: L.hsflow_gradients_device(A[0], A[1], hs.F32, rows, cols, batch,
                                                             None, None, None, ws, n, None),
            "jacobi": lambda n: L.hsflow_jacobi_device(rows, cols, batch, 5, 10, 1.0, 1, A[2], A[3],
                                                       ws, n, None),
            "pyramid_build": lambda n: L.hsflow_pyramid_build_device(
                A[0], A[1], hs.F32, rows, cols, batch, 3, levels, levels, ws, n, None),
        }
        for name, call in calls.items():
            assert call(jac - 1) == E, (name, rows, cols, batch)
            assert "workspace" in L.hsflow_last_error(None).decode()
            assert call(0) == E
        assert L.hsflow_flow_pyramid_device(A[0], A[1], hs.F32, rows, cols, batch, 3, 5, 10, 1.0,
                                            A[2], A[3], ws, pyr - 1, None) == E
        assert "workspace" in L.hsflow_last_error(None).decode()
        if batch == 1:  # nothing to launch: the exact size passes, one byte less does not
            idle = (rows, cols, batch, 5, 0, 1.0, 1, A[2], A[3], ws)
            assert L.hsflow_jacobi_device(*idle, jac, None) == hs.HSFLOW_OK
            assert L.hsflow_jacobi_device(*idle, jac - 1, None) == E
