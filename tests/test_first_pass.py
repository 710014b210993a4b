"""The fused first pass of a cold K4 solve (csrc/hsflow_strips.hip,
hs_jacobi_strip_first_kernel) against the same solve with K1 in front of it.

Fused, pass 0 reads the frames, computes K1's gradients in registers and
writes the packed plane and the flags besides (u, v).  Every case runs one
solve with the fusion on and one with it off (hsflow_set_first_pass_fusion)
and compares (u, v), the workspace's packed plane and the flags as raw
32-bit words, so NaNs and signed zeros count.  K4 is forced, so that small
shapes run it.  The two paths agree by design, so every case also checks,
through hsflow_first_pass_launches, that the fused solve launched the fused
pass (once per side-stream chain) and the other one did not."""
import contextlib

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

KINDS = ("u8", "f16", "f32", "f32n", "f64")


@contextlib.contextmanager
def _k4(hs, strip_rows=0, kb=0):
    hs.set_jacobi_kernel(4)
    hs.set_strip_rows(strip_rows)
    hs.set_iters_per_launch(kb)
    try:
        yield
    finally:
        hs.set_jacobi_kernel(0)
        hs.set_strip_rows(0)
        hs.set_iters_per_launch(0)


def _frames(kind, batch, rows, cols, seed=7, nonint=None):
    """Random 8-bit-valued frames as `kind`; "f32n" (or the pairs listed in
    `nonint`) are scaled and shifted off the integers."""
    rng = np.random.default_rng(seed + 1000 * rows + cols)
    a = rng.integers(0, 256, (batch, rows, cols)).astype(np.float64)
    b = rng.integers(0, 256, (batch, rows, cols)).astype(np.float64)
    which = range(batch) if kind == "f32n" else (nonint or ())
    for i in which:
        a[i] = a[i] * 0.73 + 0.21
        b[i] = b[i] * 0.61 + 3.3
    dt = {"u8": np.uint8, "f16": np.float16, "f32": np.float32, "f32n": np.float32,
          "f64": np.float64}[kind]
    return torch.from_numpy(a.astype(dt)).cuda(), torch.from_numpy(b.astype(dt)).cuda()


def _words(t):
    return t.contiguous().view(torch.int32)


def _planes(ws, batch, rows, cols):
    """The packed plane and the flags of a workspace (carve(): six planes of
    n * 4 bytes, each rounded up to 256, then the flags), as 32-bit words."""
    n = batch * rows * cols
    plane = (n * 4 + 255) // 256 * 256
    return (ws[:n * 4].view(torch.int32).clone(),
            ws[6 * plane:6 * plane + 4 * batch].view(torch.int32).clone())


def _solve(hs, I0, I1, w, iters, alpha, fuse, stream=None, launches=None):
    """(u, v, packed plane, flags) of one cold solve, as 32-bit words;
    `launches`: the fused first passes it must launch (None: not checked)."""
    batch, rows, cols = I0.shape
    ws = torch.full((hs.workspace_bytes(rows, cols, batch),), 0xA5, dtype=torch.uint8,
                    device="cuda")
    u = torch.full((batch, rows, cols), float("nan"), device="cuda")
    v = torch.full((batch, rows, cols), float("nan"), device="cuda")
    before = hs.first_pass_launches()
    with hs.first_pass_fusion_as(fuse):
        hs.flow_device(I0, I1, w, iters, alpha, u, v, ws, stream)
    torch.cuda.synchronize()
    if launches is not None:
        assert hs.first_pass_launches() - before == launches
    return (_words(u), _words(v)) + _planes(ws, batch, rows, cols)


def _same(a, b):
    for x, y, name in zip(a, b, ("u", "v", "packed plane", "flags")):
        assert torch.equal(x, y), name


def _ab(hs, I0, I1, w=5, iters=12, alpha=1.0, chains=1):
    """`chains`: fused passes the fused solve must launch (0: it must not fuse)."""
    on = _solve(hs, I0, I1, w, iters, alpha, True, launches=chains)
    off = _solve(hs, I0, I1, w, iters, alpha, False, launches=0)
    _same(on, off)
    return on


# 1x1 .. 2x2: reflect-101 with one row / column and both ends at once;
# 3x130, 97x209: odd widths (the column-by-column body), two and three
# strips; 90x232 at 48 rows: a segment streamed down and one up, the last
# strip partly outside; 100x140 at 84 rows: a last segment of 16 rows, too
# short for the stream's unchecked blocks
SHAPES = [(1, 1, 0), (1, 7, 0), (7, 1, 0), (2, 2, 0), (3, 130, 0), (97, 209, 0), (90, 232, 48),
          (100, 140, 84)]


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("rows,cols,strip_rows", SHAPES)
def test_fused_equals_unfused(hs, rows, cols, strip_rows, kind):
    """Every frame type (f64 takes the unfused path both times)."""
    I0, I1 = _frames(kind, 1, rows, cols)
    with _k4(hs, strip_rows):
        got = _ab(hs, I0, I1, chains=0 if kind == "f64" else 1)
    assert int(got[3][0]) == (1 if kind == "f32n" else 0)


@pytest.mark.parametrize("kind", ["u8", "f32n"])
@pytest.mark.parametrize("iters", [5, 6, 7, 12, 13])
def test_iteration_counts(hs, iters, kind):
    """6: the fused pass is the whole solve; 7 and 13: a shorter K2 pass
    after it; 5: below the depth, unfused."""
    I0, I1 = _frames(kind, 1, 97, 209)
    with _k4(hs):
        _ab(hs, I0, I1, iters=iters, chains=0 if iters < 6 else 1)


@pytest.mark.parametrize("kind", ["u8", "f16", "f32n"])
@pytest.mark.parametrize("rows,cols,strip_rows", [(97, 209, 0), (90, 232, 48)])
@pytest.mark.parametrize("w,kb", [(5, 5), (5, 4), (3, 0)])
def test_other_depths_and_window_3(hs, w, kb, rows, cols, strip_rows, kind):
    """w 5 at KB 5 and 4, w 3 at its KB 8: two full passes and a short one."""
    I0, I1 = _frames(kind, 1, rows, cols)
    with _k4(hs, strip_rows, kb):
        _ab(hs, I0, I1, w=w, iters=2 * (kb or 8) + 1)


@pytest.mark.parametrize("kind,alpha", [("u8", 0.0), ("u8", 2.5), ("f32n", 2.5)])
def test_alpha(hs, kind, alpha):
    """alpha = 0: where Ix = Iy = 0 the operator is NaN; the same pattern."""
    I0, I1 = _frames(kind, 1, 97, 209)
    I0[0, 40:60, 50:90] = 17  # a flat patch: zero gradients inside
    with _k4(hs):
        got = _ab(hs, I0, I1, alpha=alpha)
    if alpha == 0.0:
        assert torch.isnan(got[0].view(torch.float32)).any()


@pytest.mark.parametrize("streams", [1, 2])
def test_mixed_batch_per_chain_flags(hs, streams):
    """[integral, non-integral, integral]: each chain zeroes and sets its own
    slice of the flags and runs K1f for its pairs."""
    I0, I1 = _frames("f32", 3, 97, 209, nonint=(1,))
    with _k4(hs), hs.max_streams_as(streams):
        got = _ab(hs, I0, I1, chains=streams)
    assert got[3].tolist() == [0, 1, 0]


def test_captured_solve_replays_the_eager_bits(hs):
    """A capture on the origin stream with the batch split over two side
    streams (each runs its own prologue), replayed, against the eager solve."""
    I0, I1 = _frames("f32", 3, 97, 209, nonint=(1,))
    with _k4(hs):
        ref = _solve(hs, I0, I1, 5, 13, 1.0, True)
        batch, rows, cols = I0.shape
        before = hs.first_pass_launches()
        ws = torch.empty(hs.workspace_bytes(rows, cols, batch), dtype=torch.uint8, device="cuda")
        u = torch.empty(I0.shape, device="cuda")
        v = torch.empty(I0.shape, device="cuda")
        stream = torch.cuda.current_stream()
        cap = torch.cuda.Stream()
        cap.wait_stream(stream)
        with torch.cuda.stream(cap):
            hs.flow_device(I0, I1, 5, 13, 1.0, u, v, ws, cap)
        stream.wait_stream(cap)
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with hs.max_streams_as(2), torch.cuda.graph(graph, capture_error_mode="thread_local"):
            hs.flow_device(I0, I1, 5, 13, 1.0, u, v, ws, torch.cuda.current_stream())
        torch.cuda.synchronize()
        assert hs.first_pass_launches() - before == 2 + 2  # eager and captured, two chains
    u.fill_(float("nan"))
    v.fill_(float("nan"))
    ws.fill_(0xA5)
    graph.replay()
    torch.cuda.synchronize()
    _same((_words(u), _words(v)) + _planes(ws, batch, rows, cols), ref)


@pytest.mark.parametrize("rows,cols,strip_rows", [(97, 209, 0), (90, 232, 48)])
@pytest.mark.parametrize("kind,lead", [("u8", 3), ("f16", 1), ("f16", 2), ("f32", 1), ("f32", 2)])
def test_frames_inside_guarded_allocation(hs, kind, lead, rows, cols, strip_rows):
    """The frames `lead` elements into a larger allocation full of 255 / NaN
    (a base that is not 16-byte aligned; for lead 1 of f16 / f32 not even
    aligned to a column pair): a tap that leaves the pair's plane changes
    the result."""
    I0, I1 = _frames(kind, 1, rows, cols)
    n = rows * cols
    guarded = []
    for t in (I0, I1):
        big = torch.full((n + 64,), 255 if kind == "u8" else float("nan"), dtype=t.dtype,
                         device="cuda")
        big[lead:lead + n] = t.reshape(-1)
        guarded.append(big[lead:lead + n].view(1, rows, cols))
        assert guarded[-1].data_ptr() % 16 != 0
    with _k4(hs, strip_rows):
        ref = _ab(hs, I0, I1)
        got = _solve(hs, guarded[0], guarded[1], 5, 12, 1.0, True, launches=1)
    _same(got, ref)


@pytest.mark.parametrize("kind", ["u8", "f32n"])
@pytest.mark.parametrize("levels", [1, 3])
def test_pyramid_coarsest_level(hs, levels, kind):
    """The pyramid's coarsest level is a cold solve (levels = 1: the only
    one): fused once, and the finer, warm-started levels keep K1."""
    I0, I1 = _frames(kind, 1, 97, 209)
    res = []
    with _k4(hs):
        for fuse in (True, False):
            before = hs.first_pass_launches()
            with hs.first_pass_fusion_as(fuse):
                u, v = hs.flow_pyramid_device(I0, I1, levels, 5, 13, 1.0)
            torch.cuda.synchronize()
            assert hs.first_pass_launches() - before == (1 if fuse else 0)
            res.append((_words(u), _words(v)))
    assert torch.equal(res[0][0], res[1][0]) and torch.equal(res[0][1], res[1][1])


@pytest.mark.parametrize("dtype", [np.uint8, np.float32])
def test_host_buffer_solves(hs, dtype):
    """hsflow_flow and hsflow_flow_bgr (8-bit gray made on the GPU)."""
    rng = np.random.default_rng(11)
    a = rng.integers(0, 256, (97, 209)).astype(dtype)
    b = rng.integers(0, 256, (97, 209)).astype(dtype)
    bgr = rng.integers(0, 256, (2, 97, 209, 3)).astype(np.uint8)
    ctx = hs.default_context()
    res = []
    with _k4(hs):
        for fuse in (True, False):
            before = hs.first_pass_launches()
            with hs.first_pass_fusion_as(fuse):
                r = ctx.flow(a, b, 5, 13, 1.0, out_dtype=np.float32)
                g = ctx.flow_bgr(bgr[0], bgr[1], 5, 13, 1.0, out_dtype=np.float32)
            assert hs.first_pass_launches() - before == (2 if fuse else 0)
            res.append([np.ascontiguousarray(x).view(np.int32) for x in (*r, *g)])
    for x, y in zip(*res):
        assert np.array_equal(x, y)
