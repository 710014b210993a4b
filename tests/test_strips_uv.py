"""The interleaved (u, v) between K4 passes (csrc/hsflow_strips.hip, IIN /
IOUT) against K2 and against the same K4 solve with every pass planar.

Between two full-depth K4 passes the state is stored as 16-byte groups
{u0, u1, v0, v1}, even rows in the plane that otherwise holds u, odd rows in
the one that holds v; the registers and the arithmetic are the planar pass's,
so every comparison here is on raw 32-bit words.  The layout needs an even
height and width (it lives in the two planes it replaces); the odd shapes
below must plan no interleaved pass and run the planar kernels, and w 5 at
KB 4 and 5 fall back to planar as well.  K4 is forced and the segments are
short, so that small planes have several segments in both stream directions
and one to three strips.  The plan (hsflow_uv_interleave_passes) needs no GPU;
the launch counter tells, per case, that the interleaved kernels really ran.
The three C entry points are reached through hsflow.lib()."""
import contextlib

import numpy as np
import pytest
import torch

gpu = pytest.mark.gpu

KB = {5: 6, 3: 8}


@contextlib.contextmanager
def _k4(hs, strip_rows=0, kb=0, kernel=4):
    hs.set_jacobi_kernel(kernel)
    hs.set_strip_rows(strip_rows)
    hs.set_iters_per_launch(kb)
    try:
        yield
    finally:
        hs.set_jacobi_kernel(0)
        hs.set_strip_rows(0)
        hs.set_iters_per_launch(0)


@contextlib.contextmanager
def _interleave(hs, on):
    L = hs.lib()
    prev = L.hsflow_uv_interleave()
    assert L.hsflow_set_uv_interleave(int(on)) == 0
    try:
        yield
    finally:
        L.hsflow_set_uv_interleave(prev)


def _planned(hs, rows, cols, batch, w, iters):
    n = hs.lib().hsflow_uv_interleave_passes(rows, cols, batch, w, iters)
    assert n >= 0
    return n


def _launches(hs):
    return hs.lib().hsflow_uv_interleave_launches()


# ---------------------------------------------------------------- the plan
def test_plan_of_the_headline_leg(hs):
    assert hs.lib().hsflow_uv_interleave() == 1  # on by default
    assert _planned(hs, 1080, 1920, 8, 5, 300) == 49  # 50 passes, the last one planar
    assert _planned(hs, 1080, 1920, 8, 5, 6) == 0  # one pass
    # 2^29 - 4096 px: the planar kernels (an odd height)
    assert _planned(hs, 131071, 4096, 1, 5, 300) == 0
    with _interleave(hs, False):
        assert _planned(hs, 1080, 1920, 8, 5, 300) == 0
    assert hs.lib().hsflow_uv_interleave() == 1
    assert hs.lib().hsflow_uv_interleave_passes(0, 1920, 8, 5, 300) < 0


@pytest.mark.parametrize("w", [5, 3])
def test_plan_hands_planes_to_k2(hs, w):
    """iters = 3 KB + 1: three full K4 passes and a short K2 one; the third
    writes planes for it."""
    kb = KB[w]
    with _k4(hs):
        assert [_planned(hs, 100, 130, 2, w, n * kb) for n in (1, 2, 3, 4)] == [0, 1, 2, 3]
        assert _planned(hs, 100, 130, 2, w, 3 * kb + 1) == 3 - 1
        assert _planned(hs, 100, 130, 2, w, kb - 1) == 0
        # odd heights and widths stay planar, and so does K2
        assert _planned(hs, 61, 130, 2, w, 3 * kb) == 0
        assert _planned(hs, 100, 129, 2, w, 3 * kb) == 0
    with _k4(hs, kernel=2):
        assert _planned(hs, 100, 130, 2, w, 3 * kb) == 0


@pytest.mark.parametrize("kb", [4, 5])
def test_plan_shallow_depths_stay_planar(hs, kb):
    with _k4(hs, kb=kb):
        assert hs.iters_per_launch(100, 130, 2, 5) == kb
        assert _planned(hs, 100, 130, 2, 5, 4 * kb) == 0


# ---------------------------------------------------------------- the bits
def _frames(batch, rows, cols, seed=3, nonint=()):
    rng = np.random.default_rng(seed + 1000 * rows + cols)
    a = rng.integers(0, 256, (batch, rows, cols)).astype(np.float64)
    b = rng.integers(0, 256, (batch, rows, cols)).astype(np.float64)
    for i in nonint:
        a[i] = a[i] * 0.73 + 0.21
        b[i] = b[i] * 0.61 + 3.3
    return (torch.from_numpy(a.astype(np.float32)).cuda(),
            torch.from_numpy(b.astype(np.float32)).cuda())


def _words(t):
    return t.contiguous().view(torch.int32)


def _solve(hs, I0, I1, w, iters, warm=None, poison=0xA5, stream=None):
    """(u, v) as 32-bit words.  Cold: hsflow_flow_device; warm: K1, then the
    Jacobi passes from a copy of `warm`.  Every workspace byte starts as
    `poison`, (u, v) of a cold solve as NaN."""
    batch, rows, cols = I0.shape
    ws = torch.full((hs.workspace_bytes(rows, cols, batch),), poison, dtype=torch.uint8,
                    device="cuda")
    if warm is None:
        u = torch.full(I0.shape, float("nan"), device="cuda")
        v = torch.full(I0.shape, float("nan"), device="cuda")
        hs.flow_device(I0, I1, w, iters, 1.0, u, v, ws, stream)
    else:
        u, v = warm[0].clone(), warm[1].clone()
        hs.gradients_device(I0, I1, ws, stream=stream)
        hs.jacobi_device(rows, cols, batch, w, iters, 1.0, u, v, ws, warm_start=True,
                         stream=stream)
    torch.cuda.synchronize()
    return _words(u), _words(v)


def _check(hs, I0, I1, w, iters, strip_rows, kb=0, warm=None, poison=0xA5, streams=1):
    """Forced K4 with the interleave on against forced K2 and against the
    interleave off; the counter rises by the plan (per chain) or not at all."""
    batch, rows, cols = I0.shape
    with hs.max_streams_as(streams):
        with _k4(hs, strip_rows, kb):
            planned = _planned(hs, rows, cols, batch, w, iters)
            before = _launches(hs)
            on = _solve(hs, I0, I1, w, iters, warm, poison)
            assert _launches(hs) - before == planned * min(streams, batch)
            with _interleave(hs, False):
                assert _planned(hs, rows, cols, batch, w, iters) == 0
                before = _launches(hs)
                off = _solve(hs, I0, I1, w, iters, warm, poison)
                assert _launches(hs) - before == 0
        with _k4(hs, kernel=2):
            k2 = _solve(hs, I0, I1, w, iters, warm, poison)
    for name, a, b, c in zip("uv", on, off, k2):
        assert torch.equal(a, b), f"{name}: interleaved against planar K4"
        assert torch.equal(a, c), f"{name}: interleaved K4 against K2"
    return on, planned


@gpu
@pytest.mark.parametrize("w", [5, 3])
@pytest.mark.parametrize("n", ["1", "2", "3", "4", "3+1"])
def test_pass_counts(hs, w, n):
    """No interleaved pass, one buffer, both buffers, both twice, and the
    hand-over of planes to a short K2 pass."""
    kb = KB[w]
    iters = 3 * kb + 1 if n == "3+1" else int(n) * kb
    I0, I1 = _frames(2, 100, 130)
    _, planned = _check(hs, I0, I1, w, iters, 12)
    assert planned == {"1": 0, "2": 1, "3": 2, "4": 3, "3+1": 2}[n]


@gpu
@pytest.mark.parametrize("kb", [4, 5])
def test_shallow_depths_fall_back_to_planar(hs, kb):
    I0, I1 = _frames(2, 100, 130)
    _, planned = _check(hs, I0, I1, 5, 3 * kb, 12, kb=kb)
    assert planned == 0


# rows 61: an odd height (planar); rows 100 with cols 130 and 260 (and the
# extra 2, 104, 106, 208: one lane, one strip exactly, one strip and a pair,
# two strips exactly) run interleaved, the odd widths planar
@gpu
@pytest.mark.parametrize("cols", [1, 3, 105, 129, 130, 209, 260, 2, 104, 106, 208])
@pytest.mark.parametrize("rows,seg_rows", [(61, 12), (61, 16), (100, 12), (100, 16)])
def test_shapes(hs, rows, cols, seg_rows):
    I0, I1 = _frames(2, rows, cols)
    _, planned = _check(hs, I0, I1, 5, 3 * KB[5], seg_rows)
    assert planned == (2 if rows % 2 == 0 and cols % 2 == 0 else 0)


@gpu
@pytest.mark.parametrize("cols", [130, 209, 260])
@pytest.mark.parametrize("rows,seg_rows", [(61, 16), (100, 16)])
def test_shapes_window_3(hs, rows, cols, seg_rows):
    I0, I1 = _frames(3, rows, cols)
    _check(hs, I0, I1, 3, 3 * KB[3], seg_rows)


@gpu
@pytest.mark.parametrize("w", [5, 3])
@pytest.mark.parametrize("n", [1, 2, 3])
def test_warm_start(hs, w, n):
    """A random state: the first pass reads the caller's planes (n odd: a
    copy of them, the parity rule's), the later ones the interleaved state."""
    I0, I1 = _frames(2, 100, 130)
    g = torch.Generator(device="cuda").manual_seed(5)
    warm = (torch.randn(I0.shape, device="cuda", generator=g) * 0.1,
            torch.randn(I0.shape, device="cuda", generator=g) * 0.1)
    _, planned = _check(hs, I0, I1, w, n * KB[w], 12, warm=warm)
    assert planned == n - 1


@gpu
@pytest.mark.parametrize("streams", [1, 2])
def test_mixed_gradient_formats(hs, streams):
    """[integral, non-integral, integral]: the packed and the f32-gradient
    body in one launch, and per chain under a split."""
    I0, I1 = _frames(3, 100, 130, nonint=(1,))
    _, planned = _check(hs, I0, I1, 5, 3 * KB[5], 12, streams=streams)
    assert planned == 2


@gpu
@pytest.mark.parametrize("cols", [130, 209])
def test_poisoned_workspace(hs, cols):
    """Every workspace byte 0xFF (NaNs) before the solve: nothing of it is read."""
    I0, I1 = _frames(2, 100, cols)
    ref, _ = _check(hs, I0, I1, 5, 3 * KB[5], 12)
    got, _ = _check(hs, I0, I1, 5, 3 * KB[5], 12, poison=0xFF)
    for a, b in zip(got, ref):
        assert torch.equal(a, b)
        assert torch.isfinite(a.view(torch.float32)).all()


@gpu
def test_captured_solve_replays_the_eager_bits(hs):
    """A captured 3 KB solve, its outputs NaN-filled, then replayed."""
    I0, I1 = _frames(2, 100, 130)
    iters = 3 * KB[5]
    with _k4(hs, 12), hs.max_streams_as(1):
        ref = _solve(hs, I0, I1, 5, iters)
        batch, rows, cols = I0.shape
        ws = torch.empty(hs.workspace_bytes(rows, cols, batch), dtype=torch.uint8, device="cuda")
        u = torch.empty(I0.shape, device="cuda")
        v = torch.empty(I0.shape, device="cuda")
        hs.flow_device(I0, I1, 5, iters, 1.0, u, v, ws)  # warm-up outside the capture
        torch.cuda.synchronize()
        before = _launches(hs)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, capture_error_mode="thread_local"):
            hs.flow_device(I0, I1, 5, iters, 1.0, u, v, ws, torch.cuda.current_stream())
        torch.cuda.synchronize()
        assert _launches(hs) - before == 2
    u.fill_(float("nan"))
    v.fill_(float("nan"))
    ws.fill_(0xFF)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(_words(u), ref[0]) and torch.equal(_words(v), ref[1])
