"""The Jacobi kernels outside windows 3..9 against the float64 oracle:
hs_jacobi_kernel (K2w, windows 1 and 2: one wave per 64-column region, 48-row
packed and 24-row f32-gradient regions, four tiles per workgroup behind the
XCD block remap) and hs_jacobi_generic_kernel (K2g, windows 10..63, one
iteration per launch through the ping-pong planes).

Every test first asserts through hs.jacobi_kernel_name that the kernel it
means to test is the one that runs, and through hs.iters_per_launch the depth
it relies on.  Frames come from numpy (fixed seeds); every workspace is
prefilled with 0xA5 bytes and every output with NaN, so state a kernel fails
to write shows.  Reference: oracle.flow for cold solves, oracle.jacobi on
oracle.gradients for warm starts; bound: max|got - ref| / max|ref| <= 1e-4
(the TOL of test_gpu_parity.py), exactly 0 where the oracle's
plane is identically 0.  Each comparison prints its figure."""
import numpy as np
import pytest

import oracle
from conftest import norm_rel_err

TOL = 1e-4
K2W = "hs_jacobi_kernel"
K2G = "hs_jacobi_generic_kernel"
WINDOWS = (1, 2, 10, 11, 32, 63)
KINDS = ("u8", "f32n", "f16q")


def _kernel_of(w):
    return K2W if w <= 2 else K2G


def _pair(kind, rows, cols, batch=None, seed=11, nonint=()):
    """Random 8-bit-valued frames, [rows, cols] or [batch, rows, cols]: "u8";
    "f32" integer-valued float32 with the pairs in `nonint` scaled and shifted
    off the integers as "f32n" has every pair (a * 0.73 + 0.21, b * 0.61 +
    3.3); "f16q" float16 integers + 0.25 (dyadic, non-integral)."""
    rng = np.random.default_rng(seed + 1000 * rows + cols)
    shape = (batch or 1, rows, cols)
    a = rng.integers(0, 256, shape).astype(np.float64)
    b = rng.integers(0, 256, shape).astype(np.float64)
    for i in (range(shape[0]) if kind == "f32n" else nonint):
        a[i] = a[i] * 0.73 + 0.21
        b[i] = b[i] * 0.61 + 3.3
    if kind == "f16q":
        a, b = a + 0.25, b + 0.25
    dt = {"u8": np.uint8, "f32": np.float32, "f32n": np.float32, "f16q": np.float16}[kind]
    a, b = a.astype(dt), b.astype(dt)
    return (a, b) if batch else (a[0], b[0])


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _poisoned(hs, shape):
    """(u, v, workspace) for frames of `shape`: NaN planes, 0xA5 bytes."""
    import torch
    rows, cols = shape[-2:]
    batch = int(np.prod(shape[:-2], dtype=np.int64))
    ws = torch.full((hs.workspace_bytes(rows, cols, batch),), 0xA5, dtype=torch.uint8,
                    device="cuda")
    u = torch.full(tuple(shape), float("nan"), device="cuda")
    v = torch.full(tuple(shape), float("nan"), device="cuda")
    return u, v, ws


def _expect_kernel(hs, rows, cols, batch, w, kb=None):
    assert hs.jacobi_kernel_name(rows, cols, batch, w) == _kernel_of(w)
    want = kb if kb is not None else (8 if w <= 2 else 1)
    assert hs.iters_per_launch(rows, cols, batch, w) == want


def _solve(hs, I0, I1, w, iters, alpha=1.0, kb=None):
    """Cold flow_device of numpy frames -> numpy (u, v), float32."""
    import torch
    rows, cols = I0.shape[-2:]
    batch = int(np.prod(I0.shape[:-2], dtype=np.int64))
    _expect_kernel(hs, rows, cols, batch, w, kb)
    u, v, ws = _poisoned(hs, I0.shape)
    hs.flow_device(_dev(I0), _dev(I1), w, iters, alpha, u, v, ws)
    torch.cuda.synchronize()
    return u.cpu().numpy(), v.cpu().numpy()


def _f64(a):
    return np.asarray(a, np.float64)


def _close(got, ref, what):
    """got (u, v) float32 against ref (u, v) float64, plane by plane."""
    for g, r, name in zip(got, ref, "uv"):
        assert g.shape == r.shape
        if np.abs(r).max() == 0:
            print(f"{what} {name}: oracle identically 0")
            assert not g.any(), f"{what} {name}: oracle is 0"
            continue
        err = norm_rel_err(g, r)
        print(f"{what} {name}: norm_rel_err {err:.3e} (bound {TOL:.0e})")
        assert err <= TOL, f"{what} {name}: {err:.3e}"


def _same(a, b):
    """Bit for bit: float32 planes compared as 32-bit words."""
    return all(np.array_equal(x.view(np.int32), y.view(np.int32)) for x, y in zip(a, b))


# ------------------------------------------------------------- cold solves
@pytest.mark.gpu
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("w", WINDOWS)
def test_windows_and_gradient_formats(hs, w, kind):
    I0, I1 = _pair(kind, 45, 70)
    got = _solve(hs, I0, I1, w, 7)
    _close(got, oracle.flow(_f64(I0), _f64(I1), w, 7, 1.0), f"w{w} {kind} 45x70")


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["u8", "f32n"])
@pytest.mark.parametrize("rows,cols", [(5, 3), (45, 70)])
@pytest.mark.parametrize("w", [32, 63])
def test_window_larger_than_the_image_and_the_cap(hs, w, rows, cols, kind):
    """63 is HSFLOW_MAX_WINDOW (64 is refused); at 5x3 every window sum is
    the whole plane."""
    I0, I1 = _pair(kind, rows, cols, seed=5)
    got = _solve(hs, I0, I1, w, 13)
    _close(got, oracle.flow(_f64(I0), _f64(I1), w, 13, 1.0), f"w{w} {kind} {rows}x{cols}")
    with pytest.raises(hs.HsflowError):
        hs.flow_device(_dev(I0), _dev(I1), 64, 1, 1.0)
    assert hs.jacobi_kernel_name(rows, cols, 1, 64) == ""


# 49x65, 97x129: one column past K2w's 64-column tile at w 1 and one row past
# its 48-row tile (at w 2, depth 8: 56-column, 40-row tiles, 16-row f32
# regions); 41x57: one past the w 2 tile both ways; all of them cross K2g's
# 64 x 4 blocks
SHAPES = [(1, 1), (1, 7), (7, 1), (2, 2), (3, 130), (41, 57), (49, 65), (97, 129)]


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["u8", "f32n"])
@pytest.mark.parametrize("rows,cols", SHAPES)
@pytest.mark.parametrize("w", [1, 2, 11])
def test_ragged_and_tiny_shapes(hs, w, rows, cols, kind):
    I0, I1 = _pair(kind, rows, cols)
    got = _solve(hs, I0, I1, w, 13)
    _close(got, oracle.flow(_f64(I0), _f64(I1), w, 13, 1.0), f"w{w} {kind} {rows}x{cols}")


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["u8", "f32n"])
@pytest.mark.parametrize("iters", [0, 1, 7, 8, 9, 19])
@pytest.mark.parametrize("w", [1, 2])
def test_iteration_counts_per_wave_kernel(hs, w, iters, kind):
    """At depth 8: no pass (u = v = 0), a short single pass, exactly one
    pass, a pass and a remainder, two passes and a remainder."""
    I0, I1 = _pair(kind, 49, 65)
    got = _solve(hs, I0, I1, w, iters)
    _close(got, oracle.flow(_f64(I0), _f64(I1), w, iters, 1.0), f"w{w} {kind} {iters} it")


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["u8", "f32n"])
@pytest.mark.parametrize("iters", [1, 2, 7])
def test_iteration_counts_generic_kernel(hs, iters, kind):
    """One iteration per launch: the last of an odd and of an even number of
    ping-pong passes lands in the caller's planes."""
    I0, I1 = _pair(kind, 49, 65)
    got = _solve(hs, I0, I1, 11, iters)
    _close(got, oracle.flow(_f64(I0), _f64(I1), 11, iters, 1.0), f"w11 {kind} {iters} it")


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["u8", "f32n"])
@pytest.mark.parametrize("w", [1, 2])
def test_blocking_depth_is_bit_invariant(hs, w, kind):
    """hsum's promise for the per-wave kernel: depths 1, 2, 4 and 8 give the
    same bits (19 iterations: 19, 10, 5 and 3 passes, the last one shorter
    for 2, 4 and 8), and depth 1 matches the oracle."""
    I0, I1 = _pair(kind, 130, 300)
    res = {}
    try:
        for kb in (1, 2, 4, 8):
            hs.set_iters_per_launch(kb)
            res[kb] = _solve(hs, I0, I1, w, 19, kb=kb)
    finally:
        hs.set_iters_per_launch(0)
    for kb in (2, 4, 8):
        assert _same(res[kb], res[1]), kb
    _close(res[1], oracle.flow(_f64(I0), _f64(I1), w, 19, 1.0, nthreads=4),
           f"w{w} {kind} depth 1")


# ------------------------------------------------------------------ batches
@pytest.mark.gpu
@pytest.mark.parametrize("streams", [1, 2])
@pytest.mark.parametrize("w", [1, 2, 11])
def test_mixed_batch_equals_single_pairs(hs, w, streams):
    """[integral, non-integral, integral] on one stream and split over two:
    the batch equals its pairs solved alone, bit for bit, and each of them
    matches the oracle.  On one stream K2w runs 3 x 4 (w 1) or 3 x 6 (w 2)
    workgroups: the XCD remap with a quotient and a remainder, at w 1 with a
    tile count per pair (5 x 3) that is no multiple of four."""
    I0, I1 = _pair("f32", 130, 300, batch=3, nonint=(1,))
    with hs.max_streams_as(streams):
        ub, vb = _solve(hs, I0, I1, w, 9)
        for i in range(3):
            us, vs = _solve(hs, I0[i], I1[i], w, 9)
            assert _same((ub[i], vb[i]), (us, vs)), i
            _close((us, vs), oracle.flow(_f64(I0[i]), _f64(I1[i]), w, 9, 1.0),
                   f"w{w} pair {i} of the mixed batch")


# -------------------------------------------------------------- warm starts
@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["u8", "f32n"])
@pytest.mark.parametrize("w", [2, 11])
def test_warm_start(hs, w, kind):
    """gradients_device, then jacobi_device from a random (u0, v0): against
    oracle.jacobi, and 4 + 6 iterations equal 10 bit for bit."""
    import torch
    rows, cols = 47, 63
    I0, I1 = _pair(kind, rows, cols)
    _expect_kernel(hs, rows, cols, 1, w)
    rng = np.random.default_rng(3)
    u0 = rng.uniform(-2, 2, (rows, cols)).astype(np.float32)
    v0 = rng.uniform(-2, 2, (rows, cols)).astype(np.float32)
    _, _, ws = _poisoned(hs, I0.shape)
    hs.gradients_device(_dev(I0), _dev(I1), ws)
    u, v = _dev(u0), _dev(v0)
    hs.jacobi_device(rows, cols, 1, w, 10, 1.0, u, v, ws, warm_start=True)
    u2, v2 = _dev(u0), _dev(v0)
    hs.jacobi_device(rows, cols, 1, w, 4, 1.0, u2, v2, ws, warm_start=True)
    hs.jacobi_device(rows, cols, 1, w, 6, 1.0, u2, v2, ws, warm_start=True)
    torch.cuda.synchronize()
    got = (u.cpu().numpy(), v.cpu().numpy())
    assert _same((u2.cpu().numpy(), v2.cpu().numpy()), got)
    gx, gy, gt = oracle.gradients(_f64(I0), _f64(I1))
    _close(got, oracle.jacobi(gx, gy, gt, u0, v0, w, 10, 1.0), f"w{w} {kind} warm start")


# ---------------------------------------------------------------- alpha = 0
ALPHA0_CASES = [(1, 6), (2, 6), (10, 2), (11, 2)]


def _alpha0_pair():
    """A smooth 70x300 8-bit pair (sinusoids and a little noise, the second
    frame shifted): few pixels with Ix = Iy = 0 away from the corners, so the
    NaN of alpha = 0 stays local."""
    rng = np.random.default_rng(321)
    y, x = np.mgrid[0:70, 0:300].astype(np.float64)

    def frame(dy, dx):
        s = 127 + 60 * np.sin((x + dx) / 9.0) + 45 * np.cos((y + dy) / 7.0) + \
            15 * np.sin((x + dx + 2 * (y + dy)) / 5.0)
        return s

    I0 = np.clip(np.rint(frame(0, 0) + rng.integers(-2, 3, (70, 300))), 0, 255)
    I1 = np.clip(np.rint(frame(-0.75, 1.5) + rng.integers(-2, 3, (70, 300))), 0, 255)
    return I0.astype(np.uint8), I1.astype(np.uint8)


@pytest.fixture(scope="module")
def alpha0():
    I0, I1 = _alpha0_pair()
    return I0, I1, {c: oracle.flow(_f64(I0), _f64(I1), c[0], c[1], 0.0) for c in ALPHA0_CASES}


@pytest.mark.parametrize("case", ALPHA0_CASES)
def test_alpha_zero_oracle_has_both_kinds_of_pixel(alpha0, case):
    """The precondition of the GPU test below, on the reference alone: the
    oracle's alpha = 0 result has non-finite values (every image corner has
    Ix = Iy = 0) and at least half of it finite."""
    for ref in alpha0[2][case]:
        fin = np.isfinite(ref)
        print(f"alpha 0 w {case[0]} x {case[1]}: finite share {fin.mean():.3f}")
        assert not fin.all() and fin.mean() >= 0.5


@pytest.mark.gpu
@pytest.mark.parametrize("case", ALPHA0_CASES)
def test_alpha_zero_nan_pattern_matches_the_oracle(hs, alpha0, case):
    """The form of test_gpu_parity's test of the same name: non-finite exactly
    where the oracle is, the finite rest within 1e-4 of the oracle's finite
    maximum; the single pair and a batch of two."""
    w, iters = case
    I0, I1, refs = alpha0
    us, vs = _solve(hs, I0, I1, w, iters, alpha=0.0)
    ub, vb = _solve(hs, np.stack([I0, I0]), np.stack([I1, I1]), w, iters, alpha=0.0)
    for got_u, got_v in ((us, vs), (ub[0], vb[0]), (ub[1], vb[1])):
        for got, ref, name in ((got_u, refs[case][0], "u"), (got_v, refs[case][1], "v")):
            fin = np.isfinite(ref)
            assert np.array_equal(np.isfinite(got), fin)
            err = np.abs(got[fin].astype(np.float64) - ref[fin]).max() / np.abs(ref[fin]).max()
            print(f"alpha 0 w{w} x {iters} {name}: finite part {err:.3e} (bound {TOL:.0e})")
            assert err <= TOL


# ------------------------------------------------------------------ pyramid
@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["u8", "f32n"])
@pytest.mark.parametrize("w", [2, 11])
def test_pyramid_with_these_windows(hs, w, kind):
    """Three levels (45x70, 23x35, 12x18): a cold solve and two warm starts
    from the projected flow, against oracle.flow_pyramid."""
    import torch
    I0, I1 = _pair(kind, 45, 70)
    for level in range(3):
        _expect_kernel(hs, *hs.pyramid_level_size(45, 70, level), 1, w)
    u, v, _ = _poisoned(hs, I0.shape)
    ws = torch.full((hs.pyramid_workspace_bytes(45, 70, 1, 3),), 0xA5, dtype=torch.uint8,
                    device="cuda")
    hs.flow_pyramid_device(_dev(I0), _dev(I1), 3, w, 9, 1.0, u, v, ws)
    torch.cuda.synchronize()
    _close((u.cpu().numpy(), v.cpu().numpy()),
           oracle.flow_pyramid(_f64(I0), _f64(I1), 3, w, 9, 1.0), f"w{w} {kind} pyramid")
