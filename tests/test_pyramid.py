"""Config 5 (north_star): coarse-to-fine pyramid warm start + fp16 inputs.

HornSchunckOF has no pyramid, so there is no reference output to pin this
against: the C oracle's pyramid (oracle/hs_oracle.c hso_pyrdown /
hso_flow_pyramid) is checked here against an independent numpy restatement
of the same design precedent (BMOpticalFlow/.../OpticalFlow/
MultiResolution.cpp:9-97 Pyramider, OpticalFlow.cpp:197-210
Add_VectorOffset) built on the already-pinned per-level oracle pieces
(gradients, jacobi).  "Parity unpinned" w.r.t. the reference for levels > 1;
levels = 1 is the pinned getFlow path.  The GPU path is then checked against
the oracle with the module's usual tolerance (max|d|/max|ref| <= 1e-4) and
bit-exactly for integer work (level images of integer-valued pairs).
"""
import numpy as np
import pytest

import oracle
from conftest import norm_rel_err

TOL = 1e-4
W5 = np.array([2.0, 5.0, 4.0, 5.0, 2.0])  # (a/2, 1/2, a, 1/2, a/2) * 18, a = 0.4


def _refl101(p, n):
    if n == 1:
        return np.zeros_like(p)
    p = np.abs(p)
    p = np.where(p >= n, 2 * (n - 1) - p, p)
    return np.abs(p)


def pyrdown_np(img, rnd):
    """Independent twin of hso_pyrdown: separable 5-tap, stride 2, reflect-101."""
    a = np.asarray(img, np.float64)
    r, c = a.shape
    r2, c2 = (r + 1) // 2, (c + 1) // 2
    ys = _refl101(2 * np.arange(r2)[:, None] + np.arange(5)[None, :] - 2, r)  # r2 x 5
    xs = _refl101(2 * np.arange(c2)[:, None] + np.arange(5)[None, :] - 2, c)  # c2 x 5
    h = np.einsum("rxn,n->rx", a[:, xs], W5)          # r x c2
    S = np.einsum("ymx,m->yx", h[ys, :], W5)          # r2 x c2
    return np.floor((S + 162.0) / 324.0) if rnd else S / 324.0


def pyramid_np(I0, I1, levels, w, n, alpha):
    a, b = np.asarray(I0, np.float64), np.asarray(I1, np.float64)
    rnd = bool(np.all(a == np.floor(a)) and np.all(b == np.floor(b)) and a.min() >= 0
               and b.min() >= 0 and a.max() <= 255 and b.max() <= 255)
    P = [(a, b)]
    for _ in range(1, levels):
        P.append((pyrdown_np(P[-1][0], rnd), pyrdown_np(P[-1][1], rnd)))
    u = v = None
    for lv in range(levels - 1, -1, -1):
        p0, p1 = P[lv]
        if u is None:
            u0 = np.zeros_like(p0)
            v0 = np.zeros_like(p0)
        else:  # OpticalFlow.cpp:205-206, nearest projection x 2
            u0 = 2.0 * np.repeat(np.repeat(u, 2, 0), 2, 1)[:p0.shape[0], :p0.shape[1]]
            v0 = 2.0 * np.repeat(np.repeat(v, 2, 0), 2, 1)[:p0.shape[0], :p0.shape[1]]
        gx, gy, gt = oracle.gradients(p0, p1)
        u, v = oracle.jacobi(gx, gy, gt, u0, v0, w, n, alpha)
    return u, v


def _pair(rows, cols, seed=7, integral=True):
    rng = np.random.default_rng(seed)
    I0 = rng.integers(0, 256, (rows, cols)).astype(np.float64)
    # smooth-ish second frame: shift + noise
    I1 = np.clip(np.roll(I0, (1, -2), (0, 1)) + rng.integers(-3, 4, (rows, cols)), 0, 255)
    if not integral:
        I0 = I0 + 0.25
    return I0, I1


# ------------------------------------------------------------------ CPU tests
@pytest.mark.parametrize("shape", [(1, 1), (1, 6), (2, 3), (5, 7), (17, 33), (48, 64)])
@pytest.mark.parametrize("rnd", [True, False])
def test_oracle_pyrdown_matches_numpy_twin(shape, rnd):
    I0, _ = _pair(*shape, integral=rnd)
    got = oracle.pyrdown(I0, rnd)
    ref = pyrdown_np(I0, rnd)
    assert got.shape == ((shape[0] + 1) // 2, (shape[1] + 1) // 2)
    if rnd:
        assert np.array_equal(got, ref)
        assert got.min() >= 0 and got.max() <= 255
    else:
        assert np.allclose(got, ref, rtol=0, atol=1e-12)


def test_oracle_pyrdown_preserves_constants():
    # the normalised kernel has unit DC gain (MultiResolution.cpp:58-63)
    img = np.full((9, 14), 137.0)
    assert np.array_equal(oracle.pyrdown(img, True), np.full((5, 7), 137.0))


def test_oracle_integer_pair_rule():
    I0, I1 = _pair(6, 9)
    assert oracle.integer_pair(I0, I1)
    assert not oracle.integer_pair(I0 + 0.5, I1)
    J = I1.copy()
    J[0, 0] = 256
    assert not oracle.integer_pair(I0, J)


def test_oracle_pyramid_one_level_is_getflow(crop_small):
    I0, I1 = crop_small["I0"], crop_small["I1"]
    u1, v1 = oracle.flow_pyramid(I0, I1, 1, 5, 10, 1.0)
    u, v = oracle.flow(I0, I1, 5, 10, 1.0)
    assert np.array_equal(u1, u) and np.array_equal(v1, v)


@pytest.mark.parametrize("shape,levels", [((48, 64), 3), ((37, 53), 3), ((20, 9), 4)])
@pytest.mark.parametrize("integral", [True, False])
def test_oracle_pyramid_matches_numpy_twin(shape, levels, integral):
    I0, I1 = _pair(*shape, integral=integral)
    u, v = oracle.flow_pyramid(I0, I1, levels, 5, 7, 1.0)
    ur, vr = pyramid_np(I0, I1, levels, 5, 7, 1.0)
    assert norm_rel_err(u, ur) <= 1e-12 and norm_rel_err(v, vr) <= 1e-12


# ------------------------------------------------------------------ GPU tests
@pytest.fixture(scope="module")
def hs():
    import hsflow
    return hsflow


def _dev_pyr(hs, I0, I1, levels, w, n, alpha=1.0, torch_dtype=None):
    import torch
    t0 = torch.from_numpy(np.ascontiguousarray(I0)).cuda()
    t1 = torch.from_numpy(np.ascontiguousarray(I1)).cuda()
    if torch_dtype is not None:
        t0, t1 = t0.to(torch_dtype), t1.to(torch_dtype)
    u, v = hs.flow_pyramid_device(t0, t1, levels, w, n, alpha)
    torch.cuda.synchronize()
    return u.cpu().numpy(), v.cpu().numpy()


@pytest.mark.gpu
def test_f16_inputs_match_f32_bitwise(hs):
    """Config 5 stores the frames as fp16: integer-valued fp16 frames give
    exactly the f32 result (same packed gradients)."""
    import torch
    I0, I1 = hs.synth_pair(1003, 200, 331)
    t0, t1 = torch.from_numpy(I0).cuda(), torch.from_numpy(I1).cuda()
    a = hs.flow_device(t0, t1, 5, 40, 1.0)
    b = hs.flow_device(t0.half(), t1.half(), 5, 40, 1.0)
    torch.cuda.synchronize()
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    uo, vo = oracle.flow(I0, I1, 5, 40, 1.0, nthreads=8)
    assert norm_rel_err(b[0].cpu().numpy(), uo) <= TOL
    assert norm_rel_err(b[1].cpu().numpy(), vo) <= TOL


@pytest.mark.gpu
def test_f16_host_api(hs):
    I0, I1 = hs.synth_pair(1004, 64, 96)
    ctx = hs.Context(0)
    u16, v16 = ctx.flow(I0.astype(np.float16), I1.astype(np.float16), 5, 20, 1.0)
    u32, v32 = ctx.flow(I0, I1, 5, 20, 1.0)
    ctx.close()
    assert np.array_equal(u16, u32) and np.array_equal(v16, v32)


@pytest.mark.gpu
def test_pyramid_one_level_is_flow_device_bitwise(hs):
    import torch
    I0, I1 = hs.synth_pair(1005, 130, 250)
    t0, t1 = torch.from_numpy(I0).cuda(), torch.from_numpy(I1).cuda()
    a = hs.flow_device(t0, t1, 5, 30, 1.0)
    b = hs.flow_pyramid_device(t0, t1, 1, 5, 30, 1.0)
    torch.cuda.synchronize()
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


@pytest.mark.gpu
@pytest.mark.parametrize("shape", [(96, 160), (97, 161), (45, 300), (5, 3)])
@pytest.mark.parametrize("levels", [2, 3])
@pytest.mark.parametrize("w", [3, 5])
def test_pyramid_against_oracle(hs, shape, levels, w):
    I0, I1 = hs.synth_pair(1006, *shape)
    u, v = _dev_pyr(hs, I0, I1, levels, w, 25)
    uo, vo = oracle.flow_pyramid(I0, I1, levels, w, 25, 1.0, nthreads=8)
    assert norm_rel_err(u, uo) <= TOL and norm_rel_err(v, vo) <= TOL


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["u8", "f16", "f32_nonint"])
def test_pyramid_input_kinds(hs, kind):
    import torch
    I0, I1 = hs.synth_pair(1007, 150, 222)
    if kind == "u8":
        a, b, td = I0.astype(np.uint8), I1.astype(np.uint8), None
    elif kind == "f16":
        a, b, td = I0, I1, torch.float16
    else:
        a, b, td = I0 * np.float32(0.9) + np.float32(0.3), I1, None
    u, v = _dev_pyr(hs, a, b, 3, 5, 30, torch_dtype=td)
    uo, vo = oracle.flow_pyramid(np.asarray(a, np.float64), np.asarray(b, np.float64), 3, 5,
                                 30, 1.0, nthreads=8)
    assert norm_rel_err(u, uo) <= TOL and norm_rel_err(v, vo) <= TOL


@pytest.mark.gpu
def test_pyramid_host_equals_device(hs):
    I0, I1 = hs.synth_pair(1008, 120, 200)
    ctx = hs.Context(0)
    uh, vh = ctx.flow_pyramid(I0, I1, 3, 5, 20, 1.0, out_dtype=np.float32)
    ctx.close()
    ud, vd = _dev_pyr(hs, I0, I1, 3, 5, 20)
    assert np.array_equal(uh, ud) and np.array_equal(vh, vd)


@pytest.mark.gpu
def test_pyramid_batch_equals_single(hs):
    import torch
    pairs = [hs.synth_pair(1010 + k, 77, 140) for k in range(3)]
    t0 = torch.stack([torch.from_numpy(p[0]) for p in pairs]).cuda()
    t1 = torch.stack([torch.from_numpy(p[1]) for p in pairs]).cuda()
    ub, vb = hs.flow_pyramid_device(t0, t1, 3, 5, 15, 1.0)
    for k in range(3):
        us, vs = hs.flow_pyramid_device(t0[k].contiguous(), t1[k].contiguous(), 3, 5, 15, 1.0)
        assert torch.equal(ub[k], us) and torch.equal(vb[k], vs)


@pytest.mark.gpu
def test_pyramid_argument_errors(hs):
    import torch
    t = torch.zeros(8, 8, device="cuda")
    for levels in (0, hs.MAX_LEVELS + 1):
        with pytest.raises(hs.HsflowError):
            hs.flow_pyramid_device(t, t, levels, 5, 1, 1.0)
    assert hs.pyramid_level_size(4320, 7680, 2) == (1080, 1920)
    assert hs.pyramid_level_size(5, 3, 2) == (2, 1)


@pytest.mark.gpu
def test_config5_8k_fp16_pyramid(hs):
    """Config 5 shape: 7680x4320 fp16 pair, 3 levels.  Short per-level runs
    against the oracle at full size, fp16 == f32 bitwise, finite output."""
    import torch
    I0, I1 = hs.synth_pair(1000, 4320, 7680)
    t0, t1 = torch.from_numpy(I0).cuda(), torch.from_numpy(I1).cuda()
    u16, v16 = hs.flow_pyramid_device(t0.half(), t1.half(), 3, 5, 12, 1.0)
    u32, v32 = hs.flow_pyramid_device(t0, t1, 3, 5, 12, 1.0)
    torch.cuda.synchronize()
    assert torch.equal(u16, u32) and torch.equal(v16, v32)
    assert bool(torch.isfinite(u16).all()) and bool(torch.isfinite(v16).all())
    uo, vo = oracle.flow_pyramid(I0, I1, 3, 5, 12, 1.0, nthreads=16)
    assert norm_rel_err(u16.cpu().numpy(), uo) <= TOL
    assert norm_rel_err(v16.cpu().numpy(), vo) <= TOL


# ---------------------------- the level planes and the projection, directly
# hs_pyrdown_kernel through pyramid_build_device and hs_upflow_kernel through
# upflow_device against a chain of oracle.pyrdown and the numpy projection.
# The levels of an integer pair are bit-exact with the oracle (the header of
# csrc/hsflow_pyramid.hip); the others within 2e-6 * l at level l: an output
# is a sum of 25 products, at most 31 fp32 roundings including the division,
# each at most 2^-24 of the largest partial sum, and the kernel's gain is 1,
# so the errors of l levels add up (a float32 restatement of the kernel
# measures 1e-7 at levels 1 and 2).  Workspaces are prefilled with 0xA5
# bytes, outputs with NaN.
LEVELS = 4
LEVEL_TOL = 2e-6
PYR_SHAPES = [(1, 1), (1, 6), (2, 3), (5, 7), (17, 33), (48, 64), (97, 161)]
PYR_DTYPES = {"u8": np.uint8, "f16": np.float16, "f32": np.float32, "f64": np.float64}


def _int_pair(rows, cols, batch=None, seed=31):
    rng = np.random.default_rng(seed + 1000 * rows + cols)
    shape = (batch, rows, cols) if batch else (rows, cols)
    return (rng.integers(0, 256, shape).astype(np.float64),
            rng.integers(0, 256, shape).astype(np.float64))


def _build_levels(hs, I0, I1, levels=LEVELS):
    """pyramid_build_device's call on NaN planes and a 0xA5 workspace:
    ([level 1.., numpy] of I0, the same of I1)."""
    import ctypes
    import torch
    t0 = torch.from_numpy(np.ascontiguousarray(I0)).cuda()
    t1 = torch.from_numpy(np.ascontiguousarray(I1)).cuda()
    rows, cols = I0.shape[-2:]
    lead = tuple(I0.shape[:-2])
    batch = int(np.prod(lead, dtype=np.int64))
    sizes = [hs.pyramid_level_size(rows, cols, l) for l in range(1, levels)]
    P = [[torch.full(lead + s, float("nan"), device="cuda") for s in sizes] for _ in range(2)]
    ws = torch.full((hs.workspace_bytes(rows, cols, batch),), 0xA5, dtype=torch.uint8,
                    device="cuda")
    arrays = [(ctypes.c_void_p * max(1, levels - 1))(*[t.data_ptr() for t in p]) for p in P]
    codes = {"uint8": hs.U8, "float16": hs.F16, "float32": hs.F32, "float64": hs.F64}
    assert I1.dtype == I0.dtype
    rc = hs.lib().hsflow_pyramid_build_device(
        t0.data_ptr(), t1.data_ptr(), codes[I0.dtype.name], rows, cols, batch, levels,
        arrays[0], arrays[1], ws.data_ptr(), ws.numel(),
        torch.cuda.current_stream().cuda_stream)
    assert rc == hs.HSFLOW_OK
    torch.cuda.synchronize()
    return [[t.cpu().numpy() for t in p] for p in P]


def _chain(img, rnd, levels=LEVELS):
    """Levels 1.. of one frame by oracle.pyrdown."""
    out, a = [], np.asarray(img, np.float64)
    for _ in range(1, levels):
        a = oracle.pyrdown(a, rnd)
        out.append(a)
    return out


def _levels_exact(got, frame):
    for l, (g, r) in enumerate(zip(got, _chain(frame, True)), 1):
        assert g.dtype == np.float32 and g.shape == r.shape, l
        assert np.array_equal(g, r), l
        assert g.min() >= 0 and g.max() <= 255, l


def _levels_close(got, frame, what):
    for l, (g, r) in enumerate(zip(got, _chain(frame, False)), 1):
        assert g.shape == r.shape, l
        err = norm_rel_err(g, r)
        print(f"{what} level {l}: norm_rel_err {err:.3e} (bound {LEVEL_TOL * l:.0e})")
        assert err <= LEVEL_TOL * l, l


@pytest.mark.gpu
@pytest.mark.parametrize("kind", list(PYR_DTYPES))
@pytest.mark.parametrize("shape", PYR_SHAPES)
def test_levels_of_integer_pairs_are_bit_exact(hs, shape, kind):
    """Down to 1x1 and through 2- and 3-wide levels (reflect-101 bouncing
    twice); 97x161: several blocks, odd sizes at every level."""
    I0, I1 = _int_pair(*shape)
    P0, P1 = _build_levels(hs, I0.astype(PYR_DTYPES[kind]), I1.astype(PYR_DTYPES[kind]))
    _levels_exact(P0, I0)
    _levels_exact(P1, I1)


@pytest.mark.gpu
@pytest.mark.parametrize("kind", list(PYR_DTYPES))
@pytest.mark.parametrize("value", [0, 255])
def test_constant_frames_stay_constant(hs, value, kind):
    """Unit gain with the rounding: 255 must not become 254 or 256."""
    for shape in ((5, 7), (17, 33)):
        I = np.full(shape, value, PYR_DTYPES[kind])
        for P in _build_levels(hs, I, I):
            for l, g in enumerate(P, 1):
                assert g.shape == hs.pyramid_level_size(*shape, l)
                assert np.array_equal(g, np.full(g.shape, value, np.float32))


@pytest.mark.gpu
@pytest.mark.parametrize("shape", PYR_SHAPES)
def test_levels_of_non_integral_pairs(hs, shape):
    I0, I1 = _int_pair(*shape)
    a, b = (I0 * 0.73 + 0.21).astype(np.float32), (I1 * 0.61 + 3.3).astype(np.float32)
    P0, P1 = _build_levels(hs, a, b)
    _levels_close(P0, a, f"{shape} I0")
    _levels_close(P1, b, f"{shape} I1")


@pytest.mark.gpu
@pytest.mark.parametrize("shape", [(5, 7), (97, 161)])
def test_one_bad_pixel_decides_the_whole_pair(hs, shape):
    """100.5 at the last pixel of I1: no level of either frame is rounded."""
    I0, I1 = (x.astype(np.float32) for x in _int_pair(*shape))
    I1[-1, -1] = 100.5
    P0, P1 = _build_levels(hs, I0, I1)
    _levels_close(P0, I0, f"{shape} I0 beside a bad I1")
    _levels_close(P1, I1, f"{shape} bad I1")
    assert not np.array_equal(P0[0], np.rint(P0[0]))


@pytest.mark.gpu
def test_levels_of_a_mixed_batch(hs):
    """[integral, non-integral, integral]: each pair by its own flag."""
    I0, I1 = (x.astype(np.float32) for x in _int_pair(17, 33, batch=3))
    I0[1], I1[1] = I0[1] * np.float32(0.73) + np.float32(0.21), I1[1] + np.float32(0.5)
    P0, P1 = _build_levels(hs, I0, I1)
    for P, I, name in ((P0, I0, "I0"), (P1, I1, "I1")):
        for k in (0, 2):
            _levels_exact([g[k] for g in P], I[k])
        _levels_close([g[1] for g in P], I[1], f"mixed batch {name} pair 1")


@pytest.mark.gpu
@pytest.mark.parametrize("fine,coarse", [((1, 1), (1, 1)), ((2, 3), (1, 2)), ((5, 7), (3, 4)),
                                         ((96, 160), (48, 80)), ((97, 161), (49, 81))])
def test_upflow_is_the_doubled_nearest_projection(hs, fine, coarse):
    import torch
    rng = np.random.default_rng(41)
    uc = rng.uniform(-3, 3, coarse).astype(np.float32)
    vc = rng.uniform(-3, 3, coarse).astype(np.float32)
    u = torch.full(fine, float("nan"), device="cuda")
    v = torch.full(fine, float("nan"), device="cuda")
    hs.upflow_device(torch.from_numpy(uc).cuda(), torch.from_numpy(vc).cuda(), u, v)
    torch.cuda.synchronize()
    for got, src in ((u, uc), (v, vc)):
        want = 2 * np.repeat(np.repeat(src, 2, 0), 2, 1)[:fine[0], :fine[1]]
        assert np.array_equal(got.cpu().numpy(), want)
