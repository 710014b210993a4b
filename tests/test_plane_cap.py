"""The Jacobi kernels on planes at the plane-size cap, against the float64
oracle on patches.

The Jacobi kernels but K2g (K2 hs_jacobi_wg_kernel, K2w hs_jacobi_kernel, K4
hs_jacobi_strip_kernel and its fused first pass, KJ
hs_jacobi_weighted_kernel) give a lane outside the image the byte offset
0x7FFFFFF0 into a raw buffer of rows * cols * 4 bytes, and rely on the
hardware range check to read 0 and drop the store there: that is the zero
border of the reference (K2g hs_jacobi_generic_kernel tests its indices and
runs here too).  A plane of more than 0x7FFFFFF0 / 4 = 2^29 - 4
pixels holds that offset (element 2^29 - 4), so the cap of the API is 2^29 - 4
pixels; planes of 2^29 - 3, 2^29 - 2 and 2^29 - 1 pixels are refused.

The oracle cannot run on 2^29 pixels in seconds and need not: after n
iterations of window w a pixel depends on nothing farther than margin(w, n)
pixels away, so the frames (and a warm start's planes) are cropped to patches
that touch the image's real borders, the oracle runs on each patch, and only
pixels at least the margin away from a patch's artificial edges are compared.
The CPU tests below prove that helper on a small plane.  Only patches cross
to the host.

Bound: the suite's own, max|got - ref| / max|ref| <= 1e-4 per patch.  Every
workspace is prefilled with 0xA5 bytes and every output with NaN.  A warm
start plants 64.0 at the plane's element nearest the sentinel, so that one
stray read would move a border mean by 64 / w^2.

Measured on the MI355X while the cap was still 2^29 - 1, with the four larger
shapes run through the comparisons below: K2, K2w and KJ missed the bound on
every patch (norm_rel_err 0.6 to 15) and K2 and K2w lost the race for
element 2^29 - 4 of u_out; K4 missed it on the two top patches (0.06 to 0.6:
row 0's out-of-column lanes); a cold solve, which ends in a K2 pass, on every
patch (0.01 to 0.02); K2g, which indexes plainly, passed.  The two
shapes of 2^29 - 4 pixels gave at most 2.7e-7 then and give it now."""
import collections
import contextlib

import numpy as np
import pytest

import oracle
from conftest import norm_rel_err
from test_gradient_words import pack_np
from test_smoothness import jacobi_weighted_np

TOL = 1e-4
SENTINEL = 0x7FFFFFF0          # the kernels' out-of-image byte offset
SENTINEL_ELEM = SENTINEL // 4  # 2^29 - 4: the f32 element at that offset
PLANT = 64.0
MIN_PEAK = 1e-3                # every patch's max|ref|
PLANT_RATIO = 50.0             # PLANT / max|ref| of the bottom-right patch
ALPHA_WARM = 300.0
ALPHA_KJ, LAM = 100.0, 4.0
GUARD = -7.25

# 2^29 - 4 = 4 * 7 * 73 * 262657: plane bytes == SENTINEL, the largest plane.
# 1022 x 525314 has both sides even (the interleaved K4 passes run), 2044 x
# 262657 an odd width (the dword path)
AT_CAP = [(1022, 525314), (2044, 262657)]
# 2^29 - 1 = 233 * 1103 * 2089 (tall and wide), 2^29 - 2 = 18705 * 28702,
# 2^29 - 3 is prime: they hold element 2^29 - 4 and are refused
ABOVE_CAP = [(256999, 2089), (2089, 256999), (18705, 28702), (1, 536870909)]

K2, K2W, K2G, K4 = ("hs_jacobi_wg_kernel", "hs_jacobi_kernel", "hs_jacobi_generic_kernel",
                    "hs_jacobi_strip_kernel")


# ------------------------------------------------------------ the patch oracle
def margin(w, n):
    """Pixels between a compared pixel and an artificial edge: a window reaches
    at most w - 1 pixels to one side, n times; + 1 for the 3 x 3 Sobel."""
    return n * (w - 1) + 1


def reach(w, n, warm):
    """The exact dependence towards the right and the bottom, where the window
    reaches w // 2 pixels past its anchor (hornSchunck.cpp:54): a warm start's
    planes n times that; the gradients (the update reads them at the pixel
    itself) n - 1 times that, + 1 for the Sobel."""
    return n * (w // 2) if warm else (n - 1) * (w // 2) + 1


class Patch(collections.namedtuple("Patch", "name r0 r1 c0 c1 rows cols")):
    """Rows [r0, r1) x columns [c0, c1) of a rows x cols plane."""
    __slots__ = ()

    def crop(self, a):
        """The patch of a plane [..., rows, cols], numpy or torch, as numpy."""
        a = a.reshape(self.rows, self.cols)[self.r0:self.r1, self.c0:self.c1]
        return np.ascontiguousarray(a.cpu().numpy() if hasattr(a, "cpu") else a)

    def inner(self, m):
        """The slices, in patch coordinates, of the pixels at least m away from
        the patch's artificial edges (an edge on the plane's border is real)."""
        top = 0 if self.r0 == 0 else m
        left = 0 if self.c0 == 0 else m
        bottom = self.r1 - self.r0 - (0 if self.r1 == self.rows else m)
        right = self.c1 - self.c0 - (0 if self.c1 == self.cols else m)
        assert top < bottom and left < right, self
        return slice(top, bottom), slice(left, right)

    def artificial(self):
        return self.r0 > 0 or self.c0 > 0 or self.r1 < self.rows or self.c1 < self.cols

    def index_of(self, elem, m):
        """Element `elem` of the plane in inner(m) coordinates, None outside it."""
        sy, sx = self.inner(m)
        y, x = elem // self.cols - self.r0 - sy.start, elem % self.cols - self.c0 - sx.start
        inside = 0 <= y < sy.stop - sy.start and 0 <= x < sx.stop - sx.start
        return (y, x) if inside else None


def patches(rows, cols, m, keep=64):
    """The four corners, the middle of the bottom row and the middle of the
    right column: along each axis m + keep pixels from a border, 2 m + keep
    between two artificial edges, no more than the plane has; one of each."""
    def span(n, where, both):
        size = min(n, (2 * m if both else m) + keep)
        start = {"lo": 0, "hi": n - size, "mid": (n - size) // 2}[where]
        return start, start + size

    spec = [("bottom-right", "hi", "hi"), ("bottom-left", "hi", "lo"), ("top-right", "lo", "hi"),
            ("top-left", "lo", "lo"), ("bottom-middle", "hi", "mid"),
            ("right-middle", "mid", "hi")]
    out, seen = [], set()
    for name, ry, rx in spec:
        box = span(rows, ry, ry == "mid") + span(cols, rx, rx == "mid")
        if box not in seen:
            seen.add(box)
            out.append(Patch(name, *box, rows, cols))
    return out


def _f64(a):
    return np.asarray(a, np.float64)


def patch_flow(p, I0, I1, w, n, alpha, warm=None):
    """(u, v) float64 of patch p alone: oracle.flow of the cropped frames, or
    oracle.jacobi on their gradients from the cropped warm-start planes."""
    a, b = _f64(p.crop(I0)), _f64(p.crop(I1))
    if warm is None:
        return oracle.flow(a, b, w, n, alpha)
    gx, gy, gt = oracle.gradients(a, b)
    return oracle.jacobi(gx, gy, gt, p.crop(warm[0]), p.crop(warm[1]), w, n, alpha)


# ------------------------------------------- the helper, proven without a GPU
SMALL = (97, 131)
CPU_CASES = [(2, 8), (3, 8), (5, 6), (10, 3)]  # window, iterations


@pytest.fixture(scope="module")
def small():
    """A 97 x 131 pair, warm-start planes, and the whole-plane oracle per case."""
    rng = np.random.default_rng(97131)
    I0, I1 = (rng.integers(0, 256, SMALL).astype(np.uint8) for _ in range(2))
    u0, v0 = (rng.standard_normal(SMALL).astype(np.float32) for _ in range(2))
    whole = {}
    for w, n in CPU_CASES:
        whole[w, n, False] = oracle.flow(_f64(I0), _f64(I1), w, n, 1.0)
        whole[w, n, True] = oracle.jacobi(*oracle.gradients(_f64(I0), _f64(I1)), u0, v0, w, n, 1.0)
    return I0, I1, (u0, v0), whole


def _worst(p, m, part, whole):
    """max|patch - whole plane| over inner(m), u and v."""
    sy, sx = p.inner(m)
    return max(float(np.abs(a[sy, sx] - p.crop(b)[sy, sx]).max()) for a, b in zip(part, whole))


def test_patches_touch_every_border_and_are_distinct():
    ps = patches(97, 131, 9)
    assert [p.name for p in ps] == ["bottom-right", "bottom-left", "top-right", "top-left",
                                    "bottom-middle", "right-middle"]
    assert {(p.r0 == 0, p.c0 == 0, p.r1 == 97, p.c1 == 131) for p in ps} == {
        (True, True, False, False), (True, False, False, True), (False, True, True, False),
        (False, False, True, True), (False, False, True, False), (False, False, False, True)}
    for p in ps:
        sy, sx = p.inner(9)
        assert sy.stop - sy.start >= 64 and sx.stop - sx.start >= 64
    # a one-row plane has two corners and a middle, all of them one row high
    assert [p.name for p in patches(1, 1000, 9)] == ["bottom-right", "bottom-left",
                                                     "bottom-middle"]
    # the bottom-right patch holds the plane's last elements among its compared pixels
    br = ps[0]
    assert br.index_of(97 * 131 - 3, 9) == (63, 61) and br.index_of(0, 9) is None


@pytest.mark.parametrize("warm", [False, True], ids=["cold", "warm"])
@pytest.mark.parametrize("w,n", CPU_CASES)
def test_patch_oracle_equals_the_whole_plane_oracle(small, w, n, warm):
    """On the compared pixels (margin(w, n) from the artificial edges) the
    patch result is the whole-plane result to 1e-12."""
    I0, I1, uv0, whole = small
    for p in patches(*SMALL, margin(w, n)):
        part = patch_flow(p, I0, I1, w, n, 1.0, uv0 if warm else None)
        worst = _worst(p, margin(w, n), part, whole[w, n, warm])
        print(f"w {w} n {n} {p.name}: {worst:.2e}")
        assert worst <= 1e-12


@pytest.mark.parametrize("warm", [False, True], ids=["cold", "warm"])
@pytest.mark.parametrize("w,n", CPU_CASES)
def test_margin_is_a_tested_statement(small, w, n, warm):
    """The comparison sees an artificial edge that is too close.  For the
    top-left patch, whose artificial edges are the right and the bottom ones
    (the way the window reaches farthest), the smallest margin at which the
    patch equals the whole plane is reach(w, n, warm) exactly: one pixel
    closer the patch differs.  margin(w, n) is no smaller for any window, and
    one more than that reach at w = 2: the update reads the gradients at the
    pixel itself, so they spread n - 1 times, not n.  Every other patch with
    an artificial edge differs somewhere too once nothing is left out."""
    I0, I1, uv0, whole = small
    m = margin(w, n)
    ps = patches(*SMALL, m)
    tl = ps[3]
    assert tl.name == "top-left"
    part = patch_flow(tl, I0, I1, w, n, 1.0, uv0 if warm else None)
    first_equal = next(k for k in range(m + 1) if _worst(tl, k, part, whole[w, n, warm]) <= 1e-12)
    print(f"w {w} n {n}: exact from margin {first_equal}, margin() {m}")
    assert first_equal == reach(w, n, warm) <= m
    assert _worst(tl, first_equal - 1, part, whole[w, n, warm]) > 1e-6
    if w == 2:
        assert m == reach(w, n, True) + 1
    for p in ps:
        assert p.artificial()
        part = patch_flow(p, I0, I1, w, n, 1.0, uv0 if warm else None)
        assert _worst(p, 0, part, whole[w, n, warm]) > 1e-6, p.name


# ---------------------------------------------------------------- GPU helpers
def _frames(rows, cols, kind="u8"):
    """Random 8-bit frames made on the device; "f32": the same + 0.375 as
    float32 (non-integral: the f32 gradient planes)."""
    import torch
    g = torch.Generator(device="cuda")
    g.manual_seed(4)
    I0 = torch.randint(0, 256, (1, rows, cols), dtype=torch.uint8, device="cuda", generator=g)
    I1 = torch.randint(0, 256, (1, rows, cols), dtype=torch.uint8, device="cuda", generator=g)
    if kind == "f32":
        I0, I1 = I0.float().add_(0.375), I1.float().add_(0.375)
    return I0, I1


def _warm_planes(rows, cols):
    """torch.randn (u0, v0) with PLANT at the element nearest the sentinel:
    element 2^29 - 4 where the plane has it, else its last one."""
    import torch
    g = torch.Generator(device="cuda")
    g.manual_seed(5)
    u = torch.randn((1, rows, cols), device="cuda", generator=g)
    v = torch.randn((1, rows, cols), device="cuda", generator=g)
    at = min(SENTINEL_ELEM, rows * cols - 1)
    u.view(-1)[at] = PLANT
    v.view(-1)[at] = PLANT
    return u, v, at


def _workspace(hs, rows, cols):
    import torch
    return torch.full((hs.workspace_bytes(rows, cols, 1),), 0xA5, dtype=torch.uint8,
                      device="cuda")


def _ws_plane(ws, k, rows, cols, dtype):
    """Plane k of a one-pair workspace (carve(): gpack, gx, gy, gt, u2, v2,
    each rounded up to 256 bytes) as a [rows, cols] view."""
    n = rows * cols
    stride = (n * 4 + 255) // 256 * 256
    return ws[k * stride:k * stride + n * 4].view(dtype).view(rows, cols)


@contextlib.contextmanager
def _forced(hs, kernel, kb=0):
    hs.set_jacobi_kernel(kernel)
    hs.set_iters_per_launch(kb)
    try:
        yield
    finally:
        hs.set_jacobi_kernel(0)
        hs.set_iters_per_launch(0)


def _release():
    import torch
    torch.cuda.empty_cache()


def _check(what, ps, m, got, refs, plant_at=None):
    """got (u, v) device planes against refs[patch] = (u, v) float64 on every
    patch's compared pixels.  Prints every figure, then asserts: the two
    conditions on the reference (every max|ref| >= MIN_PEAK; with a plant, the
    bottom-right patch compares the planted element and PLANT >= PLANT_RATIO
    max|ref| there) and norm_rel_err <= TOL."""
    bad = []
    for p, ref in zip(ps, refs):
        sy, sx = p.inner(m)
        for plane, r, name in zip(got, ref, "uv"):
            g, r = p.crop(plane)[sy, sx], r[sy, sx]
            peak, err = float(np.abs(r).max()), norm_rel_err(g, r)
            print(f"{what} {p.name} {name}: norm_rel_err {err:.3e} (bound {TOL:.0e}), "
                  f"max|ref| {peak:.3e}")
            if not peak >= MIN_PEAK:
                bad.append(f"{p.name} {name}: max|ref| {peak:.3e} < {MIN_PEAK}")
            if not err <= TOL:
                bad.append(f"{p.name} {name}: norm_rel_err {err:.3e}")
            if plant_at is not None and p.name == "bottom-right":
                at = p.index_of(plant_at, m)
                assert at is not None, "the planted element is not compared"
                print(f"{what} element {plant_at} of {name}: got {g[at]!r}, ref {r[at]!r}; "
                      f"plant / max|ref| {PLANT / peak:.1f} (at least {PLANT_RATIO:.0f})")
                if not PLANT >= PLANT_RATIO * peak:
                    bad.append(f"plant {PLANT} < {PLANT_RATIO} x max|ref| {peak:.3e} of {name}")
    if plant_at is not None:
        assert any(p.name == "bottom-right" for p in ps)
    assert not bad, f"{what}: " + "; ".join(bad)


# (kernel setting, depth setting, window, iterations, kernel name, depth): one
# launch each, but K2g, which runs one iteration per launch, and K2w, which
# runs two.  After one launch of 8 iterations at w = 2 the plant's own remains
# are the bottom-right patch's max|ref|, 1.2 to 2.7 (2 x 2 means thin it
# slowest), and 64 is not 50 times that whatever alpha is; after 16 it is
# (the oracle on random 8-bit frames and normal planes, six seeds: max|ref|
# 0.6 at most).  alpha = 300 for all of them: alpha^2 is about |grad I|^2 of
# random 8-bit frames, so both terms of the update count, and the data term
# |It| |grad I| / (alpha^2 + |grad I|^2) <= 255 / (2 alpha) stays below 64 / 50.
WARM_RUNS = {
    "K2-w5": (2, 0, 5, 6, K2, 6),
    "K4-w3": (4, 0, 3, 8, K4, 8),
    "K4-w5": (4, 0, 5, 6, K4, 6),
    "K4-w5-kb4": (4, 4, 5, 4, K4, 4),
    "K2w-w2": (2, 0, 2, 16, K2W, 8),
    "K2g-w10": (2, 0, 10, 3, K2G, 1),
}


def _warm_run(hs, rows, cols, run, kind="u8"):
    import torch
    kernel, kb, w, n, name, depth = WARM_RUNS[run]
    m = margin(w, n)
    ps = patches(rows, cols, m)
    try:
        I0, I1 = _frames(rows, cols, kind)
        u, v, at = _warm_planes(rows, cols)
        refs = [patch_flow(p, I0, I1, w, n, ALPHA_WARM, (u, v)) for p in ps]
        ws = _workspace(hs, rows, cols)
        with _forced(hs, kernel, kb):
            assert hs.jacobi_kernel_name(rows, cols, 1, w) == name
            assert hs.iters_per_launch(rows, cols, 1, w) == depth
            hs.gradients_device(I0, I1, ws)
            hs.jacobi_device(rows, cols, 1, w, n, ALPHA_WARM, u, v, ws, warm_start=True)
        torch.cuda.synchronize()
        flag = int(ws[-256:].view(torch.int32)[0])
        assert flag == (1 if kind == "f32" else 0)
        _check(f"{rows}x{cols} {kind} {run}", ps, m, (u, v), refs, plant_at=at)
    finally:
        I0 = I1 = u = v = ws = None
        _release()


@pytest.mark.gpu
@pytest.mark.parametrize("run", list(WARM_RUNS))
@pytest.mark.parametrize("rows,cols", AT_CAP)
def test_warm_start_at_the_cap(hs, rows, cols, run):
    """gradients_device of 8-bit frames (the packed word), then jacobi_device
    from the planted random planes: each kernel forced and asserted (WARM_RUNS)."""
    _warm_run(hs, rows, cols, run)


@pytest.mark.gpu
@pytest.mark.parametrize("run", ["K2-w5", "K4-w5"])
def test_warm_start_f32_gradient_planes_at_the_cap(hs, run):
    """The same frames + 0.375 as float32: the pair is flagged and the
    kernels read the f32 gradient planes; the odd width."""
    _warm_run(hs, *AT_CAP[1], run, kind="f32")


@pytest.mark.gpu
@pytest.mark.parametrize("fusion", [True, False], ids=["fused", "unfused"])
@pytest.mark.parametrize("rows,cols", AT_CAP)
def test_cold_solve_at_the_cap(hs, rows, cols, fusion):
    """flow_device, w = 5, 13 iterations: two K4 passes (the first with K1
    fused in or behind K1) and a one-iteration K2 pass.  (u, v) against
    oracle.flow, and the packed gradient words of the workspace exactly."""
    import torch
    w, n = 5, 13
    m = margin(w, n)
    ps = patches(rows, cols, m)
    try:
        I0, I1 = _frames(rows, cols)
        refs = [patch_flow(p, I0, I1, w, n, 1.0) for p in ps]
        words = [pack_np(*oracle.gradients(_f64(p.crop(I0)), _f64(p.crop(I1)))) for p in ps]
        ws = _workspace(hs, rows, cols)
        u = torch.full((1, rows, cols), float("nan"), device="cuda")
        v = torch.full((1, rows, cols), float("nan"), device="cuda")
        before = hs.first_pass_launches()
        with _forced(hs, 4), hs.first_pass_fusion_as(fusion):
            assert hs.jacobi_kernel_name(rows, cols, 1, w) == K4
            assert hs.iters_per_launch(rows, cols, 1, w) == 6
            if rows % 2 == 0 and cols % 2 == 0:
                assert hs.lib().hsflow_uv_interleave_passes(rows, cols, 1, w, n) > 0
            hs.flow_device(I0, I1, w, n, 1.0, u, v, ws)
        torch.cuda.synchronize()
        assert hs.first_pass_launches() - before == (1 if fusion else 0)
        gpack = _ws_plane(ws, 0, rows, cols, torch.int32)
        for p, want in zip(ps, words):
            sy, sx = p.inner(1)  # the Sobel alone
            got = p.crop(gpack).view(np.uint32)
            assert np.array_equal(got[sy, sx], want[sy, sx]), f"packed words, {p.name}"
        assert int(ws[-256:].view(torch.int32)[0]) == 0
        _check(f"{rows}x{cols} cold {'fused' if fusion else 'unfused'}", ps, m, (u, v), refs)
    finally:
        I0 = I1 = u = v = ws = gpack = None
        _release()


@pytest.mark.gpu
@pytest.mark.parametrize("w", [3, 5])
@pytest.mark.parametrize("rows,cols", AT_CAP)
def test_weighted_kernel_at_the_cap(hs, rows, cols, w):
    """KJ, 7 iterations (w = 3: a launch of 6 and one of 1; w = 5: 3, 3, 1)
    from the planted planes, g from diffusivity_device of them; the reference
    is jacobi_weighted_np on the gradients and g the device holds at the patch."""
    import torch
    n = 7
    m = margin(w, n)
    ps = patches(rows, cols, m)
    try:
        I0, I1 = _frames(rows, cols)
        u, v, _ = _warm_planes(rows, cols)
        ws = _workspace(hs, rows, cols)
        g = torch.full((1, rows, cols), float("nan"), device="cuda")
        hs.gradients_device(I0, I1, ws, gx=g)  # a plane asked for: K1 writes the f32 planes
        hs.diffusivity_device(u, v, LAM, g=g)
        torch.cuda.synchronize()
        gx, gy, gt = (_ws_plane(ws, k, rows, cols, torch.float32) for k in (1, 2, 3))
        refs = [jacobi_weighted_np(p.crop(gx), p.crop(gy), p.crop(gt), p.crop(g), p.crop(u),
                                   p.crop(v), w, n, ALPHA_KJ) for p in ps]
        hs.jacobi_weighted_device(rows, cols, 1, w, n, ALPHA_KJ, g, u, v, ws)
        torch.cuda.synchronize()
        _check(f"{rows}x{cols} KJ w{w}", ps, m, (u, v), refs)
    finally:
        I0 = I1 = u = v = ws = g = gx = gy = gt = None
        _release()


@pytest.mark.gpu
@pytest.mark.parametrize("rows,cols", ABOVE_CAP)
def test_planes_that_hold_the_sentinel_are_refused(hs, rows, cols):
    """2^29 - 3, 2^29 - 2 and 2^29 - 1 pixels: every entry point that launches
    a Jacobi kernel raises "bad size" and writes nothing."""
    import torch
    assert rows * cols > SENTINEL_ELEM and hs.workspace_bytes(rows, cols, 1) == 0
    try:
        I0 = torch.zeros((1, rows, cols), dtype=torch.uint8, device="cuda")
        u, v, g = (torch.full((1, rows, cols), GUARD, device="cuda") for _ in range(3))
        ws = torch.full((4096,), 0xA5, dtype=torch.uint8, device="cuda")
        calls = {
            "flow_device": lambda: hs.flow_device(I0, I0, 5, 6, 1.0, u, v, ws),
            "gradients_device": lambda: hs.gradients_device(I0, I0, ws),
            "jacobi_device": lambda: hs.jacobi_device(rows, cols, 1, 5, 6, 1.0, u, v, ws,
                                                      warm_start=True),
            "jacobi_weighted_device": lambda: hs.jacobi_weighted_device(rows, cols, 1, 5, 3, 1.0,
                                                                        g, u, v, ws),
        }
        for name, call in calls.items():
            with pytest.raises(hs.HsflowError, match="bad size"):
                call()
        torch.cuda.synchronize()
        for t in (u, v, g):
            assert bool((t == GUARD).all())
        assert bool((ws == 0xA5).all())
        assert hs.jacobi_kernel_name(rows, cols, 1, 5) == ""
    finally:
        I0 = u = v = g = ws = None
        _release()
