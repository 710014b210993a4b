"""The sampling kernels at the sizes production runs them at: KC
(hsflow_flow_consistency_device), KI (hsflow_frame_interp_device) and KIC
(hsflow_frame_interp_bgr_device) where a block takes more than one tile of its
grid-stride loop, and on a plane of more than 2^24 pixels, where the f32
quotient of sampler::pixel_xy stops being exact and its correction runs.

The other modules hold these kernels to their float64 references on planes of
at most 37 x 131 px: one tile per block, and no pixel index that a float
cannot hold.  Here

  * "tiles": batch 64 of 211 x 397 px.  The grids are capped at 2 (KC), 6 (KI)
    and 5 (KIC) blocks per CU shared among the batch, so at 256 CUs a block
    takes 2 or 3 of KC's 21 tiles and 6 to 9 of the 164 of KI and KIC, the last
    one ragged; 83 767 mod 4 = 3, so the plane bases take all four alignments
    of KC's first-tile start.  Item k carries the data of pair k mod 3, and the
    float64 reference is computed for the three pairs only.  With 397 columns
    the correction of pixel_xy runs here too, far below 2^24: the f32
    reciprocal of 397 is rounded down, and the first pixel of 76 of the 211
    rows comes out as (cols, y - 1) before it.
  * "past 2^24": one plane of 17426 x 1023 px.  pixel_xy_f32 below restates the
    pixel -> (x, y) split in numpy float32 and names the pixels that take
    either correction (256 each, the first at p = 16 780 269); the reference is
    evaluated at those, their neighbours, the plane's edges, the rows around
    2^24 and 200 000 random pixels (consistency_at, frame_interp_at: the
    modules' float64 operations at a list of pixels).  A pixel whose correction
    went wrong would be computed at the opposite edge of a neighbouring row, so
    the backward flow and the frames carry a ramp in x: the two places differ
    by far more than any tolerance.
  * "tall": 262140 x 5, the most rows the API accepts.

The bounds are the other modules': err within 16 eps32 8 M and the mask equal
outside that band (test_consistency), |out - ref| <= 1e-4 max|ref| outside the
rim band and the flags equal outside the rim and half bands (test_interp).
test_projection_scale.py does the same for KS, KIP and the kernels added since.
"""
import functools

import numpy as np
import pytest

from conftest import norm_rel_err
from synth_ref import texture
from test_consistency import (ABS, EPS32, GAIN, REL, _check_against_ref, _smooth_flows, _terms,
                              consistency_np)
from test_interp import (BAND, TOL, _cuda, _same_bits, _sample_np, frame_interp_np,
                         warp_image_np)
from test_median import _km_planes, median_np
from test_prefilter import NORMALIZE, _kn_frames, _kn_ref, _pf
from test_smoothness import (ALPHA, _kg_flows, _kj_inputs, _kj_run, _kj_setup, diffusivity_np,
                             jacobi_weighted_np)
from test_warped import _gt_bound, _warp_grads, warp_gradients_np

TILES = ("tiles", 64, 3, 211, 397)  # name, batch, distinct pairs, rows, cols
TALL = ("tall", 1, 1, 262140, 5)
BIG = (17426, 1023)  # 17.8 M px
T3 = (0.0, 0.5, 1.0)
T16 = tuple(float(np.float32(k / 15.0)) for k in range(16))
T_BIG = 0.3
# tile sizes (px) and grid caps (blocks per CU) of the three launchers
KC_TILE, KC_PER_CU = 4096, 2
KI_TILE, KI_PER_CU = 512, 6
KIC_TILE, KIC_PER_CU = 512, 5
# (u, v) added to the forward flow of each pair of the tiles case, solver units
TILE_OFFSETS = ((0.9, -0.8), (-0.8, 0.9), (0.85, 0.85))


# ------------------------------------------------ the pixel -> (x, y) split
def pixel_xy_f32(rows, cols, ulp=0):
    """sampler::pixel_xy in numpy float32 for every pixel p of a rows x cols
    plane: y from the f32 product of (float)p and the f32 reciprocal of cols
    (moved by `ulp` ulps), x = p - y cols, then the correction by one row.
    Returns (lo, hi, x, y): the flat indices that take the x < 0 branch, those
    that take the x >= cols branch, and (x, y) after the correction."""
    inv = np.float32(1.0) / np.float32(cols)
    for _ in range(abs(ulp)):
        inv = np.nextafter(inv, np.float32(np.inf if ulp > 0 else -np.inf))
    p = np.arange(rows * cols, dtype=np.int32)
    y = (p.astype(np.float32) * inv).astype(np.int32)  # truncates, as (int)
    x = p - y * np.int32(cols)
    lo, hi = np.flatnonzero(x < 0), np.flatnonzero(x >= cols)
    x[lo] += cols
    y[lo] -= 1
    x[hi] -= cols
    y[hi] += 1
    return lo, hi, x, y


@functools.lru_cache(maxsize=None)
def _fixups(rows, cols, ulp):
    lo, hi, _, _ = pixel_xy_f32(rows, cols, ulp)
    return lo, hi


# ------------------------------------------------------ pointwise references
def _sample_at(img, u, v, x, y):
    """test_interp._sample_np at the pixels (y, x) only: img [rows, cols] or
    [rows, cols, C], (u, v) the float64 displacement of each pixel."""
    rows, cols = img.shape[:2]
    with np.errstate(invalid="ignore", over="ignore"):
        dx = np.fmin(np.fmax(GAIN * u, -float(cols)), float(cols))
        dy = np.fmin(np.fmax(GAIN * v, -float(rows)), float(rows))
        ix, iy = np.floor(dx), np.floor(dy)
        fx, fy = dx - ix, dy - iy
        X, Y = x + ix.astype(np.int64), y + iy.astype(np.int64)
        xa, xb = np.clip(X, 0, cols - 1), np.clip(X + 1, 0, cols - 1)
        ya, yb = np.clip(Y, 0, rows - 1), np.clip(Y + 1, 0, rows - 1)

        def tap(yy, xx):
            return img[yy, xx].astype(np.float64)

        wx, wy = (fx, fy) if img.ndim == 2 else (fx[:, None], fy[:, None])
        top = tap(ya, xa) + wx * (tap(ya, xb) - tap(ya, xa))
        bot = tap(yb, xa) + wx * (tap(yb, xb) - tap(yb, xa))
        val = top + wy * (bot - top)
        tx, ty = x + dx, y + dy
        inside = (tx >= -0.5) & (tx <= cols - 0.5) & (ty >= -0.5) & (ty <= rows - 0.5)
        near = np.where(fy >= 0.5, yb, ya) * cols + np.where(fx >= 0.5, xb, xa)
        rim = np.minimum(np.minimum(np.abs(tx + 0.5), np.abs(tx - (cols - 0.5))),
                         np.minimum(np.abs(ty + 0.5), np.abs(ty - (rows - 0.5))))
        half = np.minimum(np.abs(fx - 0.5), np.abs(fy - 0.5))
    return val, inside, near, rim, half


def _at(plane, idx):
    return np.asarray(plane).reshape(-1)[idx].astype(np.float64)


def consistency_at(uf, vf, ub, vb, idx, rel=REL, abs=ABS):  # noqa: A002 (the ABI's name)
    """test_consistency._terms at the flat pixel indices `idx` of one pair's
    planes: err, mask and the distance to the nearest threshold."""
    rows, cols = uf.shape
    idx = np.asarray(idx, np.int64)
    y, x = np.divmod(idx, cols)
    u, v = _at(uf, idx), _at(vf, idx)
    ub, vb = np.asarray(ub), np.asarray(vb)
    ubw, inside, _, rim, _ = _sample_at(ub, u, v, x, y)
    vbw = _sample_at(vb, u, v, x, y)[0]
    with np.errstate(invalid="ignore", over="ignore"):
        su, sv = u + ubw, v + vbw
        d2 = 64.0 * (su * su + sv * sv)
        mag = 64.0 * ((u * u + v * v) + (ubw * ubw + vbw * vbw))
        err = np.sqrt(d2)
        thr = rel * mag + abs
        out = ~inside
        mask = np.where(out, 2, np.where(~(d2 <= thr), 1, 0)).astype(np.uint8)
        near = np.where(out, rim, np.fmin(rim, np.abs(err - np.sqrt(thr))))
    return err, mask, near


def frame_interp_at(I0, I1, uf, vf, ub, vb, t, idx, mask_f=None, mask_b=None):
    """test_interp.frame_interp_np at the flat pixel indices `idx`: out ([n],
    or [n, C] for frames [rows, cols, C], each channel on its own), flags and
    the two distances."""
    rows, cols = uf.shape
    idx = np.asarray(idx, np.int64)
    y, x = np.divmod(idx, cols)
    fu, fv, bu, bv = (_at(a, idx) for a in (uf, vf, ub, vb))
    t = float(np.float32(t))
    s = 1.0 - t
    a, b, c = s * t, t * t, s * s
    with np.errstate(invalid="ignore", over="ignore"):
        u0, v0 = b * bu - a * fu, b * bv - a * fv
        u1, v1 = c * fu - a * bu, c * fv - a * bv
        s0, in0, n0, rim0, half0 = _sample_at(np.asarray(I0), u0, v0, x, y)
        s1, in1, n1, rim1, half1 = _sample_at(np.asarray(I1), u1, v1, x, y)
        wt = np.where(in0 == in1, t, np.where(in0, 0.0, 1.0))
        w = wt if s0.ndim == 1 else wt[:, None]
        out = np.where(w == 0.0, s0, np.where(w == 1.0, s1, (1.0 - w) * s0 + w * s1))
    flags = (~in0).astype(np.uint8) | ((~in1).astype(np.uint8) << 1)
    if mask_f is not None:
        flags |= (np.asarray(mask_f).reshape(-1)[n0] != 0).astype(np.uint8) << 2
    if mask_b is not None:
        flags |= (np.asarray(mask_b).reshape(-1)[n1] != 0).astype(np.uint8) << 3
    return out, flags, np.minimum(rim0, rim1), np.minimum(half0, half1)


# ------------------------------------------- inputs of the tiles and tall cases
def _frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


@functools.lru_cache(maxsize=None)
def _inputs(case):
    """The distinct pairs of a case: smooth flows, the check's masks each way
    (float64 reference, as test_interp._masks) and BGR u8 frames, whose channel
    1 is the grey u8 frame; the f32 frame is not integer-valued."""
    name, _, pairs, rows, cols = case
    uf, vf, ub, vb = _smooth_flows(pairs, rows, cols)
    if name == "tiles":
        # 7 px more per pair: on a plane of this size _smooth_flows' own 3 px
        # send only 1.6 % of the targets out of the frame
        ox, oy = (np.array(o, np.float32)[:, None, None] for o in zip(*TILE_OFFSETS))
        uf, vf, ub, vb = uf + ox, vf + oy, ub - ox, vb - oy
    flows = _frozen(uf, vf, ub, vb)
    mf = np.stack([consistency_np(uf[k], vf[k], ub[k], vb[k])[1] for k in range(pairs)])
    mb = np.stack([consistency_np(ub[k], vb[k], uf[k], vf[k])[1] for k in range(pairs)])
    bgr = [np.stack([np.stack([texture(base + 10 * c + k, 0, rows, 0, cols) for c in range(3)],
                              axis=-1) for k in range(pairs)]).astype(np.uint8)
           for base in (7000, 8000)]
    u8 = [np.ascontiguousarray(a[..., 1]) for a in bgr]
    f32 = [(u8[0] * 0.9 + 0.3).astype(np.float32), (u8[1] * 0.9 + 0.6).astype(np.float32)]
    _frozen(mf, mb, *bgr, *u8, *f32)
    return {"flows": flows, "masks": (mf, mb), "bgr": tuple(bgr), "u8": tuple(u8),
            "f32": tuple(f32)}


@functools.lru_cache(maxsize=None)
def _kc_ref(case):
    """err, mask, the pixels within the tolerance of a threshold, and the
    tolerance 16 eps32 8 M (test_consistency._smooth_ref)."""
    flows = _inputs(case)["flows"]
    tol = 16.0 * EPS32 * GAIN * max(float(np.abs(a).max()) for a in flows)
    terms = [_terms(*(a[k] for a in flows), REL, ABS) for k in range(flows[0].shape[0])]
    err, mask = np.stack([t[0] for t in terms]), np.stack([t[1] for t in terms])
    near = np.stack([t[2] <= tol for t in terms])
    return _frozen(err, mask, near) + (tol,)


@functools.lru_cache(maxsize=None)
def _interp_ref(case, kind, times):
    """out [P, nt, H, W] (kind "bgr": [P, nt, H, W, 3]), flags [P, nt, H, W] and
    the pixels left out.  Grey frames go through frame_interp_np; BGR frames
    through frame_interp_at at every pixel, which computes the targets once for
    the three channels and equals frame_interp_np per channel bit for bit
    (test_pointwise_references_equal_the_whole_plane_ones)."""
    _, _, pairs, rows, cols = case
    inp = _inputs(case)
    I0, I1 = inp[kind]
    (mf, mb), flows = inp["masks"], inp["flows"]
    out = np.empty((pairs, len(times)) + I0.shape[1:])
    flags = np.empty((pairs, len(times), rows, cols), np.uint8)
    rim, half = np.empty(flags.shape, bool), np.empty(flags.shape, bool)
    every = np.arange(rows * cols)
    for k in range(pairs):
        for j, t in enumerate(times):
            fl = [a[k] for a in flows]
            if kind == "bgr":
                o, f, r, h = (a.reshape((rows, cols) + a.shape[1:]) for a in
                              frame_interp_at(I0[k], I1[k], *fl, t, every, mf[k], mb[k]))
            else:
                o, f, r, h = frame_interp_np(I0[k], I1[k], *fl, t, mf[k], mb[k])
            out[k, j], flags[k, j], rim[k, j], half[k, j] = o, f, r <= BAND, h <= BAND
    return _frozen(out, flags, rim, half)


# ------------------------------------------------ inputs of the 2^24 case
# offsets of the staircases below for which no fixup pixel of the plane lies in
# an exclusion band (test_big_plane_inputs_make_the_fixup_pixels_tell asserts it)
STEP_OFF_U, STEP_OFF_V = 0.003, 0.002


@functools.lru_cache(maxsize=None)
def _big_flows():
    """Closed-form flows of a few pixels (float32, solver units), each a
    function of y plus a smooth function of x.  The forward flow swings +-3.2
    px (u) and +-2.4 px (v) in y with periods of 61.7 and 83.3 rows, so at the
    edge columns it points into and out of the frame in turn; its x part has
    whole periods across the plane.  The y part is a staircase of half-pixel
    steps: the edge columns, where every fixup pixel lies, then hold a few
    dozen distinct displacements, which the two offsets keep clear of the
    exclusion bands (a sinusoid puts four of the 512 fixup pixels within 1e-3
    of a fraction of 0.5 whatever its phase).  The backward flow is -(forward)
    plus a ramp in x, 0.02 -> 0.20 (u) and -0.01 -> 0.16 (v): (y, 0) and
    (y +- 1, cols - 1) differ by more than 0.05 units, and the err of a pixel
    depends on which edge it is taken at."""
    rows, cols = BIG
    y, x = np.arange(rows, dtype=np.float64), np.arange(cols, dtype=np.float64)
    two_pi = 2.0 * np.pi

    def plane(fy, fx):
        return fy.astype(np.float32)[:, None] + fx.astype(np.float32)[None, :]

    uf = plane(np.round(6.4 * np.sin(two_pi * y / 61.7)) / 16.0 + STEP_OFF_U,
               0.05 * np.sin(two_pi * x / 93.0))
    vf = plane(np.round(4.8 * np.cos(two_pi * y / 83.3)) / 16.0 + STEP_OFF_V,
               0.04 * np.sin(two_pi * x / 341.0))
    ub = -uf + (0.02 + 0.18 * x / (cols - 1)).astype(np.float32)[None, :]
    vb = -vf + (-0.01 + 0.17 * x / (cols - 1)).astype(np.float32)[None, :]
    return _frozen(uf, vf, ub, vb)


@functools.lru_cache(maxsize=None)
def _big_frames():
    """Two BGR u8 frames and two masks from an integer hash of (y, x): six
    pseudo-random bits per channel on a ramp in x of 160 (150) grey levels, so
    the two edge columns differ by at least 87; the masks are non-zero at one
    pixel in six."""
    rows, cols = BIG
    x = np.arange(cols, dtype=np.uint32)[None, :]
    y = np.arange(rows, dtype=np.uint32)[:, None]
    out = []
    for seed, lo, span in ((0x9E3779B1, 0, 160), (0x7FEB352D, 20, 150)):
        h = x * np.uint32(2654435761) + y * np.uint32(2246822519) + np.uint32(seed)
        h = (h ^ (h >> np.uint32(15))) * np.uint32(0x85EBCA6B)
        h ^= h >> np.uint32(13)
        b = h.view(np.uint8).reshape(rows, cols, 4)
        ramp = (lo + np.arange(cols) * span // (cols - 1)).astype(np.uint8)
        out.append((b[..., :3] & 63) + ramp[None, :, None])
        out.append(np.where(b[..., 3] < 43, 1 + (b[..., 3] & 1), 0).astype(np.uint8))
    B0, mf, B1, mb = out
    return _frozen(B0, B1, mf, mb)


@functools.lru_cache(maxsize=None)
def _big_points():
    """S, the pixels of the big plane that get a reference, and those of them
    that take a correction with the reciprocal as it is (ulp 0), sorted."""
    rows, cols = BIG
    plane = rows * cols
    fix = np.concatenate([np.concatenate(_fixups(rows, cols, ulp)) for ulp in (0, 1, -1)])
    y24 = (1 << 24) // cols
    whole_rows = [0, 1, rows - 2, rows - 1, y24 - 1, y24, y24 + 1]
    rng = np.random.default_rng(2024)
    S = np.concatenate([fix - 1, fix, fix + 1, rng.integers(0, plane, 200000)] +
                       [np.arange(r * cols, (r + 1) * cols) for r in whole_rows])
    S = np.unique(S[(S >= 0) & (S < plane)]).astype(np.int64)
    fix0 = np.sort(np.concatenate(_fixups(rows, cols, 0))).astype(np.int64)
    return _frozen(S, fix0)


@functools.lru_cache(maxsize=None)
def _big_kc_ref():
    flows = _big_flows()
    tol = 16.0 * EPS32 * GAIN * max(float(np.abs(a).max()) for a in flows)
    err, mask, near = consistency_at(*flows, _big_points()[0])
    return err, mask, near <= tol, tol


@functools.lru_cache(maxsize=None)
def _big_interp_ref(kind):
    B0, B1, mf, mb = _big_frames()
    if kind == "u8":
        B0, B1 = B0[..., 0], B1[..., 0]
    out, flags, rim, half = frame_interp_at(B0, B1, *_big_flows(), T_BIG, _big_points()[0], mf, mb)
    return out, flags, rim <= BAND, half <= BAND


# ------------------------------------------------------------------ CPU tests
@pytest.mark.parametrize("shape", [BIG, (4320, 7680)], ids=lambda s: "x".join(map(str, s)))
def test_pixel_xy_is_exact_after_the_correction(shape):
    rows, cols = shape
    p = np.arange(rows * cols, dtype=np.int32)
    for ulp in (0, 1, -1):
        lo, hi, x, y = pixel_xy_f32(rows, cols, ulp)
        print(f"{rows} x {cols} ulp {ulp:+d}: {lo.size} pixels take x < 0, {hi.size} x >= cols")
        assert np.array_equal(y, p // cols) and np.array_equal(x, p - (p // cols) * cols)


def test_the_big_plane_takes_both_corrections_and_only_past_2_24():
    lo, hi = _fixups(*BIG, 0)
    print(f"x < 0: {lo.size} pixels from p = {lo.min()}; x >= cols: {hi.size} from {hi.min()}")
    assert lo.size >= 100 and hi.size >= 100
    assert lo.min() >= 1 << 24 and hi.min() >= 1 << 24
    # every one lies in the first or the last column
    x = np.concatenate([lo, hi]) % BIG[1]
    assert np.all((x == 0) | (x == BIG[1] - 1))


def test_the_tiles_plane_takes_a_correction_too():
    """Not only past 2^24: where the f32 reciprocal of cols is rounded down, a
    row's first pixel can come out one row short.  211 x 397 has 76 such
    pixels, so the tiles case checks the x >= cols branch on every item."""
    _, _, _, rows, cols = TILES
    lo, hi = _fixups(rows, cols, 0)
    print(f"{rows} x {cols}: {lo.size} pixels take x < 0, {hi.size} x >= cols")
    assert lo.size + hi.size >= 50
    assert np.all(hi % cols == 0) and np.all(lo % cols == cols - 1)


@pytest.mark.parametrize("shape", [(3, 37, 131), (2, 5, 3), (1, 1, 70)],
                         ids=lambda s: "x".join(map(str, s)))
def test_pointwise_references_equal_the_whole_plane_ones(shape):
    """The same float64 operations, so bit for bit, at every pixel."""
    batch, rows, cols = shape
    flows = _smooth_flows(*shape)
    every = np.arange(rows * cols)
    for k in range(batch):
        fl = [a[k] for a in flows]
        whole = _terms(*fl, REL, ABS)
        for got, want in zip(consistency_at(*fl, every), whole):
            assert np.array_equal(got, want.ravel())
        mf, mb = whole[1], consistency_np(fl[2], fl[3], fl[0], fl[1])[1]
        bgr = [np.stack([texture(s + 10 * c + k, 0, rows, 0, cols) for c in range(3)],
                        axis=-1).astype(np.uint8) for s in (4000, 5000)]
        grey = [(a[..., 0] * 0.9 + 0.3).astype(np.float32) for a in bgr]
        val, inside, near, rim, half = _sample_np(grey[1], fl[0], fl[1])
        y, x = np.divmod(every, cols)
        for got, want in zip(_sample_at(grey[1], _at(fl[0], every), _at(fl[1], every), x, y),
                             (val, inside, near, rim, half)):
            assert np.array_equal(got, want.ravel())
        for t in (0.0, 0.3, 0.5, 1.0):
            for masks in ((mf, mb), (None, None)):
                whole = frame_interp_np(*grey, *fl, t, *masks)
                for got, want in zip(frame_interp_at(*grey, *fl, t, every, *masks), whole):
                    assert np.array_equal(got, want.ravel())
            out, flags, rim, half = frame_interp_at(*bgr, *fl, t, every, mf, mb)
            for c in range(3):
                whole = frame_interp_np(bgr[0][..., c], bgr[1][..., c], *fl, t, mf, mb)
                for got, want in zip((out[:, c], flags, rim, half), whole):
                    assert np.array_equal(got, want.ravel())


@pytest.mark.parametrize("case", [TILES, TALL], ids=lambda c: c[0])
def test_tile_inputs_cover_the_classes_and_keep_the_bands_thin(case):
    """Conditions on the inputs of the GPU comparisons, with the caps of the
    other modules: at most 1 % of the pixels within KC's tolerance of a
    threshold, at most 2 % in KI's rim and half bands; on the tiles case all
    three KC classes and flags != 0 hold at least 2 % of the pixels each."""
    _, mask, near, tol = _kc_ref(case)
    share = np.bincount(mask.ravel(), minlength=3) / mask.size
    print(f"{case[0]} KC: classes {share.round(4)}, near a threshold {near.mean():.5f}, "
          f"tol {tol:.2e} px")
    assert near.mean() <= 0.01
    for times in (T3, T16) if case == TILES else (T3,):
        _, flags, rim, half = _interp_ref(case, "f32", times)
        print(f"{case[0]} KI nt {len(times)}: near a rim {rim.mean():.5f}, near a half "
              f"{half.mean():.5f}, flags != 0 {np.mean(flags != 0):.4f}")
        assert (rim | half).mean() <= 0.02
        if case == TILES:
            assert np.mean(flags != 0) >= 0.02
    if case == TILES:
        assert (share >= 0.02).all()


def test_big_plane_inputs_make_the_fixup_pixels_tell():
    """Conditions on the inputs of the 2^24 case, met by the reference alone.
    None of the pixels that take a correction lies in an exclusion band; at
    least 50 of them have an in-frame target and at least 50 an out-of-frame
    one, for KC and for KI; at each of their rows the backward flow differs by
    at least 0.05 units and the frames by at least 16 grey levels between one
    edge column and the other edge column of the row itself and of the rows
    above and below (where a failed correction would take the pixel); and the
    excluded share of S stays within the other modules' caps."""
    rows, cols = BIG
    S, fix0 = _big_points()
    at = np.searchsorted(S, fix0)
    assert np.array_equal(S[at], fix0)
    _, mask, near, tol = _big_kc_ref()
    _, flags, rim, half = _big_interp_ref("u8")
    kc_out, ki_out = mask[at] == 2, (flags[at] & 3) != 0
    print(f"S: {S.size} pixels, {fix0.size} take a correction; KC near a threshold "
          f"{near.mean():.5f}; KI near a rim {rim.mean():.5f}, near a half {half.mean():.5f}")
    print(f"fixup pixels: KC {int((~kc_out).sum())} in-frame, {int(kc_out.sum())} out-of-frame; "
          f"KI {int((~ki_out).sum())} with both targets in-frame, {int(ki_out.sum())} with one out")
    assert not near[at].any() and not rim[at].any() and not half[at].any()
    assert (~kc_out).sum() >= 50 and kc_out.sum() >= 50
    assert (~ki_out).sum() >= 50 and ki_out.sum() >= 50
    assert near.mean() <= 0.01 and (rim | half).mean() <= 0.02
    _, _, ub, vb = _big_flows()
    B0, B1, _, _ = _big_frames()
    ys = np.unique(fix0 // cols)
    assert ys.min() >= 1 and ys.max() <= rows - 2
    for dy in (-1, 0, 1):
        for a, least in ((ub, 0.05), (vb, 0.05), (B0, 16), (B1, 16)):
            a = a.astype(np.float64)
            for here, there in ((0, cols - 1), (cols - 1, 0)):
                assert np.abs(a[ys, here] - a[ys + dy, there]).min() >= least


# ------------------------------------------------------------------ GPU tests
def _cap(per_cu, batch):
    import torch
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    return max(1, (per_cu * cus + batch - 1) // batch)


def _assert_blocks_take_three_tiles(case, tile, per_cu):
    """Fails, never skips, where the device is so wide that the case no longer
    gives a block a second and a third tile."""
    _, batch, _, rows, cols = case
    ntiles, cap = (rows * cols + tile - 1) // tile, _cap(per_cu, batch)
    print(f"{ntiles} tiles on a grid of {min(ntiles, cap)} blocks per pair")
    assert ntiles >= 2 * cap + 1


def _batched(case, a):
    """Pair k mod P of `a` [P, ...] for each of the case's batch items, on the
    device."""
    import torch
    _, batch, pairs, _, _ = case
    t = _cuda(a)
    return t[torch.arange(batch, device="cuda") % pairs].contiguous()


def _assert_items_repeat(case, t):
    """Item k holds the bits of item k mod P."""
    import torch
    _, batch, pairs, _, _ = case
    assert _same_bits(t, t[torch.arange(batch, device="cuda") % pairs])


def _check_kc(hs, case):
    """KC on the case's batch: err and mask of the distinct pairs against the
    reference, every item bit-identical to its pair's first, counts the
    histogram of the device's own mask."""
    import torch
    _, _, pairs, _, _ = case
    flows = [_batched(case, a) for a in _inputs(case)["flows"]]
    err, mask, counts = hs.consistency_device(*flows, err=True, mask=True, counts=True)
    torch.cuda.synchronize()
    _assert_items_repeat(case, err)
    _assert_items_repeat(case, mask)
    hist = torch.stack([(mask == c).sum(dim=(1, 2)) for c in range(3)], dim=1)
    assert torch.equal(counts.to(torch.int64), hist)
    ref_err, ref_mask, near, tol = _kc_ref(case)
    _check_against_ref(err[:pairs].cpu().numpy(), mask[:pairs].cpu().numpy(), ref_err, ref_mask,
                       near, tol)


def _round_u8(x):
    import torch
    return torch.clamp(torch.floor(x + 0.5), 0.0, 255.0).to(torch.uint8)


def _check_interp(case, kind, times, out, flags, trusted, out8, flags8):
    """The assertions of the tiles case on one interpolation's outputs (KI, or
    KIC with a channel axis last): items repeat, trusted counts the device's
    own flags == 0, the u8 output is the rounded f32 output, and the distinct
    pairs meet the reference."""
    import torch
    _, _, pairs, _, _ = case
    for t in (out, flags, out8):
        _assert_items_repeat(case, t)
    assert torch.equal(trusted.to(torch.int64), (flags == 0).sum(dim=(2, 3)))
    assert out8.dtype == torch.uint8 and torch.equal(out8, _round_u8(out))
    assert torch.equal(flags8, flags)
    ref, ref_flags, rim, half = _interp_ref(case, kind, times)
    got, got_flags = out[:pairs].cpu().numpy(), flags[:pairs].cpu().numpy()
    d = np.abs(got.astype(np.float64) - ref)[~rim]
    bound = TOL * float(np.abs(ref).max())
    print(f"{case[0]} {kind} nt {len(times)}: worst |out - ref| {d.max():.3e} (bound "
          f"{bound:.3e}), excluded {(rim | half).mean():.5f}")
    assert np.all(d <= bound)
    keep = ~(rim | half)
    assert np.array_equal(got_flags[keep], ref_flags[keep])


def _run_ki(hs, case, kind, times, out_dtype=None, frames=None):
    inp = _inputs(case)
    frames = inp[kind] if frames is None else frames
    return hs.frame_interp_device(
        *(_batched(case, a) for a in frames), *(_batched(case, a) for a in inp["flows"]), times,
        mask_f=_batched(case, inp["masks"][0]), mask_b=_batched(case, inp["masks"][1]),
        out_dtype=out_dtype, flags=True, trusted=True)


def _check_ki(hs, case, kind, times):
    import torch
    out, flags, trusted = _run_ki(hs, case, kind, times)
    out8, flags8, _ = _run_ki(hs, case, kind, times, out_dtype=torch.uint8)
    torch.cuda.synchronize()
    _check_interp(case, kind, times, out, flags, trusted, out8, flags8)


@pytest.mark.gpu
def test_consistency_kernel_over_several_tiles_per_block(hs):
    _assert_blocks_take_three_tiles(TILES, KC_TILE, KC_PER_CU)
    _check_kc(hs, TILES)


@pytest.mark.gpu
@pytest.mark.parametrize("kind,times", [("u8", T3), ("f32", T3), ("f32", T16)],
                         ids=["u8-3", "f32-3", "f32-16"])
def test_interp_kernel_over_several_tiles_per_block(hs, kind, times):
    _assert_blocks_take_three_tiles(TILES, KI_TILE, KI_PER_CU)
    _check_ki(hs, TILES, kind, times)


@pytest.mark.gpu
@pytest.mark.parametrize("times", [T3, T16], ids=["3", "16"])
@pytest.mark.parametrize("wide", [True, False], ids=["wide", "bytes"])
def test_colour_interp_kernel_over_several_tiles_per_block(hs, wide, times):
    """The tiles case's assertions in both forms of the tap loads, and each
    channel bit-identical to KI on that channel's plane."""
    import torch
    _assert_blocks_take_three_tiles(TILES, KIC_TILE, KIC_PER_CU)
    inp = _inputs(TILES)
    args = [_batched(TILES, a) for a in inp["bgr"] + inp["flows"]]
    mf, mb = (_batched(TILES, m) for m in inp["masks"])
    was = hs.set_interp_bgr_loads(wide)
    try:
        out, flags, trusted = hs.frame_interp_bgr_device(*args, times, mask_f=mf, mask_b=mb,
                                                         flags=True, trusted=True)
        out8, flags8, _ = hs.frame_interp_bgr_device(*args, times, mask_f=mf, mask_b=mb,
                                                     out_dtype=torch.uint8, flags=True)
        torch.cuda.synchronize()
    finally:
        hs.set_interp_bgr_loads(was)
    _check_interp(TILES, "bgr", times, out, flags, trusted, out8, flags8)
    for c in range(3):
        planes = [np.ascontiguousarray(a[..., c]) for a in inp["bgr"]]
        want, want_f, want_c = _run_ki(hs, TILES, "u8", times, frames=planes)
        assert _same_bits(out[..., c].contiguous(), want)
        assert torch.equal(flags, want_f) and torch.equal(trusted, want_c)
    torch.cuda.synchronize()


def _assert_only_at(bad, what):
    """No pixel of S is `bad`; a failure names the pixels and says whether
    they are the ones that take a correction."""
    S, fix0 = _big_points()
    lo, hi = _fixups(*BIG, 0)
    print(f"{what}: {int(bad.sum())} of {S.size} pixels fail, {int(np.isin(S[bad], fix0).sum())} "
          f"of them among the {fix0.size} that take a correction")
    assert not bad.any(), (what, S[bad][:8], np.isin(S[bad], lo).sum(), np.isin(S[bad], hi).sum())


@pytest.mark.gpu
def test_consistency_kernel_past_2_24_pixels(hs):
    """KC on 17426 x 1023: at S the bounds of the tiles case; over the plane,
    counts is the histogram of the device's own mask."""
    import torch
    S, fix0 = _big_points()
    ref_err, ref_mask, near, tol = _big_kc_ref()
    flows = [_cuda(a)[None] for a in _big_flows()]
    try:
        err, mask, counts = hs.consistency_device(*flows, err=True, mask=True, counts=True)
        torch.cuda.synchronize()
        hist = torch.stack([(mask == c).sum() for c in range(3)])
        assert torch.equal(counts[0].to(torch.int64), hist)
        s = _cuda(S)
        e, m = err.flatten()[s].cpu().numpy(), mask.flatten()[s].cpu().numpy()
    finally:
        del flows
        err = mask = counts = None
        torch.cuda.empty_cache()
    d = np.abs(e.astype(np.float64) - ref_err)
    at = np.searchsorted(S, fix0)
    print(f"KC: worst |err - ref| {d.max():.3e} px (bound {tol:.3e}), excluded {near.mean():.5f}; "
          f"device mask at the fixup pixels: {int((m[at] != 2).sum())} in-frame, "
          f"{int((m[at] == 2).sum())} out-of-frame")
    assert near.mean() <= 0.01
    _assert_only_at((d > tol) | ((m != ref_mask) & ~near), "KC")


def _check_big_interp(kind, out, flags, trusted, fn_name):
    """An interpolation of the big plane (out [1, 1, H, W(, 3)] f32) at S."""
    import torch
    S, fix0 = _big_points()
    ref, ref_flags, rim, half = _big_interp_ref(kind)
    assert int(trusted[0, 0]) == int((flags == 0).sum())
    s = _cuda(S)
    o = out.reshape((-1,) + ref.shape[1:])[s].cpu().numpy()
    f = flags.flatten()[s].cpu().numpy()
    d = np.abs(o.astype(np.float64) - ref)
    d = d if d.ndim == 1 else d.max(axis=1)
    bound = TOL * float(np.abs(ref).max())
    at = np.searchsorted(S, fix0)
    print(f"{fn_name}: worst |out - ref| {d[~rim].max():.3e} (bound {bound:.3e}), excluded "
          f"{(rim | half).mean():.5f}; device flags at the fixup pixels: "
          f"{int(((f[at] & 3) == 0).sum())} with both targets in-frame, "
          f"{int(((f[at] & 3) != 0).sum())} with one out")
    assert (rim | half).mean() <= 0.02
    _assert_only_at(((d > bound) & ~rim) | ((f != ref_flags) & ~(rim | half)), fn_name)


@pytest.mark.gpu
def test_interp_kernel_past_2_24_pixels(hs):
    """KI on 17426 x 1023, u8 frames, t = 0.3, both masks: at S the bounds of
    the tiles case; over the plane, trusted counts the device's own flags."""
    import torch
    B0, B1, mf, mb = _big_frames()
    args = [_cuda(a[..., 0])[None] for a in (B0, B1)] + [_cuda(a)[None] for a in _big_flows()]
    try:
        out, flags, trusted = hs.frame_interp_device(
            *args, (T_BIG,), mask_f=_cuda(mf)[None], mask_b=_cuda(mb)[None], flags=True,
            trusted=True)
        torch.cuda.synchronize()
        _check_big_interp("u8", out, flags, trusted, "KI")
    finally:
        del args
        out = flags = trusted = None
        torch.cuda.empty_cache()


@pytest.mark.gpu
@pytest.mark.parametrize("wide", [True, False], ids=["wide", "bytes"])
def test_colour_interp_kernel_past_2_24_pixels(hs, wide):
    """KIC on 17426 x 1023 in both forms of the tap loads: the u8 output is the
    rounded f32 output over the whole plane, and the f32 output meets the
    reference at S."""
    import torch
    B0, B1, mf, mb = _big_frames()
    args = [_cuda(a)[None] for a in (B0, B1) + _big_flows()]
    masks = dict(mask_f=_cuda(mf)[None], mask_b=_cuda(mb)[None])
    was = hs.set_interp_bgr_loads(wide)
    try:
        out, flags, trusted = hs.frame_interp_bgr_device(*args, (T_BIG,), **masks, flags=True,
                                                         trusted=True)
        out8, flags8, _ = hs.frame_interp_bgr_device(*args, (T_BIG,), **masks,
                                                     out_dtype=torch.uint8, flags=True)
        torch.cuda.synchronize()
        assert out8.dtype == torch.uint8 and torch.equal(out8, _round_u8(out))
        assert torch.equal(flags8, flags)
        _check_big_interp("bgr", out, flags, trusted, "KIC")
    finally:
        hs.set_interp_bgr_loads(was)
        del args, masks
        out = flags = trusted = out8 = flags8 = None
        torch.cuda.empty_cache()


@pytest.mark.gpu
def test_consistency_and_interp_kernels_on_the_tallest_plane(hs):
    """262140 x 5, the most rows the API accepts, through the tiles case's
    checks (batch 1, f32 frames)."""
    _check_kc(hs, TALL)
    _check_ki(hs, TALL, "f32", T3)


# The 64 x 4-block kernels at the grid's limit of 65 535 blocks in y: each
# against its own module's float64 reference and tolerance, whole plane.
TALL_SHAPE = TALL[2:]  # (1, 262140, 5)


@pytest.mark.gpu
def test_warp_gradients_kernel_on_the_tallest_plane(hs):
    """KW: gx, gy the bits of the unwarped gradient kernel, gt' within
    test_warped's bound."""
    inp = _inputs(TALL)
    I0, I1 = inp["f32"]
    u0, v0 = inp["flows"][:2]
    got, k1 = _warp_grads(hs, _cuda(I0), _cuda(I1), _cuda(u0), _cuda(v0))
    for a, b in zip(got[:2], k1[:2]):
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
    uk, vk = u0[0].astype(np.float64), v0[0].astype(np.float64)
    gx, gy, gt = warp_gradients_np(I0[0], I1[0], uk, vk)
    ratio = np.abs(got[2][0].astype(np.float64) - gt) / _gt_bound(gx, gy, uk, vk)
    print(f"KW {TALL_SHAPE}: worst err/bound {ratio.max():.4f}")
    assert np.all(ratio <= 1.0)


@pytest.mark.gpu
def test_warp_image_kernels_on_the_tallest_plane(hs):
    """KR on the f32 frame and KRC on the BGR frame, per channel: within
    test_interp's 1e-4 max(|ref|, 1), oof equal outside the rim band."""
    import torch
    inp = _inputs(TALL)
    uf, vf = inp["flows"][:2]
    u, v = _cuda(uf), _cuda(vf)
    out, oof = hs.warp_image_device(_cuda(inp["f32"][1]), u, v, oof=True)
    bgr, oof_c = hs.warp_image_bgr_device(_cuda(inp["bgr"][1]), u, v, oof=True)
    torch.cuda.synchronize()
    assert torch.equal(oof, oof_c)
    planes = [(inp["f32"][1][0], out[0].cpu().numpy())]
    planes += [(inp["bgr"][1][0, ..., c], bgr[0, ..., c].cpu().numpy()) for c in range(3)]
    for name, (img, got) in zip(("KR", "KRC b", "KRC g", "KRC r"), planes):
        ref, ref_oof, rim = warp_image_np(img, uf[0], vf[0])
        worst, bound = np.abs(got - ref).max(), TOL * max(float(np.abs(ref).max()), 1.0)
        print(f"{name} {TALL_SHAPE}: worst |out - ref| {worst:.3e} (bound {bound:.3e}), near a "
              f"rim {(rim <= BAND).mean():.5f}")
        assert worst <= bound
        keep = rim > BAND
        assert np.array_equal(oof[0].cpu().numpy()[keep], ref_oof[keep])


@pytest.mark.gpu
def test_median_kernel_on_the_tallest_plane(hs):
    """KM, 5 x 5: median_np bit for bit, the special values included."""
    import torch
    u, v = _km_planes(TALL_SHAPE, 0), _km_planes(TALL_SHAPE, 1)
    ou, ov = hs.median_device(_cuda(u), _cuda(v), 5)
    torch.cuda.synchronize()
    for got, plane in ((ou, u), (ov, v)):
        want = median_np(plane[0], 5).view(np.uint32)
        assert np.array_equal(got[0].cpu().numpy().view(np.uint32), want)


@pytest.mark.gpu
def test_diffusivity_kernel_on_the_tallest_plane(hs):
    """KG: max|g - ref| <= 1e-5 (test_smoothness)."""
    import torch
    u, v = _kg_flows(TALL_SHAPE)
    for lam in (0.1, 1.0):
        g = hs.diffusivity_device(_cuda(u), _cuda(v), lam)
        torch.cuda.synchronize()
        got = g.cpu().numpy().astype(np.float64)
        worst = float(np.abs(got[0] - diffusivity_np(u[0], v[0], lam)).max())
        print(f"KG {TALL_SHAPE} lam {lam}: worst |g - ref| {worst:.3e}, g in [{got.min():.3e}, "
              f"{got.max():.3e}]")
        assert worst <= 1e-5
        assert got.min() > 0.0 and got.max() <= 1.0


@pytest.mark.gpu
@pytest.mark.parametrize("w", [3, 5])
def test_weighted_kernel_on_the_tallest_plane(hs, w):
    """KJ, 7 iterations: max|d| <= 1e-4 max|ref| against jacobi_weighted_np on
    the planes the workspace holds (test_smoothness)."""
    _, _, _, _, u, v, g = _kj_inputs(TALL_SHAPE)
    ws, (gx, gy, gt) = _kj_setup(hs, TALL_SHAPE)
    tu, tv = _kj_run(hs, TALL_SHAPE, ws, w, (7,), _cuda(g), u, v)
    ru, rv = jacobi_weighted_np(gx[0], gy[0], gt[0], g[0], u[0], v[0], w, 7, ALPHA)
    eu, ev = norm_rel_err(tu[0].cpu().numpy(), ru), norm_rel_err(tv[0].cpu().numpy(), rv)
    print(f"KJ {TALL_SHAPE} w {w} n 7: {eu:.2e} {ev:.2e}")
    assert eu <= TOL and ev <= TOL


@pytest.mark.gpu
def test_prefilter_kernel_on_the_tallest_plane(hs):
    """KN, sigma 1.7, normalise mode at eps 1, scale 32: max|d| <= 1e-4 max|ref|
    (test_prefilter)."""
    import torch
    out = hs.prefilter_device(_cuda(_kn_frames(TALL_SHAPE, "f32")), _pf(hs, NORMALIZE, 1.7, 1.0, 32.0))
    torch.cuda.synchronize()
    ref = _kn_ref(TALL_SHAPE, "f32", NORMALIZE, 1.7)
    top = float(np.abs(ref).max())
    worst = float(np.abs(out.cpu().numpy().astype(np.float64) - ref).max())
    print(f"KN {TALL_SHAPE} sigma 1.7 mode {NORMALIZE}: worst |out - ref| {worst:.3e} (bound "
          f"{TOL * top:.3e})")
    assert top >= 1.0  # the plane has a scale of its own
    assert tuple(out.shape) == TALL_SHAPE and worst <= TOL * top
