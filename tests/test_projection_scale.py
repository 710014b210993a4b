"""The projection kernels at the sizes test_sampling_scale.py holds the older
sampling kernels at: KS (hsflow_flow_project_device) and KIP
(hsflow_frame_interp_proj_device, grey and BGR) where a block takes more than
one tile of its grid-stride loop, on a plane of more than 2^24 pixels, where
sampler::pixel_xy's correction runs and a source index no longer fits a float,
and on the tallest plane the API accepts; and on that plane the 64 x 4-block
kernels added since test_sampling_scale's list: KD, KP, KB, K0 and KU.

test_projection.py holds KS and KIP to their float64 reference on planes of at
most 96 x 128 px: one tile per block, a few blocks on one 64-bit minimum.  Here

  * "tiles" (test_sampling_scale.TILES): batch 64 of 211 x 397 px, item k the
    data of pair k mod 3.  KS has KC's tiles and cap (21 tiles of 4096 px, 2
    blocks per CU), KIP KI's (164 tiles of 512 px, 6 blocks per CU; 5 on BGR
    frames); 76 of the 211 row starts take pixel_xy's x >= cols branch.  The
    reference is project_np on the three pairs; KIP runs on the reference's
    own cells.
  * "past 2^24" (BIG, 17426 x 1023 px).  KS against project_np on two row
    bands, rows [0, 64) and [2^24 // cols - 16, rows): a target is compared
    where every row within REACH of it lies in the band or past the plane's
    edge, REACH being the rows a candidate can travel plus the rows its cost's
    taps can lie from it, both from the flows' maxima, so that nothing from
    outside the band bears on the cell.  Over the whole plane every cell of the
    GPU's must decode to a source in the plane and within the flows' travel of
    its target.  KIP takes any cell plane, so its cells are a closed form of
    (y, x) (_big_cells_at) and its reference frame_interp_proj_at below,
    frame_interp_proj_np at a list of pixels, at test_sampling_scale's S.
  * "tall" (TALL, 262140 x 5): KS and KIP through the tiles case's checks; KD,
    KP, KB, K0 and KU through their own modules' tests, called with this shape.

Tolerances are the owning modules': cells equal word for word outside the
doubt (test_projection), |out - ref| <= 1e-4 max|ref| outside the rim band and
the flags equal outside the rim and half bands (test_interp).

What the comparisons measured on an MI355X is in DESIGN.md, "Flow projection".
The tall case is the regression test of the one defect they found: KS's target
row was floorf((float)y + tau dy + 0.5f), and from row 2^17 on a float holds
1/64 px, so 0.43 % of either direction's candidates landed a row off and
17 017 of the case's 3.9 M cells differed from the reference outside the
doubt.  KS now adds the rounded displacement to the integer pixel
(hsflow_project.hip, splat) and none does.
"""
import functools

import numpy as np
import pytest

import test_finest as _finest
import test_pyramid as _pyramid
import test_temporal as _temporal
from test_interp import BAND, TOL, _cuda, _same_bits
from test_projection import (CODE_CAP, DOUBT_CAP, EMPTY, GAIN, HOLE, _cells_cuda, _decodable, _u64,
                             frame_interp_proj_np, project_np)
from test_sampling_scale import (BIG, KC_PER_CU, KC_TILE, KI_PER_CU, KI_TILE, KIC_PER_CU, KIC_TILE,
                                 T3, T16, T_BIG, TALL, TALL_SHAPE, TILES,
                                 _assert_blocks_take_three_tiles, _assert_items_repeat,
                                 _assert_only_at, _at, _batched, _big_flows, _big_frames,
                                 _big_points, _fixups, _frozen, _inputs, _round_u8, _sample_at)

KS_CASES = [("u8", T3), ("f16", T3), ("f32", T3), ("f64", T3), ("f32", T16)]
KIP_CASES = [("u8", T3), ("f32", T3), ("f32", T16)]
CASE_IDS = dict(ids=lambda c: f"{c[0]}-{len(c[1])}")
KS_BIG_TIMES = (0.0, T_BIG)
LOW31 = np.uint64(0x7FFFFFFF)


# ------------------------------------------------ the tiles and tall references
def _frames(case, kind):
    """The case's frames as the input kind's arrays: f16 from the u8 frames
    (integer-valued), f64 from the f32 ones."""
    inp = _inputs(case)
    if kind == "f16":
        return tuple(a.astype(np.float16) for a in inp["u8"])
    if kind == "f64":
        return tuple(a.astype(np.float64) for a in inp["f32"])
    return inp[kind]


@functools.lru_cache(maxsize=None)
def _cells_ref(case, kind, times):
    """project_np of the case's distinct pairs: cells and doubt, [P, nt, H, W]."""
    _, _, pairs, rows, cols = case
    G0, G1 = _frames(case, kind)
    flows = _inputs(case)["flows"]
    cells = np.empty((pairs, len(times), rows, cols), np.uint64)
    doubt = np.empty(cells.shape, bool)
    for k in range(pairs):
        for j, t in enumerate(times):
            cells[k, j], doubt[k, j] = project_np(G0[k], G1[k], *(a[k] for a in flows), t)
    return _frozen(cells, doubt)


@functools.lru_cache(maxsize=None)
def _proj_ref(case, kind, times):
    """frame_interp_proj_np on the reference's own cells with the case's masks:
    out, flags and the pixels left out, [P, nt, H, W]."""
    inp = _inputs(case)
    I0, I1 = inp[kind]
    (mf, mb), flows = inp["masks"], inp["flows"]
    cells, _ = _cells_ref(case, kind, times)
    out = np.empty(cells.shape)
    flags = np.empty(cells.shape, np.uint8)
    rim, half = np.empty(cells.shape, bool), np.empty(cells.shape, bool)
    for k in range(cells.shape[0]):
        for j, t in enumerate(times):
            o, f, r, h = frame_interp_proj_np(I0[k], I1[k], *(a[k] for a in flows), t,
                                              cells[k, j], mf[k], mb[k])
            out[k, j], flags[k, j], rim[k, j], half[k, j] = o, f, r <= BAND, h <= BAND
    return _frozen(out, flags, rim, half)


def _interior(times):
    return [j for j, t in enumerate(times) if 0.0 < t < 1.0]


def _ks_shares(case, kind, times):
    """Per time: the share of targets in doubt, of empty targets, and of the
    winners that come from direction 1."""
    cells, doubt = _cells_ref(case, kind, times)
    full = cells != EMPTY
    back = full & (((cells >> np.uint64(31)) & np.uint64(1)) != 0)
    nt = len(times)
    return ([float(doubt[:, j].mean()) for j in range(nt)],
            [float(1.0 - full[:, j].mean()) for j in range(nt)],
            [float(back[:, j].sum() / full[:, j].sum()) for j in range(nt)])


def _fmt(shares):
    return " ".join(f"{s:.4f}" for s in shares)


# ------------------------------------------------------ the 2^24 case: KS
@functools.lru_cache(maxsize=None)
def _big_travel():
    """From the flows' maxima m (px): the rows and columns a candidate's target
    can lie from it, ceil(m + 0.5), and REACH, that plus the rows the taps of
    its cost can lie from it, ceil(m) + 1."""
    uf, vf, ub, vb = _big_flows()
    mx = GAIN * max(float(np.abs(uf).max()), float(np.abs(ub).max()))
    my = GAIN * max(float(np.abs(vf).max()), float(np.abs(vb).max()))
    ty, tx = int(np.ceil(my + 0.5)), int(np.ceil(mx + 0.5))
    return ty, tx, ty + int(np.ceil(my)) + 1


def _big_grey():
    B0, B1, _, _ = _big_frames()
    return B0[..., 0], B1[..., 0]


@functools.lru_cache(maxsize=None)
def _big_ks_ref():
    """project_np on the two row bands at KS_BIG_TIMES.  Per band (r0, r1,
    cells [nt, r1 - r0, cols] with the source indices those of the whole plane,
    doubt, and the targets compared [r1 - r0] by row)."""
    rows, cols = BIG
    G0, G1 = _big_grey()
    flows = _big_flows()
    reach = _big_travel()[2]
    bands = []
    for r0, r1 in ((0, 64), ((1 << 24) // cols - 16, rows)):
        cells = np.empty((len(KS_BIG_TIMES), r1 - r0, cols), np.uint64)
        doubt = np.empty(cells.shape, bool)
        for j, t in enumerate(KS_BIG_TIMES):
            c, doubt[j] = project_np(G0[r0:r1], G1[r0:r1], *(a[r0:r1] for a in flows), t)
            cells[j] = np.where(c == EMPTY, EMPTY, c + np.uint64(r0 * cols))
        y = np.arange(r0, r1)
        # every row within `reach`: in the band, or past the plane's edge
        compared = ((y - reach >= r0) | (y - reach < 0)) & ((y + reach < r1) | (y + reach >= rows))
        assert r0 == 0 or y[compared].min() == r0 + reach
        bands.append((r0, r1) + _frozen(cells, doubt, compared))
    return tuple(bands)


def _code_at(own, other, u, v, p, x, y):
    """project_np's cost code of source pixel p of frame `own`, evaluated as if
    the pixel were (y, x): the other frame at the flow's target from there."""
    w = _sample_at(np.asarray(other), _at(u, p), _at(v, p), x, y)[0]
    c8 = np.abs(w - _at(own, p)) * 8.0
    return np.floor(np.where(c8 < CODE_CAP, c8, CODE_CAP)).astype(np.uint64)


# ------------------------------------------------------ the 2^24 case: KIP
# seed of the cells' hash for which no pixel that takes a correction lies in
# an exclusion band (test_big_cells_make_the_fixup_pixels_tell asserts it)
CELL_SEED = 0x1B873593


def _big_cells_at(y, x, seed=CELL_SEED):
    """A cell for every pixel (y, x) of the big plane from an integer hash: one
    in 16 empty; else a hash bit as the direction, the pixel displaced by up to
    +-3 px each way and clamped to the plane as the source, and 30 more hash
    bits as the upper word."""
    rows, cols = BIG
    y, x = np.asarray(y, np.int64), np.asarray(x, np.int64)
    h = x.astype(np.uint32) * np.uint32(2654435761) + y.astype(np.uint32) * np.uint32(2246822519)
    h = h + np.asarray(seed, np.uint32)
    h = (h ^ (h >> np.uint32(15))) * np.uint32(0x85EBCA6B)
    h = (h ^ (h >> np.uint32(13))) * np.uint32(0xC2B2AE35)
    h = h ^ (h >> np.uint32(16))
    g = (h * np.uint32(0x27D4EB2F)) >> np.uint32(2)
    empty = (h & np.uint32(15)) == 0
    back = ((h >> np.uint32(4)) & np.uint32(1)).astype(np.uint64)
    ox = ((h >> np.uint32(5)) & np.uint32(0xFF)).astype(np.int64) % 7 - 3
    oy = ((h >> np.uint32(13)) & np.uint32(0xFF)).astype(np.int64) % 7 - 3
    src = np.clip(y + oy, 0, rows - 1) * cols + np.clip(x + ox, 0, cols - 1)
    cell = (g.astype(np.uint64) << np.uint64(32)) | (back << np.uint64(31)) | src.astype(np.uint64)
    return np.where(empty, EMPTY, cell)


@functools.lru_cache(maxsize=None)
def _big_cells():
    rows, cols = BIG
    return _frozen(_big_cells_at(np.arange(rows)[:, None], np.arange(cols)[None, :]))[0]


def _interp_proj_at(I0, I1, uf, vf, ub, vb, t, idx, cell, mask_f, mask_b):
    """frame_interp_proj_at given the cells of the pixels `idx` themselves."""
    rows, cols = uf.shape
    idx = np.asarray(idx, np.int64)
    y, x = np.divmod(idx, cols)
    cell = np.asarray(cell, np.uint64)
    t = float(np.float32(t))
    s = 1.0 - t
    a, b, c = s * t, t * t, s * s
    hole = cell == EMPTY
    back = ((cell >> np.uint64(31)) & np.uint64(1)) != 0
    p = np.where(hole, 0, cell & LOW31).astype(np.int64)
    assert p.max() < uf.size
    fu, fv, bu, bv = (_at(f, idx) for f in (uf, vf, ub, vb))
    with np.errstate(invalid="ignore", over="ignore"):
        ut = np.where(back, -_at(ub, p), _at(uf, p))
        vt = np.where(back, -_at(vb, p), _at(vf, p))
        u0 = np.where(hole, b * bu - a * fu, -t * ut)
        v0 = np.where(hole, b * bv - a * fv, -t * vt)
        u1 = np.where(hole, c * fu - a * bu, s * ut)
        v1 = np.where(hole, c * fv - a * bv, s * vt)
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
    flags |= hole.astype(np.uint8) * np.uint8(HOLE)
    return out, flags, np.minimum(rim0, rim1), np.minimum(half0, half1)


def frame_interp_proj_at(I0, I1, uf, vf, ub, vb, t, idx, cells, mask_f=None, mask_b=None):
    """test_projection.frame_interp_proj_np at the flat pixel indices `idx`, as
    frame_interp_at is frame_interp_np there: out ([n], or [n, C] for frames
    [rows, cols, C], each channel on its own), flags (HOLE included) and the
    two distances.  cells: the pair's whole cell plane at time t."""
    cell = np.asarray(cells).reshape(-1)[np.asarray(idx, np.int64)]
    return _interp_proj_at(I0, I1, uf, vf, ub, vb, t, idx, cell, mask_f, mask_b)


@functools.lru_cache(maxsize=None)
def _big_proj_ref(kind):
    """KIP's reference on the big plane at S: out, flags, the pixels left out."""
    B0, B1, mf, mb = _big_frames()
    if kind == "u8":
        B0, B1 = B0[..., 0], B1[..., 0]
    S = _big_points()[0]
    y, x = np.divmod(S, BIG[1])
    out, flags, rim, half = _interp_proj_at(B0, B1, *_big_flows(), T_BIG, S, _big_cells_at(y, x),
                                            mf, mb)
    return out, flags, rim <= BAND, half <= BAND


# ------------------------------------------------------------------ CPU tests
@pytest.mark.parametrize("case", KS_CASES, **CASE_IDS)
def test_tile_inputs_keep_the_doubt_thin_and_have_holes_and_both_directions(case):
    """Conditions on the inputs of KS's tiles comparison, by the reference
    alone: at every time at most DOUBT_CAP of the targets in doubt and at least
    20 % of the winners from each direction; at an interior time at least 2 %
    of the targets empty."""
    kind, times = case
    doubt, holes, back = _ks_shares(TILES, kind, times)
    print(f"tiles KS {kind} nt {len(times)}: in doubt {_fmt(doubt)}; empty {_fmt(holes)}; "
          f"direction 1 wins {_fmt(back)}")
    assert max(doubt) <= DOUBT_CAP
    assert max(holes[j] for j in _interior(times)) >= 0.02
    assert min(back) >= 0.2 and max(back) <= 0.8


@pytest.mark.parametrize("case", KIP_CASES, **CASE_IDS)
def test_tile_inputs_keep_the_bands_thin_and_cover_the_flags(case):
    """Conditions on the inputs of KIP's tiles comparison: at most 2 % of the
    pixels in the rim and half bands (test_sampling_scale's cap); at an
    interior time at least 2 % with HOLE; at least 2 % with a target out of the
    frame."""
    kind, times = case
    _, flags, rim, half = _proj_ref(TILES, kind, times)
    holes = [float(np.mean(flags[:, j] & HOLE != 0)) for j in range(len(times))]
    print(f"tiles KIP {kind} nt {len(times)}: near a rim {rim.mean():.5f}, near a half "
          f"{half.mean():.5f}, HOLE {_fmt(holes)}, a target out {np.mean(flags & 3 != 0):.4f}")
    assert (rim | half).mean() <= 0.02
    assert max(holes[j] for j in _interior(times)) >= 0.02
    assert np.mean(flags & 3 != 0) >= 0.02


def test_tall_inputs_keep_the_doubt_and_the_bands_thin():
    """The tall case's conditions: test_projection's own (the doubt under the
    cap, holes and both directions present) and the 2 % cap on the bands."""
    doubt, holes, back = _ks_shares(TALL, "f32", T3)
    _, flags, rim, half = _proj_ref(TALL, "f32", T3)
    print(f"tall KS f32: in doubt {_fmt(doubt)}; empty {_fmt(holes)}; direction 1 wins "
          f"{_fmt(back)}; KIP: near a rim {rim.mean():.5f}, near a half {half.mean():.5f}")
    assert max(doubt) <= DOUBT_CAP
    assert max(holes[j] for j in _interior(T3)) > 0.0
    assert 0.0 < min(back) and max(back) < 1.0
    assert (rim | half).mean() <= 0.02 and (flags & HOLE).any()


def test_big_plane_bands_make_the_fixup_pixels_tell():
    """Conditions on KS's 2^24 comparison.  The doubt of the compared targets is
    under the cap; at each time at least 100 of the 512 pixels that take a
    correction are the source a compared, undoubted cell names; and for each of
    those the cost code differs from the one it would get where a failed
    correction evaluates it: (y - 1, cols) for the x >= cols branch, (y + 1, -1)
    for the x < 0 branch, the opposite edge of a neighbouring row."""
    rows, cols = BIG
    lo, hi = _fixups(rows, cols, 0)
    fix = np.concatenate([lo, hi]).astype(np.int64)
    y, x = np.divmod(fix, cols)
    wrong_x = np.where(np.isin(fix, lo), -1, cols)
    wrong_y = np.where(np.isin(fix, lo), y + 1, y - 1)
    assert wrong_y.min() >= 0 and wrong_y.max() < rows
    G = _big_grey()
    uf, vf, ub, vb = _big_flows()
    ty, tx, reach = _big_travel()
    print(f"travel {ty} rows, {tx} columns; reach {reach} rows")
    for j, t in enumerate(KS_BIG_TIMES):
        named, n_doubt, n_compared = [], 0, 0
        for r0, r1, cells, doubt, compared in _big_ks_ref():
            keep = compared[:, None] & ~doubt[j] & (cells[j] != EMPTY)
            named.append(cells[j][keep])
            n_doubt += int(doubt[j][compared].sum())
            n_compared += int(compared.sum()) * cols
        named = np.concatenate(named)
        named = named[np.isin(named & LOW31, fix.astype(np.uint64))]
        wins = np.unique(named & LOW31).size
        print(f"t {t}: {n_compared} targets compared, in doubt {n_doubt / n_compared:.4f}; "
              f"{wins} of {fix.size} correction pixels win a compared, undoubted target")
        assert n_doubt / n_compared <= DOUBT_CAP
        assert wins >= 100
        # each (pixel, direction) that wins: its code there and at the wrong place
        key = np.unique(named)
        order = np.argsort(fix)
        pos = order[np.searchsorted(fix[order], (key & LOW31).astype(np.int64))]
        back = ((key >> np.uint64(31)) & np.uint64(1)) != 0
        for d, (own, other, u, v) in enumerate(((G[0], G[1], uf, vf), (G[1], G[0], ub, vb))):
            sel = pos[back == bool(d)]
            true = key[back == bool(d)] >> np.uint64(32)
            assert np.array_equal(_code_at(own, other, u, v, fix[sel], x[sel], y[sel]), true)
            moved = _code_at(own, other, u, v, fix[sel], wrong_x[sel], wrong_y[sel])
            print(f"t {t} direction {d}: {sel.size} winning correction pixels, least change of "
                  f"the code at the wrong place "
                  f"{np.abs(moved.astype(np.int64) - true.astype(np.int64)).min()}")
            assert np.all(moved != true)


@pytest.mark.parametrize("shape", [(3, 37, 131), (2, 5, 3), (1, 1, 70)],
                         ids=lambda s: "x".join(map(str, s)))
def test_pointwise_projected_reference_equals_the_whole_plane_one(shape):
    """frame_interp_proj_at is frame_interp_proj_np's float64 operations, so bit
    for bit at every pixel: project_np's cells, with and without masks, grey
    frames and BGR frames by channel."""
    from synth_ref import texture
    from test_consistency import _smooth_flows, consistency_np
    batch, rows, cols = shape
    flows = _smooth_flows(*shape)
    every = np.arange(rows * cols)
    for k in range(batch):
        fl = [a[k] for a in flows]
        mf = consistency_np(*fl)[1]
        mb = consistency_np(fl[2], fl[3], fl[0], fl[1])[1]
        bgr = [np.stack([texture(s + 10 * c + k, 0, rows, 0, cols) for c in range(3)],
                        axis=-1).astype(np.uint8) for s in (4000, 5000)]
        grey = [(a[..., 0] * 0.9 + 0.3).astype(np.float32) for a in bgr]
        for t in (0.0, 0.3, 0.5, 1.0):
            cells, _ = project_np(*grey, *fl, t)
            if shape == (3, 37, 131) and 0.0 < t < 1.0:
                assert (cells == EMPTY).any()  # the hole branch is compared too
            for masks in ((mf, mb), (None, None)):
                whole = frame_interp_proj_np(*grey, *fl, t, cells, *masks)
                for got, want in zip(frame_interp_proj_at(*grey, *fl, t, every, cells, *masks),
                                     whole):
                    assert np.array_equal(got, want.ravel())
            out, flags, rim, half = frame_interp_proj_at(*bgr, *fl, t, every, cells, mf, mb)
            for c in range(3):
                whole = frame_interp_proj_np(bgr[0][..., c], bgr[1][..., c], *fl, t, cells, mf, mb)
                for got, want in zip((out[:, c], flags, rim, half), whole):
                    assert np.array_equal(got, want.ravel())


def test_big_cells_make_the_fixup_pixels_tell():
    """Conditions on KIP's 2^24 comparison, as
    test_big_plane_inputs_make_the_fixup_pixels_tell: none of the pixels that
    take a correction lies in an exclusion band; at least 50 of them have both
    targets in the frame, at least 50 one out of it, at least 20 an empty cell;
    the excluded share of S is at most 2 %.  And the cells are what the issue
    asks: one in 16 empty, both directions, sources past 2^24 and in other
    rows."""
    S, fix0 = _big_points()
    cols = BIG[1]
    at = np.searchsorted(S, fix0)
    assert np.array_equal(S[at], fix0)
    _, flags, rim, half = _big_proj_ref("u8")
    out = (flags[at] & 3) != 0
    holes = (flags[at] & HOLE) != 0
    print(f"S: {S.size} pixels, {fix0.size} take a correction: {int((~out).sum())} with both "
          f"targets in-frame, {int(out.sum())} with one out, {int(holes.sum())} on a hole; near a "
          f"rim {rim.mean():.5f}, near a half {half.mean():.5f}")
    assert not rim[at].any() and not half[at].any()
    assert (~out).sum() >= 50 and out.sum() >= 50 and holes.sum() >= 20
    assert (rim | half).mean() <= 0.02
    cell = _big_cells_at(*np.divmod(S, cols))
    full = cell != EMPTY
    src = (cell[full] & LOW31).astype(np.int64)
    back = ((cell[full] >> np.uint64(31)) & np.uint64(1)) != 0
    past = S[full] >= 1 << 24
    print(f"cells at S: empty {1.0 - full.mean():.4f}, direction 1 {back.mean():.3f}; of the "
          f"{int(past.sum())} past 2^24, {int((src[past] >= 1 << 24).sum())} name a source past "
          f"2^24 and {int((src[past] // cols != S[full][past] // cols).sum())} one in another row")
    assert abs(1.0 - full.mean() - 1.0 / 16.0) <= 0.01 and 0.4 <= back.mean() <= 0.6
    assert (src[past] >= 1 << 24).sum() >= 1000
    assert (src[past] // cols != S[full][past] // cols).sum() >= 1000
    assert np.abs(src // cols - S[full] // cols).max() == 3
    assert np.abs(src % cols - S[full] % cols).max() == 3


# ------------------------------------------------------------------ GPU tests
def _check_ks(case, kind, times):
    """KS on the case's batch, twice: the same bytes; every item the bytes of
    its pair's first; every item the reference's cells outside the doubt and
    decodable."""
    import projection
    import torch
    _, batch, pairs, rows, cols = case
    ref, doubt = _cells_ref(case, kind, times)
    args = [_batched(case, a) for a in _frames(case, kind) + _inputs(case)["flows"]]
    cells = projection.project_device(*args, times)
    again = projection.project_device(*args, times)
    torch.cuda.synchronize()
    assert tuple(cells.shape) == (batch, len(times), rows, cols)
    assert torch.equal(cells, again)
    _assert_items_repeat(case, cells)
    item = torch.arange(batch, device="cuda") % pairs
    differ = cells != _cells_cuda(ref)[item]
    outside = differ & ~_cuda(doubt)[item]
    print(f"{case[0]} KS {kind} nt {len(times)}: in doubt {doubt.mean():.4f}, cells that differ "
          f"{float(differ.float().mean()):.5f}, of them outside the doubt {int(outside.sum())}")
    assert doubt.mean() <= DOUBT_CAP
    assert not bool(outside.any())
    assert bool(((cells & 0x7FFFFFFF)[cells != -1] < rows * cols).all())
    assert _decodable(_u64(cells[:pairs]), rows * cols)


def _check_proj_interp(case, kind, times, out, flags, trusted, out8, flags8, cells):
    """test_projected_interp_kernel_against_reference's assertions on the
    case's batch (out [B, nt, H, W])."""
    import torch
    _, _, pairs, _, _ = case
    for t in (out, flags, out8):
        _assert_items_repeat(case, t)
    assert torch.equal(trusted.to(torch.int64), (flags == 0).sum(dim=(2, 3)))
    assert out8.dtype == torch.uint8 and torch.equal(out8, _round_u8(out))
    assert torch.equal(flags8, flags)
    assert torch.equal((flags & HOLE) != 0, cells == -1)  # the cells alone decide
    ref, ref_flags, rim, half = _proj_ref(case, kind, times)
    got, got_flags = out[:pairs].cpu().numpy(), flags[:pairs].cpu().numpy()
    assert got.dtype == np.float32 and got.shape == ref.shape
    d = np.abs(got.astype(np.float64) - ref)[~rim]
    bound = TOL * float(np.abs(ref).max())
    print(f"{case[0]} KIP {kind} nt {len(times)}: worst |out - ref| {d.max():.3e} (bound "
          f"{bound:.3e}), excluded {(rim | half).mean():.5f}, holes "
          f"{np.mean(ref_flags & HOLE != 0):.4f}")
    assert np.all(d <= bound)
    keep = ~(rim | half)
    assert np.array_equal(got_flags[keep], ref_flags[keep])
    assert np.array_equal(got_flags & HOLE, ref_flags & HOLE)
    assert (got_flags & HOLE).any()


def _run_kip(case, frames, times, cells, out_dtype=None):
    import projection
    inp = _inputs(case)
    return projection.frame_interp_device(
        *(_batched(case, a) for a in frames), *(_batched(case, a) for a in inp["flows"]), times,
        cells, mask_f=_batched(case, inp["masks"][0]), mask_b=_batched(case, inp["masks"][1]),
        out_dtype=out_dtype, flags=True, trusted=True)


def _check_kip(case, kind, times):
    import torch
    cells = _batched(case, _cells_ref(case, kind, times)[0].view(np.int64))
    frames = _inputs(case)[kind]
    out, flags, trusted = _run_kip(case, frames, times, cells)
    out8, flags8, _ = _run_kip(case, frames, times, cells, out_dtype=torch.uint8)
    torch.cuda.synchronize()
    _check_proj_interp(case, kind, times, out, flags, trusted, out8, flags8, cells)


@pytest.mark.gpu
@pytest.mark.parametrize("case", KS_CASES, **CASE_IDS)
def test_projection_kernel_over_several_tiles_per_block(hs, case):
    """Hundreds of blocks on the 64-bit minimum, each over two or three tiles."""
    _assert_blocks_take_three_tiles(TILES, KC_TILE, KC_PER_CU)
    _check_ks(TILES, *case)


@pytest.mark.gpu
@pytest.mark.parametrize("case", KIP_CASES, **CASE_IDS)
def test_projected_interp_kernel_over_several_tiles_per_block(hs, case):
    _assert_blocks_take_three_tiles(TILES, KI_TILE, KI_PER_CU)
    _check_kip(TILES, *case)


@pytest.mark.gpu
@pytest.mark.parametrize("wide", [True, False], ids=["wide", "bytes"])
def test_projected_colour_interp_kernel_over_several_tiles_per_block(hs, wide):
    """KIP on BGR frames in both forms of the tap loads: each channel the bits
    of the grey KIP on that channel's plane with the same cells, flags and
    trusted the grey call's.  Channel 1 is the case's u8 frame, whose grey KIP
    test_projected_interp_kernel_over_several_tiles_per_block holds to the
    reference."""
    import projection
    import torch
    _assert_blocks_take_three_tiles(TILES, KIC_TILE, KIC_PER_CU)
    inp = _inputs(TILES)
    cells = _batched(TILES, _cells_ref(TILES, "u8", T3)[0].view(np.int64))
    args = [_batched(TILES, a) for a in inp["bgr"] + inp["flows"]]
    mf, mb = (_batched(TILES, m) for m in inp["masks"])
    was = hs.set_interp_bgr_loads(wide)
    try:
        out, flags, trusted = projection.frame_interp_bgr_device(
            *args, T3, cells, mask_f=mf, mask_b=mb, flags=True, trusted=True)
        torch.cuda.synchronize()
    finally:
        hs.set_interp_bgr_loads(was)
    assert tuple(out.shape) == tuple(cells.shape) + (3,) and out.dtype == torch.float32
    for c in range(3):
        planes = [np.ascontiguousarray(a[..., c]) for a in inp["bgr"]]
        want, want_f, want_c = _run_kip(TILES, planes, T3, cells)
        assert _same_bits(out[..., c].contiguous(), want)
        assert torch.equal(flags, want_f) and torch.equal(trusted, want_c)
    torch.cuda.synchronize()
    assert int(((flags & HOLE) != 0).sum()) > 0


@pytest.mark.gpu
def test_projection_kernel_past_2_24_pixels(hs):
    """KS on 17426 x 1023, u8, t = 0 and 0.3: the reference's cells outside the
    doubt on the compared targets of the two bands; over the whole plane, two
    runs give the same bytes, every cell names a source in the plane within the
    flows' travel of its target, and at t = 0 a direction-0 cell names its own
    pixel (tau = 0) and no cell is empty."""
    import projection
    import torch
    rows, cols = BIG
    ty, tx, _ = _big_travel()
    args = [_cuda(np.ascontiguousarray(a))[None] for a in _big_grey() + _big_flows()]
    try:
        cells = projection.project_device(*args, KS_BIG_TIMES)
        again = projection.project_device(*args, KS_BIG_TIMES)
        torch.cuda.synchronize()
        assert tuple(cells.shape) == (1, len(KS_BIG_TIMES), rows, cols)
        assert torch.equal(cells, again)
        again = None
        c = cells[0]
        full = c != -1
        src = c & 0x7FFFFFFF
        back = (c >> 31) & 1
        assert bool((src[full] < rows * cols).all())
        sy = torch.div(src, cols, rounding_mode="floor")
        sx = src - sy * cols
        qy = torch.arange(rows, device="cuda")[None, :, None]
        qx = torch.arange(cols, device="cuda")[None, None, :]
        off_y, off_x = (sy - qy).abs()[full], (sx - qx).abs()[full]
        print(f"KS whole plane: empty {1.0 - float(full.float().mean()):.4f}, direction 1 wins "
              f"{float(back[full].float().mean()):.3f}, farthest source {int(off_y.max())} rows "
              f"(travel {ty}) and {int(off_x.max())} columns (travel {tx}); "
              f"{int((src[full] >= 1 << 24).sum())} sources past 2^24")
        assert int(off_y.max()) <= ty and int(off_x.max()) <= tx
        own = (qy * cols + qx)[0]
        assert bool(full[0].all())
        stay = back[0] == 0
        assert bool((src[0][stay] == own[stay]).all())
        for r0, r1, ref, doubt, compared in _big_ks_ref():
            got = _u64(c[:, r0:r1])
            differ = got != ref
            keep = compared[None, :, None] & ~doubt
            print(f"KS rows [{r0}, {r1}): {int(compared.sum())} rows compared, in doubt "
                  f"{doubt[:, compared].mean():.4f}, cells that differ "
                  f"{differ[:, compared].mean():.5f}, of them outside the doubt "
                  f"{int((differ & keep).sum())}")
            assert doubt[:, compared].mean() <= DOUBT_CAP
            assert not (differ & keep).any()
    finally:
        del args
        cells = again = c = full = src = back = sy = sx = off_y = off_x = own = stay = None
        torch.cuda.empty_cache()


def _check_big_proj(kind, out, flags, trusted, cells, fn_name):
    """A projected interpolation of the big plane (out [1, 1, H, W(, 3)] f32) at
    S, under the tiles case's bounds; HOLE against the cells over the plane."""
    import torch
    S, fix0 = _big_points()
    ref, ref_flags, rim, half = _big_proj_ref(kind)
    assert int(trusted[0, 0]) == int((flags == 0).sum())
    assert torch.equal((flags & HOLE) != 0, cells == -1)
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
          f"{int(((f[at] & 3) != 0).sum())} with one out, {int(((f[at] & HOLE) != 0).sum())} holes")
    assert (rim | half).mean() <= 0.02
    _assert_only_at(((d > bound) & ~rim) | ((f != ref_flags) & ~(rim | half)), fn_name)
    assert np.array_equal(f & HOLE, ref_flags & HOLE)


@pytest.mark.gpu
def test_projected_interp_kernel_past_2_24_pixels(hs):
    """KIP on 17426 x 1023, u8 frames, f32 out, t = 0.3, both masks, the cells
    of _big_cells_at."""
    import projection
    import torch
    _, _, mf, mb = _big_frames()
    args = [_cuda(np.ascontiguousarray(a))[None] for a in _big_grey() + _big_flows()]
    cells = _cells_cuda(_big_cells())[None, None]
    try:
        out, flags, trusted = projection.frame_interp_device(
            *args, (T_BIG,), cells, mask_f=_cuda(mf)[None], mask_b=_cuda(mb)[None], flags=True,
            trusted=True)
        torch.cuda.synchronize()
        _check_big_proj("u8", out, flags, trusted, cells, "KIP")
    finally:
        del args
        out = flags = trusted = cells = None
        torch.cuda.empty_cache()


@pytest.mark.gpu
@pytest.mark.parametrize("wide", [True, False], ids=["wide", "bytes"])
def test_projected_colour_interp_kernel_past_2_24_pixels(hs, wide):
    """KIP on the BGR frames of the big plane in both forms of the tap loads,
    each channel against the reference of its plane."""
    import projection
    import torch
    B0, B1, mf, mb = _big_frames()
    args = [_cuda(a)[None] for a in (B0, B1) + _big_flows()]
    cells = _cells_cuda(_big_cells())[None, None]
    was = hs.set_interp_bgr_loads(wide)
    try:
        out, flags, trusted = projection.frame_interp_bgr_device(
            *args, (T_BIG,), cells, mask_f=_cuda(mf)[None], mask_b=_cuda(mb)[None], flags=True,
            trusted=True)
        torch.cuda.synchronize()
        _check_big_proj("bgr", out, flags, trusted, cells, "KIP on BGR")
    finally:
        hs.set_interp_bgr_loads(was)
        del args
        out = flags = trusted = cells = None
        torch.cuda.empty_cache()


@pytest.mark.gpu
def test_projection_kernels_on_the_tallest_plane(hs):
    """262140 x 5, the most rows the API accepts, through the tiles case's
    checks (batch 1, f32 frames)."""
    _check_ks(TALL, "f32", T3)
    _check_kip(TALL, "f32", T3)


# The 64 x 4-block kernels added since test_sampling_scale's list, at the
# grid's limit in y: each through its own module's test, at this shape.
@pytest.mark.gpu
def test_downflow_kernel_on_the_tallest_plane(hs):
    """KD: down_np's bits, between guard planes (test_temporal)."""
    _temporal.test_downflow_kernel_equals_numpy_f32_bitwise(hs, TALL_SHAPE)


@pytest.mark.gpu
def test_predict_kernel_on_the_tallest_plane(hs):
    """KP: the sign flip bitwise, the sampled pair the bits of warp_image_device
    on the same planes and within TOL of predict_np (test_temporal)."""
    _temporal.test_predict_kernel(hs, TALL_SHAPE)


@pytest.mark.gpu
@pytest.mark.parametrize("cols", [5, 8], ids=["scalar", "wide"])
def test_bilinear_upflow_kernel_on_the_tallest_plane(hs, cols):
    """KB: upflow_bilinear_np's bits (test_finest).  5 columns take the scalar
    body at any base; 8 columns the scalar body at the base 4 bytes off and the
    wide body on aligned tensors, where lane 0 is its wave's first lane and
    lane 1 the row's last group."""
    _finest.test_kernel_against_the_reference(hs, TALL_SHAPE[:2] + (cols,))


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["u8", "f32"])
def test_pyrdown_kernel_on_the_tallest_plane(hs, kind):
    """K0: the levels of an integer-valued pair are bit-exact (test_pyramid);
    level 1 is 131070 x 3."""
    _pyramid.test_levels_of_integer_pairs_are_bit_exact(hs, TALL_SHAPE[1:], kind)


@pytest.mark.gpu
def test_upflow_kernel_on_the_tallest_plane(hs):
    """KU: the doubled nearest projection, exactly (test_pyramid)."""
    rows, cols = TALL_SHAPE[1:]
    _pyramid.test_upflow_is_the_doubled_nearest_projection(hs, (rows, cols),
                                                           ((rows + 1) // 2, (cols + 1) // 2))
