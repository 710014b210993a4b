"""K1's packed gradient word and integrality flag against the oracle.

The word is (csrc/hsflow_device.h pack_grad) Ix in bits 0..10, Iy in bits
11..21 and It in bits 22..30, two's complement; pack_np restates it in numpy
from oracle.gradients.  The packed plane and the flag words are read out of
the workspace (carve(): six planes of n * 4 bytes, each rounded up to 256
bytes, then the flags -- the layout test_first_pass._planes documents).

The extremes pair drives every field to its limits (|Ix|, |Iy| = 1020,
|It| = 255), where a mask one bit short, a missing sign extension or a wrong
decode constant changes the result; the Jacobi kernels' decodes (unpack_grad
in K2w, K2, K2g; unpack_grad_pair in K4) are then run on it against the
oracle.  The flag's rule -- integer, in [0, 255], both frames, per pair -- is
tested value by value.  Workspaces are prefilled with 0xA5 bytes, outputs
with NaN."""
import contextlib

import numpy as np
import pytest

import oracle
from conftest import norm_rel_err

TOL = 1e-4
DTYPES = {"u8": np.uint8, "f16": np.float16, "f32": np.float32, "f64": np.float64}


def pack_np(gx, gy, gt):
    gx, gy, gt = (np.asarray(g).astype(np.int64) for g in (gx, gy, gt))
    return ((gx & 0x7FF) | ((gy & 0x7FF) << 11) | ((gt & 0x1FF) << 22)).astype(np.uint32)


def unpack_np(p):
    """The sign-extending decode of the three fields."""
    p = np.asarray(p).astype(np.int64)

    def field(shift, bits):
        f = (p >> shift) & ((1 << bits) - 1)
        return f - ((f >> (bits - 1)) << bits)

    return field(0, 11), field(11, 11), field(22, 9)


def extremes_pair(odd=False):
    """24x40: rows 0..11 of I0 vertical bars two columns wide (0, 0, 255, 255,
    ...), rows 12..23 horizontal bars two rows high; I1 = I0 in columns 0..19
    and 255 - I0 in columns 20..39.  odd: its 23x39 crop."""
    I0 = np.zeros((24, 40), np.uint8)
    I0[:12] = np.where((np.arange(40) // 2) % 2 == 1, 255, 0)[None, :]
    I0[12:] = np.where((np.arange(12) // 2) % 2 == 1, 255, 0)[:, None]
    I1 = I0.copy()
    I1[:, 20:] = 255 - I0[:, 20:]
    if odd:
        I0, I1 = I0[:23, :39], I1[:23, :39]
    return np.ascontiguousarray(I0), np.ascontiguousarray(I1)


def _random_pair(rows, cols, batch=None, seed=23):
    rng = np.random.default_rng(seed + 1000 * rows + cols)
    shape = (batch, rows, cols) if batch else (rows, cols)
    return (rng.integers(0, 256, shape).astype(np.uint8),
            rng.integers(0, 256, shape).astype(np.uint8))


def _expected_words(I0, I1):
    """pack_np of the oracle's gradients, pair by pair, flattened."""
    a = np.asarray(I0, np.float64).reshape((-1,) + I0.shape[-2:])
    b = np.asarray(I1, np.float64).reshape((-1,) + I1.shape[-2:])
    return np.concatenate([pack_np(*oracle.gradients(x, y)).ravel() for x, y in zip(a, b)])


# ------------------------------------------------------------------ CPU tests
def test_pack_restatement_round_trips_over_the_field_ranges():
    """Each field over its whole range with the others at their limits, 0
    and +-1: the decode returns the inputs, and the word fits in 31 bits."""
    full = {"x": np.arange(-1020, 1021), "y": np.arange(-1020, 1021), "t": np.arange(-255, 256)}
    edge = {"x": np.array([-1020, -1, 0, 1, 1020]), "y": np.array([-1020, -1, 0, 1, 1020]),
            "t": np.array([-255, -1, 0, 1, 255])}
    for swept in "xyt":
        axes = [full[k] if k == swept else edge[k] for k in "xyt"]
        gx, gy, gt = np.meshgrid(*axes, indexing="ij")
        words = pack_np(gx, gy, gt)
        assert words.dtype == np.uint32 and int(words.max()) < 1 << 31
        dx, dy, dt = unpack_np(words)
        assert np.array_equal(dx, gx) and np.array_equal(dy, gy) and np.array_equal(dt, gt)


@pytest.mark.parametrize("odd", [False, True])
def test_extremes_pair_reaches_every_field_limit(odd):
    gx, gy, gt = oracle.gradients(*extremes_pair(odd))
    assert (gx.min(), gx.max()) == (-1020, 1020)
    assert (gy.min(), gy.max()) == (-1020, 1020)
    assert (gt.min(), gt.max()) == (-255, 255)
    dx, dy, dt = unpack_np(pack_np(gx, gy, gt))
    assert np.array_equal(dx, gx) and np.array_equal(dy, gy) and np.array_equal(dt, gt)


# ------------------------------------------------------------------ GPU tests
def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _dims(shape):
    return shape[-2], shape[-1], int(np.prod(shape[:-2], dtype=np.int64))


def _workspace(hs, shape):
    import torch
    return torch.full((hs.workspace_bytes(*_dims(shape)),), 0xA5, dtype=torch.uint8,
                      device="cuda")


def _planes(ws, shape):
    """(packed plane, flags) of a workspace as numpy uint32."""
    import torch
    rows, cols, batch = _dims(shape)
    n = batch * rows * cols
    plane = (n * 4 + 255) // 256 * 256
    torch.cuda.synchronize()
    words = ws[:n * 4].view(torch.int32).cpu().numpy().view(np.uint32)
    flags = ws[6 * plane:6 * plane + 4 * batch].view(torch.int32).cpu().numpy().view(np.uint32)
    return words, flags


@contextlib.contextmanager
def _kernel(hs, k, strip_rows=0):
    hs.set_jacobi_kernel(k)
    hs.set_strip_rows(strip_rows)
    try:
        yield
    finally:
        hs.set_jacobi_kernel(0)
        hs.set_strip_rows(0)


def _pairs(name):
    """The pairs of the packed-word tests by name, as uint8."""
    if name == "extremes":
        return extremes_pair()
    if name == "extremes-odd":
        return extremes_pair(True)
    dims = tuple(int(x) for x in name.split("x"))
    return _random_pair(*dims[-2:], batch=dims[0] if len(dims) == 3 else None)


K1_PAIRS = ["1x1", "1x7", "7x1", "2x2", "3x130", "33x257", "extremes", "extremes-odd",
            "3x17x33"]


@pytest.mark.gpu
@pytest.mark.parametrize("kind", list(DTYPES))
@pytest.mark.parametrize("name", K1_PAIRS)
def test_packed_word_from_k1_matches_the_oracle(hs, name, kind):
    """gradients_device: every word of the packed plane, and the flags 0."""
    I0, I1 = _pairs(name)
    ws = _workspace(hs, I0.shape)
    hs.gradients_device(_dev(I0.astype(DTYPES[kind])), _dev(I1.astype(DTYPES[kind])), ws)
    words, flags = _planes(ws, I0.shape)
    assert np.array_equal(words, _expected_words(I0, I1))
    assert not flags.any()


# test_first_pass.SHAPES (rows, cols, K4 segment rows), where that module
# proves the first pass fuses, and the extremes pairs
FUSED_PAIRS = [("1x1", 0), ("1x7", 0), ("7x1", 0), ("2x2", 0), ("3x130", 0), ("97x209", 0),
               ("90x232", 48), ("100x140", 84), ("extremes", 0), ("extremes-odd", 0),
               ("3x17x33", 0)]


@pytest.mark.gpu
@pytest.mark.parametrize("kind", list(DTYPES))
@pytest.mark.parametrize("name,strip_rows", FUSED_PAIRS)
def test_packed_word_from_the_fused_first_pass_matches_the_oracle(hs, name, strip_rows, kind):
    """A cold K4 solve with the fusion on writes the packed plane from its
    first pass (f64 frames: K1 in front of it); one chain for a single pair,
    two for the batch."""
    import torch
    I0, I1 = _pairs(name)
    ws = _workspace(hs, I0.shape)
    u = torch.full(I0.shape, float("nan"), device="cuda")
    v = torch.full(I0.shape, float("nan"), device="cuda")
    before = hs.first_pass_launches()
    with _kernel(hs, 4, strip_rows), hs.first_pass_fusion_as(True):
        assert hs.jacobi_kernel_name(*_dims(I0.shape), 5) == "hs_jacobi_strip_kernel"
        hs.flow_device(_dev(I0.astype(DTYPES[kind])), _dev(I1.astype(DTYPES[kind])), 5, 6, 1.0,
                       u, v, ws)
    words, flags = _planes(ws, I0.shape)
    chains = min(2, _dims(I0.shape)[2])
    assert hs.first_pass_launches() - before == (0 if kind == "f64" else chains)
    assert np.array_equal(words, _expected_words(I0, I1))
    assert not flags.any()
    assert bool(torch.isfinite(u).all()) and bool(torch.isfinite(v).all())


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["f16", "f32"])
@pytest.mark.parametrize("name", ["3x130", "33x257", "extremes-odd", "3x17x33"])
def test_dyadic_non_integral_frames_give_exact_f32_gradients(hs, name, kind):
    """Integers + 0.25: every fp32 operation of K1 is exact on them, so the
    f32 planes equal the oracle's bit for bit, and the pairs are flagged."""
    import torch
    I0, I1 = _pairs(name)
    a, b = (I0 + 0.25).astype(DTYPES[kind]), (I1 + 0.25).astype(DTYPES[kind])
    assert np.array_equal(a.astype(np.float64), I0 + 0.25)
    ws = _workspace(hs, I0.shape)
    g = [torch.full(I0.shape, float("nan"), device="cuda") for _ in range(3)]
    hs.gradients_device(_dev(a), _dev(b), ws, *g)
    _, flags = _planes(ws, I0.shape)
    assert flags.tolist() == [1] * _dims(I0.shape)[2]
    A = a.astype(np.float64).reshape((-1,) + a.shape[-2:])
    B = b.astype(np.float64).reshape((-1,) + b.shape[-2:])
    ref = [np.stack(p) for p in zip(*[oracle.gradients(x, y) for x, y in zip(A, B)])]
    for got, want in zip(g, ref):
        got = got.cpu().numpy().reshape(want.shape)
        assert np.array_equal(got.view(np.int32), want.astype(np.float32).view(np.int32))


# ---------------------------------------------- extremes through the decodes
def _decode_runs(w):
    """(kernel setting, fusion) runs of window w: automatic and K2 everywhere
    (K2w, the workgroup kernel or K2g by window), K4 fused and unfused where
    it is built."""
    runs = [(0, True), (2, True)]
    if w in (3, 5):
        runs += [(4, True), (4, False)]
    return runs


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["u8", "f32"])
@pytest.mark.parametrize("odd", [False, True])
@pytest.mark.parametrize("w", [1, 2, 3, 5, 7, 11])
def test_extremes_through_every_jacobi_decode(hs, w, odd, kind):
    """Nine iterations on the extremes pair through every kernel of the
    window: each within 1e-4 of oracle.flow, all of them the same bits."""
    import torch
    I0, I1 = extremes_pair(odd)
    rows, cols = I0.shape
    uo, vo = oracle.flow(I0, I1, w, 9, 1.0)
    assert np.isfinite(uo).all() and np.isfinite(vo).all()
    t0, t1 = _dev(I0.astype(DTYPES[kind])), _dev(I1.astype(DTYPES[kind]))
    names, res = [], []
    for k, fuse in _decode_runs(w):
        ws = _workspace(hs, I0.shape)
        u = torch.full(I0.shape, float("nan"), device="cuda")
        v = torch.full(I0.shape, float("nan"), device="cuda")
        with _kernel(hs, k), hs.first_pass_fusion_as(fuse):
            names.append(hs.jacobi_kernel_name(rows, cols, 1, w))
            hs.flow_device(t0, t1, w, 9, 1.0, u, v, ws)
        _, flags = _planes(ws, I0.shape)
        assert flags.tolist() == [0]
        res.append((u.cpu().numpy(), v.cpu().numpy()))
        for got, ref, name in ((res[-1][0], uo, "u"), (res[-1][1], vo, "v")):
            err = norm_rel_err(got, ref)
            print(f"extremes w{w} {kind} {names[-1]} fuse {fuse} {name}: "
                  f"norm_rel_err {err:.3e} (bound {TOL:.0e})")
            assert err <= TOL
    want = {1: "hs_jacobi_kernel", 2: "hs_jacobi_kernel", 11: "hs_jacobi_generic_kernel"}
    assert names[1] == want.get(w, "hs_jacobi_wg_kernel")
    if w in (3, 5):
        assert names[2] == names[3] == "hs_jacobi_strip_kernel"
    for u, v in res[1:]:
        assert np.array_equal(u.view(np.int32), res[0][0].view(np.int32))
        assert np.array_equal(v.view(np.int32), res[0][1].view(np.int32))


# ------------------------------------------------------------ the flag's rule
F32 = np.float32
FLAG_CASES = (
    [("f32", F32(0), 0), ("f32", F32(255), 0), ("f32", F32(-0.0), 0), ("f32", F32(256), 1),
     ("f32", F32(-1), 1), ("f32", F32(0.5), 1), ("f32", np.nextafter(F32(255), F32(0)), 1),
     ("f32", F32(np.nan), 1), ("f32", F32(np.inf), 1)] +
    [("f16", np.float16(255), 0), ("f16", np.float16(256), 1), ("f16", np.float16(0.5), 1)] +
    [("f64", 255.0, 0), ("f64", 255.0 + 1e-12, 1), ("f64", 0.5, 1)])


def _flag_after_k1(hs, a, b):
    ws = _workspace(hs, a.shape)
    hs.gradients_device(_dev(a), _dev(b), ws)
    return _planes(ws, a.shape)[1].tolist()


@pytest.mark.gpu
@pytest.mark.parametrize("frame", [0, 1])
@pytest.mark.parametrize("at", [(0, 0), (5, 8)])
@pytest.mark.parametrize("kind,value,flag", FLAG_CASES,
                         ids=[f"{k}-{float(x)!r}" for k, x, _ in FLAG_CASES])
def test_flag_rule_value_by_value(hs, kind, value, flag, at, frame):
    """One pixel of I0 or of I1 of a 6x9 integer pair replaced: its first
    pixel, or its last one (the last column of an odd width, which the
    column-pair thread handles in its single-column branch)."""
    pair = [x.astype(DTYPES[kind]) for x in _random_pair(6, 9)]
    assert _flag_after_k1(hs, *pair) == [0]
    pair[frame][at] = value
    assert pair[frame][at] == value or np.isnan(value)
    assert np.signbit(pair[frame][at]) == np.signbit(value)
    assert _flag_after_k1(hs, *pair) == [flag]
    if np.isfinite(value):
        assert oracle.integer_pair(*pair) == (flag == 0)


@pytest.mark.gpu
def test_flag_of_8_bit_frames_overwrites_stale_words(hs):
    """u8 frames are always packed: K1 stores 0 over the workspace's stale
    0xA5A5A5A5, for every pair of a batch."""
    for shape in ((6, 9), (3, 6, 9)):
        I0, I1 = _random_pair(*shape[-2:], batch=shape[0] if len(shape) == 3 else None)
        I0.reshape(-1)[-1] = 255
        assert _flag_after_k1(hs, I0, I1) == [0] * _dims(I0.shape)[2]


@pytest.mark.gpu
@pytest.mark.parametrize("kind,value", [("f32", F32(0.5)), ("f32", F32(256)),
                                        ("f16", np.float16(0.5)), ("f64", 255.0 + 1e-12)])
@pytest.mark.parametrize("frame", [0, 1])
def test_flag_is_per_pair(hs, kind, value, frame):
    """A batch of three with only the middle pair touched: [0, 1, 0]."""
    pair = [x.astype(DTYPES[kind]) for x in _random_pair(6, 9, batch=3)]
    pair[frame][1, 5, 8] = value
    assert _flag_after_k1(hs, *pair) == [0, 1, 0]
    assert [oracle.integer_pair(pair[0][i], pair[1][i]) for i in range(3)] == [True, False, True]
