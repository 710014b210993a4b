"""KF (hsflow_frame_fallback_device) at the two sizes its small tests do not
reach: a batch wide enough that a block takes several tiles of its pair, and a
plane past 2^24 pixels, where a float could no longer hold a pixel index.
fallback_np of test_fallback.py is the reference, bit for bit."""
import numpy as np
import pytest

from test_fallback import BLEND, FLAG, MIN_SHARE, NEAREST, _counts, fallback_np
from test_interp import _cuda


def _noise(seed, shape):
    return np.random.default_rng(seed).integers(0, 256, shape, dtype=np.uint8)


@pytest.mark.gpu
def test_a_block_takes_several_tiles(hs):
    """64 pairs of 211 x 397, alternating verdicts: the grid's cap leaves a few
    blocks per pair, each striding over the pair's 164 tiles.  Failed pairs
    equal the reference, the others keep their bytes."""
    import fallback
    import torch
    batch, rows, cols = 64, 211, 397
    I0, I1 = _noise(1, (batch, rows, cols)), _noise(2, (batch, rows, cols))
    verdicts = [b % 2 for b in range(batch)]
    cf, cb = _counts(rows, cols, verdicts)
    times = (1 / 3, 0.5)
    out = torch.full((batch, 2, rows, cols), 9, dtype=torch.uint8, device="cuda")
    flags = torch.full(out.shape, 1, dtype=torch.uint8, device="cuda")
    trusted = torch.full((batch, 2), 5, dtype=torch.int32, device="cuda")
    _, _, _, cut = fallback.frame_fallback_device(_cuda(I0), _cuda(I1), _cuda(cf), _cuda(cb),
                                                  fallback.Fallback(BLEND), times, out,
                                                  flags=flags, trusted=trusted)
    torch.cuda.synchronize()
    want, want_cut = fallback_np(I0, I1, cf, cb, BLEND, MIN_SHARE, times, np.uint8)
    assert cut.tolist() == verdicts == want_cut.tolist()
    got, fl = out.cpu().numpy(), flags.cpu().numpy()
    assert np.array_equal(got[1::2], want[1::2]) and (fl[1::2] == FLAG).all()
    assert (got[0::2] == 9).all() and (fl[0::2] == 1).all()
    assert trusted.cpu().numpy().tolist() == [[0, 0] if v else [5, 5] for v in verdicts]


@pytest.mark.gpu
def test_a_plane_past_2_to_24_pixels(hs):
    """17426 x 1023 (17.8 Mpx), u8 in and out, one time, failed: the first and
    last rows, the rows around pixel 2^24 and a checksum of the whole plane."""
    import fallback
    import torch
    rows, cols = 17426, 1023
    assert rows * cols > 1 << 24
    I0, I1 = _noise(3, (1, rows, cols)), _noise(4, (1, rows, cols))
    cf, cb = _counts(rows, cols, [1])
    out, flags, trusted, cut = fallback.frame_fallback_device(
        _cuda(I0), _cuda(I1), _cuda(cf), _cuda(cb), fallback.Fallback(BLEND), (0.3,),
        torch.zeros((1, 1, rows, cols), dtype=torch.uint8, device="cuda"), flags=True,
        trusted=True)
    near = fallback.frame_fallback_device(
        _cuda(I0), _cuda(I1), _cuda(cf), _cuda(cb), fallback.Fallback(NEAREST), (0.7,),
        torch.zeros((1, 1, rows, cols), dtype=torch.uint8, device="cuda"))[0]
    torch.cuda.synchronize()
    want = fallback_np(I0, I1, cf, cb, BLEND, MIN_SHARE, (0.3,), np.uint8)[0]
    got, fl = out.cpu().numpy()[0, 0], flags.cpu().numpy()[0, 0]
    mid = (1 << 24) // cols
    for band in (slice(0, 2), slice(mid - 2, mid + 3), slice(rows - 2, rows)):
        assert np.array_equal(got[band], want[0, 0][band]), band
        assert (fl[band] == FLAG).all()
    weights = np.arange(cols, dtype=np.int64) % 251 + 1
    assert int((got.astype(np.int64) * weights).sum()) == \
        int((want[0, 0].astype(np.int64) * weights).sum())
    assert int(fl.astype(np.int64).sum()) == FLAG * rows * cols
    assert cut.tolist() == [1] and trusted.tolist() == [[0]]
    assert np.array_equal(near.cpu().numpy()[0, 0], I1[0])
