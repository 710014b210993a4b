"""KIY (hs_chroma_interp_kernel) where a single pair's blocks stride: one luma
plane whose chroma plane exceeds the grid's cap -- blocks per CU x CUs x 512
samples, both figures from the library and the device -- so that every block
takes more than one tile.  KIY against the public pieces on the GPU, bit for
bit; no CPU reference at this size."""
import numpy as np
import pytest

import yuv  # noqa: F401  (the module under test)
from test_interp import _same_bits

I420, NV12 = 1, 2


def _plane_past_the_cap(cap):
    """Luma (rows, cols), both even, whose chroma plane is the smallest of 1025
    columns with more than `cap` samples plus two tiles: an odd chroma width,
    a last tile that is not full."""
    cc = 1025
    rc = (cap + 2 * 512) // cc + 1
    return 2 * rc, 2 * cc


@pytest.mark.gpu
@pytest.mark.parametrize("layout", [I420, NV12], ids=["i420", "nv12"])
def test_blocks_stride_over_the_tiles_of_a_large_plane(hs, layout):
    import temporal
    import torch
    import yuv
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    cap = yuv.blocks_per_cu() * cus * yuv.CHROMA_TILE
    rows, cols = _plane_past_the_cap(cap)
    rc, cc = rows // 2, cols // 2
    assert rc * cc > cap + yuv.CHROMA_TILE and (rc * cc) % yuv.CHROMA_TILE != 0
    g = torch.Generator(device="cuda").manual_seed(5)
    # smooth flows of a few px with a slow drift, so taps cross rows and tiles
    yy = torch.arange(rows, device="cuda", dtype=torch.float32)[:, None]
    xx = torch.arange(cols, device="cuda", dtype=torch.float32)[None, :]
    uf = (0.3 * torch.sin(xx / 97.0) + 0.2 * torch.cos(yy / 61.0)).expand(rows, cols)
    vf = (0.25 * torch.cos(xx / 83.0) - 0.15 * torch.sin(yy / 45.0)).expand(rows, cols)
    noise = 0.02 * torch.randn((2, rows, cols), device="cuda", generator=g)
    flows = [uf[None].contiguous(), vf[None].contiguous(), (-uf + noise[0])[None].contiguous(),
             (-vf + noise[1])[None].contiguous()]
    c0, c1 = ((torch.rand((1, 2, rc, cc), device="cuda", generator=g) * 256).to(torch.uint8)
              for _ in range(2))
    times = (0.25, 0.5)
    df = temporal.downflow_device(*flows[:2]) + temporal.downflow_device(*flows[2:])
    planes = [hs.frame_interp_device(c0[:, ch].contiguous(), c1[:, ch].contiguous(), *df, times,
                                     out_dtype=torch.uint8)[0] for ch in range(2)]
    want = torch.stack(planes, dim=2)  # [1, nt, 2, rc, cc]
    if layout == NV12:
        want = want.permute(0, 1, 3, 4, 2).contiguous()
        c0, c1 = (c.permute(0, 2, 3, 1).contiguous() for c in (c0, c1))
    got = yuv.chroma_interp_device(c0, c1, *flows, times, layout, out_dtype=torch.uint8)
    torch.cuda.synchronize()
    assert _same_bits(got, want)
    # the result is not trivial: the frames differ and so do the times
    assert not torch.equal(got[:, 0], got[:, 1])
    assert float((got[:, 0].float() - np.float32(127.5)).abs().mean()) > 10
