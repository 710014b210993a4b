"""KIY on 16-bit chroma where a single pair's blocks stride: one luma plane whose
chroma plane exceeds the grid's cap -- blocks per CU x CUs x 512 samples, both
figures from the library and the device -- with an odd chroma width, as
test_yuv_scale builds it.  Against the public pieces on float32 planes on the
GPU, rounded to U16, bit for bit; no CPU reference at this size."""
import numpy as np
import pytest

import yuv  # noqa: F401  (the module under test)
from test_yuv_scale import _plane_past_the_cap

I420, NV12 = 1, 2


@pytest.mark.gpu
@pytest.mark.parametrize("layout", [I420, NV12], ids=["i420", "nv12"])
def test_blocks_stride_over_the_tiles_of_a_large_16_bit_plane(hs, layout):
    import temporal
    import torch
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    cap = yuv.blocks_per_cu() * cus * yuv.CHROMA_TILE
    rows, cols = _plane_past_the_cap(cap)
    rc, cc = rows // 2, cols // 2
    assert rc * cc > cap + yuv.CHROMA_TILE and (rc * cc) % yuv.CHROMA_TILE != 0 and cc % 2 == 1
    g = torch.Generator(device="cuda").manual_seed(16)
    # smooth flows of a few px with a slow drift, so taps cross rows and tiles
    yy = torch.arange(rows, device="cuda", dtype=torch.float32)[:, None]
    xx = torch.arange(cols, device="cuda", dtype=torch.float32)[None, :]
    uf = (0.3 * torch.sin(xx / 97.0) + 0.2 * torch.cos(yy / 61.0)).expand(rows, cols)
    vf = (0.25 * torch.cos(xx / 83.0) - 0.15 * torch.sin(yy / 45.0)).expand(rows, cols)
    noise = 0.02 * torch.randn((2, rows, cols), device="cuda", generator=g)
    flows = [uf[None].contiguous(), vf[None].contiguous(), (-uf + noise[0])[None].contiguous(),
             (-vf + noise[1])[None].contiguous()]
    # sample values over the whole of 0 .. 65535, exact in float32
    f0, f1 = (torch.floor(torch.rand((1, 2, rc, cc), device="cuda", generator=g) * 65536.0)
              .clamp_(0.0, 65535.0) for _ in range(2))
    f0[0, :, 0, :5] = torch.tensor([0.0, 255.0, 256.0, 32768.0, 65535.0], device="cuda")
    times = (0.25, 0.5)
    df = temporal.downflow_device(*flows[:2]) + temporal.downflow_device(*flows[2:])
    planes = [hs.frame_interp_device(f0[:, ch].contiguous(), f1[:, ch].contiguous(), *df, times,
                                     out_dtype=torch.float32)[0] for ch in range(2)]
    want = torch.stack(planes, dim=2)  # [1, nt, 2, rc, cc]
    want = torch.floor(want + np.float32(0.5))
    want = torch.where(torch.isnan(want), torch.zeros_like(want), want).clamp_(0.0, 65535.0)
    # the 16 bits of a sample through int32 -> int16 on the host (wraps exactly)
    c0, c1 = (torch.from_numpy(f.cpu().numpy().astype(np.int64).astype(np.uint16)).cuda()
              for f in (f0, f1))
    if layout == NV12:
        want = want.permute(0, 1, 3, 4, 2).contiguous()
        c0, c1 = (torch.from_numpy(np.ascontiguousarray(c.cpu().numpy().transpose(0, 2, 3, 1)))
                  .cuda() for c in (c0, c1))
    got = yuv.chroma_interp_device(c0, c1, *flows, times, layout, out_dtype=torch.uint16)
    torch.cuda.synchronize()
    got_np = got.view(torch.int16).cpu().numpy().view(np.uint16)
    want_np = want.cpu().numpy().astype(np.int64).astype(np.uint16)
    assert got_np.shape == want_np.shape and np.array_equal(got_np, want_np)
    # the result is not trivial: the times differ, and the values span the range
    assert not np.array_equal(got_np[:, 0], got_np[:, 1])
    assert int(got_np.max()) > 60000
    assert float(np.abs(got_np.astype(np.float64) - 32767.5).mean()) > 5000
