"""KSD and KIYP (hs_cells_down_kernel, hs_chroma_interp_proj_kernel) on big
planes, against the public pieces on the GPU, bit for bit; no CPU reference at
these sizes.

1282 x 2050 luma: the chroma plane of 641 x 1025 samples exceeds KIYP's grid cap
-- blocks per CU x CUs x 512 samples -- so a single pair's blocks stride, the
chroma width is odd and the last tile is not full.
4098 x 4100 luma at one time: the plane holds more than 2^24 pixels, so a
winner's source index no longer fits a float and the row / column split has to
stay exact (pixel_xy)."""
import pytest

import yuv  # noqa: F401  (the module under test)
from test_interp import _same_bits

I420, NV12 = 1, 2


def _scene(rows, cols, seed):
    """(y0, y1, c0 I420, c1 I420, flows) of one pair on the GPU: random frames,
    smooth flows of a few px with a slow drift and a little noise, so targets
    and taps cross rows and tiles and many candidates tie in cost."""
    import torch
    g = torch.Generator(device="cuda").manual_seed(seed)
    yy = torch.arange(rows, device="cuda", dtype=torch.float32)[:, None]
    xx = torch.arange(cols, device="cuda", dtype=torch.float32)[None, :]
    uf = (0.3 * torch.sin(xx / 97.0) + 0.2 * torch.cos(yy / 61.0)).expand(rows, cols)
    vf = (0.25 * torch.cos(xx / 83.0) - 0.15 * torch.sin(yy / 45.0)).expand(rows, cols)
    noise = 0.02 * torch.randn((2, rows, cols), device="cuda", generator=g)
    flows = [uf[None].contiguous(), vf[None].contiguous(), (-uf + noise[0])[None].contiguous(),
             (-vf + noise[1])[None].contiguous()]
    y0, y1 = ((torch.rand((1, rows, cols), device="cuda", generator=g) * 256).to(torch.uint8)
              for _ in range(2))
    c0, c1 = ((torch.rand((1, 2, rows // 2, cols // 2), device="cuda", generator=g) * 256)
              .to(torch.uint8) for _ in range(2))
    return y0, y1, c0, c1, flows


def _pieces(c0, c1, flows, cells, times):
    import projection
    import temporal
    import torch
    df = temporal.downflow_device(*flows[:2]) + temporal.downflow_device(*flows[2:])
    cc = yuv.cells_down_device(cells)
    planes = [projection.frame_interp_device(c0[:, ch].contiguous(), c1[:, ch].contiguous(), *df,
                                             times, cc, out_dtype=torch.uint8)[0]
              for ch in range(2)]
    return torch.stack(planes, dim=2), cc  # [1, nt, 2, rc, cc]


def _check(rows, cols, times, layout, seed):
    import projection
    import torch
    y0, y1, c0, c1, flows = _scene(rows, cols, seed)
    cells = projection.project_device(y0, y1, *flows, times)
    # planted holes: every 7th row of blocks and a scatter of single cells
    cells[:, :, 0:rows:14] = -1
    cells[:, :, 1:rows:14] = -1
    cells[:, :, 5::11, 3::13] = -1
    want, cc = _pieces(c0, c1, flows, cells, times)
    plain = yuv.chroma_interp_device(c0, c1, *flows, times, I420, out_dtype=torch.uint8)
    hole = (cc == -1)[:, :, None].expand(want.shape)
    assert hole.any() and not hole.all()
    assert torch.equal(want[hole], plain[hole]) and not torch.equal(want, plain)
    # the winners reach the end of the plane
    index = cc[cc != -1] & 0x7FFFFFFF
    assert int(index.max()) >= (rows // 2) * (cols // 2) - cols
    del plain, hole, index
    if layout == NV12:
        want = want.permute(0, 1, 3, 4, 2).contiguous()
        c0, c1 = (c.permute(0, 2, 3, 1).contiguous() for c in (c0, c1))
    got = yuv.chroma_interp_proj_device(c0, c1, *flows, times, cells, layout,
                                        out_dtype=torch.uint8)
    torch.cuda.synchronize()
    assert _same_bits(got, want)
    return cells


@pytest.mark.gpu
@pytest.mark.parametrize("layout", [I420, NV12], ids=["i420", "nv12"])
def test_blocks_stride_over_the_tiles_of_a_large_plane(hs, layout):
    import torch
    rows, cols = 1282, 2050
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    cap = yuv.proj_blocks_per_cu() * cus * yuv.CHROMA_TILE
    plane = (rows // 2) * (cols // 2)
    assert plane > cap + yuv.CHROMA_TILE and plane % yuv.CHROMA_TILE != 0
    _check(rows, cols, (0.25, 0.5), layout, 5)


@pytest.mark.gpu
def test_a_luma_plane_past_2_to_the_24(hs):
    rows, cols = 4098, 4100
    assert rows * cols > 1 << 24
    cells = _check(rows, cols, (0.4,), I420, 7)
    # KS's own indices beyond 2^24 are there to be split
    assert int((cells[cells != -1] & 0x7FFFFFFF).max()) > 1 << 24
