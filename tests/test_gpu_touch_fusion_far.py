"""GPU: touch fusion past element 2^29 of `acc` and `weight`, the 2 GiB byte line of a float32 array.

TouchVolume takes up to 1024^3 voxels; the largest volume of test_gpu_touch_fusion.py has 106 x 104 x 102.  te_view forms the cell
count and cell / (cx * cy) in int, touch_integrate splits its block id in int, and both address acc and weight with products of
three ints.  Here one volume of 1024 x 1024 x 514 voxels (2.16 GB per array; z layer 512 begins at element 2^29 exactly) is
integrated into and extracted from on both sides of that line, against the numpy twin (tests/touch_fusion_ref.py) on small volumes
whose origin is shifted to the same place.  The voxel is 2^-4 mm and the origin lies on that lattice, so origin + h * i is exact and
the shifted small volume has the far volume's voxel coordinates to the bit.  Every comparison is on bits.

The module allocates 4.3 GB and must not run under engine_state.poison (a fill of every torch.empty would not hurt it, but the
volume's own zeros are what it starts from).  Measured on an MI355X: the module takes 3.1 s -- 0.2 s to allocate the volume, 1.0 s
for the integration test (most of it the twin's three slabs on the host), 0.03 s for each extraction test.
"""
import numpy as np
import pytest
import torch

import mesh_depth_ref as R
import touch_fusion_ref as T

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
DIMS = (1024, 1024, 514)                 # nx, ny, nz
H = 2.0 ** -4
ORIGIN = (-32.0, -32.0, -16.0)           # on the lattice of H
TAU = 4 * H
LINE = 1 << 29                           # the first element past 2 GiB
SIZE, HEIGHT_MM, G = (24, 31), 12.0, 4.4
SLABS = (0, 510, 512)                    # first layer of each compared pair of z layers


@pytest.fixture(scope="module")
def volume():
    from gelslim_depth_amd.touch_fusion import TouchVolume
    assert DIMS[0] * DIMS[1] * 512 == LINE and DIMS[0] * DIMS[1] * DIMS[2] > LINE
    vol = TouchVolume(ORIGIN, H, DIMS, TAU, device=DEV)
    yield vol
    del vol.acc, vol.weight
    torch.cuda.empty_cache()


def touches():
    """(depth (2, 2, 24, 31) fp32, widths (2,), rows (2, 12)): one image of a sphere of radius 3 mm (mesh_depth_ref.raster_ref at
    delta = 0, on the host) under two maps u = y - y0, v = z - z0, q = x - x0.  The image is 15.5 mm wide along v = 248 layers: the
    first touch is centred on layer 1 and reaches layers 0 .. 124, the second on layer 511.5 and reaches layers 388 .. 513."""
    lo, _ = R.raster_ref(R.sphere(2, 3.0, (0.0, 0.0, 0.0)), 1.0, "+y+z", (0.0, 0.0, 0.0), G, SIZE, HEIGHT_MM, delta=0.0)
    depth = np.stack([lo, lo]).astype(np.float32) + np.float32(0.0)

    def row(y0, z0, x0):
        return [0, 1, 0, -y0, 0, 0, 1, -z0, 1, 0, 0, -x0]
    rows = np.array([row(0.5, ORIGIN[2] + H * 1, 0.25), row(-0.75, ORIGIN[2] + H * 511.5, -0.5)], np.float64)
    return depth, np.array([G, G], np.float32), rows


def test_integration_on_both_sides_of_the_2_gib_line_equals_the_twin(volume):
    """z layers {0, 1}, {510, 511} and {512, 513} against touch_fusion_ref.integrate on 1024 x 1024 x 2 volumes."""
    from gelslim_depth_amd.touch_fusion import integrate_touches
    depth, widths, rows = touches()
    volume.reset()
    integrate_touches(volume, torch.from_numpy(depth).to(DEV), torch.from_numpy(widths).to(DEV), torch.from_numpy(rows).to(DEV),
                      image_height_mm=HEIGHT_MM)
    zero = np.zeros((2, DIMS[1], DIMS[0]), np.float32)
    for iz0 in SLABS:
        want_acc, want_w = T.integrate(zero, zero, (ORIGIN[0], ORIGIN[1], ORIGIN[2] + H * iz0), H, TAU, depth, widths, rows, HEIGHT_MM)
        updated = [int((want_w[k] > 0).sum()) for k in (0, 1)]
        first, last = iz0 * DIMS[0] * DIMS[1], (iz0 + 2) * DIMS[0] * DIMS[1] - 1
        print(f"layers {iz0}, {iz0 + 1} (elements {first} .. {last}): {updated} updated voxels, {int((want_acc < 0).sum())} inside the surface")
        assert min(updated) > 10000 and int((want_acc < 0).sum()) > 100, "the slab must be reached by a touch, its contact band included"
        got_acc, got_w = volume.acc[iz0:iz0 + 2].cpu().numpy(), volume.weight[iz0:iz0 + 2].cpu().numpy()
        assert got_w.tobytes() == want_w.tobytes(), f"weight, layers {iz0}, {iz0 + 1}: {int((got_w != want_w).sum())} voxels differ"
        assert got_acc.tobytes() == want_acc.tobytes(), f"acc, layers {iz0}, {iz0 + 1}: {int((got_acc != want_acc).sum())} voxels differ"
    # the compared slabs lie on both sides of the line, and next to it
    assert (SLABS[1] + 2) * DIMS[0] * DIMS[1] == LINE == SLABS[2] * DIMS[0] * DIMS[1]
    # between the touches nothing was reached: layers 125 .. 387 are still zero
    assert not bool(volume.weight[200:204].any()) and not bool(volume.acc[200:204].any())


BLOCK = 25                               # voxels per axis of the sub-block the twin extracts


def sphere_block(first):
    """acc (nz, 25, 25) fp32 of the sub-block whose first voxel is (first, first, first): |p - centre| - 6 H with the centre at voxel
    first + 12 -- the far sphere -- or, for first = 0, at voxel (5, 5, 5), where the volume's faces cut it.  The far block is
    [500, 525) in x and y; in z the volume ends with layer 513, so the block is [500, 514) and the volume's top face cuts the far
    sphere (centre layer 512, radius 6) as well: its cells lie in layers 506 .. 512."""
    sub_origin = tuple(o + H * first for o in ORIGIN)
    c = first + 12 if first else 5
    nz = min(BLOCK, DIMS[2] - first)
    acc, _ = T.sphere_field((BLOCK, BLOCK, nz), sub_origin, H, tuple(o + H * c for o in ORIGIN), 6 * H)
    return acc, sub_origin


@pytest.mark.parametrize("first", [500, 0], ids=["far", "near"])
def test_extraction_on_both_sides_of_the_2_gib_line_equals_the_twin(volume, first):
    """A sphere of radius 6 voxels centred at voxel (512, 512, 512), +1 elsewhere, weight 1: count, order, coordinates and cells
    against touch_fusion_ref.extract on the sub-block [500, 525)^2 x [500, 514); then the same at voxel (5, 5, 5) against [0, 25)^3."""
    from gelslim_depth_amd.touch_fusion import extract_surface
    sub, sub_origin = sphere_block(first)
    nz = sub.shape[0]
    # the field is positive on every face of the block that has a neighbour in the volume: no cell outside the block has a triangle
    assert (sub[:, [0, -1]] > 0).all() and (sub[:, :, [0, -1]] > 0).all() and (sub[0] > 0).all() if first else \
        (sub[-1] > 0).all() and (sub[:, -1] > 0).all() and (sub[:, :, -1] > 0).all()
    assert first + nz == DIMS[2] or nz == BLOCK
    volume.acc.fill_(1.0)
    volume.weight.fill_(1.0)
    volume.acc[first:first + nz, first:first + BLOCK, first:first + BLOCK] = torch.from_numpy(sub).to(DEV)
    want, want_cell = T.extract(sub, np.ones_like(sub), sub_origin, H)
    ix, iy, iz = want_cell % (BLOCK - 1), (want_cell // (BLOCK - 1)) % (BLOCK - 1), want_cell // ((BLOCK - 1) * (BLOCK - 1))
    cell = (ix + first) + (DIMS[0] - 1) * ((iy + first) + (DIMS[1] - 1) * (iz + first))
    got = extract_surface(volume, cells=True)
    n = len(want)
    print(f"sub-block at {first}: {int(got.count)} triangles on the device, {n} in the twin, cells {int(cell.min())} .. {int(cell.max())}")
    assert n > 500 and int(got.count) == n and tuple(got.triangles.shape) == (n, 3, 3)
    assert np.array_equal(got.cell.cpu().numpy().astype(np.int64), cell), "cells and order"
    assert got.triangles.cpu().numpy().tobytes() == want.tobytes(), "coordinates"
    if first:
        below, above = int((iz + first < 512).sum()), int((iz + first >= 512).sum())
        assert below > 100 and above > 100, "triangles from cells on both sides of iz = 512"
        # a cell on the far side reads voxels past element 2^29
        assert ((iz + first) * DIMS[1] * DIMS[0]).max() >= LINE > ((iz + first) * DIMS[1] * DIMS[0]).min()
