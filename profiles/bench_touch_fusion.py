"""Times of integrate_touches and extract_surface against a torch composition of the same definition.

    python profiles/bench_touch_fusion.py [--out profiles/touch_fusion_times.txt] [--touches 64] [--voxels 256]

Workload: 64 rendered touches (`render_depth`, 320 x 427, 12 mm tall) of section 17's icosphere of 81,920 triangles, radius 10 mm,
along all three axes (three planes, random in-hand poses, widths 17.6 .. 18.8 mm), fused into 256^3 voxels around the sphere with
a truncation of four voxels.  Device events, the median of 7 calls after 2 warm-ups; the forms (cull on, cull off) alternate in one
process.

Compared with `integrate_torch`: the same arithmetic in torch fp64 -- an affine map of the voxel grid, floor, four explicit gathers
per channel, `where` and adds, one touch at a time over z slabs (the whole grid at once would hold a dozen fp64 volumes).  The
script states whether its acc and weight equal the kernel's."""
import argparse
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.join(os.path.dirname(HERE), "tests"))

DEV = "cuda:0"
HEIGHT_MM = 12.0


def timed(fn, warm=2, runs=7, before=None):
    times = []
    for i in range(warm + runs):
        if before is not None:
            before()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        if i >= warm:
            times.append(a.elapsed_time(b))
    return float(np.median(times))


def integrate_torch(vol, depth, widths, rows, carve_weight=1.0, slab=32):
    """Section 24's sample and update with torch operations, fp64 for the geometry and fp32 for the state; in place."""
    k_n, _, hh, ww = depth.shape
    nx, ny, nz = vol.dims
    h, tau = vol.voxel_mm, vol.truncation_mm
    inv_mpp, inv_tau = 1.0 / (HEIGHT_MM / hh), 1.0 / tau
    f64 = dict(device=depth.device, dtype=torch.float64)
    px = (vol.origin[0] + h * torch.arange(nx, **f64))[None, None, :]
    py = (vol.origin[1] + h * torch.arange(ny, **f64))[None, :, None]
    one, carve = torch.tensor(1.0, device=depth.device), torch.tensor(float(carve_weight), device=depth.device)
    flat = depth.reshape(k_n, 2, hh * ww)
    for z0 in range(0, nz, slab):
        pz = (vol.origin[2] + h * torch.arange(z0, min(nz, z0 + slab), **f64))[:, None, None]
        acc, weight = vol.acc[z0:z0 + slab], vol.weight[z0:z0 + slab]
        for k in range(k_n):
            t = rows[k]
            g = widths[k].double()
            ok = (g >= 0) & torch.isfinite(g)
            u = ((t[0] * px + t[1] * py) + t[2] * pz) + t[3]
            v = ((t[4] * px + t[5] * py) + t[6] * pz) + t[7]
            q = ((t[8] * px + t[9] * py) + t[10] * pz) + t[11]
            kf = v * inv_mpp + 0.5 * ww
            k0 = torch.floor(kf)
            b = kf - k0
            for ch, s in ((0, -1.0), (1, 1.0)):
                rf = (s * u) * inv_mpp + 0.5 * hh
                r0 = torch.floor(rf)
                inside = ok & (r0 >= 0) & (r0 <= hh - 2) & (k0 >= 0) & (k0 <= ww - 2)
                at = (torch.where(inside, r0, torch.zeros_like(r0)) * ww + torch.where(inside, k0, torch.zeros_like(k0))).long().reshape(-1)
                img = flat[k, ch]
                d00, d01, d10, d11 = (img[at + o].reshape(rf.shape) for o in (0, 1, ww, ww + 1))
                usable = inside & torch.isfinite(d00) & torch.isfinite(d01) & torch.isfinite(d10) & torch.isfinite(d11)
                contact = usable & (d00 < 0) & (d01 < 0) & (d10 < 0) & (d11 < 0)
                a = rf - r0
                e00, e01, e10, e11 = d00.double(), d01.double(), d10.double(), d11.double()
                top = e00 + b * (e01 - e00)
                bot = e10 + b * (e11 - e10)
                phi = (s * q - 0.5 * g) + (top + a * (bot - top))
                surf = contact & (phi >= -tau)
                free = usable & ~contact & (phi > 0)
                val = torch.clamp(phi * inv_tau, max=1.0).float()
                acc.copy_(torch.where(surf, acc + one * val, torch.where(free, acc + carve, acc)))
                weight.copy_(torch.where(surf, weight + one, torch.where(free, weight + carve, weight)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(HERE, "touch_fusion_times.txt"))
    ap.add_argument("--touches", type=int, default=64)
    ap.add_argument("--voxels", type=int, default=256)
    ap.add_argument("--size", type=int, nargs=2, default=(320, 427))
    args = ap.parse_args()
    import ctypes as C
    import mesh_depth_ref as R
    from gelslim_depth_amd import _lib as L
    from gelslim_depth_amd.mesh_depth import MeshGrid, render_depth
    from gelslim_depth_amd.mesh_register import MeshVolume, cloud_mesh_error
    from gelslim_depth_amd.touch_fusion import TouchVolume, extract_surface, integrate_touches, touch_transforms
    size, k_n, n = tuple(args.size), args.touches, args.voxels
    tri = np.float32(R.icosphere(6, 10.0))
    rng = np.random.Generator(np.random.PCG64(24))
    planes = ("+y+z", "+x-y", "+z+x")
    depth, widths, rows = [], [], []
    for i, plane in enumerate(planes):
        m = len(range(i, k_n, 3))
        if m == 0:
            continue
        grid = MeshGrid(tri, 1.0, plane, device=DEV)
        poses = torch.from_numpy(np.float32(np.stack((rng.uniform(-1.5e-3, 1.5e-3, m), rng.uniform(-1.5e-3, 1.5e-3, m), rng.uniform(-3.1, 3.1, m)), 1))).to(DEV)
        w = torch.from_numpy(np.float32(rng.uniform(17.6, 18.8, m))).to(DEV)
        depth.append(render_depth(grid, poses, w, image_size=size, image_height_mm=HEIGHT_MM))
        widths.append(w)
        rows.append(touch_transforms(poses, grid=grid))
    depth, widths, rows = torch.cat(depth), torch.cat(widths), torch.cat(rows)
    k_n = depth.shape[0]
    h = 21.0 / (n - 1)
    tau = 4.0 * h
    vol = TouchVolume((-10.5, -10.5, -10.5), h, (n, n, n), tau, device=DEV)
    mb = depth.numel() * 4 / 1e6
    lines = [f"touch fusion, {torch.cuda.get_device_name(0)}; ms, median of 7 after 2 warm-ups, device events",
             f"{k_n} touches of 2 x {size[0]} x {size[1]} ({mb:.1f} MB) into {n}^3 voxels of {h:.4f} mm, truncation {tau:.4f} mm"]

    def run(cull):
        integrate_touches(vol, depth, widths, rows, image_height_mm=HEIGHT_MM, cull=cull, validate=False)
    state = {}
    for rnd in range(3):          # the forms alternate: three rounds of both
        for cull in (True, False):
            t = timed(lambda: run(cull), before=vol.reset)
            lines.append(f"integrate_touches  cull {'on ' if cull else 'off'} round {rnd}: {t:9.3f} ms, "
                         f"{t / k_n:7.4f} ms per touch, {n ** 3 * k_n / t / 1e6:8.1f} G voxel-touches/s")
            print(lines[-1], flush=True)
            state[cull] = (vol.acc.clone(), vol.weight.clone())
    ref = state[True]
    same = all(torch.equal(ref[0], s[0]) and torch.equal(ref[1], s[1]) for s in state.values())
    lines.append(f"cull on and off give the same bits: {same}")
    # one touch at a time, as a robot would add them
    t = timed(lambda: [integrate_touches(vol, depth[j:j + 1], widths[j:j + 1], rows[j:j + 1], image_height_mm=HEIGHT_MM, validate=False)
                       for j in range(k_n)], before=vol.reset, runs=3, warm=1)
    lines.append(f"integrate_touches  one call per touch: {t:9.3f} ms, {t / k_n:7.4f} ms per touch; same bits: "
                 f"{torch.equal(vol.acc, ref[0]) and torch.equal(vol.weight, ref[1])}")
    print(lines[-1], flush=True)
    # the torch composition
    t_torch = timed(lambda: integrate_torch(vol, depth, widths, rows), before=vol.reset, warm=1, runs=3)
    d_acc = (vol.acc.double() - ref[0].double()).abs()
    lines.append(f"torch composition (fp64 gathers, where, adds): {t_torch:9.3f} ms, {t_torch / k_n:7.4f} ms per touch; acc equals the kernel's: "
                 f"{torch.equal(vol.acc, ref[0])} ({int((d_acc > 0).sum())} voxels differ, by {float(d_acc.max()):.3e} at most), weight equals: "
                 f"{torch.equal(vol.weight, ref[1])}")
    print(lines[-1], flush=True)
    vol.acc.copy_(ref[0])
    vol.weight.copy_(ref[1])
    # extraction: the count call (count + scan kernels), the write call, and the whole Python call with its one host read
    words = int(L.lib.gsd_touch_extract_workspace(C.byref(vol.volume)))
    ws = torch.empty((words,), device=DEV, dtype=torch.int32)
    total = torch.zeros((1,), device=DEV, dtype=torch.int64)
    count = lambda: L.check(L.lib.gsd_touch_extract_count(C.byref(vol.volume), vol.acc.data_ptr(), vol.weight.data_ptr(), 0.0, total.data_ptr(),      # noqa: E731
                                                          ws.data_ptr(), words, L.stream_ptr()), "count")
    t_count = timed(count)
    rows_n = int(total)
    out = torch.empty((rows_n, 3, 3), device=DEV)
    cell = torch.empty((rows_n,), device=DEV, dtype=torch.int32)
    write = lambda: L.check(L.lib.gsd_touch_extract_write(C.byref(vol.volume), vol.acc.data_ptr(), vol.weight.data_ptr(), 0.0, 0, rows_n,      # noqa: E731
                                                          out.data_ptr(), cell.data_ptr(), ws.data_ptr(), words, L.stream_ptr()), "write")
    t_write = timed(write)
    t_all = timed(lambda: extract_surface(vol, cells=True))
    lines.append(f"extract_surface: {rows_n} triangles from {(n - 1) ** 3} cells ({words // 2 - 2} blocks, {-(-(words // 2 - 2) // 4096)} scan passes): "
                 f"count + scan {t_count:7.3f} ms, write {t_write:7.3f} ms, the Python call with its host read {t_all:7.3f} ms")
    print(lines[-1], flush=True)
    surface = extract_surface(vol)
    err = cloud_mesh_error(MeshVolume(tri, device=DEV), surface.vertices())
    lines.append(f"vertices against the icosphere: mean {float(err['mean']):.5f}, rms {float(err['rms']):.5f}, max {float(err['max']):.5f} mm "
                 f"(sqrt 3 h + sqrt 2 mpp = {3 ** 0.5 * h + 2 ** 0.5 * HEIGHT_MM / size[0]:.5f})")
    print(lines[-1], flush=True)
    with open(args.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
