"""The CPU twin of gsd_contact_patches_* (DESIGN.md section 22): numpy and plain loops, following the definition literally.

labels by flood fill in raster order, statistics with Python integers, the filter on the fp32 bit patterns.  No scipy."""
import numpy as np

COLS = 12
DQ_BITS = 20


def contact_mask(depth, contact_depth):
    """d < -(float32) c, compared in fp32: a NaN is not contact, -inf is, -c itself is not."""
    d = np.asarray(depth, dtype=np.float32)
    with np.errstate(invalid="ignore"):
        return d < -np.float32(contact_depth)


def neighbours(connectivity):
    four = [(-1, 0), (1, 0), (0, -1), (0, 1)]
    return four if connectivity == 4 else four + [(-1, -1), (-1, 1), (1, -1), (1, 1)]


def label_plane(mask, connectivity=8, min_area=1):
    """(labels int32 (H, W), count) of one plane: flood fill from every unvisited contact pixel in raster order, so that a patch
    is met at its first pixel; patches of fewer than min_area pixels get 0 and no number."""
    h, w = mask.shape
    labels = np.zeros((h, w), dtype=np.int32)
    seen = np.zeros((h, w), dtype=bool)
    nb = neighbours(connectivity)
    count = 0
    for r in range(h):
        for k in range(w):
            if not mask[r, k] or seen[r, k]:
                continue
            seen[r, k] = True
            patch, stack = [], [(r, k)]
            while stack:
                pr, pk = stack.pop()
                patch.append((pr, pk))
                for dr, dk in nb:
                    qr, qk = pr + dr, pk + dk
                    if 0 <= qr < h and 0 <= qk < w and mask[qr, qk] and not seen[qr, qk]:
                        seen[qr, qk] = True
                        stack.append((qr, qk))
            if len(patch) >= min_area:
                count += 1
                for pr, pk in patch:
                    labels[pr, pk] = count
    return labels, count


def ord32(d):
    """The order-preserving map of fp32 bits to uint32: ~u if the sign bit is set, else u | 0x80000000 (as a Python int)."""
    u = int(np.asarray(d, dtype=np.float32).view(np.uint32))
    return (~u) & 0xFFFFFFFF if u & 0x80000000 else u | 0x80000000


def ord32_inverse(o):
    u = (o - 0x80000000) if o & 0x80000000 else (~o) & 0xFFFFFFFF
    return np.array(u, dtype=np.uint32).view(np.float32)[()]


def dq(d):
    """(int) rint(double(max(d, -1024.0f)) * 2^20): exact in fp64, half to even."""
    return int(np.rint(np.float64(max(np.float32(d), np.float32(-1024.0))) * np.float64(1 << DQ_BITS)))


def peak_key(d, at):
    return (ord32(d) << 32) | int(at)


def stats_plane(depth, labels, K):
    """(K, 12) int64 of one plane: row j for patch j + 1, rows without a patch all zero."""
    h, w = labels.shape
    rows = [None] * K
    for r in range(h):
        for k in range(w):
            n = int(labels[r, k])
            if n < 1 or n > K:
                continue
            d = depth[r, k]
            key = peak_key(d, r * w + k)
            if rows[n - 1] is None:
                rows[n - 1] = [0, r, r, k, k, 0, 0, 0, 0, 0, 0, key]
            s = rows[n - 1]
            s[0] += 1
            s[1], s[2], s[3], s[4] = min(s[1], r), max(s[2], r), min(s[3], k), max(s[4], k)
            s[5] += r
            s[6] += k
            s[7] += r * r
            s[8] += k * k
            s[9] += r * k
            s[10] += dq(d)
            s[11] = min(s[11], key)
    out = np.zeros((K, COLS), dtype=np.int64)
    for j, s in enumerate(rows):
        if s is not None:
            out[j] = s
    return out


def contact_patches(depth, contact_depth=0.0, connectivity=8, min_area=1, max_patches=64):
    """(labels (B, 2, H, W) int32, counts (B, 2) int32, stats (B, 2, K, 12) int64) of depth (B, 2, H, W) fp32."""
    depth = np.asarray(depth, dtype=np.float32)
    b, c, h, w = depth.shape
    assert c == 2
    labels = np.zeros((b, 2, h, w), dtype=np.int32)
    counts = np.zeros((b, 2), dtype=np.int32)
    stats = np.zeros((b, 2, max_patches, COLS), dtype=np.int64)
    for i in range(b):
        for ch in range(2):
            labels[i, ch], counts[i, ch] = label_plane(contact_mask(depth[i, ch], contact_depth), connectivity, min_area)
            stats[i, ch] = stats_plane(depth[i, ch], labels[i, ch], max_patches)
    return labels, counts, stats


def keep_table(stats, keep_largest=None):
    """(B, 2, K) bool: the numbered patches 1..K that are kept.  keep_largest=n: the n largest of the plane, the lower number
    first on equal areas."""
    area = stats[..., 0]
    keep = area > 0
    if keep_largest is not None:
        for idx in np.ndindex(area.shape[:2]):
            order = sorted(range(area.shape[2]), key=lambda j: (-int(area[idx][j]), j))
            chosen = np.zeros(area.shape[2], dtype=bool)
            chosen[order[:keep_largest]] = True
            keep[idx] &= chosen
    return keep


def filtered_depth(depth, labels, stats, contact_depth=0.0, keep_largest=None):
    """depth bit for bit except +0.0 where a pixel is contact and its patch is not kept.  Without keep_largest every numbered
    patch is kept (numbers above K too); with it only the chosen ones among 1..K."""
    depth = np.asarray(depth, dtype=np.float32)
    bits = depth.view(np.uint32).copy()
    K = stats.shape[2]
    mask = contact_mask(depth, contact_depth)
    if keep_largest is None:
        kept = labels > 0
    else:
        table = np.zeros(stats.shape[:2] + (K + 1,), dtype=bool)
        table[..., 1:] = keep_table(stats, keep_largest)
        lab = np.where(labels <= K, labels, 0)
        kept = np.take_along_axis(table, lab.reshape(labels.shape[0], 2, -1).astype(np.int64), axis=2).reshape(labels.shape)
    bits[mask & ~kept] = 0
    return bits.view(np.float32)


def derived(stats, shape, image_height_mm=12.0):
    """The derived properties in numpy fp64 from the integer statistics, by section 22's formulas; NaN (bbox, peak_rc: -1) in
    rows without a patch."""
    h, w = shape
    mpp = float(image_height_mm) / h
    s = stats.astype(np.float64)
    used = stats[..., 0] > 0
    nan = lambda t: np.where(used.reshape(used.shape + (1,) * (t.ndim - used.ndim)), t, np.nan)      # noqa: E731
    with np.errstate(invalid="ignore", divide="ignore"):
        n = s[..., 0]
        mr, mk = s[..., 5] / n, s[..., 6] / n
        m20, m02, m11 = s[..., 7] / n - mr * mr, s[..., 8] / n - mk * mk, s[..., 9] / n - mr * mk
        half, diff = 0.5 * (m20 + m02), 0.5 * (m20 - m02)
        root = np.sqrt(diff * diff + m11 * m11)
        out = {
            "area_mm2": nan(n * (mpp * mpp)),
            "centroid_mm": nan(np.stack((mpp * (mr - h / 2), mpp * (mk - w / 2)), axis=-1)),
            "axis_angle": nan(0.5 * np.arctan2(2.0 * m11, m20 - m02)),
            "axis_lengths_mm": nan(np.stack((mpp * np.sqrt(half + root), mpp * np.sqrt(np.maximum(half - root, 0.0))), axis=-1)),
            "volume_mm3": nan(-s[..., 10] / float(1 << DQ_BITS) * (mpp * mpp)),
            "mean_depth": nan(s[..., 10] / float(1 << DQ_BITS) / n),
        }
    key = stats[..., 11]
    peak = np.full(key.shape, np.nan, dtype=np.float32)
    for idx in np.ndindex(key.shape):
        if used[idx]:
            peak[idx] = ord32_inverse(int(key[idx]) >> 32)
    at = key & 0xFFFFFFFF
    out["peak_depth"] = peak
    out["peak_rc"] = np.where(used[..., None], np.stack((at // w, at % w), axis=-1), -1)
    out["bbox"] = np.where(used[..., None], stats[..., 1:5], -1)
    return out
