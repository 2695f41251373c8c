"""World units from the integers of CarveEngine.measure_hull (vc_hull_measure; contract in include/voxcarve.h).

The device sums indices; everything in millimetres is derived here, on the host, from those sums and the grid: with s_a the
float64 grid step of axis a, (max_a - min_a) / (n_a - 1), and lo_a the axis minimum, the cell (ix, iy, iz) has its centre at
lo + s * (ix, iy, iz).

The area is the area of the voxel boundary: the exposed cell faces times their face areas.  A staircase does not converge to the
smooth surface it approximates, so this OVERSTATES a smooth surface -- by 1.5 x for a sphere in the limit of fine grids (the mean
of |n_x| + |n_y| + |n_z| over the unit sphere), by 1 x for an axis-aligned box.  Compare such areas with each other, not with a
tape measure."""
import numpy as np

S2_PAIRS = ((0, 0), (1, 1), (2, 2), (0, 1), (0, 2), (1, 2))      # the order of vc_measure_t::s2


def grid_metric(grid, bounds):
    """(lo float64 [3], step float64 [3]) of the grid: the axis minima and the steps in mm (0 on an axis of one cell)."""
    lo = np.array([bounds[0], bounds[2], bounds[4]], dtype=np.float64)
    hi = np.array([bounds[1], bounds[3], bounds[5]], dtype=np.float64)
    n = np.array(grid, dtype=np.float64)
    step = np.where(n > 1, (hi - lo) / np.where(n > 1, n - 1, 1.0), 0.0)
    return lo, step


def covariance_mm2(voxels, s1, s2, step):
    """float64 [3, 3]: the covariance of the group's solid in mm^2 -- of the cell centres, the numerators voxels s2_ab - s1_a s1_b
    formed in Python integers (they pass 2^64), plus s_a^2 / 12 on the diagonal for the extent of a cell."""
    n = int(voxels)
    s1 = [int(v) for v in s1]
    s2 = [int(v) for v in s2]
    c = np.zeros((3, 3), dtype=np.float64)
    for k, (a, b) in enumerate(S2_PAIRS):
        num = n * s2[k] - s1[a] * s1[b]
        c[a, b] = c[b, a] = float(step[a]) * float(step[b]) * (num / (n * n))
    for a in range(3):
        c[a, a] += float(step[a]) ** 2 / 12.0
    return c


def principal_axes(cov):
    """(std_mm float64 [3], axes float64 [3, 3]) by numpy.linalg.eigh: standard deviations in descending order, axes[k] the unit
    vector of the k-th, signed so that its largest component is positive."""
    w, v = np.linalg.eigh(cov)
    order = np.argsort(w)[::-1]
    w, v = w[order], v[:, order].T
    for k in range(3):
        if v[k, np.argmax(np.abs(v[k]))] < 0:
            v[k] = -v[k]
    return np.sqrt(np.maximum(w, 0.0)), v


def describe(measure, grid, bounds):
    """The dict of CarveEngine.fetch_measure in world units: dict of numpy arrays over the G groups --
    voxels u64; volume_mm3 = voxels s_x s_y s_z; area_mm2 = the exposed faces times their areas (the voxel boundary: see the
    module's note, 1.5 x a smooth sphere's); centroid_mm [G, 3] = lo + s * (s1 / voxels); covariance_mm2 [G, 3, 3]; std_mm [G, 3]
    and axes [G, 3, 3], the principal standard deviations (descending) and directions; lean_deg, the angle between the major
    axis and the z line (0 upright, 90 lying); height_mm = the box's extent in z, cells included; top_mm = the z of the centre of
    the highest voxel (world up is -z: the smallest); mean_rgb [G, 3] over the seen records.  A group without a record (or without
    a seen one, for mean_rgb) has NaN where a mean would be."""
    lo, step = grid_metric(grid, bounds)
    G = int(np.asarray(measure["voxels"]).size)
    out = {"voxels": np.asarray(measure["voxels"], dtype=np.uint64).copy(),
           "volume_mm3": np.zeros(G), "area_mm2": np.zeros(G), "centroid_mm": np.full((G, 3), np.nan),
           "covariance_mm2": np.full((G, 3, 3), np.nan), "std_mm": np.full((G, 3), np.nan), "axes": np.full((G, 3, 3), np.nan),
           "lean_deg": np.full(G, np.nan), "height_mm": np.zeros(G), "top_mm": np.full(G, np.nan), "mean_rgb": np.full((G, 3), np.nan)}
    face_area = np.array([step[1] * step[2]] * 2 + [step[0] * step[2]] * 2 + [step[0] * step[1]] * 2)
    for g in range(G):
        n = int(measure["voxels"][g])
        out["area_mm2"][g] = float((np.asarray(measure["faces"][g], dtype=np.float64) * face_area).sum())
        if n == 0:
            continue
        out["volume_mm3"][g] = n * step[0] * step[1] * step[2]
        out["centroid_mm"][g] = lo + step * (np.asarray(measure["s1"][g], dtype=np.float64) / n)
        cov = covariance_mm2(n, measure["s1"][g], measure["s2"][g], step)
        std, axes = principal_axes(cov)
        out["covariance_mm2"][g], out["std_mm"][g], out["axes"][g] = cov, std, axes
        out["lean_deg"][g] = float(np.degrees(np.arccos(min(1.0, abs(float(axes[0, 2]))))))
        out["height_mm"][g] = (int(measure["hi"][g][2]) - int(measure["lo"][g][2]) + 1) * step[2]
        out["top_mm"][g] = lo[2] + step[2] * int(measure["lo"][g][2])
        seen = int(measure["seen"][g])
        if seen:
            out["mean_rgb"][g] = np.asarray(measure["rgb"][g], dtype=np.float64) / seen
    return out


def profile_mm(profile, grid, bounds):
    """The u64 [G, nz, 3] of CarveEngine.fetch_measure_profile in world units: (area_mm2 [G, nz], the cross-section's cell
    area per layer; centre_mm [G, nz, 2], its centre line in (x, y), NaN on a layer without a voxel; z_mm [nz])."""
    lo, step = grid_metric(grid, bounds)
    p = np.asarray(profile, dtype=np.float64)
    n = p[:, :, 0]
    with np.errstate(invalid="ignore", divide="ignore"):
        centre = np.stack([lo[0] + step[0] * p[:, :, 1] / n, lo[1] + step[1] * p[:, :, 2] / n], axis=2)
    centre[n == 0] = np.nan
    return n * step[0] * step[1], centre, lo[2] + step[2] * np.arange(p.shape[1])
