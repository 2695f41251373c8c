"""The restatement of vc_hull_measure (contract in include/voxcarve.h): the records of a hull reduced per group to counts, first
and second moments of (ix, iy, iz), exposed faces, colour sums and the box -- once as a literal loop over the records
(measure_literal) and once vectorised (measure).  Python integers and u64 only; both return the dict CarveEngine.fetch_measure
returns, and `profile` the u64 [G, nz, 3] of fetch_measure_profile."""
import numpy as np

NONE = 0xffffffff                # the label of a record in no group
GEO_UNREACHED = 255
MAX_GROUPS = 4096
MAX_AXIS = 65536
MAX_PROFILE = 1 << 20
EMPTY_LO, EMPTY_HI = 0xffffffff, 0
FIELDS = ("voxels", "surface", "seen", "s1", "s2", "faces", "rgb", "lo", "hi")
# the neighbour of each face, in the order of vc_measure_t::faces: -x, +x, -y, +y, -z, +z as (dx, dy, dz)
FACES = ((-1, 0, 0), (1, 0, 0), (0, -1, 0), (0, 1, 0), (0, 0, -1), (0, 0, 1))
S2_PAIRS = ((0, 0), (1, 1), (2, 2), (0, 1), (0, 2), (1, 2))


def pack_records(idx, rgb=None, seen=None):
    """u64 records {u32 idx, r, g, b, seen} of the ascending indices idx."""
    idx = np.asarray(idx, dtype=np.uint64)
    rgb = np.zeros((idx.size, 3), np.uint64) if rgb is None else np.asarray(rgb, dtype=np.uint64)
    seen = np.ones(idx.size, np.uint64) if seen is None else np.asarray(seen, dtype=np.uint64)
    return idx | (rgb[:, 0] << np.uint64(32)) | (rgb[:, 1] << np.uint64(40)) | (rgb[:, 2] << np.uint64(48)) | (seen << np.uint64(56))


def _check(grid, G, nlabels, S, with_profile):
    nx, ny, nz = grid
    if max(grid) > MAX_AXIS:
        raise ValueError("an axis of more than %d cells" % MAX_AXIS)
    if not 1 <= G <= MAX_GROUPS:
        raise ValueError("G = %d not in [1, %d]" % (G, MAX_GROUPS))
    if nlabels != S:
        raise ValueError("%d labels for %d records" % (nlabels, S))
    if with_profile and G * nz > MAX_PROFILE:
        raise ValueError("a profile of %d x %d entries" % (G, nz))


def _empty(G):
    return {"voxels": np.zeros(G, np.uint64), "surface": np.zeros(G, np.uint64), "seen": np.zeros(G, np.uint64),
            "s1": np.zeros((G, 3), np.uint64), "s2": np.zeros((G, 6), np.uint64), "faces": np.zeros((G, 6), np.uint64),
            "rgb": np.zeros((G, 3), np.uint64), "lo": np.full((G, 3), EMPTY_LO, np.uint32), "hi": np.full((G, 3), EMPTY_HI, np.uint32)}


def labels_of(source, S, labels=None, groups=None):
    """(u32 labels [S] with NONE for "no group", G) of a source: "all"; ("clusters", u8 labels, K); ("geodesic", u8 labels,
    extremities); or host labels with G = groups."""
    if source == "all":
        return np.zeros(S, np.uint32), 1
    lab = np.asarray(labels).astype(np.uint32)
    if source == "geodesic":
        return np.where(lab == GEO_UNREACHED, np.uint32(NONE), lab).astype(np.uint32), int(groups) + 1
    return lab, int(groups)


def measure_literal(records, grid, labels, G, with_profile=False):
    """The contract read out loud: one loop over the records, a set of the survivors for the faces."""
    nx, ny, nz = grid
    records = [int(r) for r in np.asarray(records, dtype=np.uint64)]
    labels = [int(v) for v in np.asarray(labels)]
    _check(grid, G, len(labels), len(records), with_profile)
    hull = set(r & 0xffffffff for r in records)
    acc = [dict(voxels=0, surface=0, seen=0, s1=[0] * 3, s2=[0] * 6, faces=[0] * 6, rgb=[0] * 3, lo=[EMPTY_LO] * 3, hi=[EMPTY_HI] * 3)
           for _ in range(G)]
    prof = [[[0, 0, 0] for _ in range(nz)] for _ in range(G)] if with_profile else None
    for r, g in zip(records, labels):
        if g == NONE:
            continue
        if g >= G:
            raise ValueError("label %d not below G = %d" % (g, G))
        i = r & 0xffffffff
        iy, ix, iz = i % ny, (i // ny) % nx, i // (nx * ny)
        c = (ix, iy, iz)
        a = acc[g]
        a["voxels"] += 1
        exposed = 0
        for f, (dx, dy, dz) in enumerate(FACES):
            jx, jy, jz = ix + dx, iy + dy, iz + dz
            inside = 0 <= jx < nx and 0 <= jy < ny and 0 <= jz < nz
            if not inside or ((jz * nx + jx) * ny + jy) not in hull:
                a["faces"][f] += 1
                exposed += 1
        a["surface"] += 1 if exposed else 0
        if (r >> 56) & 1:
            a["seen"] += 1
            for k in range(3):
                a["rgb"][k] += (r >> (32 + 8 * k)) & 255
        for k in range(3):
            a["s1"][k] += c[k]
            a["lo"][k] = min(a["lo"][k], c[k])
            a["hi"][k] = max(a["hi"][k], c[k])
        for k, (p, q) in enumerate(S2_PAIRS):
            a["s2"][k] += c[p] * c[q]
        if with_profile:
            prof[g][iz][0] += 1
            prof[g][iz][1] += ix
            prof[g][iz][2] += iy
    out = _empty(G)
    for g in range(G):
        for k in FIELDS:
            out[k][g] = acc[g][k]
    if with_profile:
        out["profile"] = np.array(prof, dtype=np.uint64).reshape(G, nz, 3)
    return out


def _sum_by(labels, G, values):
    """u64 [G]: the exact sums of non-negative int64 values below 2^33 per label (bincount adds in float64: split in halves)."""
    v = np.asarray(values, dtype=np.int64)
    lo = np.bincount(labels, weights=(v & 0xffff).astype(np.float64), minlength=G)
    hi = np.bincount(labels, weights=(v >> 16).astype(np.float64), minlength=G)
    return np.array([int(a) + (int(b) << 16) for a, b in zip(lo, hi)], dtype=np.uint64)


def measure(records, grid, labels, G, with_profile=False):
    nx, ny, nz = grid
    records = np.asarray(records, dtype=np.uint64)
    lab = np.asarray(labels).astype(np.int64)
    _check(grid, G, lab.size, records.size, with_profile)
    if ((lab >= G) & (lab != NONE)).any():
        raise ValueError("a label not below G = %d" % G)
    idx = (records & np.uint64(0xffffffff)).astype(np.int64)
    occ = np.zeros((nz + 2, nx + 2, ny + 2), dtype=bool)         # a border of OFF cells: outside the grid is exposed
    iy, ix, iz = idx % ny, (idx // ny) % nx, idx // (nx * ny)
    occ[iz + 1, ix + 1, iy + 1] = True
    exposed = np.stack([~occ[iz + 1 + dz, ix + 1 + dx, iy + 1 + dy] for dx, dy, dz in FACES], axis=1)     # [S, 6]
    seen = ((records >> np.uint64(56)) & np.uint64(1)).astype(np.int64)
    rgb = np.stack([((records >> np.uint64(s)) & np.uint64(255)).astype(np.int64) for s in (32, 40, 48)], axis=1) * seen[:, None]
    keep = lab != NONE
    l = lab[keep]
    c = np.stack([ix, iy, iz], axis=1)[keep]
    out = _empty(G)
    ones = np.ones(l.size, np.int64)
    out["voxels"] = _sum_by(l, G, ones)
    out["surface"] = _sum_by(l, G, exposed[keep].any(axis=1))
    out["seen"] = _sum_by(l, G, seen[keep])
    for k in range(3):
        out["s1"][:, k] = _sum_by(l, G, c[:, k])
        out["rgb"][:, k] = _sum_by(l, G, rgb[keep][:, k])
    for k, (p, q) in enumerate(S2_PAIRS):
        out["s2"][:, k] = _sum_by(l, G, c[:, p] * c[:, q])
    for f in range(6):
        out["faces"][:, f] = _sum_by(l, G, exposed[keep][:, f])
    for g in np.unique(l):
        m = c[l == g]
        out["lo"][g], out["hi"][g] = m.min(axis=0), m.max(axis=0)
    if with_profile:
        key = l * nz + c[:, 2]
        out["profile"] = np.stack([_sum_by(key, G * nz, ones), _sum_by(key, G * nz, c[:, 0]), _sum_by(key, G * nz, c[:, 1])],
                                  axis=1).reshape(G, nz, 3)
    return out


def stats(records, labels, G):
    lab = np.asarray(labels).astype(np.int64)
    measured = int((lab != NONE).sum())
    return {"survivors": int(np.asarray(records).size), "groups": int(G), "measured": measured, "unlabelled": int(lab.size) - measured}


def same(a, b, with_profile=False):
    """Asserts two results equal field by field, dtype and shape included."""
    for k in FIELDS + (("profile",) if with_profile else ()):
        x, y = np.asarray(a[k]), np.asarray(b[k])
        assert x.dtype == y.dtype and x.shape == y.shape, (k, x.dtype, y.dtype, x.shape, y.shape)
        assert np.array_equal(x, y), (k, x, y)


def component_ranks(labels, comp_label, comp_size):
    """u32 [S]: the rank of each record's component, size descending then label ascending."""
    order = sorted(range(len(comp_label)), key=lambda k: (-int(comp_size[k]), int(comp_label[k])))
    rank = {int(comp_label[k]): r for r, k in enumerate(order)}
    return np.array([rank[int(v)] for v in labels], dtype=np.uint32)
