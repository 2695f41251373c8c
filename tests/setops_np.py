"""The contract of vc_hull_combine and vc_hull_compare (include/voxcarve.h) restated in numpy: a set
operation between the current hull A and a kept hull B, the records it leaves, and the comparison of the two.  Integers only.

  combine_sets / combine_sets_literal   R from A and B, on whole volumes / voxel by voxel
  combine / combine_literal             the 8-byte records and `added` bytes the device leaves, and the stats
  compare / compare_literal             counts, the index box of the symmetric difference, the directed Hausdorff distances

A hull is a boolean volume occ[iz, ix, iy] (linear index i = (iz nx + ix) ny + iy, the grid's order: dn.volume / dn.indices); records
are uint64 with the index in the low 32 bits, ascending."""
import numpy as np

import closing_np as cl
import distance_np as dn

OPS = ("copy", "and", "or", "andnot", "xor")
LOW = np.uint64(0xffffffff)
U32_MAX = 0xffffffff
U64_MAX = (1 << 64) - 1


def combine_sets(a, b, op):
    a, b = np.asarray(a, dtype=bool), np.asarray(b, dtype=bool)
    if op == "copy":
        return b.copy()
    if op == "and":
        return a & b
    if op == "or":
        return a | b
    if op == "andnot":
        return a & ~b
    if op == "xor":
        return a ^ b
    raise ValueError("op %r, expected one of %s" % (op, OPS))


def combine_sets_literal(a, b, op):
    """The definition, one voxel at a time."""
    if op not in OPS:
        raise ValueError("op %r, expected one of %s" % (op, OPS))
    fa, fb = np.asarray(a).reshape(-1), np.asarray(b).reshape(-1)
    out = []
    for v in range(fa.size):
        ina, inb = bool(fa[v]), bool(fb[v])
        out.append({"copy": inb, "and": ina and inb, "or": ina or inb, "andnot": ina and not inb, "xor": ina != inb}[op])
    return np.array(out, dtype=bool).reshape(np.asarray(a).shape)


def _stats(a, b, r):
    return {"survivors_before": int(a.sum()), "other": int(b.sum()), "common": int((a & b).sum()), "survivors_after": int(r.sum()),
            "added": int((r & ~a).sum()), "removed": int((a & ~r).sum())}


def _of(records, occ):
    records = np.asarray(records, dtype=np.uint64)
    assert np.array_equal((records & LOW).astype(np.int64), np.flatnonzero(np.asarray(occ).reshape(-1))), "the records are the hull's"
    return records


def combine(rec_a, a, b, rec_b, op, grid, bounds, cam=None, frame=None, H=None, W=None):
    """(records, added, R, stats) after vc_hull_combine.  rec_a: A's records; rec_b: B's, or None for a register without records.
    A record of A & R keeps its bytes; a voxel of R & ~A takes B's record, or without one a fresh record as closing_np.records_after
    colours it; "copy" from records is B's records verbatim.  added = 1 where the voxel was not in A."""
    a, b = np.asarray(a, dtype=bool), np.asarray(b, dtype=bool)
    rec_a = _of(rec_a, a)
    r = combine_sets(a, b, op)
    flat_a, flat_r = a.reshape(-1), r.reshape(-1)
    idx_a = (rec_a & LOW).astype(np.int64)
    kept = rec_a[flat_r[idx_a]]
    if rec_b is None:
        out, added = cl.records_after(kept, r, grid, bounds, cam, frame, H, W)
    else:
        rec_b = _of(rec_b, b)
        idx_r = np.flatnonzero(flat_r)
        was = flat_a[idx_r]
        idx_b = (rec_b & LOW).astype(np.int64)
        from_b = np.zeros(flat_r.size, dtype=np.uint64)
        from_b[idx_b] = rec_b
        out = from_b[idx_r]
        if op != "copy":
            out[was] = kept
        added = (~was).astype(np.uint8)
    return out, added, r, _stats(a, b, r)


def combine_literal(rec_a, a, b, rec_b, op, grid, bounds, cam=None, frame=None, H=None, W=None):
    """The same by a loop over the voxels (fresh records: one closing_np.records_after call per voxel)."""
    fa, fb = np.asarray(a, dtype=bool).reshape(-1), np.asarray(b, dtype=bool).reshape(-1)
    of_a = {int(x) & U32_MAX: int(x) for x in np.asarray(rec_a, dtype=np.uint64)}
    of_b = None if rec_b is None else {int(x) & U32_MAX: int(x) for x in np.asarray(rec_b, dtype=np.uint64)}
    r = combine_sets_literal(a, b, op).reshape(-1)
    out, added = [], []
    for v in range(fa.size):
        if not r[v]:
            continue
        if fa[v] and not (op == "copy" and of_b is not None):
            out.append(of_a[v])
        elif of_b is not None:
            out.append(of_b[v])
        else:
            one = np.zeros(fa.size, dtype=bool)
            one[v] = True
            out.append(int(cl.records_after(np.empty(0, np.uint64), one.reshape(np.asarray(a).shape), grid, bounds, cam, frame, H, W)[0][0]))
        added.append(0 if fa[v] else 1)
    return np.array(out, dtype=np.uint64), np.array(added, dtype=np.uint8), r.reshape(np.asarray(a).shape)


def _box(occ):
    """(lo, hi) in x, y, z of a volume occ[iz, ix, iy]; UINT32_MAX and 0 for an empty one."""
    if not occ.any():
        return (U32_MAX,) * 3, (0,) * 3
    z, x, y = np.nonzero(occ)
    return (int(x.min()), int(y.min()), int(z.min())), (int(x.max()), int(y.max()), int(z.max()))


def _directed(x, y, q):
    """(h2, arg) of x against y: max over x & ~y of the distance to the nearest voxel of y, the smallest index that attains it."""
    d = (x & ~y).reshape(-1)
    if not d.any():
        return 0, U32_MAX
    f = dn.outside(y, q).reshape(-1)
    idx = np.flatnonzero(d)
    h2 = int(f[idx].max())
    return h2, int(idx[f[idx] == np.uint64(h2)].min())


def compare(a, b, q=None):
    """The stats of vc_hull_compare; q = the steps in um (dn.steps_um) asks for the distances."""
    a, b = np.asarray(a, dtype=bool), np.asarray(b, dtype=bool)
    lo, hi = _box(a ^ b)
    out = {"a": int(a.sum()), "b": int(b.sum()), "common": int((a & b).sum()), "only_a": int((a & ~b).sum()), "only_b": int((b & ~a).sum()),
           "diff_lo": lo, "diff_hi": hi}
    if q is not None:
        out["h2_ab"], out["arg_ab"] = _directed(a, b, q)
        out["h2_ba"], out["arg_ba"] = _directed(b, a, q)
        out["q"] = tuple(int(v) for v in q)
    return out


def compare_literal(a, b, q):
    """The definition: every voxel of the one-sided difference against every voxel of the other hull, in Python integers."""
    a, b = np.asarray(a, dtype=bool), np.asarray(b, dtype=bool)
    nz, nx, ny = a.shape

    def cells(occ):
        return [(int(x), int(y), int(z)) for z, x, y in zip(*np.nonzero(occ))]

    def directed(x, y):
        sites = cells(y)
        best, arg = 0, U32_MAX
        for v in cells(x & ~y):
            d = min([sum((q[k] * (v[k] - w[k])) ** 2 for k in range(3)) for w in sites], default=U64_MAX)
            i = (v[2] * nx + v[0]) * ny + v[1]
            if d > best or (d == best and i < arg):
                best, arg = d, i
        return best, arg

    diff = cells(a ^ b)
    out = {"a": len(cells(a)), "b": len(cells(b)), "common": len(cells(a & b)), "only_a": len(cells(a & ~b)), "only_b": len(cells(b & ~a)),
           "diff_lo": tuple(min(c[k] for c in diff) for k in range(3)) if diff else (U32_MAX,) * 3,
           "diff_hi": tuple(max(c[k] for c in diff) for k in range(3)) if diff else (0,) * 3, "q": tuple(int(v) for v in q)}
    out["h2_ab"], out["arg_ab"] = directed(a, b)
    out["h2_ba"], out["arg_ba"] = directed(b, a)
    return out


def derived(st):
    """iou, dice and hausdorff_mm as CarveEngine.compare_hull derives them."""
    union = st["common"] + st["only_a"] + st["only_b"]
    worst = max(st["h2_ab"], st["h2_ba"]) if "h2_ab" in st else None
    return {"iou": st["common"] / union if union else None, "dice": 2 * st["common"] / (st["a"] + st["b"]) if union else None,
            "hausdorff_mm": float(np.sqrt(float(worst))) / 1000.0 if worst is not None and union and worst != U64_MAX else None}
