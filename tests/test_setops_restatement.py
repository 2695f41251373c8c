"""The restatement of the set algebra on hulls (tests/setops_np.py) against itself, voxcarve.hullio, and the ABI surface of the seven
calls: no GPU."""
import os

import numpy as np
import pytest

import distance_np as dn
import fixtures_util as fx
import setops_np as sn

LOW = np.uint64(0xffffffff)


def _random_hull(rng, grid, p):
    nx, ny, nz = grid
    occ = rng.random((nz, nx, ny)) < p
    idx = dn.indices(occ).astype(np.uint64)
    rec = idx | (rng.integers(0, 1 << 25, idx.size, dtype=np.uint64) << np.uint64(32))
    return occ, rec


@pytest.mark.parametrize("grid,seed", [((5, 7, 3), 1), ((4, 3, 6), 2), ((9, 11, 7), 3)])
def test_literal_equals_vectorised(grid, seed):
    rng = np.random.default_rng(seed)
    cams3, _, frames3 = fx.random_scene(seed, C=3)
    cam = fx.oracle_cams(cams3)[1]
    H, W = frames3[1].shape[:2]
    for pa, pb in ((0.5, 0.5), (0.0, 0.4), (0.4, 0.0), (1.0, 0.3), (0.2, 1.0)):
        a, ra = _random_hull(rng, grid, pa)
        b, rb = _random_hull(rng, grid, pb)
        for op in sn.OPS:
            assert np.array_equal(sn.combine_sets(a, b, op), sn.combine_sets_literal(a, b, op)), op
            for with_records in (True, False):
                got = sn.combine(ra, a, b, rb if with_records else None, op, grid, fx_bounds(), cam, frames3[1], H, W)
                lit = sn.combine_literal(ra, a, b, rb if with_records else None, op, grid, fx_bounds(), cam, frames3[1], H, W)
                assert np.array_equal(got[0], lit[0]) and np.array_equal(got[1], lit[1]) and np.array_equal(got[2], lit[2]), (op, with_records)
                r, st = got[2], got[3]
                assert np.array_equal(got[0] & LOW, dn.indices(r).astype(np.uint64))
                assert st["survivors_after"] == st["survivors_before"] + st["added"] - st["removed"] == int(got[1].size)
                assert int(got[1].sum()) == st["added"]
                if op in ("and", "andnot"):
                    assert st["added"] == 0
    with pytest.raises(ValueError):
        sn.combine_sets(a, b, "nor")


def fx_bounds():
    from voxcarve import DEFAULT_BOUNDS
    return DEFAULT_BOUNDS


def test_set_identities():
    rng = np.random.default_rng(5)
    grid = (6, 9, 5)
    a, ra = _random_hull(rng, grid, 0.45)
    b, rb = _random_hull(rng, grid, 0.55)
    and_, or_, xor, andnot = (sn.combine_sets(a, b, op) for op in ("and", "or", "xor", "andnot"))
    assert np.array_equal(and_ | xor, or_) and not (and_ & xor).any()
    assert np.array_equal(andnot | and_, a) and not (andnot & and_).any()
    # COPY from records is B verbatim, whatever A holds; added marks what A did not have
    out, added, r, st = sn.combine(ra, a, b, rb, "copy", grid, fx_bounds())
    assert np.array_equal(out, rb) and np.array_equal(r, b)
    assert np.array_equal(added.astype(bool), ~a.reshape(-1)[(rb & LOW).astype(np.int64)])
    # OR from records: A's bytes where A was, B's elsewhere
    out, added, r, st = sn.combine(ra, a, b, rb, "or", grid, fx_bounds())
    assert np.array_equal(out[added == 0], ra) and np.array_equal(out[added == 1], rb[~a.reshape(-1)[(rb & LOW).astype(np.int64)]])
    # without records and without a colour camera a fresh record is its index
    out, added, r, st = sn.combine(ra, a, b, None, "xor", grid, fx_bounds())
    assert np.array_equal(out[added == 1], dn.indices(b & ~a).astype(np.uint64)) and np.array_equal(out[added == 0], ra[~b.reshape(-1)[(ra & LOW).astype(np.int64)]])


@pytest.mark.parametrize("grid,seed", [((5, 7, 3), 1), ((4, 6, 5), 2)])
def test_compare_literal_equals_vectorised(grid, seed):
    rng = np.random.default_rng(seed)
    q = dn.steps_um(grid, (0.0, 400.0, -300.0, 300.0, 10.0, 310.0))       # anisotropic steps
    for pa, pb in ((0.3, 0.3), (0.0, 0.3), (0.3, 0.0), (0.0, 0.0), (0.9, 0.05)):
        a, _ = _random_hull(rng, grid, pa)
        b, _ = _random_hull(rng, grid, pb)
        assert sn.compare(a, b, q) == sn.compare_literal(a, b, q), (pa, pb)
    st = sn.compare(a, a, q)
    assert st["only_a"] == st["only_b"] == st["h2_ab"] == st["h2_ba"] == 0 and st["diff_lo"] == (sn.U32_MAX,) * 3 and st["diff_hi"] == (0, 0, 0)
    assert st["arg_ab"] == st["arg_ba"] == sn.U32_MAX
    assert sn.derived(st)["iou"] == 1.0 and sn.derived(st)["hausdorff_mm"] == 0.0
    empty = np.zeros_like(a)
    st = sn.compare(a, empty, q)
    assert st["h2_ab"] == sn.U64_MAX and st["arg_ab"] == int(dn.indices(a)[0]) and st["h2_ba"] == 0 and st["arg_ba"] == sn.U32_MAX
    assert sn.derived(st) == {"iou": 0.0, "dice": 0.0, "hausdorff_mm": None}
    assert sn.derived(sn.compare(empty, empty, q)) == {"iou": None, "dice": None, "hausdorff_mm": None}
    assert "h2_ab" not in sn.compare(a, b)


def test_hullio_operands():
    from voxcarve import hullio
    n = 100
    occ = np.zeros(n, dtype=bool)
    occ[[0, 5, 63, 64, 99]] = True
    kind, bits = hullio.as_operand(occ, n)
    assert kind == "bits" and bits.dtype == np.uint8 and bits.size == 16
    assert np.array_equal(np.unpackbits(bits, bitorder="little")[:n].astype(bool), occ) and not np.unpackbits(bits, bitorder="little")[n:].any()
    kind2, bits2 = hullio.as_operand(occ.reshape(4, 25), n)                  # a volume of the right size is flattened
    assert kind2 == "bits" and np.array_equal(bits2, bits)
    kind3, bits3 = hullio.as_operand(np.array([0, 5, 63, 64, 99], dtype=np.uint32), n)
    assert kind3 == "bits" and np.array_equal(bits3, bits)
    rec = np.array([0, 5, 63, 64, 99], dtype=np.uint64) | (np.uint64(0x01a0b0c0) << np.uint64(32))
    kind4, out = hullio.as_operand(rec, n)
    assert kind4 == "records" and out.dtype == np.uint64 and np.array_equal(out, rec)
    assert hullio.as_operand(np.empty(0, np.uint64), n)[0] == "records"
    assert hullio.as_operand(np.empty(0, np.uint32), n)[0] == "bits"
    for bad in (np.zeros(n + 1, dtype=bool), np.zeros(n - 1, dtype=bool),                  # wrong size
                np.array([5, 3], dtype=np.uint32), np.array([5, 3], dtype=np.uint64),      # descending
                np.array([3, 3], dtype=np.uint32), np.array([3, 3 | (1 << 40)], dtype=np.uint64),   # duplicates
                np.array([3, n], dtype=np.uint32), np.array([3, n], dtype=np.uint64),      # at or beyond n
                np.array([1, 2], dtype=np.int64), np.array([1.0]), np.zeros((2, 2), dtype=np.uint32)):
        with pytest.raises(ValueError):
            hullio.as_operand(bad, n)


def test_hullio_round_trip(tmp_path):
    from voxcarve import hullio
    grid, bounds = (5, 7, 3), (-1.0, 2.5, 0.0, 10.0, -3.0, 3.0)
    rng = np.random.default_rng(3)
    _, rec = _random_hull(rng, grid, 0.4)
    path = os.path.join(str(tmp_path), "hull.npz")
    hullio.save(path, grid, bounds, rec)
    assert os.path.exists(path)
    g, b, r = hullio.load(path)
    assert g == grid and b == bounds and r.dtype == np.uint64 and np.array_equal(r, rec)
    with pytest.raises(ValueError):
        hullio.save(path, grid, bounds, rec[::-1])
    with pytest.raises(ValueError):
        hullio.save(path, (2, 2, 2), bounds, rec)


def test_abi_surface():
    from voxcarve import _lib
    header = open(os.path.join(fx.ROOT, "include", "voxcarve.h")).read()
    for line in ("int vc_hull_keep(vc_ctx *ctx, uint32_t reg);",
                 "int vc_hull_upload(vc_ctx *ctx, uint32_t reg, const uint8_t *bits, const uint64_t *records, uint64_t n_records);",
                 "int vc_hull_release(vc_ctx *ctx, uint32_t reg);",
                 "int vc_fetch_kept(vc_ctx *ctx, uint32_t reg, uint8_t *bits /* NULL ok */, uint64_t *records /* NULL ok */, uint64_t *count, "
                 "uint32_t *has_records);",
                 "int vc_hull_combine(vc_ctx *ctx, uint32_t op, uint32_t reg, uint32_t flags /* must be 0 */, vc_setop_stats_t *stats);",
                 "int vc_fetch_combined(vc_ctx *ctx, uint8_t *added);",
                 "int vc_hull_compare(vc_ctx *ctx, uint32_t reg, uint32_t flags, vc_compare_stats_t *stats);",
                 "#define VC_HULL_REGISTERS 4", "#define VC_SETOP_COPY   0u", "#define VC_SETOP_AND    1u", "#define VC_SETOP_OR     2u",
                 "#define VC_SETOP_ANDNOT 3u", "#define VC_SETOP_XOR    4u", "#define VC_COMPARE_DISTANCE 1u",
                 "#define VC_KERNEL_KINDS 28", "#define VC_WORK_KINDS 10"):
        assert line in header, line
    assert _lib.VC_KERNEL_KINDS == 28 and len(_lib.KERNEL_KINDS) == 28 and _lib.VC_WORK_KINDS == 10
    assert (_lib.VC_SETOP_COPY, _lib.VC_SETOP_AND, _lib.VC_SETOP_OR, _lib.VC_SETOP_ANDNOT, _lib.VC_SETOP_XOR) == (0, 1, 2, 3, 4)
    assert _lib.VC_HULL_REGISTERS == 4 and _lib.VC_COMPARE_DISTANCE == 1
    for name, nargs in (("vc_hull_keep", 2), ("vc_hull_upload", 5), ("vc_hull_release", 2), ("vc_fetch_kept", 6), ("vc_hull_combine", 5),
                        ("vc_fetch_combined", 2), ("vc_hull_compare", 4)):
        assert name in _lib.SIGNATURES and len(_lib.SIGNATURES[name][1]) == nargs, name
    assert [f for f, _ in _lib.VcSetopStats._fields_] == ["survivors_before", "other", "common", "survivors_after", "added", "removed", "setop_ms"]
    assert [f for f, _ in _lib.VcCompareStats._fields_] == ["a", "b", "common", "only_a", "only_b", "diff_lo", "diff_hi", "h2_ab", "h2_ba",
                                                            "arg_ab", "arg_ba", "q", "compare_ms"]
    import ctypes
    assert ctypes.sizeof(_lib.VcSetopStats) == 56 and ctypes.sizeof(_lib.VcCompareStats) == 120
    from voxcarve import CarveEngine
    assert sorted(CarveEngine.SETOPS) == sorted(sn.OPS)
    for method in ("keep_hull", "upload_hull", "release_hull", "fetch_kept", "combine_hull", "fetch_combined", "compare_hull", "save_hull",
                   "load_hull", "set_hull"):
        assert callable(getattr(CarveEngine, method))


def test_configure_checks_the_operands():
    from voxcarve import assignment
    try:
        for bad in (5, [1, 2], (True,)):
            with pytest.raises(ValueError):
                assignment.configure(hull_subtract=bad)
            with pytest.raises(ValueError):
                assignment.configure(hull_clip=bad)
        assignment.configure(hull_subtract=np.zeros(8, dtype=bool), hull_clip="somewhere.npz")
        with pytest.raises(RuntimeError):
            assignment.hull_ops()
    finally:
        assignment.configure(hull_subtract=None, hull_clip=None)
