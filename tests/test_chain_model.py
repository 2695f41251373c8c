"""tests/chain_model.py without a GPU: the chains that tests/test_gpu_chain.py walks are not hollow, and the model agrees with itself.

The coverage conditions below are conditions on the INPUTS of the GPU test (chain_model.SEEDS, the draw weights), asserted here so that
it cannot pass by doing nothing; where one fails, the seeds or the weights change, never the thresholds.  Then: the scene's three
frame sets differ, the chains and replay() are deterministic, the literal twin of every restatement that has an affordable one gives
the model's bytes at states the chains reach, and one deliberately wrong model -- a mistake of the kind the chains exist to catch --
is told apart from the right one by the records alone.

Not run here: footprint_np.carve_literal, whose loop over every pixel of every voxel's box takes minutes at the chains' grids
(tests/test_footprint_restatement.py holds it to the vectorised form on its own grids)."""
import collections

import numpy as np
import pytest

import chain_model as cm
import closing_np as cl
import distance_np as dn
import surface_np as sn
from oracle import carve_c, carve_np


@pytest.fixture(scope="module")
def traces():
    return {seed: cm.trace(seed) for seed in cm.SEEDS}


def test_seed_list():
    assert len(cm.SEEDS) == len(set(cm.SEEDS)) == 24 and cm.CHAIN_LEN == 10
    assert set(cm.PRODUCTS) == set(cm.REFUSAL) | cm.BUILT          # (the product names of test_gpu_result_generation, imported)


def test_the_three_frame_sets_differ():
    """Different hulls and different colours per slot, on every grid: a pass that took the wrong slot changes the bytes."""
    for grid in cm.GRIDS:
        sc = cm.scene(grid)
        recs = [sc.carve_records(slot, sc.C, 1) for slot in range(3)]
        idx = [set(cm.index_of(r).tolist()) for r in recs]
        for a, b in ((0, 1), (0, 2), (1, 2)):
            assert len(idx[a] ^ idx[b]) > 100 and len(idx[a] & idx[b]) > 100, (grid, a, b)
            both = np.intersect1d(cm.index_of(recs[a]), cm.index_of(recs[b]))
            ca = cm.rgb_of(recs[a])[np.searchsorted(cm.index_of(recs[a]), both)]
            cb = cm.rgb_of(recs[b])[np.searchsorted(cm.index_of(recs[b]), both)]
            assert (ca != cb).any(axis=1).mean() > 0.9, (grid, a, b)
        assert all(1000 <= len(i) <= 8000 for i in idx), (grid, [len(i) for i in idx])
        assert all((sc.frames[s][c] is not None) == (c in cm.SLOT_IMAGES[s]) for s in range(3) for c in range(sc.C))


def test_the_two_carve_oracles_agree_on_the_scenes():
    """oracle.carve_np (vectorised numpy) and oracle.carve_c (the model's, for its speed): the same records on every frame set."""
    for grid in cm.GRIDS:
        sc = cm.scene(grid)
        for slot, mv, cc in ((0, 4, 1), (1, 3, 2), (2, 3, 1)):
            w = carve_np.carve(*grid, sc.oc, sc.masks[slot], sc.frames[slot], bounds=sc.bounds, min_views=mv, color_cam=cc)
            rec = cm.pack(w["idx"], w["bgr"][:, ::-1], w["color_seen"])
            assert np.array_equal(rec, sc.carve_records(slot, mv, cc)), (grid, slot, mv, cc)
            c = carve_c.carve(*grid, sc.oc, sc.masks[slot], sc.frames[slot], bounds=sc.bounds, min_views=mv, color_cam=cc)
            assert np.array_equal(c["idx"], w["idx"])


def test_coverage_of_the_chains(traces):
    """What the 24 chains exercise; test_gpu_chain.py walks exactly these."""
    ran = collections.Counter()                  # operation kind -> runs on a non-empty hull
    changed = collections.Counter()              # hull-changing kind -> runs that changed the hull
    slots = collections.Counter()
    through_empty = rows_of_three = pipelined = other_slot = seen0 = painted = 0
    for seed, rows in traces.items():
        assert len(rows) == cm.CHAIN_LEN and rows[0]["op"] == "carve"
        row_len = best = 0
        went_empty = carried_seen0 = carried_paint = False
        for k, r in enumerate(rows):
            if r["op"] == "carve":
                slots[r["params"]["slot"]] += 1
                pipelined += r["params"]["first"] is not None
                ran["carve"] += r["after"] > 0
            elif r["before"] > 0:
                ran[r["op"]] += 1
            if r["changed"]:
                assert r["op"] in cm.HULL_CHANGERS
                changed[r["op"]] += 1
            row_len = row_len + 1 if r["changed"] else 0     # consecutive passes that each changed the hull: nothing in between
            best = max(best, row_len)
            went_empty |= r["op"] != "carve" and r["before"] > 0 and r["after"] == 0 and k + 1 < len(rows)
            other_slot += r["op"] in cm.COLOUR_PASSES and r["params"]["slot"] != r["carve_slot"]
            if r["op"] in cm.HULL_CHANGERS and r["before"] > 0:
                carried_seen0 |= r["seen0"]
                carried_paint |= r["painted"]
        through_empty += went_empty
        rows_of_three += best >= 3
        seen0 += carried_seen0
        painted += carried_paint
    counts = {k: ran[k] for k in cm.KINDS}
    print("operations on a non-empty hull:", counts)
    print("hull changes:", {k: changed[k] for k in cm.HULL_CHANGERS})
    print("carves per slot:", dict(slots), "pipelined:", pipelined, "through the empty hull:", through_empty,
          "three changes in a row:", rows_of_three, "colour passes on another slot:", other_slot, "seen == 0 carried:", seen0,
          "painted colours carried:", painted)
    assert all(counts[k] >= 8 for k in cm.KINDS), counts
    assert all(changed[k] >= 8 for k in cm.HULL_CHANGERS), dict(changed)
    assert through_empty >= 4
    assert rows_of_three >= 12
    assert all(slots[s] >= 4 for s in range(3)), dict(slots)
    assert pipelined >= 6
    assert other_slot >= 6
    assert seen0 >= 6
    assert painted >= 6


def test_chains_and_replay_are_deterministic(traces):
    for seed in cm.SEEDS[:3]:
        sc, ops = cm.draw_chain(seed)
        sc2, ops2 = cm._draw_chain(seed)                         # (drawn again, past the cache)
        assert sc2 is sc and [cm.describe_op(o) for o in ops2] == [cm.describe_op(o) for o in ops]
        assert all(np.array_equal(a.get("palette"), b.get("palette")) for a, b in zip(ops, ops2))
        a, b = cm.replay(seed), cm.replay(seed)
        assert np.array_equal(a.records, b.records) and a.products == b.products and a.carve == b.carve
        for upto in (1, 4, 7):
            m = cm.replay(seed, upto=upto)
            assert cm.hashlib.sha1(m.records.tobytes()).hexdigest() == traces[seed][upto - 1]["digest"], (seed, upto)


def _smallest_state(traces, kind, at_least=200):
    """(seed, step) of the run of `kind` on the fewest records (but at_least) among all chains."""
    found = [(r["before"], seed, r["step"]) for seed, rows in traces.items() for r in rows if r["op"] == kind and r["before"] >= at_least]
    assert found, kind
    return min(found)[1:]


@pytest.mark.parametrize("kind", ["filter_components", "color_visible", "photo_carve", "clusters", "geodesic", "hull_normals"])
def test_literal_twins_give_the_models_bytes(traces, kind):
    """The pass applied to a state a chain reaches, by the vectorised form and by its literal twin: equal records and products."""
    seed, step = _smallest_state(traces, kind)
    op = cm.draw_chain(seed)[1][step]
    if kind == "photo_carve":
        op = dict(op, max_rounds=1)                              # (the twin projects point by point: one round, then the colouring)
    a, b = cm.replay(seed, upto=step), cm.replay(seed, upto=step)
    b.literal = True
    out_a, out_b = a.apply(op), b.apply(op)
    assert np.array_equal(a.records, b.records), (seed, step, cm.describe_op(op))
    assert a.products == b.products
    assert out_a["survivors"] == out_b["survivors"] and out_a.get("stats") == out_b.get("stats")


def test_literal_twins_of_the_morphology_on_a_window(traces):
    """closing_np and distance_np's literal forms loop over all pairs of voxels: they run on a window of a hull the chains reach,
    cut around its centre of mass, against the separable forms the model uses (whole-grid and box forms)."""
    seed, step = _smallest_state(traces, "close", at_least=1000)
    m = cm.replay(seed, upto=step)
    occ, q = m.occ(), m.scene.q
    c = [int(round(v)) for v in np.argwhere(occ).mean(axis=0)]
    half = (4, 5, 6)
    win = np.ascontiguousarray(occ[tuple(slice(max(c[a] - half[a], 0), c[a] + half[a]) for a in range(3))])
    assert 50 < win.sum() < win.size - 50
    for factor in ("below", 1):
        r2 = dn.radius_r2(m.scene.mm(factor))
        dl = cl.dilate_literal(win, q, r2)
        assert np.array_equal(dl, cl.dilate(win, q, r2)) and np.array_equal(dl, cl.dilate_box(win, q, r2))
        cs = cl.close_literal(win, q, r2)
        assert np.array_equal(cs, cl.close_(win, q, r2)[0]) and np.array_equal(cs, cl.close_box(win, q, r2)[0])
        for border in dn.BORDERS:
            assert np.array_equal(dn.erode_literal(win, q, r2 // 16, border), dn.erode(win, q, r2 // 16, border))
            assert np.array_equal(dn.open_literal(win, q, r2 // 16, border), dn.open_(win, q, r2 // 16, border)[0])


def test_literal_twin_of_the_surface_refinement(traces):
    seed, step = _smallest_state(traces, "surface_mesh")
    m = cm.replay(seed, upto=step)
    op = cm.draw_chain(seed)[1][step]
    sc = m.scene
    masks = np.stack([x > 0 for x in sc.masks[m.carve["slot"]]])
    want = m.apply(op)["mesh"]
    pick = np.linspace(0, want["verts"].shape[0] - 1, 60).astype(np.int64)
    verts, refined = sn.refine_literal(m.occ().reshape(-1), m.grid, m.bounds, sc.oc, masks, m.min_views(), op["refine_steps"], vertices=pick)
    assert np.array_equal(verts.view(np.uint64), want["verts"][pick].view(np.uint64)) and np.array_equal(refined, want["refined"][pick])


@pytest.mark.parametrize("fault", ["grow_slot0", "drop_paint"])
def test_a_wrong_model_is_told_apart(traces, fault):
    """The chains are not hollow: a model that colours added voxels from slot 0 instead of the carve's slot, or that loses the
    painted colours at a compaction, gives other records than the right one in at least one chain -- the comparison of
    tests/test_gpu_chain.py, fed on the CPU."""
    told = []
    for seed in cm.SEEDS:
        for step, op, out, model in cm.run(seed, fault):
            if cm.hashlib.sha1(model.records.tobytes()).hexdigest() != traces[seed][step]["digest"]:
                told.append((seed, step, op["op"]))
                break
        if len(told) >= 3:
            break
    print("%s told apart at (seed, step, op):" % fault, told)
    assert told, "no chain tells the %s model from the right one" % fault
