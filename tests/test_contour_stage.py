"""The contour stage of extract_foreground_mask (background_subtraction.py:171-193) without a GPU: the literal restatement of
cv2's border following / fill / draw (contour_literal) checked on masks with known answers, and the component formulation the
device implements (contour_components, csrc/vc_contour.h) held to it on random masks."""
import numpy as np
import pytest

import contour_components as cc
import contour_literal as lit
import contour_masks as cm


def _rect(h, w, H=12, W=14, y=2, x=3):
    m = np.zeros((H, W), np.uint8)
    m[y:y + h, x:x + w] = 255
    return m


@pytest.mark.parametrize("h,w", [(4, 6), (2, 2), (1, 5), (7, 3)])
def test_rectangle_area_and_outer_sign(h, w):
    contours, hier, holes = lit.find_contours_tree(_rect(h, w))
    assert len(contours) == 1 and not holes[0] and tuple(hier[0]) == (-1, -1, -1, -1)
    assert lit.contour_area(contours[0]) == (w - 1) * (h - 1)
    if h > 1 and w > 1:
        assert lit.contour_area(contours[0], True) == -(w - 1) * (h - 1)


def test_hole_areas_are_positive():
    m = _rect(3, 3)
    m[3, 4] = 0
    contours, hier, holes = lit.find_contours_tree(m)
    assert holes == [False, True] and hier[1][3] == 0 and hier[0][2] == 1
    assert lit.contour_area(contours[0], True) == -4 and lit.contour_area(contours[1], True) == 2
    m = _rect(3, 4)
    m[3, 4:6] = 0
    contours, _, _ = lit.find_contours_tree(m)
    assert lit.contour_area(contours[1], True) == 4


def test_nested_rings_depth():
    m = cm.rings(6)                                          # 6 fg rings + 6 holes: 12 levels below the frame
    contours, hier, holes = lit.find_contours_tree(m)
    assert len(contours) == 12
    depth, k = 0, len(contours) - 1
    while k != -1:
        k = hier[k][3]
        depth += 1
    assert depth == 12
    for T, t in cm.THRESHOLDS + [(10, 0), (30, 20), (0, -1e9), (100, 1e9)]:
        want = lit.fill_figures(m, T, t)
        assert np.array_equal(cc.fill_figures(m, T, t), want), (T, t)


def test_large_hole_is_refilled():
    m = _rect(30, 30, 40, 40, 5, 5)
    m[10:30, 10:30] = 0                                      # hole of area 19*19 + ... >= T: itself a figure
    out = lit.fill_figures(m, 100, 0)
    assert np.array_equal(out, _rect(30, 30, 40, 40, 5, 5))
    assert np.array_equal(cc.fill_figures(m, 100, 0), out)


def test_island_in_cleared_hole():
    m = _rect(30, 30, 40, 40, 5, 5)
    m[10:30, 10:30] = 0
    m[15:20, 15:20] = 255                                    # island, its area 16 < T
    out = lit.fill_figures(m, 500, 0)                        # outer 841 >= T, hole 441 < T and >= t: cleared, the island with it
    want = _rect(30, 30, 40, 40, 5, 5)
    want[10:30, 10:30] = 0
    assert np.array_equal(out, want)
    assert np.array_equal(cc.fill_figures(m, 500, 0), out)
    out2 = lit.fill_figures(m, 500, 1e9)                     # nothing passes the inner threshold: the whole square
    assert np.array_equal(out2, _rect(30, 30, 40, 40, 5, 5))


def test_masks_touching_the_edge():
    for m in (_rect(12, 14, 12, 14, 0, 0), _rect(5, 14, 12, 14, 0, 0), _rect(12, 3, 12, 14, 0, 11)):
        m = m.copy()
        m[m.shape[0] // 2, 1:-1] = 0 if m.shape[1] > 2 else m[m.shape[0] // 2, 1:-1]
        for T, t in cm.THRESHOLDS + [(5, 1), (5, -100)]:
            assert np.array_equal(cc.fill_figures(m, T, t), lit.fill_figures(m, T, t)), (T, t)


def test_fill_boundary_choice_does_not_matter():
    for m in cm.family(7, 60):
        for T, t in cm.THRESHOLDS + [(4, 1), (2, -3)]:
            assert np.array_equal(lit.fill_figures(m, T, t, boundary=True), lit.fill_figures(m, T, t, boundary=False)), (m.shape, T, t)


@pytest.mark.parametrize("seed", range(4))
def test_component_formulation_equals_literal(seed):
    for m in cm.family(100 + seed, 70):
        for T, t in cm.THRESHOLDS + [(8, 2), (3, -4)]:
            assert np.array_equal(cc.fill_figures(m, T, t), lit.fill_figures(m, T, t)), (m.shape, T, t)


def test_component_formulation_equals_literal_full_size():
    rng = np.random.default_rng(486)
    for m in (cm.blobs(rng, 486, 644, k=40), cm.mix(rng, 486, 644)):
        for T, t in cm.THRESHOLDS:
            assert np.array_equal(cc.fill_figures(m, T, t), lit.fill_figures(m, T, t)), (T, t)
