"""CPU suite: the exact Delaunay, removeOutliers and the prior boxes on point sets that reach the 14-bit coordinate limit
(frames up to 16383 px a side, tests/fullrange.py): the oracle's Delaunay against the reference's Triangle, the product's
host Delaunay (whole and split) and its host removeOutliers (plain and on fork-join threads) against the oracle's and,
where its build is present, the reference's; the prior boxes of the plain and the threaded form against each other."""
import numpy as np
import pytest

import fullrange as FR
from conftest import pkg


def _same(a, b):
    return len(a) == len(b) and a.tobytes() == b.tobytes()


def _oracle_tris(B, p):
    return FR.canon(B.delaunay("oracle", p.astype(np.float32)))


@pytest.mark.parametrize("w,h", FR.EXTENTS)
def test_oracle_delaunay_equals_triangle(B, w, h):
    if not B.have_ref():
        pytest.skip("oracle/_ref not built")
    for name, p in FR.point_sets(w, h, seed=w ^ h):
        if len(np.unique(p, axis=0)) < 2:
            continue
        assert np.array_equal(_oracle_tris(B, p), FR.canon(B.delaunay("ref", p.astype(np.float32)))), (w, h, name)


@pytest.mark.parametrize("w,h", FR.EXTENTS)
def test_host_delaunay_equals_oracle(B, w, h):
    vm = pkg("visomatch")
    for name, p in FR.point_sets(w, h, seed=w ^ h):
        want = _oracle_tris(B, p)
        for threads in (1, 8):
            assert np.array_equal(want, FR.canon(vm.host_delaunay(p, threads=threads))), (w, h, name, threads)
        for leaf, top in ((3, 0), (56, 480), (480, -1)):
            assert np.array_equal(want, FR.canon(vm.host_delaunay_split(p, leaf, top))), (w, h, name, leaf, top)


@pytest.mark.parametrize("w,h", FR.EXTENTS)
def test_host_remove_outliers_equals_oracle(B, w, h):
    """survivors byte for byte for all three methods, plain and on eight fork-join threads; the prior boxes of the two forms
    equal (the stage goldens pin the plain form's)"""
    vm = pkg("visomatch")
    for name, lst in FR.match_lists(vm, w, h, seed=w ^ h):
        for method in (0, 1, 2):
            want = B.remove_outliers("oracle", lst, method)
            plain, rg1, _ = vm.remove_outliers(lst, method, w, h)
            got, rg8, _ = vm.remove_outliers(lst, method, w, h, threads=8)
            assert _same(want, plain), (w, h, name, method, len(want), len(plain))
            assert _same(want, got), (w, h, name, method, len(want), len(got))
            assert np.array_equal(rg1, rg8), (w, h, name, method)


@pytest.mark.parametrize("w,h", FR.EXTENTS)
def test_host_remove_outliers_equals_reference(B, w, h):
    if not B.have_ref():
        pytest.skip("oracle/_ref not built")
    vm = pkg("visomatch")
    for name, lst in FR.match_lists(vm, w, h, seed=w ^ h):
        if FR.one_pixel_only(lst):
            continue
        assert _same(B.remove_outliers("ref", lst, 2), vm.remove_outliers(lst, 2, w, h, threads=8)[0]), (w, h, name)


def test_point_families_reach_the_limits():
    """the generators do what the tests above rely on: coordinates at 0 and at 16382 (bits 12 and 13 of x and y set),
    exactly cocircular lattice points, rows whose circumcircles leave the signed 16-bit range"""
    c = FR.circle_7735()
    assert np.all((c[:, 0] - 8191) ** 2 + (c[:, 1] - 8191) ** 2 == 7735 ** 2)
    allp = np.concatenate([p for _, p in FR.point_sets(16383, 16383, seed=1)])
    assert allp.min() == 0 and allp[:, 0].max() == 16382 and allp[:, 1].max() == 16382
    assert np.any(allp[:, 0] & 0x3000 == 0x3000) and np.any(allp[:, 1] & 0x3000 == 0x3000)
    r = FR.rows(16383, 64, 1).astype(float)
    (ax, ay), (bx, by), (cx, cy) = r[0], r[1], r[3]
    d = 2 * (ax * (by - cy) + bx * (cy - ay) + cx * (ay - by))
    ux = ((ax ** 2 + ay ** 2) * (by - cy) + (bx ** 2 + by ** 2) * (cy - ay) + (cx ** 2 + cy ** 2) * (ay - by)) / d
    uy = ((ax ** 2 + ay ** 2) * (cx - bx) + (bx ** 2 + by ** 2) * (ax - cx) + (cx ** 2 + cy ** 2) * (bx - ax)) / d
    assert np.hypot(ux - ax, uy - ay) > 32767
