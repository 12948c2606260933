"""CPU suite: the degenerate match families and kernel inputs of tests/mono_content.py.  Every family reaches the
condition it is named for; the oracle's monocular egomotion equals the reference's on them (live in a fresh process where
oracle/_ref is built, and against tests/golden/mono_content.npz recorded from it); the product's host path equals the
oracle's; the oracle's per-piece exports (inlier count, triangulation, plane vote) are consistent with its whole estimate."""
import os
import subprocess
import sys

import numpy as np
import pytest

import mono_content as MC
from conftest import pkg

HERE = os.path.dirname(os.path.abspath(__file__))


def _golden():
    return np.load(os.path.join(HERE, "golden", "mono_content.npz"))


@pytest.fixture(scope="module")
def oracle_results(B):
    return MC.replay(B.OracleMonoVO, B.oracle_sampler_seed, after=lambda vo: B.oracle_mono_last_in_front())


# ---- the families are what they claim -------------------------------------------------------------------------------------

def test_families_reach_their_conditions():
    fam = {name: MC.matches(name) for name in MC.FAMILIES}
    assert all(10 <= len(m) <= 700 for m in fam.values())
    s = fam["stationary"]
    assert np.array_equal(s["u1c"], s["u1p"]) and np.array_equal(s["v1c"], s["v1p"])
    so = fam["stationary_outliers"]
    assert int(np.sum((so["u1c"] != so["u1p"]) | (so["v1c"] != so["v1p"]))) == 30
    for k in ("u1p", "v1p", "u1c", "v1c"):
        assert np.array_equal(fam["integer"][k], np.rint(fam["integer"][k]))
        h2 = fam["half_pixel"][k] * 2
        assert np.array_equal(h2, np.rint(h2)) and np.any(h2 % 2 == 1)
    assert len(np.unique(MC.points_of(fam["repeated"]), axis=0)) == 40
    assert len(set(fam["one_row"]["v1p"]) | set(fam["one_row"]["v1c"])) == 1
    assert set(fam["one_column"]["u1p"]) | set(fam["one_column"]["u1c"]) == {np.float32(MC.CU)}
    for name in ("dup10", "dup12"):
        assert len(fam[name]) == int(name[3:]) and len(np.unique(MC.points_of(fam[name]), axis=0)) == 6
    # a rank below 8 of ALL rows: no sample of 8 can have more
    for name in MC.RANK_DEFICIENT:
        assert MC.rank(MC.constraint_matrix(MC.normalised(fam[name]))) < 8, name
    # pure rotation: x2 = H x1, a three-dimensional null space up to the float rounding of the coordinates
    sv = np.linalg.svd(MC.constraint_matrix(MC.normalised(fam["pure_rotation"])), compute_uv=False)
    assert sv[6] < 1e-5 * sv[0] and sv[5] > 1e-3 * sv[0]
    assert MC.rank(MC.constraint_matrix(MC.normalised(fam["control"]))) == 9


def test_points_in_front_and_the_vote_threshold(oracle_results):
    """which families have the 512 points in front of the camera from which the vote runs on the device; the pair that
    straddles the threshold hits 511 and 512 exactly"""
    front = {name: r[3] for name, r in oracle_results.items()}
    on_device = tuple(n for n in MC.FAMILIES if oracle_results[n][0] and front[n] >= MC.VOTE_MIN_POINTS)
    assert set(on_device) == set(MC.VOTE_ON_DEVICE), front
    assert front["front511"] == 511 and front["front512"] == 512
    assert oracle_results["front511"][0] and oracle_results["front512"][0]
    assert len([n for n in on_device if not n.startswith("front")]) >= 2


def test_fit_inputs_have_their_properties():
    for K in (1, 15, 16, 17, 33, 200):
        pts, picks, props = MC.fit_inputs(K)
        assert picks.min() >= 0 and picks.max() < len(pts)
        for k in range(K):
            assert MC.has_property(MC.constraint_matrix(pts, picks[k]), props[k]), (K, k, props[k])
        for w in range(0, K, 4):     # the hypotheses of one 64-lane wave of k_mono_fit
            if min(K, w + 4) - w >= 2:
                assert len(set(props[w:w + 4])) >= 2, (K, w)
    assert set(props) == set(MC.FIT_PROPERTIES)
    r = np.abs(MC.fit_points()).reshape(len(MC.FIT_SCALES), -1).max(axis=1)
    assert r[0] < 1e-2 and r[-1] > 1e3


# ---- oracle = reference ---------------------------------------------------------------------------------------------------

_LIVE = r"""
import sys, numpy as np
sys.path.insert(0, {root!r}); sys.path.insert(0, {tests!r})
from oracle import bindings as B
import mono_content as MC
bad = 0
for name in MC.FAMILIES:
    m = MC.matches(name)
    a = B.RefMonoVO(MC.F, MC.CU, MC.CV, **MC.PARAMS); b = B.OracleMonoVO(MC.F, MC.CU, MC.CV, **MC.PARAMS)
    ra = a.process_matches(m); rb = b.process_matches(m)
    if not (ra[0] == rb[0] and ra[1].tobytes() == rb[1].tobytes() and np.array_equal(a.inliers(), b.inliers())):
        bad += 1; print("DIFF", name, ra[0], rb[0], len(a.inliers()), len(b.inliers()))
    a.close(); b.close()
print("RESULT", bad)
"""


def test_oracle_vs_reference_live(B, have_ref):
    if not have_ref:
        pytest.skip("oracle/_ref not built (needs the reference's sources)")
    code = _LIVE.format(root=os.path.dirname(HERE), tests=HERE)
    out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-2000:]
    assert "RESULT 0" in out.stdout, out.stdout[-3000:]


def test_oracle_vs_golden(oracle_results):
    MC.assert_equals_golden(oracle_results, _golden())


@pytest.mark.parametrize("threads", [1, 4])
def test_host_path_vs_oracle(oracle_results, threads):
    from test_host_mono import HostMonoVO
    vm = pkg("visomatch")
    got = MC.replay(lambda *a, **k: HostMonoVO(vm, threads, *a, **k), vm.vo_sampler_seed)
    for name in MC.FAMILIES:
        ok, T, inl, _ = got[name]
        ok_o, T_o, inl_o, _ = oracle_results[name]
        assert ok == ok_o and np.array_equal(inl, inl_o), name
        if ok:   # (a failed estimate leaves the identity in both)
            assert T.tobytes() == T_o.tobytes(), name


# ---- the oracle's per-piece exports -----------------------------------------------------------------------------------------

def test_oracle_pieces(B):
    # the count is the length of the inlier list the whole estimate reports for its winner
    pts, Fm, thr = MC.edge_threshold(B)
    m = MC.as_matches(pts)
    assert 0 < thr < 1
    below, at, above = (B.oracle_mono_inlier_count(m, Fm, t) for t in (np.nextafter(thr, 0), thr, np.nextafter(thr, 1)))
    assert below == at and above > at     # the distance of point 5 IS thr: `<` excludes it, the next double admits it
    assert B.oracle_mono_inlier_count(m, np.zeros((3, 3)), 1.0) == 0       # 0 / 0
    assert B.oracle_mono_inlier_count(m, MC.HUGE_F, 1.0) == 0              # inf / inf
    # triangulation: a clean scene lies in front of exactly one of the four candidates
    R4, t4 = MC.rt_candidates()
    tm = MC.triangulation_matches(65)
    chir = [B.oracle_mono_triangulate(tm, MC.F, MC.CU, MC.CV, R4[c], t4[c])[1] for c in range(4)]
    assert max(chir) > 40 and sorted(chir)[-2] < 20, chir
    # vote: ties exist where the input is built for them, and the first wins
    d, threshold, weight = MC.vote_inputs("grid_ties", 513)
    sums, idx = B.oracle_mono_plane_vote(d, threshold, weight)
    assert int(np.sum(sums == sums.max())) >= 2 and idx == int(np.argmax(sums)) and idx > 0
    assert B.oracle_mono_plane_vote(*MC.vote_inputs("none_above", 512))[1] == 0
    sums, idx = B.oracle_mono_plane_vote(*MC.vote_inputs("huge_weight", 512))
    assert set(np.unique(sums)) <= {0.0, 1.0, 2.0, 3.0} and sums.max() == 3.0 and idx == int(np.argmax(sums))
    sums, idx = B.oracle_mono_plane_vote(*MC.vote_inputs("all_equal", 512))
    assert np.all(sums == 512.0) and idx == 0
