"""CPU suite: host_pairs_motions (vsm_host_pairs_motions) and chain_poses (vsm_chain_poses) - the batched monocular motions'
definition on host threads, no GPU.  Per pair the result equals vo_sampler_seed(71) + host_estimate_motion_mono on the same
list (rc, the bytes of tr6 / T16, the inliers); it depends neither on the thread count nor on the pairs' order, and leaves the
process-wide sampler where it was.  chain_poses equals its restatement in plain Python floats by its bytes.  The image
case of tests/test_motions_gpu.py is proven non-empty here, on the oracle's lists."""
import ctypes as C

import numpy as np
import pytest

import mono_content as MC
import motions_cases as MO
from conftest import pkg


@pytest.fixture(scope="module")
def vm():
    return pkg("visomatch")


@pytest.fixture(scope="module")
def results(vm):
    """every batch through the host view once, on 4 threads"""
    out = {}
    for name in MO.BATCHES:
        lists, par, bucket = MO.batch(name)
        out[name] = vm.host_pairs_motions(lists, par, bucket=bucket, threads=4)
    return out


def per_pair(vm, m, par):
    vm.vo_sampler_seed(71)
    return vm.host_estimate_motion_mono(m, par)


def assert_is_per_pair(vm, res, k, m, par, what):
    rc, tr, T, inl = per_pair(vm, m, par)
    assert res.rc[k] == rc, (what, k)
    assert (res.stage[k] == 6) == (rc == 1) and (res.stage[k] < 2) == (rc == -1), (what, k, res.stage[k])
    if rc == 1:
        assert res.tr[k].tobytes() == tr.tobytes() and res.T[k].tobytes() == T.tobytes(), (what, k)
    else:
        assert not res.tr[k].any() and np.array_equal(res.T[k], np.eye(4)), (what, k)
    assert np.array_equal(res.inliers(k), inl if rc >= 0 else np.zeros(0, np.int32)), (what, k)


@pytest.mark.parametrize("name", [n for n in MO.BATCHES if not MO.BATCHES[n][2]])
def test_equals_the_per_pair_estimate(vm, results, name):
    lists, par, _ = MO.batch(name)
    res = results[name]
    for k, m in enumerate(lists):
        assert res.matches(k).tobytes() == m.tobytes(), (name, k)
        assert_is_per_pair(vm, res, k, m, par, name)
    assert sum(res.stats.values()) == len(lists)


def test_families_equal_the_golden_file(vm, results):
    """every family as a pair of its own: a fresh sampler each, which is how golden/mono_content.npz was not recorded (one
    sampler ran through all families) - except for the first family, whose result must be the recorded one"""
    g = np.load(MC.os.path.join(MC.HERE, "golden", "mono_content.npz"))
    res, name = results["families"], MC.FAMILIES[0]
    assert bool(res.rc[0] == 1) == bool(g[name + "_ok"])
    assert np.array_equal(res.inliers(0), g[name + "_inliers"])
    assert res.T[0].tobytes() == g[name + "_T"].tobytes()


def test_the_stage_lists_end_where_they_say(results):
    names = MO.BATCHES["stages"][0]
    assert [int(s) for s in results["stages"].stage] == [MO.STAGES[n] for n in names]
    assert [int(r) for r in results["stages"].rc] == [-1, -1, 0, 0, 0, 1]
    assert len(results["stages"].inliers(0)) == 0 and len(results["stages"].inliers(1)) == 0
    assert 0 < len(results["stages"].inliers(2)) < 10
    # the 9 / 10 boundary, K = 0, the empty list
    assert int(results["sizes_small"].stage[0]) == 0 and int(results["sizes_small"].stage[1]) >= 2   # 10 matches enter the RANSAC
    assert all(int(s) == 2 for s in results["k0"].stage) and all(len(results["k0"].inliers(k)) == 0 for k in range(2))
    assert int(results["empty_between"].stage[1]) == 0 and int(results["empty_between"].rc[1]) == -1
    assert all(int(s) == 6 for s in results["front"].stage)


def test_front_lists_have_their_points_in_front(B):
    """511 / 512 / 513 points in front of the chosen camera pair (the oracle's count)"""
    for n in (511, 512, 513):
        B.oracle_sampler_seed(71)
        vo = B.OracleMonoVO(MC.F, MC.CU, MC.CV, **MC.PARAMS)
        ok, _ = vo.process_matches(MO.one(f"front{n}"))
        assert ok and B.oracle_mono_last_in_front() == n
        vo.close()


def test_the_same_list_twice(results):
    res = results["twice"]
    assert res.rc[0] == res.rc[2] == 1 and res.T[0].tobytes() == res.T[2].tobytes() and np.array_equal(res.inliers(0), res.inliers(2))


def test_bucketing(vm, results):
    """bucket=True: the list is what bucketing with a rand() stream seeded 0 keeps, the estimate is the per-pair one on it"""
    lists, par, _ = MO.batch("bucket")
    res = results["bucket"]
    removed = 0
    for k, m in enumerate(lists):
        kept = res.matches(k)
        assert len(kept) <= len(m)
        removed += len(m) - len(kept)
        whole = {x.tobytes() for x in m}
        assert all(x.tobytes() in whole for x in kept), k
        if len(kept):
            assert np.array_equal(res.inliers(k), res.inliers(k)[res.inliers(k) < len(kept)])
        assert_is_per_pair(vm, res, k, kept, par, "bucket")
    assert removed > 500   # the dense lists lose matches
    # the same lists in another order bucket the same: a stream per pair
    again = vm.host_pairs_motions(lists[::-1], par, bucket=True, threads=2)
    for k in range(len(lists)):
        assert again.matches(len(lists) - 1 - k).tobytes() == res.matches(k).tobytes(), k


def test_threads_and_order_do_not_matter(vm, results):
    lists, par, _ = MO.batch("seven")
    base = results["seven"]
    for threads in (1, 3, 16):
        MO.assert_same(vm.host_pairs_motions(lists, par, threads=threads), base, f"{threads} threads")
    order = [3, 6, 0, 5, 2, 1, 4]
    res = vm.host_pairs_motions([lists[i] for i in order], par, threads=4)
    for j, i in enumerate(order):
        assert res.rc[j] == base.rc[i] and res.stage[j] == base.stage[i] and res.T[j].tobytes() == base.T[i].tobytes()
        assert np.array_equal(res.inliers(j), base.inliers(i))


def test_the_process_wide_sampler_is_left_alone(vm):
    """draw from it - an estimate of the per-frame path - before and after a batch: the second estimate is what it is without
    the batch in between"""
    lists, par, _ = MO.batch("bucket")
    m = MO.one("control")
    vm.vo_sampler_seed(71)
    first = vm.host_estimate_motion_mono(m, par)
    second = vm.host_estimate_motion_mono(m, par)
    assert first[3].tobytes() != second[3].tobytes() or first[1].tobytes() != second[1].tobytes()   # the sampler has moved
    vm.vo_sampler_seed(71)
    vm.host_estimate_motion_mono(m, par)
    vm.host_pairs_motions(lists, par, bucket=True, threads=4)
    after = vm.host_estimate_motion_mono(m, par)
    assert after[0] == second[0] and after[1].tobytes() == second[1].tobytes() and np.array_equal(after[3], second[3])


# ---- chain_poses ------------------------------------------------------------------------------------------------------------

def _motions(n, seed=3):
    rs = np.random.RandomState(seed)
    out = np.zeros((n, 4, 4))
    for k in range(n):
        tr = np.concatenate([rs.uniform(-0.05, 0.05, 3), rs.uniform(-1, 1, 3)])
        rx, ry, rz = tr[:3]
        sx, cx, sy, cy, sz, cz = np.sin(rx), np.cos(rx), np.sin(ry), np.cos(ry), np.sin(rz), np.cos(rz)
        out[k] = np.array([[cy * cz, -cy * sz, sy, tr[3]], [sx * sy * cz + cx * sz, -sx * sy * sz + cx * cz, -sx * cy, tr[4]],
                           [-cx * sy * cz + sx * sz, cx * sy * sz + sx * cz, cx * cy, tr[5]], [0, 0, 0, 1]])
    return out


CHAINS = {
    # name: (frames, pairs, rc, root, frames that get a pose)
    "chain": (5, [(0, 1), (1, 2), (2, 3), (3, 4)], [1, 1, 1, 1], 0, 5),
    "failed_middle": (5, [(0, 1), (1, 2), (2, 3), (3, 4)], [1, 0, 1, 1], 0, 2),
    "failed_before_rc": (4, [(0, 1), (1, 2), (2, 3)], [1, -1, 1], 0, 2),
    "loop_closure": (4, [(0, 1), (1, 2), (2, 3), (3, 0), (0, 2)], [1, 1, 1, 1, 1], 0, 4),
    "reversed": (4, [(1, 0), (2, 1), (3, 2)], [1, 1, 1], 0, 4),
    "later_pairs_first": (4, [(2, 3), (1, 2), (0, 1)], [1, 1, 1], 0, 4),
    "root_in_the_middle": (5, [(0, 1), (1, 2), (2, 3), (3, 4)], [1, 1, 1, 1], 2, 5),
    "self_pair": (3, [(0, 0), (0, 1), (1, 1), (1, 2)], [1, 1, 1, 1], 0, 3),
    "skip_one_bridges": (5, [(0, 1), (1, 2), (2, 3), (3, 4), (0, 2), (2, 4)], [1, 0, 0, 1, 1, 1], 0, 5),
    "no_pairs": (3, [], [], 1, 1),
}


@pytest.mark.parametrize("name", sorted(CHAINS))
def test_chain_poses(vm, name):
    n, pairs, rc, root, posed = CHAINS[name]
    T = _motions(len(pairs))
    poses, valid, got = vm.chain_poses(n, pairs, T, rc, root=root)
    want_p, want_v = MO.chain_poses_ref(n, pairs, T, rc, root)
    assert got == posed == int(want_v.sum())
    assert valid.tobytes() == want_v.tobytes()
    assert poses.tobytes() == want_p.tobytes()
    assert np.array_equal(poses[root], np.eye(4)[:3].reshape(12))
    if name == "chain":   # the reference's accumulation: Tr_total = Tr_total * inv(motion)
        acc = np.eye(4)
        for k in range(4):
            acc = acc @ np.linalg.inv(T[k])
        assert np.allclose(poses[4].reshape(3, 4), acc[:3], atol=1e-12)
    if name == "root_in_the_middle":
        assert np.allclose(poses[1].reshape(3, 4), T[1][:3], atol=1e-15)
    if name == "failed_middle":
        assert valid.tolist() == [1, 1, 0, 0, 0] and not poses[2:].any()


def test_chain_poses_errors(vm):
    T = _motions(2)
    for n, pairs, root in ((3, [(0, 1), (1, 3)], 0), (3, [(0, 1), (-1, 2)], 0), (3, [(0, 1), (1, 2)], 3), (3, [(0, 1), (1, 2)], -1), (0, [(0, 1), (1, 2)], 0)):
        with pytest.raises(vm.VisoMatchError, match="VSM_EARG"):
            vm.chain_poses(n, pairs, T, [1, 1], root=root)


# ---- argument errors ----------------------------------------------------------------------------------------------------------

def test_argument_errors(vm):
    lists, par, _ = MO.batch("twice")
    with pytest.raises(vm.VisoMatchError, match="VSM_EARG"):
        vm.host_pairs_motions(lists, None)
    with pytest.raises(vm.VisoMatchError, match="VSM_EARG"):
        vm.host_pairs_motions([], par)
    with pytest.raises(vm.VisoMatchError, match="VSM_EARG"):
        vm.host_pairs_motions([lists[0], None, lists[1]], par, counts=[len(lists[0]), 5, len(lists[1])])
    with pytest.raises(vm.VisoMatchError, match="VSM_EARG"):
        vm.host_pairs_motions(lists, par, counts=[len(lists[0]), -1, len(lists[2])])
    with pytest.raises(vm.VisoMatchError, match="VSM_EARG"):
        vm.host_pairs_motions(lists, MO.params(-1))
    bad = lists[1].copy()
    bad["v1c"][7] = np.nan
    with pytest.raises(vm.VisoMatchError, match="VSM_EARG"):
        vm.host_pairs_motions([lists[0], bad], par)
    neg = lists[1].copy()
    neg["u1c"][3] = -1.0
    assert len(vm.host_pairs_motions([lists[0], neg], par)) == 2   # fine without bucketing
    with pytest.raises(vm.VisoMatchError, match="VSM_EARG"):
        vm.host_pairs_motions([lists[0], neg], par, bucket=True)
    # the outputs are untouched by a rejected call
    rc = np.full(3, 77, np.int32)
    cnt = np.array([len(lists[0]), -1, len(lists[2])], np.int32)
    ptrs = (C.c_void_p * 3)(*[l.ctypes.data for l in lists])
    got = vm.lib().vsm_host_pairs_motions(C.byref(par), 3, ptrs, cnt.ctypes.data_as(C.c_void_p), 0, 1, rc.ctypes.data_as(C.c_void_p), *([None] * 7))
    assert got == vm.Matcher.EARG and rc.tolist() == [77, 77, 77]


# ---- the image case of the GPU suite is not empty ------------------------------------------------------------------------------

def test_road_clip_succeeds_on_the_host(vm, B, synth):
    """the oracle's flow lists of the street clip: every list has more than 10 matches after bucketing, at least one pair's
    motion succeeds, the chain gives every frame a pose, and at least one track becomes a kept 3-D point"""
    frames = MO.road_frames(synth)
    lists = []
    for a, b in MO.ROAD_PAIRS:
        cm = B.CpuMatcher("oracle")
        cm.push_back(frames[a])
        cm.push_back(frames[b])
        cm.match(0)
        lists.append(MO._as_pmatch(cm.matches()))
    par = MO.road_params()
    res = vm.host_pairs_motions(lists, par, bucket=True, threads=4)
    assert all(len(res.matches(k)) > 10 for k in range(len(lists)))
    assert int((res.rc == 1).sum()) >= 1
    poses, valid, posed = vm.chain_poses(MO.ROAD_N, MO.ROAD_PAIRS, res.T, res.rc)
    assert posed == MO.ROAD_N
    assert poses[MO.ROAD_N - 1][11] > 0.5   # the camera drives forward: frame 5 lies ahead of frame 0 (the scale is the ground plane's)
    tr = vm.host_tracks(MO.ROAD_N, MO.ROAD_PAIRS, lists)
    import points_cases as PC
    uv = PC.gather(tr.obs, lists, 0)
    pts = vm.host_triangulate(poses, par.f, par.cu, par.cv, tr.offsets, tr.obs[:, 0], uv, flags=tr.flags, pose_valid=valid, params=MO.ROAD_POINT_PARAMS)
    assert int(pts.kept.sum()) >= 1
