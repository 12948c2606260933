"""GPU suite (run with -m gpu on an MI355X): the location's three kernels (csrc/vsm_locate.hip) one by one, each through its
vsm_debug_locate_* entry - one launch with the call's geometry on tables of the test's - and then every hypothesis of whole
calls through vsm_debug_locate_hypotheses.  The device is compared with the host entries vsm_host_locate_sample / _fit / _count,
which test_locate_kernels_cpu.py pins to a restatement of the definition, and the winner with locate_ref.winner and the rigid
inverse of tests/resect_ref.py: ints equal, doubles by their bytes, except that where the host's double is NaN the device's only
has to be NaN too (x86 and gfx950 may differ in the sign bit of a generated NaN).  No tolerance anywhere.

Sizes are the smallest that reach each edge: hypothesis counts on either side of a wave's four groups and of a fit block's
sixteen, so that two jobs share a block; rows on either side of a wave and of a tile of 256 and into the third tile; hypothesis
counts on either side of the winner's 256 threads, so that its stride loop runs."""
import numpy as np
import pytest

import locate_cases as LC
import locate_ref as LR
import resect_ref as RR
from conftest import pkg

pytestmark = pytest.mark.gpu

F, CU, CV = LC.F, LC.CU, LC.CV
MIN_DEPTH = 1e-10
FILL = -7.5  # what a state holds before a fit: found again where the fit writes none


@pytest.fixture(scope="module")
def vm():
    m = pkg("visomatch")
    m.lib()  # raises if the HIP library is missing: no silent fallback
    return m


@pytest.fixture(scope="module")
def matcher(vm):
    m = vm.Matcher()
    yield m
    m.close()


def same_doubles(got, want):
    got, want = np.ascontiguousarray(got, dtype=np.float64), np.ascontiguousarray(want, dtype=np.float64)
    if got.shape != want.shape:
        return False
    nan = np.isnan(want)
    return bool(np.all(np.isnan(got[nan]))) and got[~nan].tobytes() == want[~nan].tobytes()


def stacked(frames):
    """[(uv, xyz)] -> (row_off, uv, xyz) of one launch"""
    off = np.cumsum([0] + [len(u) for u, _ in frames]).astype(np.int32)
    return off, np.concatenate([u for u, _ in frames]), np.concatenate([x for _, x in frames])


# ---- k_locate_fit -------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def fit_frames():
    """three frames: the degenerate samples' rows behind 17 ordinary ones, the noisy frame of statuses, outliers frame 0"""
    c = LC.cases()
    uv, xyz, special = LC.degenerate_rows()
    return [(uv, xyz), LC.frame_rows(c["statuses"], 6), LC.frame_rows(c["outliers"], 0)], special


def fit_picks(vm, frames, special, n_jobs, K):
    """picks [J, K, 6]: the library's own draw; in job 0 the degenerate samples sit at k = 1, 2, 4, 5, 7, .. among ordinary ones, so
    that the four groups of a wave take different branches of the decomposition"""
    picks = np.zeros((n_jobs, K, 6), np.int32)
    for j in range(n_jobs):
        E = 17 if j == 0 else len(frames[j][0])
        picks[j] = vm.host_locate_sample(71 + j, E, K)
    at = [k for k in range(K) if k % 3 != 0]
    for k, name in zip(at, [n for n in special if n != "ordinary"]):
        picks[0, k] = special[name]
    return picks


def host_fit_tables(vm, frames, picks, live):
    J, K = picks.shape[:2]
    states, valid = np.full((J, K, 12), FILL), np.full((J, K), 0xA5, np.uint8)
    for j in range(J):
        if live[j]:
            states[j], valid[j] = vm.host_locate_fit(F, CU, CV, *frames[j], picks[j], MIN_DEPTH, fill=FILL)
    return states, valid


@pytest.mark.parametrize("n_jobs", [2, 3])
@pytest.mark.parametrize("K", [1, 15, 16, 17, 33, 200])
def test_fit(vm, fit_frames, K, n_jobs):
    """every state and every validity of every job; with K = 15, 17 and 33 a block of sixteen groups holds the end of one job and
    the start of the next, and with J K no multiple of 16 the last block is partly empty"""
    frames, special = fit_frames
    picks = fit_picks(vm, frames, special, n_jobs, K)
    off, uv, xyz = stacked(frames[:n_jobs])
    want_s, want_v = host_fit_tables(vm, frames, picks, [True] * n_jobs)
    job_E = [len(frames[j][0]) for j in range(n_jobs)]
    got_s, got_v = vm.device_locate_fit(F, CU, CV, off, uv, xyz, np.arange(n_jobs), job_E, picks, np.full((n_jobs, K, 12), FILL), np.full((n_jobs, K), 0xA5, np.uint8),
                                        MIN_DEPTH)
    assert got_v.tolist() == want_v.tolist()
    bad = [(j, k) for j in range(n_jobs) for k in range(K) if not same_doubles(got_s[j, k], want_s[j, k])]
    assert not bad, bad[:8]
    if K >= 15:  # the degenerate samples are in: refused ones keep the pattern, and the wave around them is untouched by them
        assert (want_s[0] == FILL).all(axis=1).sum() >= 2 and 0 < want_v[0].sum() < K


def test_fit_skips_a_job_without_hypotheses(vm, fit_frames):
    """job_E = 0 between two live jobs, K = 17: the dead job's states and validity come back as they went up, and its neighbours in
    the two blocks it shares are right; the jobs' frames are not in job order"""
    frames, special = fit_frames
    K = 17
    picks = fit_picks(vm, frames, special, 3, K)
    picks[1] = 10 ** 6  # (never read)
    order = [2, 0, 1]  # frame g of the launch is frames[order[g]]
    off, uv, xyz = stacked([frames[g] for g in order])
    job_frame = [order.index(j) for j in range(3)]
    want_s, want_v = host_fit_tables(vm, frames, picks, [True, False, True])
    got_s, got_v = vm.device_locate_fit(F, CU, CV, off, uv, xyz, job_frame, [len(frames[0][0]), 0, len(frames[2][0])], picks, np.full((3, K, 12), FILL),
                                        np.full((3, K), 0xA5, np.uint8), MIN_DEPTH)
    assert (got_s[1] == FILL).all() and (got_v[1] == 0xA5).all()
    assert got_v.tolist() == want_v.tolist() and all(same_doubles(got_s[j, k], want_s[j, k]) for j in range(3) for k in range(K))


def test_fit_argument_checks(vm, fit_frames):
    frames, special = fit_frames
    off, uv, xyz = stacked(frames[:2])
    picks = fit_picks(vm, frames, special, 2, 3)
    s, v = np.zeros((2, 3, 12)), np.zeros((2, 3), np.uint8)
    n0 = len(frames[0][0])
    out = picks.copy()
    out[0, 1, 2] = n0  # a row of the next frame
    neg = picks.copy()
    neg[1, 0, 0] = -1
    for args in ((off, uv, xyz, [0, 1], [n0, 40], out), (off, uv, xyz, [0, 1], [n0, 40], neg), (off, uv, xyz, [0, 2], [n0, 40], picks),
                 (off, uv, xyz, [0, 1], [n0 + 1, 40], picks), (off[::-1].copy(), uv, xyz, [0, 1], [n0, 40], picks)):
        with pytest.raises(vm.VisoMatchError, match="VSM_EARG"):
            vm.device_locate_fit(F, CU, CV, *args, s, v)


# ---- k_locate_count -----------------------------------------------------------------------------------------------------------

COUNT_ROWS = (10, 63, 64, 65, 255, 256, 257, 513)
COUNT_KS = (1, 16, 17, 33)
NOT_ELIGIBLE = (0, 63, 64, 255, 256, -1)


@pytest.fixture(scope="module")
def count_frames():
    """frames of COUNT_ROWS rows of one camera with 30 % planted outliers as in outliers_case, each frame with draws of its own;
    rows that are not eligible - a NaN or infinite pixel or point - at positions 0, 63, 64, 255, 256 and last where the frame has
    them"""
    import points_cases as PC
    import resect_cases as RC
    rng = np.random.default_rng(46)
    pose = PC.camera_path(2)[1]
    pts = LC.volume(max(COUNT_ROWS), rng)
    frames = []
    for n in COUNT_ROWS:
        uv = []
        for X in pts[:n]:
            bad = rng.uniform() < 0.3
            a, r = rng.uniform(0, 2 * np.pi), rng.uniform(50, 120)
            uv.append(RC.pixel(pose, X, (r * np.cos(a), r * np.sin(a)) if bad else (0.0, 0.0)))
        uv, xyz = np.array(uv, np.float32), pts[:n].copy()
        for i, at in enumerate(sorted({p % n for p in NOT_ELIGIBLE if p < n})):
            if i % 4 == 0:
                uv[at, 0] = np.nan
            elif i % 4 == 1:
                xyz[at, 2] = np.inf
            elif i % 4 == 2:
                uv[at, 1] = -np.inf
            else:
                xyz[at, 0] = np.nan
        frames.append((uv, xyz))
    return frames


@pytest.fixture(scope="module")
def count_tables(vm, count_frames):
    """{K: (states [J, K, 12], hvalid [J, K], the host's counts [J, K])}: the host fit's states on samples of the eligible rows,
    every fifth hypothesis marked invalid by hand"""
    out = {}
    for K in COUNT_KS:
        states, valid, counts = [], [], []
        for uv, xyz in count_frames:
            elig = np.nonzero(np.isfinite(uv).all(axis=1) & np.isfinite(xyz).all(axis=1))[0]
            picks = elig[vm.host_locate_sample(71, len(elig), K)].astype(np.int32)
            s, v = vm.host_locate_fit(F, CU, CV, uv, xyz, picks, MIN_DEPTH)
            v[4::5] = 0
            states.append(s), valid.append(v), counts.append(vm.host_locate_count(F, CU, CV, uv, xyz, s, v, 2.0, MIN_DEPTH))
        out[K] = (np.array(states), np.array(valid), np.array(counts))
    return out


@pytest.mark.parametrize("K", COUNT_KS)
def test_count(vm, count_frames, count_tables, K):
    """eight frames in one launch: every wave of every tile adds a number of its own, so a lost or a doubled wave or tile shows"""
    states, valid, want = count_tables[K]
    off, uv, xyz = stacked(count_frames)
    J = len(count_frames)
    job_E = [int((np.isfinite(u).all(axis=1) & np.isfinite(x).all(axis=1)).sum()) for u, x in count_frames]
    got = vm.device_locate_count(F, CU, CV, off, uv, xyz, np.arange(J), job_E, states, valid, 2.0, MIN_DEPTH)
    assert got.tolist() == want.tolist()
    assert (want[:, 4::5] == 0).all() and (want.max(axis=1) > np.array(COUNT_ROWS) // 2).sum() >= (4 if K > 1 else 0)
    # the kernel adds to what it finds: the entry that launches it owns the clearing
    twice = vm.device_locate_count(F, CU, CV, off, uv, xyz, np.arange(J), job_E, states, valid, 2.0, MIN_DEPTH, launches=2)
    assert twice.tolist() == (2 * want).tolist()


def test_count_skips_a_job_without_hypotheses(vm, count_frames, count_tables):
    states, valid, want = count_tables[17]
    off, uv, xyz = stacked(count_frames)
    J = len(count_frames)
    job_E = np.array([len(u) for u, _ in count_frames], np.int32)
    job_E[[2, 5]] = 0
    got = vm.device_locate_count(F, CU, CV, off, uv, xyz, np.arange(J), job_E, states, valid, 2.0, MIN_DEPTH)
    assert (got[[2, 5]] == 0).all() and np.delete(got, [2, 5], axis=0).tolist() == np.delete(want, [2, 5], axis=0).tolist()


def test_count_threshold_on_the_edge(vm, count_frames, count_tables):
    """inlier_threshold squared is exactly one row's squared residual: the strict `<` leaves the row out, the next double takes it
    in"""
    states, valid, want = count_tables[17]
    j = COUNT_ROWS.index(257)
    uv, xyz = count_frames[j]
    k = int(np.argmax(want[j]))
    S = states[j, k]
    thr = None
    for i in range(len(uv)):
        t = LR.residual(S, xyz[i], uv[i, 0], uv[i, 1], F, CU, CV, MIN_DEPTH) if np.isfinite(uv[i]).all() and np.isfinite(xyz[i]).all() else None
        if t is None or not 0.0 < t < 4.0:
            continue
        for cand in (np.nextafter(np.sqrt(t), 0), np.sqrt(t), np.nextafter(np.sqrt(t), np.inf)):
            if float(cand) * float(cand) == t:
                thr = float(cand)
        if thr is not None:
            break
    assert thr is not None
    off, uv1, xyz1 = stacked([(uv, xyz)])
    got = {}
    for name, x in (("below", np.nextafter(thr, 0)), ("at", thr), ("above", np.nextafter(thr, np.inf))):
        got[name] = int(vm.device_locate_count(F, CU, CV, off, uv1, xyz1, [0], [len(uv)], states[j, k:k + 1][None], [[1]], x, MIN_DEPTH)[0, 0])
        assert got[name] == int(vm.host_locate_count(F, CU, CV, uv, xyz, S[None], [1], x, MIN_DEPTH)[0]) == LR.count(S, uv, xyz, F, CU, CV, float(x), MIN_DEPTH), name
    assert got["below"] == got["at"] < got["above"]


# ---- k_locate_winner ----------------------------------------------------------------------------------------------------------

MIN_INLIERS = 10
TOP = 2 ** 31 - 1


def winner_jobs(K, rng):
    """the tables of one launch with K hypotheses per job: [(counts [K], hvalid [K])], every job a scenario that K has room for"""
    jobs = []

    def background(top):
        """valid hypotheses counting below `top` all over, invalid ones with counts that would win"""
        c = rng.integers(0, max(top, 1), K).astype(np.int64)
        v = np.ones(K, np.uint8)
        dead = rng.uniform(size=K) < 0.2
        v[dead] = 0
        c[dead] = TOP
        return c, v

    def peak(at, top=500):
        c, v = background(top)
        for k in at:
            c[k], v[k] = top, 1
        jobs.append((c, v))

    for at in ((0,), (K - 1,), (256,), (300,), (70, 300), (255, 256), (511,), (63, 64), (0, K - 1)):
        if max(at) < K:
            peak(at)
    jobs.append((np.zeros(K, np.int64), np.ones(K, np.uint8)))  # all valid, all counts 0
    jobs.append((rng.integers(0, 500, K), np.zeros(K, np.uint8)))  # none valid
    c = np.full(K, TOP, np.int64)  # the only valid hypothesis is the last one
    v = np.zeros(K, np.uint8)
    v[K - 1], c[K - 1] = 1, 12
    jobs.append((c, v))
    peak((K // 2,), MIN_INLIERS - 1)
    peak((K // 2,), MIN_INLIERS)
    peak((K - 1,), TOP)  # the key's packing: the largest count an int32 holds
    if K > 300:
        peak((300, 5), TOP)
    return jobs


DEAD_JOBS = (3, 9)  # where test_winner puts a job without hypotheses between the scenarios


@pytest.mark.parametrize("K", [1, 63, 64, 65, 255, 256, 257, 513])
def test_winner(vm, K):
    """injected tables, one job per scenario; frames that are no job and jobs without hypotheses between the live ones"""
    rng = np.random.default_rng(K)
    jobs = winner_jobs(K, rng)
    for at in DEAD_JOBS:
        jobs.insert(at, (np.full(K, 500, np.int64), np.ones(K, np.uint8)))
    J = len(jobs)
    counts = np.array([c for c, _ in jobs]).astype(np.int32)
    hvalid = np.array([v for _, v in jobs], np.uint8)
    states = rng.uniform(-3, 3, (J, K, 12))
    job_E = np.full(J, 40, np.int32)
    job_E[list(DEAD_JOBS)] = 0
    frame_job = []
    for j in range(J):
        frame_job += [j] if j % 3 else [-1, j]
    frame_job.append(-1)
    verdict, best, inliers, lin, lin_valid = vm.device_locate_winner(frame_job, job_E, counts, hvalid, states, MIN_INLIERS)
    seen = set()
    for g, j in enumerate(frame_job):
        if j < 0 or job_E[j] == 0:
            assert (verdict[g], best[g], inliers[g], lin_valid[g]) == (-1, -1, 0, 0) and (lin[g] == 0).all(), (g, j)
            continue
        want = LR.winner(counts[j], hvalid[j], MIN_INLIERS)
        seen.add(want[0])
        assert (verdict[g], best[g], inliers[g]) == want, (g, j, want)
        assert lin_valid[g] == (want[0] == 0)
        want_lin = RR.rigid_inverse([float(x) for x in states[j, want[1]]]) if want[1] >= 0 else [0.0] * 12
        assert lin[g].tobytes() == np.array(want_lin).tobytes(), (g, j)
    assert seen == {0, 3, 4} or K == 1


def test_winner_of_257_frames(vm):
    """more frames than a block has threads, 300 hypotheses each, a job per second frame"""
    rng = np.random.default_rng(5)
    Fr, K = 257, 300
    frame_job = np.where(np.arange(Fr) % 2 == 0, np.arange(Fr) // 2, -1).astype(np.int32)
    J = int(frame_job.max()) + 1
    counts = rng.integers(0, 40, (J, K)).astype(np.int32)
    hvalid = (rng.uniform(size=(J, K)) < 0.7).astype(np.uint8)
    counts[::5] %= 30  # too few inliers
    counts[1::7] = np.minimum(counts[1::7], 38)  # the one winner sits behind the block's 256 threads
    counts[1::7, 280], hvalid[1::7, 280] = 39, 1
    states = rng.uniform(-3, 3, (J, K, 12))
    verdict, best, inliers, lin, lin_valid = vm.device_locate_winner(frame_job, np.full(J, 40, np.int32), counts, hvalid, states, 39)
    want = [LR.winner(counts[j], hvalid[j], 39) if j >= 0 else (-1, -1, 0) for j in frame_job]
    assert list(zip(verdict.tolist(), best.tolist(), inliers.tolist())) == want
    assert (np.array([w[1] for w in want]) > 255).any() and {w[0] for w in want} == {-1, 0, 4}
    for g, j in enumerate(frame_job):
        assert lin[g].tobytes() == np.array(RR.rigid_inverse([float(x) for x in states[j, best[g]]]) if best[g] >= 0 else [0.0] * 12).tobytes()


def test_winner_argument_checks(vm):
    c, v, s = np.zeros((2, 3), np.int32), np.ones((2, 3), np.uint8), np.zeros((2, 3, 12))
    for frame_job in ([0, 2], [-2, 1]):
        with pytest.raises(vm.VisoMatchError, match="VSM_EARG"):
            vm.device_locate_winner(frame_job, [40, 40], c, v, s, 10)


# ---- in situ: every hypothesis of whole calls ---------------------------------------------------------------------------------

def test_no_location_held(vm):
    m = vm.Matcher()
    with pytest.raises(vm.VisoMatchError, match="VSM_ENOTREADY"):
        m.locate_hypotheses()
    m.close()


@pytest.mark.parametrize("name", ["iters_17", "iters_33", "outliers", "outliers_tiles", "rows_family", "frames_257"])
def test_hypotheses_of_a_call(vm, matcher, name):
    """the call's own launches - fit blocks shared between jobs, the tiles of unequal frames, the samples drawn on the pool -: the
    samples are the host draw's mapped through the eligible rows, and every state, validity and count is the host entries'"""
    c = LC.cases()[name]
    a, kw = c.args()
    r = matcher.locate(*a, **kw)
    LC.assert_same(r, LC.host(name), name)
    p = vm.locate_params(**c.params)
    picks, states, hvalid, counts = matcher.locate_hypotheses()
    asked = np.ones(c.n_frames, bool) if c.locate is None else c.locate.astype(bool)
    job_frame = [g for g in range(c.n_frames) if asked[g] and r.rows[g] >= p.min_inliers]
    assert picks.shape == (len(job_frame), p.ransac_iters, 6) and states.shape[:2] == hvalid.shape == counts.shape == picks.shape[:2]
    live = 0
    for j, g in enumerate(job_frame):
        if r.eligible[g] < p.min_inliers:
            continue
        live += 1
        uv, xyz, want_picks, want_s, want_v, want_c = LC.host_hypotheses(vm, c, g, p, fill=FILL)
        assert picks[j].tolist() == want_picks.tolist(), (name, g)
        written = ~(want_s == FILL).all(axis=1)
        assert hvalid[j].tolist() == want_v.tolist() and counts[j].tolist() == want_c.tolist(), (name, g)
        assert same_doubles(states[j][written], want_s[written]), (name, g)
        assert LR.winner(counts[j], hvalid[j], p.min_inliers)[1:] == (r.best[g], r.inliers[g])
    assert live > 0
