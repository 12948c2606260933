"""GPU suite (run with -m gpu on an MI355X): the matching passes' ordered compaction and the Delaunay chains' keys it writes
(k_compact_quad, k_compact_count / k_compact_write; option fused_keys) alone, on acceptance flags and per-query records of the
test's own, through vsm_debug_compact_keys.  The expectation is plain numpy: the accepted records in query order (flow /
stereo: minus the queries whose pixel an accepted query up to three indices in front already has), and for list position d
below the key array's capacity key[d] = u1c << 34 | v1c << 20 | d.  Everything is byte equality; list and key arrays are
pre-filled with 0xA5 bytes, so the words the kernels must leave alone are compared too.  The keys are asked for three ways -
the compaction's store, its host-mapped second target, and k_dc2_keys behind the plain compaction - and must agree."""
import numpy as np
import pytest

from conftest import pkg

pytestmark = pytest.mark.gpu

SIZES = [0, 1, 3, 4, 5, 1023, 1024, 1025, 2049]  # the 4-flag loads, the 1024-query span and the 256-query block on either side
PATTERNS = ["all", "none", "alternating", "last", "first of the second span"]
MODES = [0, 2, 1]  # the compaction's key store, its host-mapped target, k_dc2_keys


@pytest.fixture(scope="module")
def vm():
    m = pkg("visomatch")
    m.lib()  # raises if the HIP library is missing: no silent fallback
    return m


def records(vm, rng, n):
    """n per-query records with pixel coordinates over the whole 14-bit range, both ends on both axes among them"""
    r = np.zeros(n, dtype=vm.P_MATCH)
    for name in r.dtype.names:
        if name.startswith("i"):
            r[name] = rng.integers(0, 1 << 20, n)
        else:
            r[name] = rng.integers(0, 16384, n).astype(np.float32)
    for i, (u, v) in enumerate([(0, 0), (16383, 16383), (0, 16383), (16383, 0)]):
        for at in (i, n - 1 - i):  # (the first and the last queries: accepted by most patterns)
            if 0 <= at < n:
                r["u1c"][at], r["v1c"][at] = u, v
    return r


def flags_of(pattern, n, rng):
    f = np.zeros(n, dtype=np.int32)
    if pattern == "all":
        f[:] = 1
    elif pattern == "alternating":
        f[::2] = 1
    elif pattern == "last" and n:
        f[-1] = 1
    elif pattern == "first of the second span" and n > 1024:
        f[1024] = 1
    elif pattern == "random":
        f[:] = rng.integers(0, 2, n) * rng.integers(1, 1 << 30, n)  # (any non-zero word accepts)
    return f


def expected(vm, flag, raw, cap, method):
    n = len(flag)
    keep = flag != 0
    if method < 2:  # first come, first served per pixel among the accepted queries up to three indices in front
        for i in range(n):
            for j in range(max(i - 3, 0), i):
                if flag[i] and flag[j] and raw["u1c"][j] == raw["u1c"][i] and raw["v1c"][j] == raw["v1c"][i]:
                    keep[i] = False
    lst = raw[keep]
    list_out = np.frombuffer(b"\xa5" * (vm.P_MATCH.itemsize * (n + 1)), dtype=vm.P_MATCH).copy()
    list_out[:len(lst)] = lst
    keys = np.full(cap + vm.COMPACT_KEY_GUARD, 0xA5A5A5A5A5A5A5A5, dtype=np.uint64)
    m = min(len(lst), cap)
    d = np.arange(m, dtype=np.uint64)
    keys[:m] = (lst["u1c"][:m].astype(np.int32).astype(np.uint64) << np.uint64(34)) | (lst["v1c"][:m].astype(np.int32).astype(np.uint64) << np.uint64(20)) | d
    return list_out, len(lst), keys


def check(vm, flags, raws, caps, method, pass_=1):
    want = [expected(vm, f, r, c, method) for f, r, c in zip(flags, raws, caps)]
    for mode in MODES:
        got = vm.device_compact_keys(flags, raws, caps, method=method, pass_=pass_, old_keys=mode)
        for k, ((gl, gn, gk), (wl, wn, wk)) in enumerate(zip(got, want)):
            what = (method, pass_, mode, k, len(flags[k]), caps[k])
            assert gn == wn, what
            assert gl.tobytes() == wl.tobytes(), what
            assert gk.tobytes() == wk.tobytes(), what
    return want


@pytest.mark.parametrize("pattern", PATTERNS)
def test_quad_sizes_and_patterns(vm, pattern):
    """every size in ONE launch of nine pairs of different lengths (the empty one among them), per flag pattern"""
    rng = np.random.default_rng(11)
    raws = [records(vm, rng, n) for n in SIZES]
    flags = [flags_of(pattern, n, rng) for n in SIZES]
    want = check(vm, flags, raws, [max(n, 1) for n in SIZES], 2)
    if pattern == "all":
        assert [w[1] for w in want] == SIZES


@pytest.mark.parametrize("pass_", [0, 1])
def test_quad_three_pairs_random_flags(vm, pass_):
    """three pairs of different lengths, one of them empty, random flags (any non-zero word accepts), either pass's slots"""
    rng = np.random.default_rng(12 + pass_)
    sizes = [2049, 0, 1025]
    raws = [records(vm, rng, n) for n in sizes]
    flags = [flags_of("random", n, rng) for n in sizes]
    want = check(vm, flags, raws, [2049, 4, 1025], 2, pass_)
    assert want[0][1] > 900 and want[1][1] == 0 and want[2][1] > 400


def test_quad_capacity_below_the_count(vm):
    """key arrays shorter than the lists: the keys stop at the capacity (where k_dc2_keys clamps), the list and its count do
    not, and the words behind every array keep their pattern (the comparison with `expected` covers them)"""
    rng = np.random.default_rng(13)
    sizes = [2049, 1025, 5, 1024]
    raws = [records(vm, rng, n) for n in sizes]
    flags = [flags_of("all", n, rng) for n in sizes]
    want = check(vm, flags, raws, [1500, 1024, 0, 1], 2)
    assert [w[1] for w in want] == sizes
    guard = np.uint64(0xA5A5A5A5A5A5A5A5)
    for (_, _, keys), cap in zip(want, [1500, 1024, 0, 1]):
        assert (keys[cap:] == guard).all() and (cap == 0 or keys[cap - 1] != guard)


def test_quad_sixty_four_pairs_with_empty_blocks_and_the_last_slot(vm):
    """the hook's maximum of pairs in one launch: empty pairs, pairs of one query, pairs on either side of the 256-query
    block, key arrays of capacity 0 (no room but the guard) among them - the first and the last pair's slots included"""
    rng = np.random.default_rng(15)
    sizes = [[0, 1, 255, 256, 257][k % 5] for k in range(63)] + [257]
    caps = [0 if k % 3 == 0 else max(n, 1) for k, n in enumerate(sizes)]
    assert len(sizes) == 64 and caps[0] == 0 and caps[63] == 0 and {(n, c == 0) for n, c in zip(sizes, caps)} >= {(n, z) for n in (0, 1, 255, 256, 257) for z in (False, True)}
    raws = [records(vm, rng, n) for n in sizes]
    flags = [flags_of("random", n, rng) for n in sizes]
    want = check(vm, flags, raws, caps, 2)
    assert [w[1] for w in want[:2]] == [0, int(flags[1][0] != 0)] and want[63][1] > 100


@pytest.mark.parametrize("method", [0, 1])
@pytest.mark.parametrize("pattern", ["all", "alternating", "random"])
def test_flow_and_stereo_with_the_pixel_dedup(vm, method, pattern):
    """k_compact_write: accepted queries that share a pixel within three indices - across a 256-query block border too - lose
    all but the first; the keys number the survivors"""
    rng = np.random.default_rng(14)
    sizes = [0, 1, 5, 255, 257, 1025, 2049]
    raws = [records(vm, rng, n) for n in sizes]
    for r in raws:
        for a, b in ((2, 4), (254, 256), (255, 256), (600, 603), (700, 704), (1023, 1024)):  # (700, 704): four apart - both stay
            if b < len(r):
                r["u1c"][b], r["v1c"][b] = r["u1c"][a], r["v1c"][a]
    flags = [flags_of(pattern, n, rng) for n in sizes]
    want = check(vm, flags, raws, [max(n, 1) for n in sizes[:-1]] + [1000], method)
    if pattern == "all":  # (2, 4), (255, 256), (600, 603), (1023, 1024) cost a match each; (700, 704) costs none
        lost = [n - w[1] for n, w in zip(sizes, want)]
        assert lost[0] == lost[1] == 0 and lost[2] >= 1 and lost[3] >= 1 and lost[4] >= 2 and 4 <= lost[5] <= 8 and 4 <= lost[6] <= 8, lost
