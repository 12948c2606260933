"""GPU suite (run with -m gpu on an MI355X): Matcher.triangulate and Matcher.tracks against the reference's own Reconstruction
class (viso/reconstruction.{h,cpp}).  The class's outputs on the families and sequences of tests/recon_cases.py are recorded in
tests/golden/reconstruction_ref.npz, inputs included, so nothing outside the repository is read; where the compiled reference
(oracle/_ref/libvisoref.so) has travelled, it is run live as well.  The comparison and its bound are recon_cases.compare's, the
same as on the CPU (test_points_vs_ref.py, whose text has the measured figures; recon_cases' has the input convention).

Every family runs at 1, 15, 17, 63, 65, 255 and 257 tracks - both sides of a 16-lane group, a wave and a workgroup - taken as
prefixes, so that a group that mixes statuses and lengths is part of every run; and the device equals vsm_host_triangulate by its
bytes on the same inputs, as in test_points_gpu.py."""
import numpy as np
import pytest

import points_ref as R
import recon_cases as RC
from conftest import pkg
from oracle import bindings as B

pytestmark = pytest.mark.gpu

FX = RC.load()
LIVE = B.have_ref_reconstruction()


@pytest.fixture(scope="module", autouse=True)
def vm():
    m = pkg("visomatch")
    L = m.lib()  # raises if the HIP library is missing: no silent fallback
    assert hasattr(L, "vsm_triangulate_run") and hasattr(L, "vsm_tracks_run")
    return m


@pytest.fixture(scope="module")
def matcher(vm):
    m = vm.Matcher()
    yield m
    m.close()


@pytest.mark.parametrize("name", sorted(FX.families))
def test_family(vm, matcher, name):
    fam, ref = FX.families[name], FX.refs[name]
    assert len(fam) == RC.N_TRACKS
    live = fam.reference(B) if LIVE else None
    for n in RC.COUNTS + (len(fam),):
        part = fam.prefix(n)
        a, kw = part.ours()
        got = matcher.triangulate(*a, **kw)
        assert len(got) == n
        share = RC.compare(got, RC.prefix_ref(ref, n), part, (name, n, "device against the recorded reference"))
        if live is not None:
            RC.compare(got, RC.prefix_ref(live, n), part, (name, n, "device against the live reference"))
        R.assert_same(vm.host_triangulate(*a, **kw), got, (name, n, "host view against the device"))
    assert share <= 0.01  # (of the whole family, the last run)
    assert [got.stats[k] for k in vm.POINT_STATUS] == np.bincount(got.status, minlength=10).tolist()


@pytest.mark.skipif(not LIVE, reason="the compiled reference with the Reconstruction entries did not travel")
def test_recorded_reference_is_the_live_one():
    for name, fam in FX.families.items():
        live, ref = fam.reference(B), FX.refs[name]
        for k, dt in RC.REF_FIELDS:
            assert getattr(live, k).astype(dt).tobytes() == np.ascontiguousarray(getattr(ref, k)).astype(dt).tobytes(), (name, k)


@pytest.mark.parametrize("name", sorted(n for n in FX.lists if n != RC.SHARED))
def test_linking(matcher, name):
    """every track the reference finished with n pixels and last_idx at update k is a component of n observations that ends in
    node (k - 1, last_idx), and there are no others"""
    tr = matcher.tracks(RC.N_IMAGES, RC.PAIRS, FX.lists[name], 0, 2)
    assert RC.linking(tr) == sorted(tuple(x) for x in FX.finished[name].tolist()) and not tr.flags.any()


def test_linking_shared_i1p(matcher):
    """two matches of one list start at one feature: the reference gave the second a two-pixel track of its own; the device joins
    both ends to one component and flags it (test_points_vs_ref.py has the case in full)"""
    lists = FX.lists[RC.SHARED]
    extra = lists[2][-1]
    tr = matcher.tracks(RC.N_IMAGES, RC.PAIRS, lists, 0, 2)
    flagged = np.nonzero(tr.flags & 1)[0]
    assert len(flagged) == 1
    a, f = int(FX.shared_track[0]), FX.shared_track[1:].tolist()
    nodes = sorted([(a + j, x) for j, x in enumerate(f)] + [(3, int(extra["i1c"]))])
    assert tr.track(int(flagged[0]))[:, :2].tolist() == [list(x) for x in nodes]
    want = sorted(tuple(x) for x in FX.finished[RC.SHARED].tolist())
    assert (3, 2, int(extra["i1c"])) in want and (a + len(f) - 1, len(f), f[-1]) in want
    want.remove((3, 2, int(extra["i1c"])))
    want.remove((a + len(f) - 1, len(f), f[-1]))
    assert RC.linking(tr, skip=(int(flagged[0]),)) == want
