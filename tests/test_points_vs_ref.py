"""CPU suite: the track triangulation and the track linking against the reference's own Reconstruction class
(viso/reconstruction.{h,cpp}), compiled in place into oracle/_ref/libvisoref.so and driven through oracle/ref_harness.cpp
(ref_recon_tracks, ref_recon_sequence).  The whole file is skipped without that library, or with one from before these entries.

test_points_cpu.py proves that vsm_host_triangulate, csrc/vsm_points.h and tests/points_ref.py are one reading of the class; this
file proves that the reading is the class's: 1 the per-track driver of the harness restates update() (byte-equal points, update
after update); 2 + 3 the library's definition against the driver on the families of tests/recon_cases.py, whose module text has
the input convention; 4 the linking; 5 the recorded fixture is what a fresh run gives.

Measured here (vsm_host_triangulate, all kept tracks of all families): the largest |ours - reference| / max(1, |reference|) over
xyz, dist and angle is 7.6e-7 (recon_cases.MEASURED; in the family "stray", 5.4e-8 to 8.0e-8 in the others), float32 rounding of
the reference's point; at the bound of 4 times that, 3.04e-6, no track of any family is near a threshold, and status and type
agree on every track.  No misreading of the class was found."""
import numpy as np
import pytest

import points_ref as R
import recon_cases as RC
from conftest import pkg
from oracle import bindings as B

if not B.have_ref_reconstruction():
    pytest.skip("needs oracle/_ref/libvisoref.so with the Reconstruction entries (make -C oracle ref)", allow_module_level=True)


@pytest.fixture(scope="module")
def vm():
    return pkg("visomatch")


@pytest.fixture(scope="module")
def refs():
    """the class on every family, once"""
    return {name: fam.reference(B) for name, fam in RC.families().items()}


@pytest.fixture(scope="module")
def hosts(vm):
    out = {}
    for name, fam in RC.families().items():
        a, kw = fam.ours()
        out[name] = vm.host_triangulate(*a, **kw)
    return out


# ---- 1: the harness equals update() ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", sorted(RC.sequences()))
def test_harness_equals_update(name):
    """The points Reconstruction::update appended, update after update, against the per-track driver on the tracks that update
    finished - their pixels collected from the lists as update() collects them, the frame states read out of the object after that
    update (so in its coordinates), a track's first state n - 1 from the back of the deque.  Byte-equal and in the list's order."""
    seq = RC.sequences()[name]
    recs = B.ref_recon_sequence(RC.F, RC.CU, RC.CV, seq.lists, seq.Tr, **seq.params)
    fin = RC.finished(seq, recs)
    assert len(recs) == RC.N_IMAGES and not len(recs[-1]["live"])
    with_points, stages = 0, set()
    for r, rec in enumerate(recs):
        # what lives on is what a match continued, then what a match started, in the order of the list
        if r < len(seq.lists):
            before = {int(last): int(n) for n, last in recs[r - 1]["live"]} if r else {}
            cont = {int(m["i1p"]): int(m["i1c"]) for m in seq.lists[r]}
            want = [(n + 1, cont[last]) for last, n in before.items() if last in cont] + [(2, int(m["i1c"])) for m in seq.lists[r] if int(m["i1p"]) not in before]
            assert rec["live"].tolist() == [list(x) for x in want], (name, r)
        if not fin[r]:
            assert len(rec["points"]) == 0
            continue
        offsets, uv, first = [0], [], []
        for n, last in fin[r]:
            uv += RC.chain(seq, r, last, n)
            offsets.append(len(uv))
            first.append(len(rec["fwd"]) - n)
        assert min(first) >= 0
        got = B.ref_recon_tracks(RC.F, RC.CU, RC.CV, rec["fwd"], offsets, uv, first, **seq.params)
        kept = got.xyz[got.stage == 0]
        assert kept.tobytes() == rec["points"].tobytes(), (name, r, len(kept), len(rec["points"]))
        with_points += len(kept) > 0
        stages |= set(got.stage.tolist())
    assert with_points >= 4 and len(stages) >= 3, (name, with_points, stages)  # tracks end, and are kept, at different updates


# ---- 2 + 3: our definition against the class -------------------------------------------------------------------------------------

def test_families_reach_every_stage(refs, hosts):
    stages, types = set(), set()
    for r in refs.values():
        stages |= set(r.stage.tolist())
        types |= set(r.type.tolist())
    assert stages == {0, 3, 4, 5, 6, 7, 8, 9} and types == {-2, -1, 0, 1, 2}
    assert refs["degenerate"].stage[0::3].tolist() == [4] * 87, "one pixel, translated cameras: at infinity"
    assert (refs["degenerate"].stage[1::3] == 5).all() and (refs["degenerate"].type[1::3] == -1).all(), "one pixel, rotated camera: in the centre"
    assert (refs["stray"].stage == 7).sum() >= 5 and (refs["stray"].stage == 6).sum() >= 5
    assert hosts["stray"].updates[220] == 22 and refs["stray"].stage[220] == 8, "converged with the last of the 22 updates"


def test_bound_is_what_was_measured(refs, hosts):
    worst = {name: RC.measure(hosts[name], refs[name], RC.families()[name].params) for name in refs}
    print("largest |ours - reference| / max(1, |reference|) over the kept tracks:", worst)
    assert RC.BOUND == 4 * RC.MEASURED and RC.BOUND < 1e-4
    assert 0 < max(worst.values()) <= RC.BOUND


@pytest.mark.parametrize("name", sorted(RC.families()))
def test_near_threshold_share(refs, name):
    """a condition on the inputs, met by the reference alone: at most 1 % of a family's tracks are near a threshold"""
    near = RC.near_threshold(refs[name], RC.families()[name].params, RC.BOUND)
    print(name, "near a threshold:", int(near.sum()), "of", len(near))
    assert near.mean() <= 0.01


def test_stray_family_is_stable():
    """where the Gauss-Newton iteration of a stray track ends does not hang on the pixels' last bit: the reference's own stage
    and type stay when the pixels move one float32 ulp up, down, or either way by a coin per coordinate"""
    fam = RC.families()["stray"]
    ref = fam.reference(B)
    for k in range(8):
        moved = RC.nudged(fam, k).reference(B)
        assert (moved.stage == ref.stage).all() and (moved.type == ref.type).all(), k


@pytest.mark.parametrize("name", sorted(RC.families()))
def test_host_view_against_class(refs, hosts, name):
    fam = RC.families()[name]
    share = RC.compare(hosts[name], refs[name], fam, name)
    assert share <= 0.01


@pytest.mark.parametrize("name", sorted(RC.families()))
def test_restatement_against_class(refs, hosts, name):
    fam = RC.families()[name]
    a, kw = fam.ours()
    got = R.triangulate(*a, **kw)
    assert RC.compare(got, refs[name], fam, name) <= 0.01
    R.assert_same(hosts[name], got, (name, "host view against the restatement"))


# ---- 4: track linking ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", sorted(RC.sequences()))
def test_linking(vm, name):
    """every track the reference finishes with n pixels and last_idx at update k is a component of n observations that ends in
    node (k - 1, last_idx), and there are no others"""
    seq = RC.sequences()[name]
    for m in seq.lists:
        assert len(set(m["i1p"].tolist())) == len(m) == len(set(m["i1c"].tolist()))
    recs = B.ref_recon_sequence(RC.F, RC.CU, RC.CV, seq.lists, seq.Tr, **seq.params)
    want = sorted((r, n, last) for r, fin in enumerate(RC.finished(seq, recs)) for n, last in fin)
    tr = vm.host_tracks(RC.N_IMAGES, RC.PAIRS, seq.lists, 0, 2)
    assert RC.linking(tr) == want and not tr.flags.any()
    # ... which is what the generator put in
    assert want == sorted((a + len(f) - 1, len(f), f[-1]) for a, f in seq.tracks)
    assert len({r for r, _, _ in want}) == RC.N_IMAGES - 1 and {n for _, n, _ in want} == {2, 3, 4, 5, 6}


def test_linking_shared_i1p(vm):
    """The documented divergence: two matches of one list start at one feature.  The reference gives the second a track of its
    own, of two pixels; the library joins both ends to the one component, which then has two observations in that image, and
    flags it.  Everything else is as in test_linking."""
    seq = RC.all_sequences()[RC.SHARED]
    extra = seq.lists[2][-1]
    assert (seq.lists[2]["i1p"] == extra["i1p"]).sum() == 2
    recs = B.ref_recon_sequence(RC.F, RC.CU, RC.CV, seq.lists, seq.Tr, **seq.params)
    want = sorted((r, n, last) for r, fin in enumerate(RC.finished(seq, recs)) for n, last in fin)
    truth = sorted((a + len(f) - 1, len(f), f[-1]) for a, f in seq.tracks)
    second = (3, 2, int(extra["i1c"]))
    assert want == sorted(truth + [second]), "the reference: every track as generated, and the second match's own"
    tr = vm.host_tracks(RC.N_IMAGES, RC.PAIRS, seq.lists, 0, 2)
    flagged = np.nonzero(tr.flags & 1)[0]
    assert len(flagged) == 1 and len(tr) == len(truth)
    a, f = next((a, f) for a, f in seq.tracks if a <= 2 < a + len(f) - 1 and f[2 - a] == int(extra["i1p"]))
    nodes = sorted([(a + j, x) for j, x in enumerate(f)] + [(3, int(extra["i1c"]))])
    assert tr.track(int(flagged[0]))[:, :2].tolist() == [list(x) for x in nodes]
    assert RC.linking(tr, skip=(int(flagged[0]),)) == sorted(set(truth) - {(a + len(f) - 1, len(f), f[-1])})


# ---- 5: the fixture ---------------------------------------------------------------------------------------------------------------

def test_fixture_is_a_fresh_run():
    fresh = RC.record(B)
    with np.load(RC.FIXTURE) as z:
        assert sorted(z.files) == sorted(fresh)
        for k in z.files:
            a, b = z[k], np.asarray(fresh[k])
            assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes(), k
