"""The three posterior calls on the MI355X on the input families of tests/posterior_ref.py: mass at
the band's edges, bands that slide several positions a frame or hardly at all, beams 1 to 3, near one-hot rows with cells
down to 2^-120 and below, and shapes that straddle the block, lane, slot and form boundaries.  Every case runs through
ka_ctc_state_posteriors_f32, ka_ctc_label_posteriors_f32 and ka_ctc_path_posteriors_batch_f32 as built and, where that is the
one-wavefront form, once more in the generic form: the same lattice with unused -inf columns up to V = 80, whose reference
is the same.  Whether the second run has the bits of the first is printed for each output, not asserted: both forms are
held to the reference, not to each other.  Outputs are prefilled with
sentinels and their pitches padded.  Checked per cell against the float64 reference with posterior_ref.state_tolerance, label_tolerance, path_tolerance and z_tolerance (through the *_ratio functions: a cell the
reference puts below 2^-120 must come out below 2^-119), and exactly: gamma(T-1, s*) = 1.0, the zero tail, band_lo, the
untouched padding, and one Z from the state and label calls (the path call's within 1e-9 max(1, |Z|), as its own tests ask).
Every figure is printed before it is asserted; KA_ACCURACY_OUT=<file> collects them (fb_harness.record)."""
import numpy as np
import pytest

import posterior_ref as R
from fb_harness import band_width, engine, label_call_one, path_call, record, state_call_one

pytestmark = pytest.mark.gpu

CASES = R.edge_cases()
SHAPES = R.case_shapes()
assert set(SHAPES) == set(CASES)
# (case, V the kernels see): as built, and the one-wavefront cases once more in the generic form
RUNS = [(n, SHAPES[n][2]) for n in CASES] + [(n, 80) for n in CASES if R.fast_form(*SHAPES[n][1:])]
_BUILT = {}
_AS_BUILT = {}                                           # case -> what the three calls gave in the form the case was built for


@pytest.fixture(scope="module")
def env():
    return engine()


def _built(name):
    if name not in _BUILT:
        _BUILT.clear()                                   # the two runs of a case follow each other: keep one
        lp, labels, term, beam, mm = CASES[name]()
        ref = R.ref_at(lp, labels, term, beam, mm)
        assert ref["status"] == R.OK, name
        _BUILT[name] = (lp, labels, term, beam, mm, ref)
    return _BUILT[name]


@pytest.mark.parametrize("name,V", sorted(RUNS), ids=[f"{n}-V{v}" for n, v in sorted(RUNS)])
def test_family_case_through_the_three_calls(env, name, V):
    ka, _lib, eng = env
    lp0, labels, term, beam, mm, ref = _built(name)
    T, S = lp0.shape[0], len(labels)
    lp = lp0 if V == lp0.shape[1] else R.pad_vocabulary(lp0, V)
    assert R.fast_form(S, V, beam, mm) == (V == lp0.shape[1] and R.fast_form(S, lp0.shape[1], beam, mm))
    W = band_width(S, beam)
    lo, hi = R.windows(T, 2 * S + 1, beam)

    # state posteriors: the frames round the block boundaries and the last short block, rows of pitch W + 3
    frames = R.query_frames(T)
    rows, blo, z_state, rc = state_call_one(eng, _lib, lp, labels, term, frames, beam, mm, ld_out=W + 3, fill=-7.0)
    assert rc == 0, (name, rc)
    assert np.all(rows[:, W:] == -7.0), name
    assert np.array_equal(blo, lo[frames]), name
    for k, f in enumerate(frames):
        n = hi[f] - lo[f]
        assert np.all(rows[k, n:W] == 0.0), (name, f)
    want = np.zeros(W, np.float32)
    want[term - lo[T - 1]] = 1.0
    assert frames[-1] == T - 1 and np.array_equal(rows[-1, :W], want), name
    record("state", R.state_ratio(rows, frames, ref, name), R.M_STATE)
    record("z", R.z_ratio(z_state, ref), R.M_Z)

    # label occupancy: rows of pitch V + 5
    occ, z_label = label_call_one(eng, _lib, lp, labels, term, beam, mm, ld_out=V + 5, fill=-7.0)
    assert np.all(occ[:, V:] == -7.0), name
    assert z_label == z_state, (name, z_label, z_state)
    assert occ[T - 1, R.expand(labels)[term]] == 1.0, name
    assert np.all(occ[:, lp0.shape[1]:V] == 0.0), name                       # the padded columns carry no label
    record("label", R.label_ratio(occ[:, :V], ref, labels, name), R.M_LABEL)

    # path posteriors along a path through the likeliest states, the band's lowest and highest cells and position 0
    path = R.mixed_path(ref, (lo, hi), term)
    pref = R.forward_backward(lp0, labels, path, beam, mm)
    posts, ll, st, rc = path_call(eng, _lib, [lp], [labels], [path], beam, mm)
    assert rc == 0 and st[0] == 0, (name, rc, st)
    assert posts[0][-1] == 1.0, name
    assert abs(ll[0] - z_state) <= 1e-9 * max(1.0, abs(z_state)), (name, ll[0], z_state)
    record("path", R.path_ratio(posts[0], pref, name), R.M_PATH)
    record("z", R.z_ratio(ll[0], pref), R.M_Z)

    # the generic form of a one-wavefront case beside the run as built (a figure, not a requirement)
    V0 = lp0.shape[1]
    got = (rows[:, :W].copy(), occ[:, :V0].copy(), posts[0], np.array([z_state, z_label, ll[0]]))
    if V == V0:
        _AS_BUILT.clear()
        _AS_BUILT[name] = got
    elif name in _AS_BUILT:
        for what, a, b in zip(("state", "label", "path", "Z"), _AS_BUILT[name], got):
            same = np.array_equal(a.view(np.int32 if a.dtype == np.float32 else np.int64),
                                  b.view(np.int32 if b.dtype == np.float32 else np.int64))
            print(name, what, "generic form has the bits of the one-wavefront form:", same)
