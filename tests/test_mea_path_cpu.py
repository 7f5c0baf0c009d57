"""The float64 reference of the maximum-expected-accuracy alignment (tests/mea_ref.py) without a GPU:
against brute-force enumeration of every band path, on peaked lattices, under its seeded faults on every input family the GPU
tests use, the condition of those inputs (few near ties), and the three symbols in the header, the binding and the library."""
import functools

import numpy as np
import pytest

import mea_ref as MR
import posterior_ref as R
from fb_harness import assert_declared_exported_bound

CASES = R.edge_cases()
SHAPES = R.case_shapes()
SMALL = [k for k, sh in SHAPES.items() if sh[0] <= 700]            # the cases tests/test_mea_path_gpu.py holds against this reference (all of them)


@functools.lru_cache(maxsize=None)
def _reference(name):
    lp, labels, terminal, beam, mm = CASES[name]()
    ref = R.ref_at(lp, labels, terminal, beam, mm)
    assert ref["status"] == R.OK, name
    return labels, terminal, beam, mm, ref, MR.reference(ref, labels, terminal, beam, mm)


def _tiny(rng, T, L, mm, beam):
    """A tiny lattice with label value 0 in the transcript, random float32 gammas over its band (any non-negative numbers
    serve the recursion) in which ties are common, and a terminal some band path reaches that is not L - 1 where one exists."""
    S = (L - 1) // 2
    labels = rng.integers(0, 3, size=S).astype(np.int32)
    lo, hi = R.windows(T, L, beam)
    gamma = [(rng.integers(0, 4, size=hi[t] - lo[t]) / 4.0).astype(np.float32) for t in range(T)]
    live = [int(lo[T - 1] + k) for k in range(hi[T - 1] - lo[T - 1])
            if MR.brute_force(gamma, lo, hi, labels, int(lo[T - 1] + k), mm)[1] is not None]
    below = [s for s in live if s != L - 1]
    return gamma, lo, hi, labels, (below or live or [None])[int(rng.integers(0, max(len(below or live), 1)))]


@pytest.mark.parametrize("mm", [1, 2, 3, 4, 5, 6])
def test_the_reference_equals_brute_force_enumeration(mm):
    rng = np.random.default_rng(100 + mm)
    checked = below = 0
    for T in (1, 2, 3, 4, 5, 6) if mm <= 4 else (1, 2, 3, 4, 5):
        for L in (1, 3, 5, 7, 9):
            for beam in (2, 4, 1000):
                gamma, lo, hi, labels, terminal = _tiny(rng, T, L, mm, beam)
                if terminal is None:
                    continue
                got = MR.mea(gamma, lo, hi, labels, terminal, mm)
                value, path = MR.brute_force(gamma, lo, hi, labels, terminal, mm)
                assert got["status"] == R.OK and got["value"] == value, (T, L, beam, got["value"], value)
                assert np.array_equal(got["path"], path), (T, L, beam, got["path"], path)             # the tie rule's path
                assert MR.validity(got["path"], lo, hi, labels, terminal, mm) is None
                checked += 1
                below += terminal != L - 1
    assert checked >= 30 and below >= 10


# (T, S, V, beam, max_move, seed): seeds under which no frame's blank can be swapped for its neighbour blank (a move of 3 past
# a label leaves the choice), which the assertion on the path's mass checks
@pytest.mark.parametrize("shape", [(150, 30, 39, 16, 4, 5), (200, 38, 39, 7, 3, 1), (129, 30, 39, 7, 2, 1), (180, 38, 39, 12, 6, 4),
                                   (64, 20, 39, 1000, 4, 12)])
def test_on_a_peaked_lattice_the_path_is_the_unique_best_path(shape):
    T, S, V, beam, mm, seed = shape
    lp, labels, states = MR.unique_peaked(T, S, V, beam, mm, seed)
    ref = R.ref_at(lp, labels, int(states[-1]), beam, mm)
    assert ref["status"] == R.OK
    assert all(g[states[t] - lo] > 1.0 - 1e-9 for t, (lo, g) in enumerate(ref["gamma"]))      # the path holds all the mass
    got = MR.reference(ref, labels, int(states[-1]), beam, mm)
    assert np.array_equal(got["path"], states)
    assert 0.0 <= T - got["value"] <= T * 1e-9 + MR.M_MEA * MR.error_bounds(ref)[0]            # T within the model
    assert MR.near_tie_share(ref, got, labels, mm) == 0.0


def _differs(bad, good):
    return bad["status"] != good["status"] or not np.array_equal(bad["path"], good["path"]) or bad["value"] != good["value"]


def test_every_fault_shows_on_the_tiny_lattices():
    """On arbitrary gammas (the brute-force family: quarter-valued, ties everywhere) each of the six seeded faults changes
    the path or the value somewhere."""
    shown = set()
    for mm in (3, 4, 5):
        rng = np.random.default_rng(100 + mm)
        for T, L, beam in [(T, L, beam) for T in (2, 3, 4, 5, 33, 40) for L in (5, 7, 9) for beam in (2, 4, 1000)]:
            gamma, lo, hi, labels, terminal = _tiny(rng, T, L, mm, beam) if T <= 5 else _tiny_long(rng, T, L, mm, beam)
            if terminal is None:
                continue
            good = MR.mea(gamma, lo, hi, labels, terminal, mm)
            shown |= {f for f in MR.FAULTS if _differs(MR.mea(gamma, lo, hi, labels, terminal, mm, f), good)}
    assert shown == set(MR.FAULTS), set(MR.FAULTS) - shown


def _tiny_long(rng, T, L, mm, beam):
    """_tiny() over more than one 32-frame block (no enumeration: any terminal of the last band that the recursion reaches)."""
    labels = rng.integers(0, 3, size=(L - 1) // 2).astype(np.int32)
    lo, hi = R.windows(T, L, beam)
    gamma = [(rng.integers(0, 4, size=hi[t] - lo[t]) / 4.0).astype(np.float32) for t in range(T)]
    live = [s for s in range(lo[T - 1], hi[T - 1]) if MR.mea(gamma, lo, hi, labels, s, mm)["status"] == R.OK]
    return gamma, lo, hi, labels, (live[0] if live else None)


# which seeded faults change the path or the value in some case of each family of posterior_ref.edge_cases(), on the float64
# reference's gamma
SHOWN = {"edge": {"no_veto", "next_band", "block_edge"}, "steep": {"no_veto", "next_band", "block_edge"},
         "flat": {"next_band", "block_edge"}, "peaked": {"no_veto", "tie_high", "block_edge"}, "geom": {"no_veto", "block_edge"}}


def test_which_faults_show_on_the_gpu_families():
    """The GPU families feed the recursion a true posterior, and on a true posterior two of the seeded faults cannot show at
    all: every cell with gamma > 0 lies on a band path of positive mass that starts at an allowed start and ends at the
    terminal.  A path that ends elsewhere (terminal_free) collects 0 from its last cell with gamma > 0 on, while the
    positive-mass continuation of that cell collects more and ends at the terminal with gamma = 1; a path that starts
    elsewhere (start_free) loses to the positive-mass approach of its first cell with gamma > 0 in the same way.  So the free
    optimum is the constrained one, path and value - asserted here for every case; the two faults are shown on arbitrary
    gammas above.  block_edge shows in every family; no_veto, next_band and tie_high where a family has vetoed moves near the
    path, a band narrower than L, or exact ties (SHOWN: flat lattices rarely skip, whole-lattice bands have no edge, and
    only peaked gammas tie exactly)."""
    shown = {}
    for name in SMALL:
        labels, terminal, beam, mm, ref, good = _reference(name)
        family = name.split("_")[0]
        for fault in MR.FAULTS:
            hit = _differs(MR.reference(ref, labels, terminal, beam, mm, fault), good)
            assert not (hit and fault in ("terminal_free", "start_free")), (name, fault)
            if hit:
                shown.setdefault(family, set()).add(fault)
    assert shown == SHOWN, shown
    assert all("block_edge" in v for v in shown.values()) and set().union(*shown.values()) == set(MR.FAULTS) - {"terminal_free", "start_free"}


@pytest.mark.parametrize("name", SMALL)
def test_the_inputs_have_few_near_ties(name):
    """The inputs' condition on the reference alone: at most 1 % of a case's steps are near ties (mea_ref.near_tie_share) in
    every case but the five of mea_ref.NEAR_TIED (measured: 1.5 % to 6.5 %), no more and no fewer.  The GPU test against the
    float64 reference holds choices to a tolerance, which a near tie cannot fail, and runs all of them."""
    labels, terminal, beam, mm, ref, good = _reference(name)
    T = len(good["path"])
    lo, hi = R.windows(T, 2 * len(labels) + 1, beam)
    assert good["status"] == R.OK and MR.validity(good["path"], lo, hi, labels, terminal, mm) is None
    assert 0.0 < good["value"] <= T * (1 + 1e-12)
    step, total = MR.choice_ratio(good["path"], ref, good, labels, mm)
    assert step == 0.0 and abs(total) <= 1e-9 / MR.error_bounds(ref)[0]
    share = MR.near_tie_share(ref, good, labels, mm)
    print(name, "near ties: %.4f" % share)
    assert (share > 0.01) == (name in MR.NEAR_TIED), (name, share)


def test_segment_path_disagreement_on_a_toy():
    import kokoro_align_amd as ka
    best = [0, 0, 1, 2, 3, 4, 4, 5, 6, 6]
    mea = [0, 1, 1, 2, 2, 3, 4, 5, 5, 6]
    # boundary frames 0, 3, 7; cuts 0, 2, 4: best reaches them at 0, 3, 5, mea at 0, 3, 6; text indices differ at frames 5 and 8
    shift, share = ka.segment_path_disagreement(best, mea, [3, 7, 12], 3)
    assert shift.tolist() == [0, 0, 1] and share.tolist() == [0.0, 0.25, 1 / 3]
    shift, share = ka.segment_path_disagreement(best, best, [3, 7, 12], 3)
    assert shift.tolist() == [0, 0, 0] and share.tolist() == [0.0, 0.0, 0.0]
    p, l, s = ka.path_outputs(np.log(np.full((3, 4), 0.25, np.float32)), [1, 2], [0, 1, 3])
    assert p.dtype == l.dtype == np.int32 and s.dtype == np.float32 and l.tolist() == [0, 1, 2] and np.allclose(s, np.log(0.25))
    with pytest.raises(ValueError):
        ka.path_outputs(np.zeros((3, 4), np.float32), [1, 2], [0, 1, 5])


def test_the_symbols_are_declared_exported_and_bound():
    lib = assert_declared_exported_bound(["ka_ctc_mea_path_f32", "ka_ctc_mea_path_batch_f32", "ka_mea_path_workspace_bytes"])
    assert lib.ka_version() == 104
