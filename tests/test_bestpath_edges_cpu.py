"""What tests/test_bestpath_edges_gpu.py and tests/test_forward_checkpoints_gpu.py stand on, without a GPU (DESIGN.md section
4.25).  These are conditions on the reference, not measurements: every case of tests/bestpath_cases.py equals the C oracle bit
for bit; the hugging and bait cases put the oracle's path on the band's edges; the border cases cross the tile borders by every
move at every frame class; every seeded fault shows in the path or the total and in a checkpoint cell - and on hash log-probs of
the same shapes a window one position off at every frame shows nowhere, which is why this file exists."""
import functools

import numpy as np
import pytest

import bestpath_cases as B
import pbt_ref as P
from oracle import oracle as O

# (lower, upper) share of frames the oracle's path must spend on an edge; the issue's measurements lie in 0.20 - 0.45
FLOOR, NOTE = 0.10, 0.15
# unreachable checkpoint cells (the reference holds -inf; they ARE compared on the GPU): capped all the same
CAP_TABLE, CAP_CASE = 0.15, 0.50
# the six cases of pbt_ref that the checkpoint test runs as well
PBT_ROWS = ("t33_w7_zero", "w401_wrap", "w402_wrap_m3_zero", "w1009_ring_zero", "steep_w400", "w1049")


@functools.lru_cache(maxsize=None)
def pbt_reference(name):
    lp, lab, beam, mm = P.case(name)
    return P.best_path_with_moves(lp, lab, beam, mm, maps=False)


@pytest.mark.parametrize("name", B.NAMES)
def test_reference_equals_the_oracle_bit_for_bit(name):
    lp, lab, beam, mm = B.case(name)
    assert np.all(np.isfinite(lp)), name      # (a -inf would send the lattice to the exact kernels)
    path, labels, scores, total, end = O.ctc_best_path_c(lp, lab, beam, mm, return_total=True)
    ref = B.reference(name)
    assert np.array_equal(ref.path, path) and ref.end == end
    assert np.array_equal(ref.labels, labels)
    assert np.array_equal(ref.scores.view(np.int32), scores.view(np.int32))
    assert np.float32(ref.total).view(np.int32) == np.float32(total).view(np.int32)
    assert len(ref.rows) == (ref.T - 1) // P.CK
    # the row's cell on the path is the running total of the path's scores (the same float32 add chain)
    for k in (0, len(ref.rows) - 1):
        t = P.CK * (k + 1) - 1
        run = np.float32(0.0)
        for x in scores[:t + 1]:
            run = np.float32(run + x)
        assert ref.rows[k][path[t] - ref.lo[t]].view(np.int32) == run.view(np.int32), (name, k)


@pytest.mark.parametrize("name", B.HUG + B.BAITS)
def test_the_path_is_on_the_band_s_edges(name):
    lower, upper = B.edge_shares(B.reference(name))
    print(f"{name}: on lo at {lower:.3f} of the frames with lo > 0, on hi - 1 at {upper:.3f} of those with hi < L")
    side = B.CASES[name][7] if name in B.BAITS else None      # bait cases hug one side each
    if side != "hi":
        assert lower >= FLOOR, name
        assert lower >= NOTE or name in (), name      # (no case of the table sits below 0.15)
    if side != "lo":
        assert upper >= FLOOR, name
        assert upper >= NOTE or name in (), name


@pytest.mark.parametrize("name", B.BAITS)
def test_the_cell_outside_beats_the_edge_cell_in_every_bait_frame(name):
    lp, lab, beam, mm = B.case(name)
    ref, frames, side = B.reference(name), B.bait_frames(name), B.CASES[name][7]
    ext = P.expand(lab)
    assert len(frames) >= ref.T // 10, name
    edge = ref.hi[frames] - 1 if side == "hi" else ref.lo[frames]
    outside = ref.hi[frames] if side == "hi" else ref.lo[frames] - 1
    assert np.all((outside >= 0) & (outside < ref.L))
    assert np.all(lp[frames, ext[outside]] > lp[frames, ext[edge]]), name
    assert np.all(ext[outside] != 0)
    # ... and the oracle's path is on that edge cell there (all but a few frames, where a tie took it elsewhere), the band
    # moving as the family says
    on_edge = float(np.mean(ref.path[frames] == edge))
    print(f"{name}: {len(frames)} bait frames, the path on the edge cell in {on_edge:.3f} of them")
    assert on_edge >= 0.9, name
    if side == "hi":
        assert np.all(ref.hi[frames + 1] > ref.hi[frames])
    else:
        assert np.all(ref.lo[frames] > ref.lo[frames - 1])


def test_the_border_cases_cross_by_every_move_at_every_frame_class():
    seen = set()
    for name in B.BORDERS:
        got = B.realised(B.reference(name).path, B.CASES[name][1])
        print(name, sorted(got))
        seen |= got
    assert seen == B.BORDER_PRODUCT, (B.BORDER_PRODUCT - seen, seen - B.BORDER_PRODUCT)


# ---- the faults ----
def _shows_in_path(name, fault):
    """Does the fault change the path or the total of the case?  The two faults of the maps change neither the recurrence nor the
    rows' contents: rise_short shows in the entries a chunk-parallel backtrace chains from the maps, no_ring_mask in what is read."""
    if fault in ("rise_short", "no_ring_mask"):
        lp, lab, beam, mm = B.case(name)
        ref = _with_maps(name, None)
        if fault == "rise_short":
            rises = _with_maps(name, fault).rise
        else:
            R, ring = P.ring_of(ref.T, (ref.L - 1) // 2, beam, "wave")
            rises = P.read_maps(P.pack_maps(ref, R, ring), ref, R, ring, fault=fault)
        return not np.array_equal(B.chain_entries(ref, rises), ref.entries)
    return not B.same_result(B.reference(name), B.reference(name, fault))


@functools.lru_cache(maxsize=None)
def _with_maps(name, fault):
    lp, lab, beam, mm = B.case(name)
    return P.best_path_with_moves(lp, lab, beam, mm, fault=fault)


def _cells_changed(name, fault):
    ref = B.reference(name)
    if fault == "no_ring_mask":
        R, ring = P.ring_of(ref.T, (ref.L - 1) // 2, ref.beam, "wave")
        img = B.pack_rows(ref, R, ring)
        assert B.rows_differ(ref, B.read_rows(img, ref, R, ring)) == 0      # packing and reading back loses nothing
        return B.rows_differ(ref, B.read_rows(img, ref, R, ring, fault=fault))
    return B.row_cells_changed(ref, B.reference(name, fault))


MAP_FAULT_CASES = ("bait_hi_w401_wrap", "hug_w1004_q")


@pytest.mark.parametrize("fault", B.FAULTS)
def test_every_fault_changes_the_path_or_the_total_under_a_wide_band(fault):
    names = MAP_FAULT_CASES if fault in ("rise_short", "no_ring_mask") else B.FAULT_CASES
    hit = [n for n in names if _shows_in_path(n, fault)]
    print(fault, "shows in", len(hit), "of", len(names), "cases:", hit)
    assert all(B.band_width(n) >= 300 for n in names)
    assert hit, fault
    if fault in B.WINDOW_FAULTS + ("stale_label",):
        assert any(B.band_width(n) >= 1000 for n in hit), (fault, hit)


@pytest.mark.parametrize("fault", B.FAULTS)
def test_every_fault_changes_an_in_band_checkpoint_cell(fault):
    names = MAP_FAULT_CASES if fault in ("rise_short", "no_ring_mask") else B.FAULT_CASES
    cells = {n: _cells_changed(n, fault) for n in names}
    print(fault, cells)
    if fault == "last_max":
        # which of two equal candidates wins changes the back-pointer and never the score: the rows cannot see this fault
        # (the path does, above), and that no cell moves is asserted rather than left out
        assert not any(cells.values()), fault
        return
    assert any(cells.values()), fault
    if fault in B.WINDOW_FAULTS:
        # the rows see more than the path does: over the cases more cells change than frames of the path (in single cases
        # too, but for hi_plus_one on hug_w400_q_zero: 4 cells, 19 frames), and cells change where the path does not
        frames = {n: B.path_frames_changed(B.reference(n), B.reference(n, fault)) for n in names}
        print("   frames of the path:", frames)
        assert sum(cells.values()) > sum(frames.values()), fault
        assert any(cells[n] and not frames[n] for n in names), fault


@pytest.mark.parametrize("shape", B.BLIND)
def test_on_hash_log_probs_the_window_faults_change_nothing(shape):
    """The reason for this file: a window one position off at EVERY frame leaves the path and the total of the suite's usual
    inputs as they are (the path never comes within a hundred positions of an edge), so no parity test can see it."""
    T, S, V, beam, mm, seed, quantised = shape
    lp, lab = P.inputs(T, S, V, seed, quantised, False)
    ref = P.best_path_with_moves(lp, lab, beam, mm, maps=False)
    low, high = B.edge_distance(ref)
    print(shape, "closest to lo", low, "closest to hi - 1", high)
    assert low >= 35 and high >= 35
    for fault in B.WINDOW_FAULTS:
        assert B.same_result(ref, P.best_path_with_moves(lp, lab, beam, mm, fault=fault, maps=False)), (shape, fault)


def test_unreachable_checkpoint_cells_stay_under_the_cap():
    table = [0, 0]
    for n, ref in [(n, B.reference(n)) for n in B.NAMES] + [(n, pbt_reference(n)) for n in PBT_ROWS]:
        u, cells = B.unreachable_share(ref)
        print(f"{n}: {u} of {cells} checkpoint cells unreachable ({100.0 * u / max(cells, 1):.1f} %)")
        assert u <= CAP_CASE * cells, n
        table[0] += u
        table[1] += cells
    print(f"table: {table[0]} of {table[1]} ({100.0 * table[0] / table[1]:.1f} %)")
    assert table[0] <= CAP_TABLE * table[1]


def test_every_case_names_the_forms_that_can_run_it():
    for n in B.NAMES:
        assert (B.CASES[n][8] == B.WAVE) == (B.band_width(n) <= P.FAST_MAX_BAND), n
        assert B.CASES[n][8] in (B.WAVE, B.WIDE)
        assert B.CASES[n][1] <= 4000
    widths = {B.band_width(n) for n in B.NAMES}
    assert {16, 64, 400, 401, 300, 1000, 1004, 1009, 1010, 1100} <= widths
    assert {B.CASES[n][5] for n in B.NAMES} == {2, 3, 4}
