"""What tests/test_parallel_backtrace_gpu.py stands on, without a GPU: the float32 reference with back-pointers
(tests/pbt_ref.py) is the C oracle bit for bit on every case, the case table reaches every class of the map kernels'
geometry, every seeded fault shows in an entry or in a reachable map cell, and the map cells the reference cannot reach
(score -inf: every candidate ties) stay a small share of what is compared."""
import ctypes
import functools

import numpy as np
import pytest

import pbt_ref as P
from oracle import oracle as O

# Unreachable map cells: at most 15 % over the whole table and 50 % of any one case (the reachable front climbs
# max_move - 1 positions a frame from position 0, so a steep lattice keeps the top of its band dark for a long time).
CAP_TABLE, CAP_CASE = 0.15, 0.50


@pytest.mark.parametrize("name", P.NAMES)
def test_reference_equals_the_oracle_bit_for_bit(name):
    lp, lab, beam, mm = P.case(name)
    path, labels, scores, total, end = O.ctc_best_path_c(lp, lab, beam, mm, return_total=True)
    ref = P.reference(name)
    assert np.array_equal(ref.path, path) and ref.end == end
    assert np.array_equal(ref.labels, labels)
    assert np.array_equal(ref.scores.view(np.int32), scores.view(np.int32))
    assert np.float32(ref.total).view(np.int32) == np.float32(total).view(np.int32)
    # entries are the path read at the chunks' and super-chunks' last frames
    assert np.array_equal(ref.entries, path[P.chunk_last_frames(len(path))])
    assert np.array_equal(ref.super_entries, path[P.super_last_frames(len(path))])
    assert ref.super_entries[-1] == ref.entries[-1] == end


@pytest.mark.parametrize("name", P.NAMES)
def test_rise_of_the_path_cell_is_the_path(name):
    """The one map cell per chunk that the parity tests see: on the best path the rise is the path's own."""
    ref = P.reference(name)
    for c in range(1, len(ref.te)):
        te = int(ref.te[c])
        k = int(ref.entries[c] - ref.lo[te])
        assert ref.reachable[c][k]
        assert ref.rise[c][k] == ref.entries[c] - ref.entries[c - 1], (name, c)
        assert 0 <= ref.rise[c].min() and ref.rise[c].max() <= 3 * P.CK
        assert not np.any(ref.rise[c][~ref.reachable[c]])      # every candidate ties at -inf: move 0, rise 0


@functools.lru_cache(maxsize=None)
def _faulted(name, fault):
    lp, lab, beam, mm = P.case(name)
    try:
        return P.best_path_with_moves(lp, lab, beam, mm, fault=fault)
    except ValueError:
        return None      # the fault empties the beam: as different as it gets


@pytest.mark.parametrize("fault", [f for f in P.FAULTS if f != "no_ring_mask"])
def test_every_seeded_fault_changes_an_entry_or_a_reachable_cell(fault):
    hit = [n for n in P.NAMES if _faulted(n, fault) is None or P.differs(P.reference(n), _faulted(n, fault))]
    print(fault, "shows in", len(hit), "of", len(P.NAMES), "cases:", hit)
    assert hit, fault
    assert not any(P.differs(P.reference(n), P.reference(n)) for n in hit[:3])      # (the comparison itself finds nothing in equal maps)


@pytest.mark.parametrize("form", ["wave", "tiled"])
def test_a_map_row_read_without_the_ring_mask_differs(form):
    hit = []
    for n in P.NAMES:
        T, S, _, beam, _, _, _, _, forms = P.CASES[n]
        if form not in {f.partition("/")[0] for f in forms}:
            continue
        ref = P.reference(n)
        R, ring = P.ring_of(T, S, beam, form)
        m0 = P.pack_maps(ref, R, ring)
        good, bad = P.read_maps(m0, ref, R, ring), P.read_maps(m0, ref, R, ring, fault="no_ring_mask")
        for c in range(1, len(ref.te)):
            assert np.array_equal(good[c], ref.rise[c]), (n, c)      # packing and reading back loses nothing
        if any(np.any((bad[c] != ref.rise[c]) & ref.reachable[c]) for c in range(1, len(ref.te))):
            hit.append(n)
    print(form, "no_ring_mask shows in", hit)
    assert hit, form


def test_the_cases_cover_every_geometry_class():
    seen = set().union(*(P.geometry(n) for n in P.NAMES))
    assert seen == P.GEOMETRY, (P.GEOMETRY - seen, seen - P.GEOMETRY)
    # a case on each side of each switch of the launch code (cm_out_for, max_seg in enqueue_backtrace)
    width = {n: max(1, min(P.CASES[n][3], 2 * P.CASES[n][1] + 1)) for n in P.NAMES}
    for w in (401, 1041, 2089):
        assert any(x <= w for x in width.values()) and any(x > w for x in width.values())
    assert {401, 402, 1041, 1042} <= set(width.values())
    # the one-wavefront form takes bands up to 1009 positions; wider ones run tiled only
    for n in P.NAMES:
        assert ("wave" in P.CASES[n][8]) == (width[n] <= P.FAST_MAX_BAND), n


@pytest.mark.parametrize("positions", [256, 128])
def test_map_row_pitch_is_the_planner_s(positions):
    """pbt_ref.ring_of restates plan_tiles' checkpoint row, which is the map row: R = checkpoint_pitch / 4."""
    from kokoro_align_amd import _lib
    lib = _lib.load_library()
    for n in P.NAMES:
        T, S, V, beam, mm = P.CASES[n][:5]
        pitch = ctypes.c_int64(0)
        assert lib.ka_debug_plan_tiles_width(T, S, V, beam, mm, positions, None, None, 0, ctypes.byref(pitch)) > 0, n
        R, ring = P.ring_of(T, S, beam, "tiled")
        assert pitch.value == 4 * R, n
        L = 2 * S + 1
        assert (ring and L > R and R & (R - 1) == 0) or (not ring and L <= R), n


def test_unreachable_cells_stay_under_the_cap():
    table = [0, 0]
    for n in P.NAMES:
        u, cells = P.excluded_share(P.reference(n))
        print(f"{n}: {u} of {cells} map cells unreachable ({100.0 * u / max(cells, 1):.1f} %)")
        assert u <= CAP_CASE * cells, n
        table[0] += u
        table[1] += cells
    print(f"table: {table[0]} of {table[1]} ({100.0 * table[0] / table[1]:.1f} %)")
    assert table[0] <= CAP_TABLE * table[1]
