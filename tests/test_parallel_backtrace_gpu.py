"""The chunk-parallel backtrace's intermediate results on the GPU, cell by cell: every chunk entry,
every super-chunk entry and EVERY cell of every chunk map - the rise of the best path into each position the band holds at
a chunk's last frame - against the float32 reference with back-pointers of tests/pbt_ref.py, which
tests/test_parallel_backtrace_cpu.py pins to the C oracle.  All comparisons are exact integer comparisons.

The parity tests see one cell of each map, the one on the lattice's best path; the others are the answers for other end
positions, and the lane cells at segment edges, at the ring's wrap and next to the warm-up positions are among them.

Unreachable cells (reference score -inf) are asserted too, as rise 0: chunk_map_task holds cells outside the band at -inf,
so such a cell's candidates are all -inf in every frame of the chunk, as in the reference; `feq(c0, s)` then keeps move 0
(the first maximum) and the cell keeps its own origin.  Their share of the map cells is capped by the CPU file all the same.

ka_debug_chunk_entries reports descriptor 0 of the last launch: every case runs alone and then as the longest of three
lattices of different T and S in one launch, whose chunks are numbered across the lattices.
"""
import ctypes
import os

import numpy as np
import pytest

import pbt_ref as P
from oracle import oracle as O

pytestmark = pytest.mark.gpu

FORMS = ["wave+parallel", "tiled/256+parallel", "tiled/128+parallel"]


PAIRS = [(f, n) for f in FORMS for n in P.NAMES if f.partition("+")[0] in P.CASES[n][8]]


@pytest.fixture(scope="module")
def env():
    """The engine every call of the package goes through; the forms are set per test and `auto` is restored at the end."""
    import torch
    assert torch.cuda.is_available()
    import kokoro_align_amd as ka
    from kokoro_align_amd import _lib
    assert os.path.exists(ka.library_path()), "HIP library not built"
    eng = _lib.default_engine(torch.cuda.current_device())
    yield ka, eng
    eng.set_mode("auto")
    eng.set_tile_width(0)
    eng.set_backtrace("auto")


def _set_form(eng, form):
    mode, _, bt = form.partition("+")
    mode, _, width = mode.partition("/")
    eng.set_mode(mode)
    eng.set_tile_width(int(width or 0))
    eng.set_backtrace(bt)
    return form.partition("+")[0]


def _row(eng, form, name):
    """(R, ring) of the map rows, from the code's own rules: 1024 slots in the one-wavefront form (Lattice::ck_pitch = 4096,
    ck_mask = 1023), plan_tiles' checkpoint row in the tiled forms (a ring when the label axis does not fit it)."""
    T, S, V, beam, mm = P.CASES[name][:5]
    if form == "wave":
        return P.WAVE_RING, True
    pitch = ctypes.c_int64(0)
    n = eng.lib.ka_debug_plan_tiles_width(T, S, V, beam, mm, int(form.partition("/")[2]), None, None, 0, ctypes.byref(pitch))
    assert n > 0, (name, "not tileable")
    R = pitch.value // 4
    assert (R, 2 * S + 1 > R) == P.ring_of(T, S, beam, form), name
    return R, 2 * S + 1 > R


def _check(eng, form, name, what):
    ref = P.reference(name)
    nck, nsup = len(ref.te), len(ref.super_entries)
    R, ring = _row(eng, form, name)
    ent = np.full(nck + nsup + 1, -7, np.int32)
    m0 = np.full(nck * R, 255, np.uint8)
    n = eng.lib.ka_debug_chunk_entries(eng.handle, ent.ctypes.data, ent.size, m0.ctypes.data, m0.size)
    assert n == nck + nsup, (name, what, n)
    bad = np.nonzero(ent[:nck] != ref.entries)[0]
    assert bad.size == 0, (name, what, "chunk entries", bad[:8], ent[bad[:8]], ref.entries[bad[:8]])
    assert np.array_equal(ent[nck:nck + nsup], ref.super_entries), (name, what, "super-chunk entries", ent[nck:nck + nsup], ref.super_entries)
    got = P.read_maps(m0, ref, R, ring)
    for c in range(1, nck):
        te = int(ref.te[c])
        bad = np.nonzero(got[c] != ref.rise[c])[0]
        assert bad.size == 0, (name, what, f"map of chunk {c}: {bad.size} of {len(got[c])} cells, band {ref.lo[te]}..{ref.hi[te]}, first at",
                               (bad[:8] + ref.lo[te]).tolist(), "got", got[c][bad[:8]].tolist(), "want", ref.rise[c][bad[:8]].tolist(),
                               "reachable", ref.reachable[c][bad[:8]].tolist())


def _same(got, want):
    return all(np.array_equal(np.asarray(g).view(np.int32), np.asarray(w).view(np.int32)) for g, w in zip(got, want))


@pytest.mark.parametrize("form,name", PAIRS)
def test_every_entry_and_every_map_cell(env, form, name):
    ka, eng = env
    form = _set_form(eng, form)
    lp, lab, beam, mm = P.case(name)
    want = O.ctc_best_path_c(lp, lab, beam, mm)
    # alone
    res, status, _ = ka.ctc_best_path_batch([lp], [lab], beam, mm, return_status=True)
    assert status == [0] and _same(res[0], want), name
    _check(eng, form, name, "alone")
    # as the longest of three lattices in one launch
    others = P.companions(name)
    res, status, _ = ka.ctc_best_path_batch([lp] + [o[0] for o in others], [lab] + [o[1] for o in others], beam, mm, return_status=True)
    assert status[0] == 0 and _same(res[0], want), name
    for (olp, olab), r, st in zip(others, res[1:], status[1:]):
        try:
            w = O.ctc_best_path_c(olp, olab, beam, mm)
        except ValueError:
            assert st == -1, name
            continue
        assert st == 0 and _same(r, w), name
    _check(eng, form, name, "in a launch of three")
