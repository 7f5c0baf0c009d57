"""The forward kernels' checkpoint rows on the GPU, cell by cell.  Every 32 frames forward_ck and the
two tile pipelines store the score row; the backtrace reads a window of 124 positions of one row per chunk, so the parity
tests see a few cells of each.  Here every cell of the band of frame 32 (k + 1) - 1 in row k is compared, as int32 bits,
with the float32 reference of tests/pbt_ref.py (pinned to the C oracle by the CPU files) - -inf where the reference holds
-inf included: the tiled forms keep a tile alive from the frame the band reaches it to the frame the band has left it
(plan_tiles: t_in, t_end), so every in-band cell is written and none is left out of the comparison.

Slots outside the band may hold anything and are not compared, with one exception asserted on its
own: forward_ck masks its scores on checkpoint frames, so in the one-wavefront form the dead slots of the ring hold -inf.

ka_debug_checkpoints reports descriptor 0 of the last launch: every case runs alone and then as the longest of three
lattices of different T and S in one launch.
"""
import ctypes
import os

import numpy as np
import pytest

import bestpath_cases as B
import pbt_ref as P
from oracle import oracle as O

pytestmark = pytest.mark.gpu

FORMS = ("wave", "tiled/256", "tiled/128")
PBT = ("t33_w7_zero", "w401_wrap", "w402_wrap_m3_zero", "w1009_ring_zero", "steep_w400", "w1049")
PAIRS = [(f, "B", n) for f in FORMS for n in B.NAMES if f in B.CASES[n][8]] + [(f, "P", n) for f in FORMS for n in PBT if f in P.CASES[n][8]]
_refs = {}


def reference(table, name):
    """(lp, labels, beam, max_move, reference, companions), computed once per case and shared by the forms."""
    if (table, name) not in _refs:
        mod = B if table == "B" else P
        lp, lab, beam, mm = mod.case(name)
        ref = B.reference(name) if table == "B" else P.best_path_with_moves(lp, lab, beam, mm, maps=False)
        _refs[table, name] = (lp, lab, beam, mm, ref, mod.companions(name))
    return _refs[table, name]


@pytest.fixture(scope="module")
def env():
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


def read_back(eng, ref):
    """(rows, floats per row, image) of descriptor 0 of the last launch."""
    n_rows = len(ref.rows)
    pitch = ctypes.c_int64(-1)
    assert eng.lib.ka_debug_checkpoints(eng.handle, None, 0, ctypes.byref(pitch)) == n_rows, (n_rows, pitch.value)
    if n_rows == 0:
        return 0, 0, np.zeros(0, np.float32)
    R = pitch.value // 4
    img = np.full(n_rows * R, np.nan, np.float32)
    assert eng.lib.ka_debug_checkpoints(eng.handle, img.ctypes.data, img.size, ctypes.byref(pitch)) == n_rows
    assert pitch.value == 4 * R
    return n_rows, R, img


def check(eng, form, name, ref, what):
    n_rows, R, img = read_back(eng, ref)
    if form == "wave":
        assert R == P.WAVE_RING or n_rows == 0
    ring = ref.L > R
    assert not ring or R & (R - 1) == 0
    got = B.read_rows(img, ref, R, ring or form == "wave")
    d = B.first_difference(ref, got)
    assert d is None, (f"{name} [{form}] {what}: row {d[0]} (frame {d[1]}) differs in {d[7]} of its cells, first at position {d[2]}: got {d[3]!r}, "
                       f"want {d[4]!r}; {d[5]} above lo, {d[6]} below hi - 1; {B.rows_differ(ref, got)} cells differ in all")
    return img, R


def check_dead_slots(name, ref, img, R, what):
    for k, dead in enumerate(B.dead_slots(img, ref, R)):
        bad = np.nonzero(dead.view(np.int32) != P.NEG.view(np.int32))[0]
        assert bad.size == 0, f"{name} [wave] {what}: row {k}: {bad.size} of {dead.size} dead slots do not hold -inf, first {dead[bad[0]]!r}"


@pytest.mark.parametrize("form,table,name", PAIRS)
def test_every_in_band_cell_of_every_checkpoint_row(env, form, table, name):
    ka, eng = env
    mode, _, width = form.partition("/")
    eng.set_mode(mode)
    eng.set_tile_width(int(width or 0))
    eng.set_backtrace("serial")
    lp, lab, beam, mm, ref, others = reference(table, name)
    res, status, _ = ka.ctc_best_path_batch([lp], [lab], beam, mm, return_status=True)
    assert list(status) == [0] and np.array_equal(res[0][0], ref.path), name
    img, R = check(eng, form, name, ref, "alone")
    if form == "wave":
        check_dead_slots(name, ref, img, R, "alone")
    # as the longest of three lattices in one launch (descriptor 0 whatever its place in the call)
    res, status, _ = ka.ctc_best_path_batch([others[0][0], lp, others[1][0]], [others[0][1], lab, others[1][1]], beam, mm, return_status=True)
    assert status[1] == 0 and np.array_equal(res[1][0], ref.path), name
    img, R = check(eng, form, name, ref, "in a launch of three")
    if form == "wave":
        check_dead_slots(name, ref, img, R, "in a launch of three")


def test_no_rows_where_no_checkpoints_are_stored(env):
    """The exact form stores back-pointers, the generic kernels too, and a lattice with a -inf is declined by the
    checkpointed forms: ka_debug_checkpoints reports no rows."""
    ka, eng = env
    lp, lab = P.inputs(200, 40, 39, 5, False, False)
    pitch = ctypes.c_int64(-1)
    eng.set_tile_width(0)
    eng.set_backtrace("serial")
    eng.set_mode("wave_exact")
    ka.ctc_best_path_batch([lp], [lab], 64, 4)
    assert eng.lib.ka_debug_checkpoints(eng.handle, None, 0, ctypes.byref(pitch)) == 0 and pitch.value == 0
    eng.set_mode("wave")
    ka.ctc_best_path_batch([lp], [lab], 64, 4)
    assert eng.lib.ka_debug_checkpoints(eng.handle, None, 0, ctypes.byref(pitch)) == (200 - 1) // 32 and pitch.value == 4096
    ka.ctc_best_path_batch([lp], [lab], 64, 6)      # max_move 6: the generic kernels
    assert eng.lib.ka_debug_checkpoints(eng.handle, None, 0, ctypes.byref(pitch)) == 0 and pitch.value == 0
    holed = lp.copy()
    holed[7, 3] = -np.inf
    for mode in ("wave", "tiled"):
        eng.set_mode(mode)
        res = ka.ctc_best_path_batch([holed], [lab], 64, 4)
        assert np.array_equal(res[0][0], O.ctc_best_path_c(holed, lab, 64, 4)[0])
        assert eng.lib.ka_debug_checkpoints(eng.handle, None, 0, ctypes.byref(pitch)) == 0 and pitch.value == 0, mode
