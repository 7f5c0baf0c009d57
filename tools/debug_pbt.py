#!/usr/bin/env python3
"""Chunk entries and chunk maps of the parallel backtrace for ONE shape given by hand, every cell against the float32
reference with back-pointers of tests/pbt_ref.py (the test of the same comparison: tests/test_parallel_backtrace_gpu.py).

    python tools/debug_pbt.py [--checkpoints] [T V S beam [mode [max_move]]]      mode: wave | tiled/256 | tiled/128

Prints the chunks and cells that differ; exit status 1 if any does.  With --checkpoints the forward pass's checkpoint rows
are compared instead (ka_debug_checkpoints, every in-band cell as bits; the test: tests/test_forward_checkpoints_gpu.py) and
the first cell that differs is printed: row, frame, position, both values and the distances to lo and to hi - 1.
"""
import ctypes
import faulthandler
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
faulthandler.dump_traceback_later(90, exit=True)
import numpy as np
import kokoro_align_amd as ka
from kokoro_align_amd import _lib
from oracle import oracle as O
import pbt_ref as P

checkpoints = "--checkpoints" in sys.argv
if checkpoints:
    sys.argv.remove("--checkpoints")
T, V, S, beam = (int(x) for x in sys.argv[1:5]) if len(sys.argv) >= 5 else (3000, 39, 700, 1000)
form = sys.argv[5] if len(sys.argv) > 5 else "wave"
mm = int(sys.argv[6]) if len(sys.argv) > 6 else 4
mode, _, width = form.partition("/")
lp = O.hash_logprobs(T, V, 3)
lab = O.hash_labels(S, V, 3)
ref = P.best_path_with_moves(lp, lab, beam, mm)
eng = _lib.default_engine(0)
eng.set_mode(mode)
eng.set_tile_width(int(width or 0))
eng.set_backtrace("serial" if checkpoints else "parallel")
try:
    got = ka.ctc_best_path(lp, lab, beam_size=beam, max_move=mm, verbose=False)
    if checkpoints:
        import bestpath_cases as B
        pitch = ctypes.c_int64(0)
        rows = eng.lib.ka_debug_checkpoints(eng.handle, None, 0, ctypes.byref(pitch))
        img = np.full(rows * pitch.value // 4, np.nan, np.float32)
        eng.lib.ka_debug_checkpoints(eng.handle, img.ctypes.data, img.size, ctypes.byref(pitch))
    R, ring = P.WAVE_RING, True
    if mode == "tiled":
        pitch = ctypes.c_int64(0)
        assert eng.lib.ka_debug_plan_tiles_width(T, S, V, beam, mm, int(width or 256), None, None, 0, ctypes.byref(pitch)) > 0, "not tileable"
        R, ring = pitch.value // 4, 2 * S + 1 > pitch.value // 4
    nck, nsup = len(ref.te), len(ref.super_entries)
    ent = np.zeros(nck + nsup, np.int32)
    m0 = np.full(nck * R, 255, np.uint8)
    n = eng.lib.ka_debug_chunk_entries(eng.handle, ent.ctypes.data, ent.size, m0.ctypes.data, m0.size)
finally:
    eng.set_mode("auto")
    eng.set_tile_width(0)
    eng.set_backtrace("auto")
if checkpoints:
    R = pitch.value // 4
    print(f"{form}: {rows} checkpoint rows of {R} floats (the reference has {len(ref.rows)}), path equal {np.array_equal(got[0], ref.path)}")
    if rows != len(ref.rows):
        sys.exit(1)
    rows_got = B.read_rows(img, ref, R, mode == "wave" or ref.L > R)
    d = B.first_difference(ref, rows_got)
    if d is None:
        print("checkpoints: all in-band cells equal")
        sys.exit(0)
    print(f"first difference: row {d[0]} (frame {d[1]}), position {d[2]}: got {d[3]!r}, want {d[4]!r}; {d[5]} above lo, {d[6]} below hi - 1; "
          f"{d[7]} cells of that row differ, {B.rows_differ(ref, rows_got)} in all")
    sys.exit(1)
print(f"{form}: row of {R} slots ({'ring' if ring else 'whole axis'}), entries returned {n} of {nck} + {nsup}, path equal {np.array_equal(got[0], ref.path)}")
bad = np.nonzero(ent[:nck] != ref.entries)[0]
print("wrong chunk entries", len(bad), bad[:20], "true", ref.entries[bad[:8]], "got", ent[bad[:8]])
print("super entries", ent[nck:], "true", ref.super_entries)
wrong = len(bad) + int(np.sum(ent[nck:] != ref.super_entries)) + (n != nck + nsup)
maps = P.read_maps(m0, ref, R, ring)
for c in range(1, nck):
    d = np.nonzero(maps[c] != ref.rise[c])[0]
    if d.size:
        wrong += 1
        lo = int(ref.lo[ref.te[c]])
        print(f"chunk {c}: {d.size} of {len(maps[c])} positions differ ({int(np.sum(ref.reachable[c][d]))} reachable); first {(d[:16] + lo).tolist()}")
        print("   true", ref.rise[c][d[:16]], "got", maps[c][d[:16]])
print("maps: all cells equal" if not wrong else f"{wrong} differences")
sys.exit(1 if wrong else 0)
