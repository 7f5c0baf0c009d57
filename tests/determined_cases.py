"""Inputs of the determined-prefix tests (tests/test_determined_cpu.py asserts on tests/determined_ref.py that they do what their
names say; tests/test_determined_gpu.py runs them through the kernels).  Named families, each at the smallest shape that reaches
its condition.

A case is a dict: lp, lab, beam, mm, init (a start row or None), end (-1 highest, -2 best, or a position), and either
  table  [T] the caller's band (ka_ctc_best_path_determined), or
  first_lo, period  the self-steering band (ka_ctc_best_path_tracking_determined).
``form``: "wave" (the case runs as it is in the one-wavefront form, and widened past V = 64 in the generic form), or "generic"
(the case itself needs the generic form: a band above 1009, V above 64 or max_move above 4).
"""
import numpy as np

import band_cases as C
import determined_ref as DR
import posterior_ref as PR
import track_resume_ref as TR
from oracle import oracle as O

V_HASH = 39


def diagonal(T, L, beam):
    t = np.arange(int(T), dtype=np.int64)
    return np.maximum(0, np.int64(L) * t // np.int64(T) - np.int64(beam // 2))


def free_row(L, lo=0, hi=None):
    row = np.full(L, np.nan, np.float32)
    row[lo:L if hi is None else hi] = 0.0
    return row


def banded(lp, lab, table, beam, mm=4, init=None, end=-1, form="wave"):
    return dict(lp=np.ascontiguousarray(lp, np.float32), lab=np.asarray(lab, np.int32), table=np.asarray(table, np.int64), beam=beam, mm=mm,
                init=init, end=end, form=form)


def tracking(lp, lab, beam, period, mm=4, first_lo=0, init=None, end=-1, form="wave"):
    return dict(lp=np.ascontiguousarray(lp, np.float32), lab=np.asarray(lab, np.int32), first_lo=int(first_lo), period=period, beam=beam,
                mm=mm, init=init, end=end, form=form)


def hash_lattice(T, S, seed, V=V_HASH):
    return O.hash_logprobs(T, V, seed), O.hash_labels(S, V, seed)


def flat_lattice(T, S, V=C.V):
    return np.zeros((T, V), np.float32), (np.arange(S, dtype=np.int32) % (V - 1)) + 1


def peaked_lattice(T, S, beam, seed, V=C.V):
    lp, lab, _ = PR.peaked(T, S, V, beam, 4, seed)
    return lp.astype(np.float32), lab


# ---- the families ----
def _short(T, track):
    def make():
        lp, lab = C.random_lattice(700 + T, T, 10)
        if track:
            return tracking(lp, lab, 12, 4)
        return banded(lp, lab, diagonal(T, 21, 12), 12)
    return make


def _s0():
    lp, lab = C.random_lattice(711, 5, 0)
    return banded(lp, lab, np.zeros(5, np.int64), 4)


def _one_cell():
    # a band of one cell that climbs a position every second frame: one live cell throughout, determined = T
    lp, lab, lo, beam, mm = C.case("beam1")
    return banded(lp, lab, lo, beam, mm)


def _flat_wide(free):
    def make():
        T, S = 120, 12
        lp, lab = flat_lattice(T, S)
        return banded(lp, lab, np.zeros(T, np.int64), 1000, init=free_row(2 * S + 1) if free else None)
    return make


def _inside(kind, big):
    def make():
        T, S, beam = (300, 100, 64) if big else (64, 20, 16)
        if kind == "hash":
            lp, lab = hash_lattice(T, S, 31 + big)
        elif kind == "flat":
            lp, lab = flat_lattice(T, S)
        else:
            lp, lab = peaked_lattice(T, S, beam, 41 + big)
        return banded(lp, lab, diagonal(T, 2 * S + 1, beam), beam)
    return make


RING_T, RING_S, RING_BEAM = 400, 600, 64


def _ring(k):
    """the first k frames of the T = 400, S = 600 lattice under its diagonal band: the band straddles position 1024 there"""
    def make():
        lp, lab = hash_lattice(RING_T, RING_S, 51)
        return banded(lp[:k], lab, diagonal(RING_T, 2 * RING_S + 1, RING_BEAM)[:k], RING_BEAM)
    return make


def find_ring_cut():
    """the cuts of the ring lattice at which a set of more than one cell crosses slot 1023 -> 0 during the walk"""
    out = []
    for k in range(330, 360):
        c = _ring(k)()
        d, st = DR.determined(c["lp"], c["lab"], c["table"], None, c["beam"], c["mm"], with_stats=True)
        if st["wrap"]:
            out.append(k)
    return out


RING_CUT = 345


def _wide(beam, V=V_HASH, mm=4, form="wave"):
    def make():
        T, S = 24, 520
        lp, lab = hash_lattice(T, S, 61, V)
        return banded(lp, lab, np.zeros(T, np.int64), beam, mm, init=free_row(2 * S + 1, 0, 1041), form=form)
    return make


def _wide_flat(beam, form="wave"):
    def make():
        T, S = 24, 520
        lp, lab = flat_lattice(T, S)
        return banded(lp, lab, np.zeros(T, np.int64), beam, init=free_row(2 * S + 1, 3, 700), form=form)
    return make


def _moves(mm):
    def make():
        lp, lab = C.random_lattice(720 + mm, 33, 10)
        if mm == 1:   # (only position 0 is ever live: the band stays on it)
            return banded(lp, lab, np.zeros(33, np.int64), 12, mm)
        return banded(lp, lab, diagonal(33, 21, 12), 12, mm)
    return make


def _label0():
    lp, lab = C.random_lattice(731, 40, 16)
    lab[::3] = 0
    return banded(lp, lab, diagonal(40, 33, 12), 12)


def _ninf_cells():
    lp, lab = C.random_lattice(732, 40, 16, ninf=True)
    return banded(lp, lab, diagonal(40, 33, 16), 16)


def _ninf_frames():
    # the last three frames are -inf in every column: every live cell scores -inf, and they tie
    lp, lab = C.random_lattice(733, 40, 16)
    lp[-3:] = -np.inf
    return banded(lp, lab, diagonal(40, 33, 16), 16)


def _ninf_row():
    lp, lab = C.random_lattice(734, 20, 16)
    row = free_row(33, 0, 12)
    row[0:12:2] = -np.inf
    return banded(lp, lab, np.zeros(20, np.int64), 16, init=row)


def _empties():
    lp, lab, lo, beam, mm = C.case("no_overlap")
    return banded(lp, lab, lo, beam, mm)


def _dead_end():
    c = _inside("hash", False)()
    live = DR.live_cells(c["lp"], c["lab"], c["table"], None, c["beam"], c["mm"])
    dead = [p for p in range(2 * len(c["lab"]) + 1) if p not in set(live.tolist())]
    c["end"] = int(dead[-1])
    return c


def _live_end():
    c = _inside("hash", False)()
    live = DR.live_cells(c["lp"], c["lab"], c["table"], None, c["beam"], c["mm"])
    c["end"] = int(live[0])
    return c


def _bad_label():
    c = _inside("hash", False)()
    c["lab"] = c["lab"].copy()
    c["lab"][3] = 1000   # (no vocabulary of these tests is that large, widened or not)
    return c


def _nan():
    c = _inside("hash", False)()
    c["lp"] = c["lp"].copy()
    c["lp"][7, 2] = np.nan
    return c


def _bad_table():
    c = _inside("hash", False)()
    c["table"] = c["table"].copy()
    c["table"][5] = c["table"][4] - 1 if c["table"][4] > 0 else 2 * len(c["lab"]) + 1
    c["table"][20] = c["table"][19] + 5
    c["table"][21] = c["table"][19]
    return c


def _pinf_row():
    c = _inside("hash", False)()
    row = free_row(41, 0, 5)
    row[2] = np.inf
    c["init"] = row
    return c


def _track(kind, period, part):
    """a T = 64, S = 20, beam 16 lattice under the self-steering band, whole ("all"), or cut at frame 32: its first chunk ("a")
    and its second from the first's last row and next_lo ("b")"""
    def make():
        T, S, beam = 64, 20, 16
        if kind == "hash":
            lp, lab = hash_lattice(T, S, 71)
        else:
            lp, lab = peaked_lattice(T, S, beam, 72)
        if part == "all":
            return tracking(lp, lab, beam, period)
        if part == "a":
            return tracking(lp[:32], lab, beam, period)
        a = TR.best_path_tracking_resume(lp[:32], lab, 0, None, TR.END_HIGHEST, beam, 4, period)
        return tracking(lp[32:], lab, beam, period, first_lo=a[7], init=a[6])
    return make


def _track_free():
    lp, lab = flat_lattice(40, 12)
    return tracking(lp, lab, 1000, 8, init=free_row(25))


def _track_generic():
    lp, lab = hash_lattice(48, 30, 75, 65)
    return tracking(lp, lab, 20, 8, mm=5, form="generic")


CASES = {
    "S0": _s0, "one_cell": _one_cell, "flat_wide_null": _flat_wide(False), "flat_wide_free": _flat_wide(True),
    "ring_wrap": _ring(RING_CUT),
    "wide1009": _wide(1009), "wide1009_flat": _wide_flat(1009), "wide1010": _wide(1010, form="generic"), "wide1010_flat": _wide_flat(1010, "generic"),
    "V65": _wide(64, V=65, form="generic"), "mm5": _wide(64, mm=5, form="generic"),
    "label0": _label0, "ninf_cells": _ninf_cells, "ninf_frames": _ninf_frames, "ninf_row": _ninf_row, "empties": _empties,
    "dead_end": _dead_end, "live_end": _live_end, "bad_label": _bad_label, "nan": _nan, "bad_table": _bad_table, "pinf_row": _pinf_row,
    "track_free": _track_free, "track_generic": _track_generic,
}
SHORT_T = (1, 2, 5, 17, 33, 66)
CASES.update({f"T{T}": _short(T, False) for T in SHORT_T})
CASES.update({f"track_T{T}": _short(T, True) for T in SHORT_T})
INSIDE = [f"{kind}_{'big' if big else 'small'}" for kind in ("hash", "flat", "peaked") for big in (0, 1)]
CASES.update({f"{kind}_{'big' if big else 'small'}": _inside(kind, big) for kind in ("hash", "flat", "peaked") for big in (0, 1)})
CASES.update({f"mm{mm}": _moves(mm) for mm in (1, 2, 3, 4)})
CASES.update({f"track_{kind}_p{period}_{part}": _track(kind, period, part)
              for kind in ("hash", "peaked") for period in (4, 16) for part in ("all", "a", "b")})
NAMES = list(CASES)
FAILING = {"bad_label": -5, "nan": -6, "bad_table": -2, "pinf_row": -2}   # the lattice's own status
_made, _want = {}, {}


def case(name):
    if name not in _made:
        _made[name] = CASES[name]()
    return _made[name]


def reference(c, fault=None, with_stats=False):
    if "table" in c:
        return DR.determined(c["lp"], c["lab"], c["table"], c["init"], c["beam"], c["mm"], fault, with_stats)
    return DR.tracking_determined(c["lp"], c["lab"], c["first_lo"], c["init"], c["beam"], c["mm"], c["period"], fault, with_stats)


def want(name):
    """(determined, stats) of the reference, computed once"""
    if name not in _want:
        _want[name] = reference(case(name), with_stats=True)
    return _want[name]
