"""Inputs of the resumable best-path tests beyond tests/band_cases.py (tests/test_resume_cpu.py asserts on tests/resume_ref.py
that they do what their names say; tests/test_resume_gpu.py runs them through the kernels).

Block-edge cuts: a lattice of 24 frames cut at frame 12, where the table steps to a low end that is a multiple of 16 (16; 1024
and 1040, which lie on the wrapped ring of 1024 slots).  The planted path sits d = 1, 2 or 3 cells below that low end in frame
11 and inside the band in frame 12, so chunk B's ``entry`` is one of the three cells below its ring's lowest block: the cells
its kernel cannot take from a neighbouring lane.  The positions are far from 0, so the whole lattice starts from a row too
(three free cells around the plant's first position).

Excerpt: a recording that holds positions 50 .. 89 of its text.
"""
import numpy as np

import band_cases as C
import resume_ref as RR

EDGE_T, EDGE_CUT, EDGE_BEAM = 24, 12, 32
EDGE_MOVE = {1: 2, 2: 3, 3: 3}   # the plant's move at the cut, from d below the low end
# (low end at the cut, S, d) -> the seed of planted_lattice for which the reference's path does follow the plant over the cut
EDGE_SEEDS = {(16, 40, 1): 0, (16, 40, 2): 1, (16, 40, 3): 1, (1024, 560, 1): 1, (1024, 560, 2): 2, (1024, 560, 3): 1,
              (1040, 560, 1): 1, (1040, 560, 2): 2, (1040, 560, 3): 3}


def free_row(L, lo, hi):
    row = np.full(L, np.nan, np.float32)
    row[lo:hi] = 0.0
    return row


def edge_plant(lo_new, d):
    k = EDGE_CUT
    true = np.empty(EDGE_T, np.int64)
    true[:k] = lo_new - d - (k - 1 - np.arange(k))
    if d == 2:
        # lo - 2 and lo are both blanks and share the predecessor lo - 3, and the cell lo + 1 takes the nearer of two equal
        # predecessors.  So the plant comes to lo - 2 from lo - 5 (a move of 3, which lo cannot make) a frame early and waits:
        # lo is then strictly worse in both frames.
        true[k - 2] = lo_new - 2
        true[:k - 2] = lo_new - 5 - (k - 3 - np.arange(k - 2))
    true[k:] = lo_new - d + EDGE_MOVE[d] + np.arange(EDGE_T - k)
    return true


def block_edge(lo_new, S, d, seed=None):
    """(lp, labels, band_lo, init row, beam, max_move, the planted path)"""
    true = edge_plant(lo_new, d)
    L = 2 * S + 1
    lp, lab = C.planted_lattice(EDGE_SEEDS[(lo_new, S, d)] if seed is None else seed, EDGE_T, S, true)
    lo = np.full(EDGE_T, max(true[0] - 4, 0), np.int64)
    lo[EDGE_CUT:] = lo_new
    return lp, lab, lo, free_row(L, true[0] - 1, true[0] + 2), EDGE_BEAM, 4, true


def edge_entry_depth(case):
    """d as the reference sees it: how far below chunk B's first low end its entry lies (None without a path)"""
    lp, lab, lo, init, beam, mm, _ = case
    k = EDGE_CUT
    try:
        a = RR.best_path_resume(lp[:k], lab, lo[:k], init, RR.END_HIGHEST, beam, mm)
        b = RR.best_path_resume(lp[k:], lab, lo[k:], a[5], RR.END_HIGHEST, beam, mm)
    except ValueError:
        return None
    return int(lo[k]) - b[4]


def find_edge_seed(lo_new, S, d, tries=300):
    for seed in range(tries):
        if edge_entry_depth(block_edge(lo_new, S, d, seed)) == d:
            return seed
    return None


EDGE_KEYS = [(lo_new, S, d) for lo_new, S in ((16, 40), (1024, 560), (1040, 560)) for d in (1, 2, 3)]


# ---- excerpt ----
def excerpt():
    """(lp, labels, band_lo, beam, max_move): S = 60, T = 40, a plant on positions 50 .. 89, beam 2L (unbanded)"""
    S, T = 60, 40
    lp, lab = C.planted_lattice(77, T, S, 50 + np.arange(T))
    return lp, lab, np.zeros(T, np.int64), 2 * (2 * S + 1), 4


# ---- what the GPU tests run, as scenarios: a function of ``run(lp, labels, band_lo, init, end, beam, max_move)``, which answers
# ("ok", path, labels, scores, total, entry, final), ("empty", final) or ("bad_args",), that returns the list of the answers
# it got.  tests/test_resume_cpu.py runs them on the reference with and without a planted fault, tests/test_resume_gpu.py on
# the kernels. ----
def ref_run(fault=None):
    def run(lp, lab, lo, init, end, beam, mm):
        try:
            return ("ok",) + RR.best_path_resume(lp, lab, lo, init, end, beam, mm, fault=fault)
        except RR.EmptyBeam as e:
            return ("empty", e.final)
        except RR.BadArgs:
            return ("bad_args",)
    return run


def chain(run, lp, lab, lo, k, init, beam, mm):
    """cut and resume at frame k: chunk A, chunk B from A's last row, A again with end = B's entry"""
    out = [run(lp[:k], lab, lo[:k], init, RR.END_HIGHEST, beam, mm)]
    if out[0][0] == "ok":
        out.append(run(lp[k:], lab, lo[k:], out[0][6], RR.END_HIGHEST, beam, mm))
        if out[1][0] == "ok":
            out.append(run(lp[:k], lab, lo[:k], init, out[1][5], beam, mm))
    return out


def joined(out):
    """(path, labels, scores, total) of a chain that came through, else None"""
    if len(out) < 3 or out[2][0] != "ok":
        return None
    return tuple(np.concatenate([out[2][i], out[1][i]]) for i in (1, 2, 3)) + (out[1][4],)


def same_answers(a, b):
    if len(a) != len(b):
        return False
    for x, y in zip(a, b):
        if x[0] != y[0] or len(x) != len(y):
            return False
        for u, v in zip(x[1:], y[1:]):
            if not (RR.same_bits(np.atleast_1d(np.float32(u)), np.atleast_1d(np.float32(v))) if np.ndim(u) == 0 and isinstance(u, (float, np.floating))
                    else (u == v if np.ndim(u) == 0 else RR.same_bits(u, v))):
                return False
    return True


CUT_NAMES = ("staircase", "ride_hi", "ring_wrap", "ninf", "step1009", "mm2", "mm3", "beam1", "T5", "T6", "T7")
# the cuts of band_cases at which chunk B's entry lies below its first low end (every cut for T <= 130, every 7th frame above:
# tests/test_resume_cpu.py finds these again)
BELOW_CUTS = {"ride_lo": tuple(range(1, 32)),
              "shifted": (3, 4, 6, 7, 21, 26, 27, 29, 30, 31, 33, 34, 39, 64, 65, 69, 70, 75, 79, 80, 83, 87, 88, 96, 100, 107),
              "ninf": (43, 49, 52), "step1009": (350,), "beam1": (2, 4, 6, 8, 10, 12, 14, 16, 18)}


def cuts_of(name):
    T = C.case(name)[0].shape[0]
    ks = set(BELOW_CUTS.get(name, ()))
    if name in CUT_NAMES:
        ks |= {k for k in (1, 2, 3, 4, 5, T - 3, T - 2, T - 1) if 1 <= k < T}
    return sorted(ks)


CUT_CASES = [n for n in C.NAMES if n in CUT_NAMES or n in BELOW_CUTS]


def cut_scenario(name, k):
    lp, lab, lo, beam, mm = C.case(name)
    return lambda run: chain(run, lp, lab, lo, k, None, beam, mm)


def edge_scenario(key):
    lp, lab, lo, init, beam, mm, _ = block_edge(*key)
    return lambda run: chain(run, lp, lab, lo, EDGE_CUT, init, beam, mm)


def flat():
    """every live cell scores 0.0: the best cell is the FIRST maximum, the lowest live position"""
    T, S = 6, 10
    return np.zeros((T, C.V), np.float32), np.arange(1, S + 1, dtype=np.int32) % (C.V - 1) + 1, np.zeros(T, np.int64), 50, 4


def start_row_scenarios():
    """single calls on const0 (band [0, 40), L = 121) and shifted: rows that leave no live cell, a +inf cell, the three ends"""
    lp, lab, lo, beam, mm = C.case("const0")
    L = 2 * len(lab) + 1
    lo20 = lo + 20                      # band [20, 60): frame 0 reads cells 17 .. 59
    lp6, lo6 = lp[:6], lo[:6]          # after 6 frames the band's upper cells are not reached yet
    plain = RR.best_path_resume(lp6, lab, lo6, None, RR.END_HIGHEST, beam, mm)
    live = np.nonzero(~np.isnan(plain[5]))[0]
    dead_in_band = int(live[-1]) + 1
    assert dead_in_band < beam
    pinf = free_row(L, 20, 30)
    pinf[25] = np.inf
    pinf_outside = free_row(L, 20, 30)
    pinf_outside[100] = np.inf
    ninf_row = free_row(L, 17, 40)
    ninf_row[17:40:3] = -np.inf
    flp, flab, flo, fbeam, fmm = flat()
    elp, elab, elo, ebeam, emm = excerpt()
    eL = 2 * len(elab) + 1
    return {
        "above_hi": lambda run: [run(lp, lab, lo20, free_row(L, 60, 70), RR.END_HIGHEST, beam, mm)],
        "below_reach": lambda run: [run(lp, lab, lo20, free_row(L, 0, 17), RR.END_HIGHEST, beam, mm)],
        "lowest_reach": lambda run: [run(lp, lab, lo20, free_row(L, 17, 18), RR.END_HIGHEST, beam, mm)],
        "all_dead": lambda run: [run(lp, lab, lo20, free_row(L, 0, 0), RR.END_HIGHEST, beam, mm)],
        "ninf_cells": lambda run: [run(lp, lab, lo20, ninf_row, e, beam, mm) for e in (RR.END_HIGHEST, RR.END_BEST)],
        "pinf": lambda run: [run(lp, lab, lo20, pinf, RR.END_HIGHEST, beam, mm)],
        "pinf_outside": lambda run: [run(lp, lab, lo20, pinf_outside, RR.END_HIGHEST, beam, mm)],
        "end_live": lambda run: [run(lp6, lab, lo6, None, int(p), beam, mm) for p in (live[0], live[len(live) // 2], live[-1])],
        "end_dead_in_band": lambda run: [run(lp6, lab, lo6, None, dead_in_band, beam, mm)],
        "end_outside_band": lambda run: [run(lp6, lab, lo6, None, L - 1, beam, mm)],
        "end_best": lambda run: [run(lp6, lab, lo6, None, RR.END_BEST, beam, mm)],
        "flat_best": lambda run: [run(flp, flab, flo, i, RR.END_BEST, fbeam, fmm) for i in (None, free_row(2 * len(flab) + 1, 2, 9))],
        "excerpt": lambda run: [run(elp, elab, elo, free_row(eL, 0, eL), RR.END_BEST, ebeam, emm), run(elp, elab, elo, None, RR.END_BEST, ebeam, emm)],
    }
