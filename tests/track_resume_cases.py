"""Inputs of the resumable tracking best-path tests (tests/test_tracking_resume_cpu.py asserts on tests/track_resume_ref.py that
they do what their names say; tests/test_tracking_resume_gpu.py runs them through the kernels).

A scenario is a function of ``run(lp, labels, first_lo, init, end, beam, max_move, period)``, which answers
("ok", path, labels, scores, table, total, entry, final, next_lo), ("empty", final, table, next_lo) or ("bad_args",), that
returns the list of the answers it got.  SCENARIOS holds:
  * the cuts of the tests/track_cases.py families at k = period, at the last multiple of the period below T and, for T <= 130, at
    every multiple of the period (chain: chunk A, chunk B from A's last row and next_lo, A again with end = B's entry), and
    every family uncut through the new entry point;
  * the three cuts at which chunk B's entry lies 1, 2 and 3 cells below its first_lo (DEPTH_CUTS);
  * the same three depths with a first_lo that is a multiple of 16 (EDGE_CUTS): the cells a lane of the one-wavefront form
    cannot take from its neighbour.  A cut found by search with an even first_lo, moved up by an even number of positions: filler
    labels in front of the transcript, a start row with one live cell, first_lo on that cell - the recurrence is the same;
  * T = 4 and 8 at period 4; single calls on start rows, ends and first_lo values that fail or nearly do.
"""
import numpy as np

import band_cases as C
import track_cases as TC
import track_resume_ref as R

END_OF = {"highest": R.END_HIGHEST, "best": R.END_BEST}

# (seed of band_cases.random_lattice(1000 + seed, T, S), T, S, beam, max_move, period, cut) -> depth
DEPTH_CUTS = {1: (57, 23, 27, 4, 4, 8, 16), 2: (5, 34, 17, 8, 4, 4, 20), 3: (2688, 17, 6, 12, 4, 4, 4)}
# ... with an even first_lo behind the cut, and the shift that takes it to 16
EDGE_CUTS = {1: ((103, 23, 11, 4, 4, 4, 12), 14), 2: ((6837, 26, 23, 8, 4, 4, 4), 14), 3: ((746, 24, 16, 12, 4, 8, 8), 12)}


def free_row(L, lo, hi):
    row = np.full(L, np.nan, np.float32)
    row[lo:hi] = 0.0
    return row


def ref_run(fault=None):
    def run(lp, lab, first_lo, init, end, beam, mm, period):
        try:
            return ("ok",) + R.best_path_tracking_resume(lp, lab, first_lo, init, end, beam, mm, period, fault=fault)
        except R.EmptyBeam as e:
            return ("empty", e.final, e.band_lo, e.next_lo)
        except R.BadArgs:
            return ("bad_args",)
    return run


def chain(run, lp, lab, k, first_lo, init, end, beam, mm, period):
    """cut and resume at frame k: chunk A, chunk B from A's last row and next_lo with the lattice's end, A again with end = B's entry"""
    out = [run(lp[:k], lab, first_lo, init, R.END_HIGHEST, beam, mm, period)]
    if out[0][0] == "ok":
        out.append(run(lp[k:], lab, out[0][8], out[0][7], end, beam, mm, period))
        if out[1][0] == "ok":
            out.append(run(lp[:k], lab, first_lo, init, out[1][6], beam, mm, period))
    return out


def joined(out):
    """(path, labels, scores, table, B's total, B's last row, B's next_lo) of a chain that came through, else None"""
    if len(out) < 3 or out[2][0] != "ok":
        return None
    return tuple(np.concatenate([out[2][i], out[1][i]]) for i in (1, 2, 3, 4)) + (out[1][5], out[1][7], out[1][8])


def same_answers(a, b):
    if len(a) != len(b):
        return False
    for x, y in zip(a, b):
        if x[0] != y[0] or len(x) != len(y):
            return False
        for u, v in zip(x[1:], y[1:]):
            if np.ndim(u) == 0 and isinstance(u, (float, np.floating)):
                same = R.same_bits(np.atleast_1d(np.float32(u)), np.atleast_1d(np.float32(v)))
            else:
                same = u == v if np.ndim(u) == 0 else R.same_bits(u, v)
            if not same:
                return False
    return True


# ---- the cuts of the track_cases families ----
def cuts_of(name, every=False):
    lp, _, _, _, P, _ = TC.case(name)
    T = lp.shape[0]
    ks = {P, T - (T % P or P)}
    if T <= 130 or every:
        ks |= set(range(P, T, P))
    return sorted(k for k in ks if P <= k < T)


def cut_scenario(name, k):
    lp, lab, beam, mm, P, end_rule = TC.case(name)
    return lambda run: chain(run, lp, lab, k, 0, None, END_OF[end_rule], beam, mm, P)


def uncut_scenario(name):
    lp, lab, beam, mm, P, end_rule = TC.case(name)
    return lambda run: [run(lp, lab, 0, None, END_OF[end_rule], beam, mm, P)]


# ---- entry below first_lo ----
def depth_case(d):
    seed, T, S, beam, mm, P, k = DEPTH_CUTS[d]
    lp, lab = C.random_lattice(1000 + seed, T, S)
    return lp, lab, k, 0, None, R.END_HIGHEST, beam, mm, P


def edge_case(d):
    (seed, T, S, beam, mm, P, k), shift = EDGE_CUTS[d]
    lp, lab = C.random_lattice(1000 + seed, T, S)
    lab = np.concatenate([np.full(shift // 2, 1, lab.dtype), lab])
    return lp, lab, k, shift, free_row(2 * len(lab) + 1, shift, shift + 1), R.END_HIGHEST, beam, mm, P


def depth_of(out):
    """how far below chunk B's first_lo its entry lies, and that first_lo (None for a chain that did not come through)"""
    if len(out) < 2 or out[1][0] != "ok":
        return None
    return out[0][8] - out[1][6], out[0][8]


# ---- short lattices at period 4 ----
def short_case(T):
    lp, lab = C.random_lattice(90 + T, T, 6)
    return lp, lab, 8, 4, 4


# ---- single calls ----
def single_scenarios():
    lp, lab = C.random_lattice(95, 12, 20)
    L = 2 * len(lab) + 1
    beam, mm, P = 16, 4, 4
    plain = R.best_path_tracking_resume(lp[:3], lab, 0, None, R.END_HIGHEST, beam, mm, P)
    live = np.nonzero(~np.isnan(plain[6]))[0]
    dead_in_band = next(p for p in range(int(plain[3][-1]), int(plain[3][-1]) + beam) if p not in live)
    ninf_row = free_row(L, 8, 24)
    ninf_row[8:24:3] = -np.inf
    pinf = free_row(L, 8, 24)
    pinf[12] = np.inf
    pinf_outside = free_row(L, 8, 24)
    pinf_outside[L - 1] = np.inf
    glp, glab = C.random_lattice(96, 12, 20, V=65)   # the generic form
    gpinf = free_row(L, 8, 24)
    gpinf[9] = np.inf
    return {
        # a NULL row is the cell 0: out of frame 0's reach from first_lo = max_move on
        "null_row_lo3": lambda run: [run(lp, lab, mm - 1, None, R.END_HIGHEST, beam, mm, P)],
        "null_row_lo4": lambda run: [run(lp, lab, mm, None, R.END_HIGHEST, beam, mm, P)],
        "null_row_lo1030": lambda run: [run(lp, np.resize(lab, 600), 1030, None, R.END_HIGHEST, beam, mm, P)],
        "null_row_lo4_generic": lambda run: [run(glp, glab, mm, None, R.END_HIGHEST, beam, mm, P)],
        "row_above_hi": lambda run: [run(lp, lab, 4, free_row(L, 20, 30), R.END_HIGHEST, beam, mm, P)],
        "row_below_reach": lambda run: [run(lp, lab, 12, free_row(L, 0, 9), R.END_HIGHEST, beam, mm, P)],
        "row_lowest_reach": lambda run: [run(lp, lab, 12, free_row(L, 9, 10), R.END_HIGHEST, beam, mm, P)],
        "first_lo_top": lambda run: [run(lp, lab, L - 1, free_row(L, L - 3, L), e, beam, mm, P) for e in (R.END_HIGHEST, R.END_BEST, L - 1)],
        "ninf_cells": lambda run: [run(lp, lab, 10, ninf_row, e, beam, mm, P) for e in (R.END_HIGHEST, R.END_BEST)],
        "ninf_cells_generic": lambda run: [run(glp, glab, 10, ninf_row, e, beam, mm, P) for e in (R.END_HIGHEST, R.END_BEST)],
        "pinf": lambda run: [run(lp, lab, 10, pinf, R.END_HIGHEST, beam, mm, P)],
        "pinf_outside": lambda run: [run(lp, lab, 10, pinf_outside, R.END_HIGHEST, beam, mm, P)],
        "pinf_generic": lambda run: [run(glp, glab, 10, gpinf, R.END_HIGHEST, beam, mm, P)],
        "end_live": lambda run: [run(lp[:3], lab, 0, None, int(p), beam, mm, P) for p in (live[0], live[len(live) // 2], live[-1])],
        "end_dead_in_band": lambda run: [run(lp[:3], lab, 0, None, dead_in_band, beam, mm, P)],
        "end_dead_generic": lambda run: [run(glp[:3], glab, 0, None, L - 1, beam, mm, P)],
        "end_outside_band": lambda run: [run(lp[:3], lab, 0, None, L - 1, beam, mm, P)],
        "end_best": lambda run: [run(lp[:3], lab, 0, None, R.END_BEST, beam, mm, P)],
        "end_dead_T8": lambda run: [run(lp[:8], lab, 0, None, L - 1, beam, mm, P)],   # T % period == 0: next_lo is a retarget
    }


def _short_scenarios():
    out = {}
    for T in (4, 8):
        lp, lab, beam, mm, P = short_case(T)
        out[f"short:T{T}"] = (lambda lp, lab: lambda run: [run(lp, lab, 0, None, e, beam, mm, P) for e in (R.END_HIGHEST, R.END_BEST)])(lp, lab)
    lp, lab, beam, mm, P = short_case(8)
    out["short:T8:4"] = lambda run: chain(run, lp, lab, 4, 0, None, R.END_HIGHEST, beam, mm, P)
    return out


SCENARIOS = {}
for _n in TC.NAMES:
    SCENARIOS[f"uncut:{_n}"] = uncut_scenario(_n)
    for _k in cuts_of(_n):
        SCENARIOS[f"cut:{_n}:{_k}"] = cut_scenario(_n, _k)
for _d in (1, 2, 3):
    SCENARIOS[f"depth{_d}"] = (lambda c: lambda run: chain(run, *c))(depth_case(_d))
    SCENARIOS[f"edge{_d}"] = (lambda c: lambda run: chain(run, *c))(edge_case(_d))
SCENARIOS.update(_short_scenarios())
SCENARIOS.update({f"single:{k}": v for k, v in single_scenarios().items()})

_want = {}


def want(name):
    """the reference's answers to a scenario, computed once"""
    if name not in _want:
        _want[name] = SCENARIOS[name](ref_run())
    return _want[name]
