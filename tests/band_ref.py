"""Best path over a caller-given band: a float32 NumPy restatement of kokoro_align/align.py:62-107 in which the band's low end
comes from a table, lo_t = band_lo[t], hi_t = min(lo_t + beam, L) - the reference of tests/test_banded_cpu.py and
tests/test_banded_gpu.py.  TEST INFRASTRUCTURE, not product code.

It keeps the reference's data flow (oracle.ctc_best_path_numpy's): the compacted live list, per move a scatter of its
candidates into a (max_move, width) table, np.argmax over the moves (the first maximum), np.choose, compaction of the cells
that have a predecessor, the terminal np.argmax over the live positions (ValueError on an empty list), one walk back.

``fault`` plants one of five mistakes (FAULTS), for the tests that show the test cases would catch them.
"""
import numpy as np

FAULTS = ("hi_unclamped", "stale_band", "last_max", "veto_position", "argmax_terminal")


def best_path_banded(log_probs, labels, band_lo, beam_size=1000, max_move=4, fault=None, return_total=False, return_cells=False):
    """(best_path int32 [T], best_labels int32 [T], best_scores float32 [T]) [+ total float32] [+ per frame (positions, scores)
    of the live cells]."""
    assert fault is None or fault in FAULTS
    log_probs = np.asarray(log_probs, dtype=np.float32)
    labels = np.asarray(labels).reshape(-1)
    S = labels.shape[0]
    L = 2 * S + 1
    T = log_probs.shape[0]
    band_lo = np.asarray(band_lo)
    assert band_lo.shape == (T,)
    # (the planted unclamped hi lets positions run past L: give them blanks to land on)
    ext = np.zeros(L + (int(beam_size) + max_move if fault == "hi_unclamped" else 0), dtype=np.int32)
    ext[1:L:2] = labels

    live_pos = np.zeros(1, dtype=np.int64)
    live_score = np.zeros(1, dtype=np.float32)
    trail, cells = [], []
    for t in range(T):
        lo = int(band_lo[t - 1 if (fault == "stale_band" and t > 0) else t])
        hi = lo + beam_size if fault == "hi_unclamped" else min(lo + beam_size, L)
        width = max(hi - lo, 0)
        back = np.full((max_move, width), -1, dtype=np.int32)
        cand = np.full((max_move, width), -np.inf, dtype=np.float32)
        row = log_probs[t]
        if fault == "veto_position":
            veto_cols = (np.arange(lo, lo + width) % 2) == 0
        else:
            veto_cols = ext[lo:lo + width] == 0
        for j in range(max_move):
            tgt = live_pos + j
            sel, = np.nonzero((tgt >= lo) & (tgt < hi))
            dst = tgt[sel]
            back[j, dst - lo] = sel
            cand[j, dst - lo] = live_score[sel] + row[ext[dst]]
            if j > 0 and j % 2 == 0:
                cand[j, veto_cols] = -np.inf
        if fault == "last_max":
            move = (max_move - 1) - np.argmax(cand[::-1], axis=0)
        else:
            move = np.argmax(cand, axis=0)
        back = np.choose(move, back) if width else back[0]
        cand = np.choose(move, cand) if width else cand[0]
        keep, = np.nonzero(back >= 0)
        live_score = cand[keep].copy()
        trail.append((keep + lo, back[keep].copy()))
        live_pos = keep + lo
        if return_cells:
            cells.append((live_pos.copy(), live_score.copy()))
    last_pos = trail[-1][0]
    if fault == "argmax_terminal":
        cur = int(np.argmax(live_score))
    else:
        cur = int(np.argmax(last_pos))  # ValueError on empty, as align.py:101
    total = np.float32(live_score[cur])
    path = np.empty(T, dtype=np.int32)
    for t in range(T - 1, -1, -1):
        pos, back = trail[t]
        path[t] = pos[cur]
        cur = back[cur]
    best_labels = ext[path]
    best_scores = log_probs[np.arange(T), best_labels]
    out = (path, best_labels, best_scores)
    if return_total:
        out += (total,)
    if return_cells:
        out += (cells,)
    return out


def diagonal_lo(T, L, beam_size):
    """align.py:64 in Python integers: the table against which the package's diagonal_band is checked."""
    return [max(0, L * t // T - beam_size // 2) for t in range(T)]
