"""Best path over a self-steering band: tests/band_ref.py's float32 NumPy data flow with the table computed on the fly - the
reference of tests/test_tracking_cpu.py and tests/test_tracking_gpu.py.  TEST INFRASTRUCTURE, not
product code.

  lo_0 = 0;  t > 0, t % period != 0: lo_t = lo_{t-1}
  t > 0, t % period == 0: c = live_pos[np.argmax(live_score)] of the compacted live list after frame t-2 (after frame -1: the
      virtual state {0: 0.0}); lo_t = min(max(lo_{t-1}, c - beam // 2), L - 1); an empty list keeps lo_{t-1}
  hi_t = min(lo_t + beam, L); the frame itself, the walk back and the outputs are band_ref.best_path_banded's.
  end_rule "highest": the path ends at the highest live position of frame T-1; "best": at live_pos[np.argmax(live_score)].

``fault`` plants one of six mistakes (FAULTS), for the tests that show the test cases would catch them.
"""
import numpy as np

FAULTS = ("lag1", "last_max", "not_monotone", "centre_ceil", "all_cells", "end_highest_when_best")
END_RULES = {"highest": 0, "best": 1}


def _first_max(pos, score, lo, hi, fault):
    """position of the first maximum over the live list (None if it is empty)"""
    if fault == "all_cells":   # over every cell of the band, dead ones as -inf
        if hi <= lo:
            return None
        full = np.full(hi - lo, -np.inf, np.float32)
        full[pos - lo] = score
        return lo + int(np.argmax(full))
    if pos.size == 0:
        return None
    if fault == "last_max":
        return int(pos[pos.size - 1 - int(np.argmax(score[::-1]))])
    return int(pos[int(np.argmax(score))])


def best_path_tracking(log_probs, labels, beam_size=1000, max_move=4, period=16, end_rule="highest", fault=None, return_total=False,
                       return_cells=False):
    """(best_path int32 [T], best_labels int32 [T], best_scores float32 [T], band_lo int32 [T]) [+ total float32] [+ per frame
    (positions, scores) of the live cells].  ValueError where no state is live in the last frame."""
    assert fault is None or fault in FAULTS
    assert end_rule in END_RULES and period >= 4 and period % 4 == 0
    log_probs = np.asarray(log_probs, dtype=np.float32)
    labels = np.asarray(labels).reshape(-1)
    S = labels.shape[0]
    L = 2 * S + 1
    T = log_probs.shape[0]
    B = int(beam_size)
    ext = np.zeros(L, dtype=np.int32)
    ext[1:L:2] = labels
    half = (B + 1) // 2 if fault == "centre_ceil" else B // 2

    live_pos = np.zeros(1, dtype=np.int64)
    live_score = np.zeros(1, dtype=np.float32)
    # after[k + 1] = (positions, scores, lo, hi) after frame k; after[0] is the virtual state before frame 0
    after = [(live_pos, live_score, 0, 1)]
    band_lo = np.zeros(T, dtype=np.int32)
    trail, cells = [], []
    lo = 0
    for t in range(T):
        if t > 0 and t % period == 0:
            k = t - 1 if fault == "lag1" else t - 2
            c = _first_max(*after[k + 1], fault)
            if c is not None:
                new = c - half
                if fault == "not_monotone":
                    new = max(new, 0)
                else:
                    new = max(lo, new)
                lo = min(new, L - 1)
        band_lo[t] = lo
        hi = min(lo + B, L)
        width = max(hi - lo, 0)
        back = np.full((max_move, width), -1, dtype=np.int32)
        cand = np.full((max_move, width), -np.inf, dtype=np.float32)
        row = log_probs[t]
        veto_cols = ext[lo:lo + width] == 0
        for j in range(max_move):
            tgt = live_pos + j
            sel, = np.nonzero((tgt >= lo) & (tgt < hi))
            dst = tgt[sel]
            back[j, dst - lo] = sel
            cand[j, dst - lo] = live_score[sel] + row[ext[dst]]
            if j > 0 and j % 2 == 0:
                cand[j, veto_cols] = -np.inf
        move = np.argmax(cand, axis=0)
        back = np.choose(move, back) if width else back[0]
        cand = np.choose(move, cand) if width else cand[0]
        keep, = np.nonzero(back >= 0)
        live_score = cand[keep].copy()
        trail.append((keep + lo, back[keep].copy()))
        live_pos = keep + lo
        after.append((live_pos, live_score, lo, hi))
        if return_cells:
            cells.append((live_pos.copy(), live_score.copy()))
    last_pos = trail[-1][0]
    if end_rule == "best" and fault == "all_cells":   # a dead cell of the band may win: no path ends there
        c = _first_max(live_pos, live_score, lo, hi, fault)
        at, = np.nonzero(last_pos == (-1 if c is None else c))
        if at.size == 0:
            raise ValueError("attempt to get argmax of an empty sequence")
        cur = int(at[0])
    elif end_rule == "best" and fault != "end_highest_when_best":
        cur = int(np.argmax(live_score))  # ValueError on empty
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
    out = (path, best_labels, best_scores, band_lo)
    if return_total:
        out += (total,)
    if return_cells:
        out += (cells,)
    return out
