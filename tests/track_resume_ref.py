"""The resumable tracking best path (ka_ctc_best_path_tracking_resume): tests/track_ref.py's float32
NumPy data flow (the compacted live list, per move a scatter of its candidates, np.argmax over the moves, np.choose, compaction
of the cells that have a predecessor, one walk back, the table computed on the fly) with tests/resume_ref.py's boundary
conditions - the reference of tests/test_tracking_resume_cpu.py and tests/test_tracking_resume_gpu.py.  TEST INFRASTRUCTURE, not
product code.

  * the start row's live list (the cells that are not NaN, -inf included) in place of {0: 0.0}; no band applies to it;
  * lo_0 = first_lo; local frame t > 0 with t % period == 0: c = live_pos[np.argmax(live_score)] of the live list after local
    frame t-2, lo_t = min(max(lo_{t-1}, c - beam // 2), L - 1), an empty list keeps lo_{t-1}; frame 0 never retargets;
  * next_lo: what local frame T would get - that rule on lo_{T-1} and the list after frame T-2 if T % period == 0, else lo_{T-1};
  * the three ends, ``entry`` and the last row of resume_ref.

``fault`` plants one of six mistakes (FAULTS), for the tests that show the test cases would catch them.
"""
import numpy as np

from resume_ref import DEAD, END_BEST, END_HIGHEST, BadArgs, same_bits  # noqa: F401

FAULTS = ("next_lo_lag1", "next_lo_off_phase", "first_lo_zero", "retarget_frame0", "band_on_row", "next_lo_applied")


class EmptyBeam(ValueError):
    """No live cell after the last frame, or the given end cell is not live; the forward pass's outputs are there all the same."""

    def __init__(self, what, final, band_lo, next_lo):
        super().__init__(what)
        self.final, self.band_lo, self.next_lo = final, band_lo, next_lo


def _retarget(lo, cells, half, L):
    pos, score = cells
    if pos.size == 0:
        return lo
    return min(max(lo, int(pos[int(np.argmax(score))]) - half), L - 1)


def best_path_tracking_resume(log_probs, labels, first_lo=0, init_scores=None, end=END_HIGHEST, beam_size=1000, max_move=4, period=16,
                              fault=None, _walk=None):
    """(best_path int32 [T], best_labels int32 [T], best_scores float32 [T], band_lo int32 [T], total float32, entry int,
    final float32 [L], next_lo int).  ``_walk``: (t0, lo) - frames from t0 on are walked under lo (the fault next_lo_applied)."""
    assert fault is None or fault in FAULTS
    assert period >= 4 and period % 4 == 0
    log_probs = np.asarray(log_probs, dtype=np.float32)
    labels = np.asarray(labels).reshape(-1)
    S = labels.shape[0]
    L = 2 * S + 1
    T = log_probs.shape[0]
    B = int(beam_size)
    half = B // 2
    assert 0 <= first_lo < L and -2 <= end < L and T >= 1
    ext = np.zeros(L, dtype=np.int32)
    ext[1:L:2] = labels
    lo = 0 if fault == "first_lo_zero" else int(first_lo)

    if init_scores is None:
        live_pos = np.zeros(1, dtype=np.int64)
        live_score = np.zeros(1, dtype=np.float32)
    else:
        row = np.asarray(init_scores, dtype=np.float32)
        assert row.shape == (L,)
        if np.any(np.isposinf(row)):
            raise BadArgs("a start cell is +inf")
        live_pos, = np.nonzero(~np.isnan(row))
        if fault == "band_on_row":
            live_pos = live_pos[live_pos >= lo]
        live_score = row[live_pos].copy()
    start_pos = live_pos
    after = [(live_pos, live_score)]   # after[k + 1]: the live list after frame k
    band_lo = np.zeros(T, dtype=np.int32)
    trail = []
    with np.errstate(invalid="ignore"):
        for t in range(T):
            if _walk is not None and t >= _walk[0]:
                lo = _walk[1]
            elif t > 0 and t % period == 0:
                lo = _retarget(lo, after[t - 1], half, L)
            elif t == 0 and fault == "retarget_frame0":
                lo = _retarget(lo, after[0], half, L)
            band_lo[t] = lo
            hi = min(lo + B, L)
            width = max(hi - lo, 0)
            back = np.full((max_move, width), -1, dtype=np.int64)
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
            after.append((live_pos, live_score))
    # the low end frame T would get: after[T - 1] is the list after frame T-2
    if fault == "next_lo_lag1":
        next_lo = _retarget(lo, after[T], half, L) if T % period == 0 else lo
    elif T % period == 0 or (fault == "next_lo_off_phase" and T >= 2):
        next_lo = _retarget(lo, after[T - 1], half, L)
    else:
        next_lo = lo
    if fault == "next_lo_applied" and _walk is None:
        t0 = T - (T % period or period)
        return best_path_tracking_resume(log_probs, labels, first_lo, init_scores, end, beam_size, max_move, period, fault,
                                         _walk=(max(t0, 1), next_lo))
    final = np.full(L, DEAD, np.float32)
    final[live_pos] = live_score
    if live_pos.size == 0:
        raise EmptyBeam("no live cell after the last frame", final, band_lo, next_lo)
    if end == END_HIGHEST:
        cur = int(np.argmax(live_pos))
    elif end == END_BEST:
        cur = int(np.argmax(live_score))
    else:
        at, = np.nonzero(live_pos == end)
        if at.size == 0:
            raise EmptyBeam("the end cell is not live", final, band_lo, next_lo)
        cur = int(at[0])
    total = np.float32(live_score[cur])
    path = np.empty(T, dtype=np.int32)
    for t in range(T - 1, -1, -1):
        pos, back = trail[t]
        path[t] = pos[cur]
        cur = back[cur]
    entry = int(start_pos[cur])
    best_labels = ext[path]
    best_scores = log_probs[np.arange(T), best_labels]
    return path, best_labels, best_scores, band_lo, total, entry, final, next_lo
