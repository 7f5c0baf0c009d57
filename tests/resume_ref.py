"""The resumable best path (ka_ctc_best_path_resume): tests/band_ref.py's float32 NumPy restatement of
kokoro_align/align.py:62-107 with the caller's boundary conditions - the reference of tests/test_resume_cpu.py and
tests/test_resume_gpu.py.  TEST INFRASTRUCTURE, not product code.

The data flow is band_ref's (the compacted live list, per move a scatter of its candidates, np.argmax over the moves, np.choose,
compaction of the cells that have a predecessor, one walk back) with
  * the start row's live list (the cells that are not NaN, -inf included) in place of {0: 0.0}; no band applies to it;
  * three end rules: the highest live position (np.argmax over the positions), the first maximum of the scores (np.argmax over
    the scores), a given position (which must be live);
  * ``entry``: the cell of the start list the walk ends on;
  * the last row: the live cells' scores, DEAD (the quiet NaN 0x7fc00000) elsewhere.

``fault`` plants one of six mistakes (FAULTS), for the tests that show the test cases would catch them.
"""
import numpy as np

FAULTS = ("drop_below_lo", "dead_as_ninf", "entry_is_path0", "best_last_max", "final_whole_ring", "accept_pinf")
DEAD = np.array([0x7fc00000], np.uint32).view(np.float32)[0]
END_HIGHEST, END_BEST = -1, -2


class EmptyBeam(ValueError):
    """No live cell after the last frame, or the given end cell is not live; ``final`` is the last row all the same."""

    def __init__(self, what, final):
        super().__init__(what)
        self.final = final


class BadArgs(ValueError):
    """A +inf cell in the start row."""


def best_path_resume(log_probs, labels, band_lo, init_scores=None, end=END_HIGHEST, beam_size=1000, max_move=4, fault=None):
    """(best_path int32 [T], best_labels int32 [T], best_scores float32 [T], total float32, entry int, final float32 [L])"""
    assert fault is None or fault in FAULTS
    log_probs = np.asarray(log_probs, dtype=np.float32)
    labels = np.asarray(labels).reshape(-1)
    S = labels.shape[0]
    L = 2 * S + 1
    T = log_probs.shape[0]
    band_lo = np.asarray(band_lo)
    assert band_lo.shape == (T,) and -2 <= end < L
    ext = np.zeros(L, dtype=np.int32)
    ext[1:L:2] = labels

    if init_scores is None:
        live_pos = np.zeros(1, dtype=np.int64)
        live_score = np.zeros(1, dtype=np.float32)
    else:
        row = np.asarray(init_scores, dtype=np.float32)
        assert row.shape == (L,)
        if fault != "accept_pinf" and np.any(np.isposinf(row)):
            raise BadArgs("a start cell is +inf")
        if fault == "dead_as_ninf":
            row = np.where(np.isnan(row), np.float32(-np.inf), row)
        live_pos, = np.nonzero(~np.isnan(row))
        if fault == "drop_below_lo":
            live_pos = live_pos[live_pos >= int(band_lo[0])]
        live_score = row[live_pos].copy()
    start_pos = live_pos
    trail = []
    with np.errstate(invalid="ignore"):
        for t in range(T):
            lo = int(band_lo[t])
            hi = min(lo + beam_size, L)
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
    final = np.full(L, DEAD, np.float32)
    if fault == "final_whole_ring":   # what the ring's registers hold where no cell is live: -inf
        ring0 = (int(band_lo[-1]) >> 4) << 4
        final[ring0:min(ring0 + 1024, L)] = -np.inf
    final[live_pos] = live_score
    if live_pos.size == 0:
        raise EmptyBeam("no live cell after the last frame", final)
    if end == END_HIGHEST:
        cur = int(np.argmax(live_pos))
    elif end == END_BEST:
        cur = int(np.argmax(live_score))
        if fault == "best_last_max":
            cur = live_score.size - 1 - int(np.argmax(live_score[::-1]))
    else:
        at, = np.nonzero(live_pos == end)
        if at.size == 0:
            raise EmptyBeam("the end cell is not live", final)
        cur = int(at[0])
    total = np.float32(live_score[cur])
    path = np.empty(T, dtype=np.int32)
    for t in range(T - 1, -1, -1):
        pos, back = trail[t]
        path[t] = pos[cur]
        cur = back[cur]
    entry = int(path[0]) if fault == "entry_is_path0" else int(start_pos[cur])
    best_labels = ext[path]
    best_scores = log_probs[np.arange(T), best_labels]
    return path, best_labels, best_scores, total, entry, final


def cut_and_resume(log_probs, labels, band_lo, k, beam_size=1000, max_move=4, fault=None, run=best_path_resume):
    """Property 2: chunk A = frames [0, k), chunk B = frames [k, T) from A's last row, A again with end = B's entry.  Returns
    (path, labels, scores, B's total, B's entry, A's first answer, B's answer); EmptyBeam from whichever chunk has none."""
    kw = dict(beam_size=beam_size, max_move=max_move)
    if fault is not None:
        kw["fault"] = fault
    a0 = run(log_probs[:k], labels, band_lo[:k], None, END_HIGHEST, **kw)
    b = run(log_probs[k:], labels, band_lo[k:], a0[5], END_HIGHEST, **kw)
    a = run(log_probs[:k], labels, band_lo[:k], None, b[4], **kw)
    return tuple(np.concatenate([a[i], b[i]]) for i in range(3)) + (b[3], b[4], a0, b)


def same_bits(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and a.dtype.itemsize == b.dtype.itemsize and \
        np.array_equal(a.view(np.uint32) if a.dtype.itemsize == 4 else a, b.view(np.uint32) if b.dtype.itemsize == 4 else b)
