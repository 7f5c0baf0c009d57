"""The determined prefix of a resumed best path (ka_ctc_best_path_determined, ka_ctc_best_path_tracking_determined, DESIGN.md
section 4.36): tests/resume_ref.py's and tests/track_resume_ref.py's float32 NumPy data flow with the trail walk of the
reference's flush_determined_path (kokoro_align/align.py:21-40) - the reference of tests/test_determined_cpu.py and
tests/test_determined_gpu.py.  TEST INFRASTRUCTURE, not product code.

The forward pass is resume_ref's, list for list (the compacted live list, per move a scatter of its candidates, np.argmax over
the moves, np.choose, compaction of the cells that have a predecessor); it keeps every frame's (positions, indices into the
list before).  The walk starts from ALL entries of the last list and takes np.unique over their predecessors until one is left:
  determined = 1 + the last frame t in [-1, T-1] whose set has one entry, -1 without one (frame -1: the start list).
A tracking lattice is walked over the table tests/track_resume_ref.py computes for it (its property 3).

``fault`` plants one of six mistakes (FAULTS), for the tests that show the test cases would catch them.
"""
import numpy as np

import resume_ref as RR
import track_resume_ref as TR

FAULTS = ("end_cell_only", "merge_off_by_one", "start_row_not_counted", "drop_block_crossers", "ninf_as_dead", "distinct_lanes")


def forward_trail(log_probs, labels, band_lo, init_scores, beam_size, max_move):
    """resume_ref.best_path_resume's forward pass: (start positions, trail, the last list's positions and scores), or None for
    what the call rejects (a label outside [0, V), a NaN log-prob, a bad table, a +inf start cell)."""
    log_probs = np.asarray(log_probs, dtype=np.float32)
    labels = np.asarray(labels).reshape(-1)
    T, V = log_probs.shape
    S = labels.shape[0]
    L = 2 * S + 1
    band_lo = np.asarray(band_lo, dtype=np.int64)
    if np.any(labels < 0) or np.any(labels >= V) or np.any(np.isnan(log_probs)):
        return None
    if band_lo.shape != (T,) or np.any(band_lo < 0) or np.any(band_lo >= L) or np.any(np.diff(band_lo) < 0):
        return None
    ext = np.zeros(L, dtype=np.int32)
    ext[1:L:2] = labels
    if init_scores is None:
        live_pos = np.zeros(1, dtype=np.int64)
        live_score = np.zeros(1, dtype=np.float32)
    else:
        row = np.asarray(init_scores, dtype=np.float32)
        assert row.shape == (L,)
        if np.any(np.isposinf(row)):
            return None
        live_pos, = np.nonzero(~np.isnan(row))
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
    return start_pos, trail, live_pos, live_score


def walk(start_pos, trail, live_pos, live_score, end_index=None, fault=None):
    """(determined, stats).  stats: frames (walked back), cross1 / cross2 / cross3 (a set of more than one cell held a cell whose
    move of 1 / 2 / 3 crossed a block-of-16 boundary), wrap (... crossed slot 1023 -> 0 of the ring, a multiple of 1024)."""
    assert fault is None or fault in FAULTS
    stats = {"frames": 0, "cross1": False, "cross2": False, "cross3": False, "wrap": False}
    T = len(trail)
    cur = np.arange(live_pos.size)
    if fault == "end_cell_only" and cur.size:
        cur = cur[[int(np.argmax(live_pos)) if end_index is None else end_index]]
    if fault == "ninf_as_dead":
        cur = cur[~np.isneginf(live_score)]
    if cur.size == 0:
        return -1, stats

    def single(idx, pos):
        if fault == "distinct_lanes":
            return np.unique((pos[idx] >> 4) & 63).size == 1
        return idx.size == 1

    for t in range(T - 1, -1, -1):
        pos, back = trail[t]
        if single(cur, pos):
            return (t if fault == "merge_off_by_one" else t + 1), stats
        before = trail[t - 1][0] if t > 0 else start_pos
        moves = pos[cur] - before[back[cur]]
        for j in (1, 2, 3):
            if np.any((moves == j) & ((pos[cur] >> 4) != ((pos[cur] - j) >> 4))):
                stats[f"cross{j}"] = True
        if np.any((pos[cur] >> 10) != ((pos[cur] - moves) >> 10)):
            stats["wrap"] = True
        if fault == "drop_block_crossers":
            cur = cur[(pos[cur] >> 4) == ((pos[cur] - moves) >> 4)]
            if cur.size == 0:
                return -1, stats
        cur = np.unique(back[cur])
        stats["frames"] += 1
    if fault == "start_row_not_counted":
        return 1, stats
    return (0 if single(cur, start_pos) else -1), stats


def determined(log_probs, labels, band_lo, init_scores=None, beam_size=1000, max_move=4, fault=None, with_stats=False):
    """``determined`` of ka_ctc_best_path_determined on these inputs (whatever the end: it depends on the live cells alone; the
    fault end_cell_only walks from the highest live cell)."""
    fw = forward_trail(log_probs, labels, band_lo, init_scores, beam_size, max_move)
    if fw is None:
        d, stats = -1, {"frames": 0, "cross1": False, "cross2": False, "cross3": False, "wrap": False}
    else:
        d, stats = walk(*fw, fault=fault)
    return (d, stats) if with_stats else d


def tracking_table(log_probs, labels, first_lo, init_scores, beam_size, max_move, period):
    """the table track_resume_ref walks on these inputs, or None where the call rejects them"""
    log_probs = np.asarray(log_probs, dtype=np.float32)
    labels = np.asarray(labels).reshape(-1)
    if np.any(labels < 0) or np.any(labels >= log_probs.shape[1]) or np.any(np.isnan(log_probs)):
        return None
    try:
        return TR.best_path_tracking_resume(log_probs, labels, first_lo, init_scores, TR.END_HIGHEST, beam_size, max_move, period)[3]
    except TR.EmptyBeam as e:
        return e.band_lo
    except TR.BadArgs:
        return None


def tracking_determined(log_probs, labels, first_lo=0, init_scores=None, beam_size=1000, max_move=4, period=16, fault=None, with_stats=False):
    """``determined`` of ka_ctc_best_path_tracking_determined on these inputs"""
    table = tracking_table(log_probs, labels, first_lo, init_scores, beam_size, max_move, period)
    if table is None:
        d, stats = -1, {"frames": 0, "cross1": False, "cross2": False, "cross3": False, "wrap": False}
        return (d, stats) if with_stats else d
    return determined(log_probs, labels, table, init_scores, beam_size, max_move, fault, with_stats)


def live_cells(log_probs, labels, band_lo, init_scores=None, beam_size=1000, max_move=4):
    """the live positions after the last frame (empty for what the call rejects)"""
    fw = forward_trail(log_probs, labels, band_lo, init_scores, beam_size, max_move)
    return np.zeros(0, np.int64) if fw is None else fw[2]
