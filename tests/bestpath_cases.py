"""Inputs that put the best path where the best-path kernels' band code works: on the band's edges,
next to a cell outside the band that would do better, and across the 128- and 256-position tile borders at the frames
around a checkpoint.  With hash or N(0, 1) log-probs and a band of 300 or more the best path stays hundreds of positions
from either edge, and a window one position off at every frame changes nothing.

Three families, all with finite log-probs (a -inf sends a lattice to the exact kernels):
  hug      posterior_ref.edge_hugging: N(0, 1) logits with 12 nats on the label of the band's lowest cell in the first half of
           the frames and of its highest cell after; plain, quantised to halves (ties on the edge) and with every fifth label
           value renamed to 0 (the family itself has a 0 at every 17th transcript position)
  bait     a dictated path (near one-hot rows, the others 20 to 60 nats below) that runs on one edge, and 5 nats more than the
           path's own cell gets on the label of the cell just outside: above hi in the frame before hi advances, below lo in
           the frame in which lo has advanced
  border   a dictated path along the band's middle that waits on the position below each multiple of 128 and crosses it by a
           move of 1, 2 or 3 at a frame with t mod 32 in {31, 0, 1}
The dictated families use a transcript without 0 in which no label value recurs within (V - 1) // 3 positions and no stretch
repeats (spaced_labels).  The reference is pbt_ref.best_path_with_moves, which the CPU file pins to the C oracle; its rows[k] are the
checkpoint rows the forward kernels store.  No product file imports this module.
"""
import functools

import numpy as np

import pbt_ref as P
import posterior_ref as R

FAULTS = P.FAULTS + P.EDGE_FAULTS
WINDOW_FAULTS = ("lo_plus_one", "lo_minus_one", "hi_minus_one", "hi_plus_one")
BAIT = 5.0          # nats by which the cell outside the band beats the path's cell in a bait frame
BORDER = 128        # the narrower tile; every other border is one of the 256-position tiles too
CLASSES = (31, 0, 1)       # t mod 32 of a crossing: the checkpoint frame, the first and the second frame of a chunk

WAVE = ("wave", "wave_exact", "tiled/256", "tiled/128", "wave+parallel", "tiled/256+parallel", "tiled/128+parallel", "auto")
WIDE = ("tiled/256", "tiled/128", "tiled/256+parallel", "tiled/128+parallel", "auto")      # bands over 1009: no one-wavefront form


def spaced_labels(S, V, seed):
    """Random permutations of 1 .. V - 1 one after the other, none beginning with what the one before ended on: no label value
    recurs within (V - 1) // 3 transcript positions, there is no 0, and no stretch repeats (a cyclic transcript lets a path one
    period below the dictated one read the same labels)."""
    rng = np.random.default_rng(seed)
    h = (V - 1) // 3
    out, tail = [], set()
    while len(out) < S:
        perm = rng.permutation(np.arange(1, V)).tolist()
        block = [x for x in perm if x not in tail] + [x for x in perm if x in tail]
        out += block
        tail = set(block[-h:])
    return np.array(out[:S], np.int32)


def _feasible(d, n, mm):
    """Can a path over a transcript without 0 climb d positions in n frames?  Move 2 is legal onto label cells only."""
    if mm >= 4:
        return 0 <= d <= 3 * n and d != 3 * n - 1
    if mm == 3:
        return 0 <= d <= max(2 * n - 1, 0)
    return 0 <= d <= (n if mm >= 2 else 0)


def walk(T, ext, lo, hi, mm, want):
    """A legal in-band path that ends on L - 1: in every frame the move that brings it closest to want(t, s)."""
    L = len(ext)
    s, states = 0, []
    for t in range(T):
        ok = [j for j in range(mm) if lo[t] <= s + j < hi[t] and not (j >= 2 and j % 2 == 0 and ext[s + j] == 0)
              and _feasible(L - 1 - s - j, T - 1 - t, mm)]
        assert ok, ("walk(): no legal move", t, s, int(lo[t]), int(hi[t]))
        w = want(t, s)
        s += min(ok, key=lambda j: (abs(s + j - w), j))
        states.append(s)
    assert states[-1] == L - 1
    return np.array(states, np.int64)


def _rows(T, V, ext, states, seed, bait_label):
    """Near one-hot rows along `states`; bait_label[t] >= 0 gets BAIT nats more than the path's own label in frame t."""
    rng = np.random.default_rng(seed)
    logits = -rng.uniform(20.0, 60.0, size=(T, V))
    t = np.arange(T)
    logits[t, ext[states]] = 0.0
    on = bait_label >= 0
    logits[t[on], bait_label[on]] = BAIT
    return R._normalise(logits)


def bait(T, S, V, beam, mm, seed, side):
    """(lp, labels, frames): the path runs on hi - 1 (side "hi") or on lo (side "lo"); `frames` are the bait frames."""
    labels = spaced_labels(S, V, seed)
    ext = P.expand(labels)
    L = len(ext)
    lo, hi = P.band(T, L, beam)
    if side == "hi":
        states = walk(T, ext, lo, hi, mm, lambda t, s: hi[t] - 1)
        # the frame before hi advances, the cell above the band a label cell (a blank outside would pay every blank inside)
        t = np.arange(T - 1)
        on = (states[t] == hi[t] - 1) & (hi[t + 1] > hi[t]) & (hi[t] < L) & (hi[t] % 2 == 1)
        outside = hi[t]
    else:
        states = walk(T, ext, lo, hi, mm, lambda t, s: lo[t])
        # the frame in which lo has advanced off a label cell the path stood on
        t = np.arange(1, T)
        on = (states[t] == lo[t]) & (lo[t] > lo[t - 1]) & (states[t - 1] == lo[t] - 1) & (lo[t] % 2 == 0)
        outside = lo[t] - 1
    frames = t[on]
    assert np.all(ext[outside[on]] != ext[states[frames]])
    bait_label = np.full(T, -1, np.int64)
    bait_label[frames] = ext[outside[on]]
    return _rows(T, V, ext, states, seed, bait_label), labels, frames


def crossings(T, L, offset):
    """{border: (frame, move)} of the border family: border 128 i is crossed from 128 i - 1 by move 1 + k % 3 at the first frame
    of class CLASSES[k // 3 % 3] after the band's middle has reached it, k = i // 2 + offset (i's parity is the border's
    residue mod 256, so nine borders of each parity run through the product)."""
    out = {}
    for i in range(1, (L - 4) // BORDER + 1):
        k = i // 2 + offset
        t = -(-(BORDER * i) * T // L)
        while t % 32 != CLASSES[k // 3 % 3]:
            t += 1
        if t < T - 40:
            out[BORDER * i] = (t, 1 + k % 3)
    return out


def border(T, S, V, beam, mm, seed, offset):
    assert mm == 4
    labels = spaced_labels(S, V, seed)
    ext = P.expand(labels)
    L = len(ext)
    lo, hi = P.band(T, L, beam)
    plan = crossings(T, L, offset)
    at = {t: (b, j) for b, (t, j) in plan.items()}
    assert len(at) == len(plan)
    pending = sorted(plan)

    def want(t, s):
        while pending and pending[0] <= s:
            pending.pop(0)
        if t in at and at[t][0] in pending:
            return at[t][0] - 1 + at[t][1]
        if t - 1 in at and at[t - 1] == (s, 1):
            return s + 1      # (from the blank on the border to its label: a climb of 3 from there ties with a crossing by 3)
        mid = L * t // T
        return min(mid, pending[0] - 1) if pending else mid

    states = walk(T, ext, lo, hi, mm, want)
    return _rows(T, V, ext, states, seed, np.full(T, -1, np.int64)), labels


def realised(path, T):
    """The (move, t mod 32, border mod 256) of every step of `path` that crosses a multiple of 128 from the position below it."""
    out = set()
    for t in np.nonzero(np.diff(path) > 0)[0] + 1:
        a, b = int(path[t - 1]), int(path[t])
        edge = b // BORDER * BORDER
        if a == edge - 1 and t % 32 in CLASSES:
            out.add((b - a, int(t % 32), edge % 256))
    return out


BORDER_PRODUCT = {(j, c, r) for j in (1, 2, 3) for c in CLASSES for r in (0, 128)}


def hug(T, S, V, beam, seed, quantised, zero):
    lp, labels = R.edge_hugging(T, S, V, beam, seed)
    if quantised:
        lp = (np.round(lp * 2) / 2).astype(np.float32)
    if zero:
        labels = np.where(labels % 5 == 0, 0, labels).astype(np.int32)     # the columns stay: those cells now read the blank's
    return lp, labels


# name: (family, T, S, V, beam, max_move, seed, option, forms)     option: hug (quantised, zero) | bait side | border offset
# The shapes are the smallest at which each mechanism of the band code exists (DESIGN.md section 4.25 has the table).
CASES = {
    # narrow controls
    "hug_w16": ("hug", 400, 150, 39, 16, 4, 41, (False, False), WAVE),
    "hug_w64_q": ("hug", 400, 150, 39, 64, 4, 42, (True, False), WAVE),
    "bait_hi_w64": ("bait", 400, 150, 39, 64, 4, 43, "hi", WAVE),
    "bait_lo_w16": ("bait", 400, 150, 39, 16, 4, 44, "lo", WAVE),
    # tile borders under a mid-width band
    "hug_w400": ("hug", 1025, 500, 39, 400, 4, 45, (False, False), WAVE),
    "hug_w400_q_zero": ("hug", 1025, 500, 39, 400, 4, 50, (True, True), WAVE),
    "bait_hi_w400": ("bait", 1025, 500, 39, 400, 4, 47, "hi", WAVE),
    "bait_lo_w400": ("bait", 1025, 500, 39, 400, 4, 48, "lo", WAVE),
    "border_w400": ("border", 1025, 500, 39, 400, 4, 49, 0, WAVE),
    # the 1024-slot wrap
    "hug_w401_wrap": ("hug", 2049, 1000, 64, 401, 4, 50, (False, False), WAVE),
    "hug_w401_wrap_q": ("hug", 2049, 1000, 64, 401, 4, 51, (True, False), WAVE),
    "bait_hi_w401_wrap": ("bait", 2049, 1000, 64, 401, 4, 52, "hi", WAVE),
    "bait_lo_w401_wrap": ("bait", 2049, 1000, 64, 401, 4, 53, "lo", WAVE),
    "border_w401_wrap": ("border", 2049, 1000, 64, 401, 4, 54, 3, WAVE),
    # max_move 3 with label 0; max_move 2 (L / T = 0.42: at (1200, 500) with beam 300 a path that climbs one position a frame
    # from position 0 does not reach hi - 1 before hi = L, so no input can hug that upper edge)
    "hug_w300_m3_zero": ("hug", 2049, 1200, 64, 300, 3, 55, (False, False), WAVE),
    "bait_hi_w300_m3": ("bait", 2049, 1200, 64, 300, 3, 56, "hi", WAVE),
    "hug_w300_m2": ("hug", 2400, 500, 39, 300, 2, 57, (False, False), WAVE),
    "bait_lo_w300_m2": ("bait", 2400, 500, 39, 300, 2, 58, "lo", WAVE),
    # the mask of the one-wavefront form every 8th frame (beam 1000: 24 dead slots) and every 4th (1004: 20)
    "hug_w1000": ("hug", 3000, 1500, 39, 1000, 4, 59, (False, False), WAVE),
    "bait_hi_w1000": ("bait", 3000, 1500, 39, 1000, 4, 60, "hi", WAVE),
    "hug_w1004_q": ("hug", 3000, 1500, 39, 1004, 4, 61, (True, False), WAVE),
    "bait_lo_w1004": ("bait", 3000, 1500, 39, 1004, 4, 62, "lo", WAVE),
    "border_w1004": ("border", 3000, 1500, 39, 1004, 4, 63, 5, WAVE),
    # the widest one-wavefront band: 15 dead slots
    "hug_w1009": ("hug", 4000, 1500, 39, 1009, 4, 64, (False, False), WAVE),
    "hug_w1009_zero": ("hug", 4000, 1500, 39, 1009, 4, 65, (False, True), WAVE),
    "bait_hi_w1009": ("bait", 4000, 1500, 39, 1009, 4, 66, "hi", WAVE),
    "bait_lo_w1009": ("bait", 4000, 1500, 39, 1009, 4, 67, "lo", WAVE),
    # tiled only
    "hug_w1010": ("hug", 3000, 1500, 39, 1010, 4, 68, (False, False), WIDE),
    "hug_w1100_q": ("hug", 3000, 1500, 39, 1100, 4, 69, (True, False), WIDE),
    "bait_hi_w1100": ("bait", 3000, 1500, 39, 1100, 4, 70, "hi", WIDE),
    "bait_lo_w1010": ("bait", 3000, 1500, 39, 1010, 4, 71, "lo", WIDE),
    "border_w1100": ("border", 3000, 1500, 39, 1100, 4, 72, 7, WIDE),
}
NAMES = tuple(CASES)
HUG = tuple(n for n in NAMES if CASES[n][0] == "hug")
BAITS = tuple(n for n in NAMES if CASES[n][0] == "bait")
BORDERS = tuple(n for n in NAMES if CASES[n][0] == "border")
# the hash-logit inputs of three of the shapes above, on which the window faults change nothing: (T, S, V, beam, max_move, seed, quantised)
BLIND = ((1025, 500, 39, 400, 4, 81, False), (2049, 1000, 64, 401, 4, 82, True), (3000, 1500, 39, 1004, 4, 83, False))
# the cases the faults are tried on: one of every family at a band of 300 to 401, and the same at 1000 and more
FAULT_CASES = ("hug_w400_q_zero", "bait_hi_w401_wrap", "bait_lo_w400", "border_w401_wrap", "hug_w300_m3_zero",
               "hug_w1004_q", "bait_hi_w1000", "bait_lo_w1004")


def band_width(name):
    _, T, S, V, beam, mm = CASES[name][:6]
    return max(1, min(beam, 2 * S + 1))


@functools.lru_cache(maxsize=None)
def _built(name):
    family, T, S, V, beam, mm, seed, option, _ = CASES[name]
    frames = None
    if family == "hug":
        lp, lab = hug(T, S, V, beam, seed, *option)
    elif family == "bait":
        lp, lab, frames = bait(T, S, V, beam, mm, seed, option)
    else:
        lp, lab = border(T, S, V, beam, mm, seed, option)
    assert np.all(np.isfinite(lp))
    lp.setflags(write=False)
    lab.setflags(write=False)
    return lp, lab, frames


def case(name):
    """(log_probs, labels, beam, max_move) of a case; shared and never written to."""
    lp, lab, _ = _built(name)
    return lp, lab, CASES[name][4], CASES[name][5]


def bait_frames(name):
    return _built(name)[2]


@functools.lru_cache(maxsize=None)
def reference(name, fault=None):
    """The float32 reference of a case (None where a fault empties the beam); the rises of the maps are not computed."""
    lp, lab, beam, mm = case(name)
    try:
        return P.best_path_with_moves(lp, lab, beam, mm, fault=fault, maps=False)
    except ValueError:
        return None


def companions(name):
    """Two lattices of other T and S (hash log-probs) that share a launch with the case.  `first`: the case is the middle one
    of the caller's three; both are shorter, so the case stays descriptor 0 - the one ka_debug_checkpoints reports."""
    _, T, S, V, beam, mm, seed = CASES[name][:7]
    return [P.inputs(t, s, V, seed + 100 * (i + 1), False, False) for i, (t, s) in enumerate([(T * 2 // 3, S // 2), (T // 3, S // 5)])]


def edge_shares(ref):
    """(share of the frames with lo > 0 at which the path is on lo, share of the frames with hi < L on hi - 1)."""
    lower, upper = ref.lo > 0, ref.hi < ref.L
    return (float(np.mean(ref.path[lower] == ref.lo[lower])) if lower.any() else 0.0,
            float(np.mean(ref.path[upper] == ref.hi[upper] - 1)) if upper.any() else 0.0)


def edge_distance(ref):
    """Closest approach of the path to lo and to hi - 1 over the frames where that edge is a real edge."""
    lower, upper = ref.lo > 0, ref.hi < ref.L
    return (int((ref.path - ref.lo)[lower].min()) if lower.any() else None, int((ref.hi - 1 - ref.path)[upper].min()) if upper.any() else None)


def same_result(a, b):
    return b is not None and np.array_equal(a.path, b.path) and np.float32(a.total).view(np.int32) == np.float32(b.total).view(np.int32)


def path_frames_changed(a, b):
    return a.T if b is None else int(np.sum(a.path != b.path))


def row_cells_changed(a, b):
    """In-band checkpoint cells of `a` that `b` (a faulted reference of the same lattice) holds otherwise, by absolute position;
    a cell outside b's band counts as -inf there."""
    if b is None:
        return sum(len(r) for r in a.rows)
    n = 0
    for k, row in enumerate(a.rows):
        t = P.CK * (k + 1) - 1
        pos = np.arange(a.lo[t], a.hi[t])
        j = pos - b.lo[t]
        inside = (j >= 0) & (j < b.hi[t] - b.lo[t])
        theirs = np.where(inside, b.rows[k][np.clip(j, 0, len(b.rows[k]) - 1)], P.NEG)
        n += int(np.sum(theirs.view(np.int32) != row.view(np.int32)))
    return n


def first_difference(ref, rows_got):
    """(k, frame, position, got, want, distance to lo, distance to hi - 1) of the first in-band checkpoint cell that differs
    in bits, or None; rows_got[k] is indexed like ref.rows[k]."""
    for k, row in enumerate(ref.rows):
        bad = np.nonzero(np.asarray(rows_got[k]).view(np.int32) != row.view(np.int32))[0]
        if bad.size:
            t = P.CK * (k + 1) - 1
            p = int(ref.lo[t] + bad[0])
            return k, t, p, float(rows_got[k][bad[0]]), float(row[bad[0]]), p - int(ref.lo[t]), int(ref.hi[t]) - 1 - p, int(bad.size)
    return None


# ---- the checkpoint rows as the kernels lay them out: R floats per row, position p at p & (R - 1) of a ring, else at p ----
def pack_rows(ref, R, ring):
    """The reference's rows stored the way the forward kernels store them (flat, row k at k R); NaN where nothing is stored."""
    img = np.full(len(ref.rows) * R, np.nan, np.float32)
    for k, row in enumerate(ref.rows):
        t = P.CK * (k + 1) - 1
        img[k * R + P.map_index(np.arange(ref.lo[t], ref.hi[t], dtype=np.int64), R, ring)] = row
    return img


def read_rows(img, ref, R, ring, fault=None):
    """Per row k the floats of the band of frame 32 (k + 1) - 1, read back from a flat image (NaN past its end)."""
    out = []
    for k in range(len(ref.rows)):
        t = P.CK * (k + 1) - 1
        idx = k * R + P.map_index(np.arange(ref.lo[t], ref.hi[t], dtype=np.int64), R, ring, fault)
        out.append(np.where(idx < img.size, img[np.minimum(idx, img.size - 1)], np.float32(np.nan)).astype(np.float32))
    return out


def dead_slots(img, ref, R):
    """Per row k of a ring of R slots the floats of the slots no band position of frame 32 (k + 1) - 1 maps to."""
    out = []
    for k in range(len(ref.rows)):
        t = P.CK * (k + 1) - 1
        dead = np.ones(R, bool)
        dead[np.arange(ref.lo[t], ref.hi[t]) & (R - 1)] = False
        out.append(img[k * R:(k + 1) * R][dead])
    return out


def rows_differ(ref, rows_got):
    return sum(int(np.sum(np.asarray(g).view(np.int32) != r.view(np.int32))) for g, r in zip(rows_got, ref.rows))


def chain_entries(ref, rises):
    """The chunk entries a chunk-parallel backtrace builds from the end position and a set of map rows."""
    e = np.empty(len(ref.te), np.int64)
    e[-1] = ref.end
    for c in range(len(ref.te) - 1, 0, -1):
        k = int(e[c] - ref.lo[ref.te[c]])
        e[c - 1] = e[c] - (int(rises[c][k]) if 0 <= k < len(rises[c]) else 0)
    return e


def unreachable_share(ref):
    """(cells that hold -inf, all) in-band checkpoint cells."""
    cells = sum(len(r) for r in ref.rows)
    return cells - sum(int(np.isfinite(r).sum()) for r in ref.rows), cells
