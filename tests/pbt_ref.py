"""Float32 reference of the chunk-parallel backtrace (ka_parallel_bt.hpp): the banded best-path DP with the move taken at
EVERY band cell, and from it what the three map kernels compute - the rise of every band position over every 32-frame chunk,
the entry position of every chunk and of every super-chunk.

The recurrence is the project's restatement of align.py:62-93 (the same one as oracle.ctc_best_path_numpy, dense over the
band instead of compacted): band lo(t) = max(0, L t // T - beam // 2), hi(t) = min(lo + beam, L); moves 0 .. max_move - 1;
move 2 vetoed wherever the expanded transcript holds 0 (blanks, and labels that are 0); the first move that attains the
maximum wins; scores are a float32 add chain.  A cell is `reachable` when its score is finite - with finite log-probs that
is the reference's live set.  tests/test_parallel_backtrace_cpu.py pins path, labels, scores and total to the C oracle
bit for bit on every case below.

``fault=`` seeds one deliberate error (FAULTS) so that the CPU tests can show that the cases hold the ties, zero labels,
band edges and ring wraps at which a wrong kernel would differ.  No product file imports this module.
"""
import functools

import numpy as np

from oracle import oracle as O

CK = 32          # frames per chunk (kCkFrames)
SUPER = 32       # chunks per super-chunk (kSuperChunks)
CM_OUT = 408     # positions an 8-cell map wavefront delivers (kCmOut)
CM_OUT_WIDE = 1048   # ... and an 18-cell one (kCmOutWide)
FAST_MAX_BAND = 1009   # widest band of the one-wavefront form (kFastMaxBand)
WAVE_RING = 1024

# last_max: the LAST move that attains the maximum wins;  no_veto: move 2 is never vetoed;  lo_plus_one: the band starts one
# position higher wherever it has left 0;  rise_short: the rise is measured to the first frame of the chunk instead of the last
# frame of the chunk before (one move too few);  no_ring_mask: a map row is indexed with p instead of p & (R - 1)
FAULTS = ("last_max", "no_veto", "lo_plus_one", "rise_short", "no_ring_mask")
# ... and four more for the band edges of the forward pass (tests/bestpath_cases.py; kept apart so that the
# map tests' table of faults stays what it was).  hi_minus_one / hi_plus_one: the band ends one position lower / higher wherever
# its end is a real edge (hi < L);  lo_minus_one: it starts one position lower wherever it has left 0;  stale_label: a position
# that enters the band at the upper edge keeps the label of position - 1024 (the slot's last owner in a ring of 1024) for one frame
EDGE_FAULTS = ("hi_minus_one", "hi_plus_one", "lo_minus_one", "stale_label")

NEG = np.float32(-np.inf)


def expand(labels):
    ext = np.zeros(2 * len(labels) + 1, np.int64)
    ext[1::2] = labels
    return ext


def band(T, L, beam, fault=None):
    """lo(t), hi(t) of every frame (align.py:64-65)."""
    t = np.arange(T, dtype=np.int64)
    lo = np.maximum(0, L * t // T - beam // 2)
    if fault == "lo_plus_one":
        lo = np.where(lo > 0, lo + 1, lo)
    hi = np.minimum(lo + beam, L)
    if fault == "hi_minus_one":
        hi = np.where(hi < L, np.maximum(hi - 1, lo + 1), hi)
    elif fault == "hi_plus_one":
        hi = np.where(hi < L, hi + 1, hi)
    elif fault == "lo_minus_one":
        lo = np.where(lo > 0, lo - 1, lo)
    return lo, hi


def chunk_last_frames(T):
    nck = (T - 1) // CK + 1
    return np.minimum(np.arange(nck, dtype=np.int64) * CK + CK - 1, T - 1)


def super_last_frames(T):
    nck = (T - 1) // CK + 1
    nsup = (nck + SUPER - 1) // SUPER
    return np.array([min(min(s * SUPER + SUPER, nck) * CK - 1, T - 1) for s in range(nsup)], np.int64)


class Ref:
    """What best_path_with_moves returns; rise[c] / reachable[c] are indexed by p - lo[te[c]] (None for chunk 0); rows[k] is
    the score row after frame 32 (k + 1) - 1, indexed by p - lo of that frame: checkpoint k of the forward kernels."""


def best_path_with_moves(log_probs, labels, beam_size=1000, max_move=4, fault=None, maps=True):
    """maps=False leaves the rises out (rise and reachable stay [None]): half the time, for callers that want the path, the
    total and the checkpoint rows only."""
    assert fault is None or fault in FAULTS + EDGE_FAULTS, fault
    lp = np.ascontiguousarray(log_probs, np.float32)
    ext = expand(labels)
    T, L = lp.shape[0], ext.shape[0]
    lo, hi = band(T, L, beam_size, fault)
    wmax = int((hi - lo).max())
    moves = np.zeros((T, wmax), np.int8)
    finite = np.zeros((T, wmax), bool)
    vetoed = np.zeros(L, bool) if fault == "no_veto" else ext == 0
    pad = max_move - 1
    prev = np.full(L + pad, NEG, np.float32)     # prev[pad + p]: score of position p after the frame before
    prev[pad] = 0.0
    rows = []
    for t in range(T):
        a, b = int(lo[t]), int(hi[t])
        w = b - a
        lab_t, veto_t = ext[a:b], vetoed[a:b]
        if fault == "stale_label" and t > 0 and b > max(int(hi[t - 1]), WAVE_RING):
            fresh = np.arange(max(int(hi[t - 1]), WAVE_RING, a), b)
            lab_t, veto_t = lab_t.copy(), veto_t.copy()
            lab_t[fresh - a] = ext[fresh - WAVE_RING]
            veto_t[fresh - a] = vetoed[fresh - WAVE_RING]
        e = lp[t, lab_t]
        cand = np.full((max_move, w), NEG, np.float32)
        for j in range(max_move):
            cand[j] = prev[pad + a - j:pad + b - j] + e
            if j > 0 and j % 2 == 0:
                cand[j, veto_t] = NEG
        if fault == "last_max":
            mv = max_move - 1 - np.argmax(cand[::-1], axis=0)
        else:
            mv = np.argmax(cand, axis=0)
        sc = cand[mv, np.arange(w)]
        moves[t, :w] = mv
        finite[t, :w] = np.isfinite(sc)
        prev = np.full(L + pad, NEG, np.float32)
        prev[pad + a:pad + b] = sc
        if t % CK == (CK - 2 if fault == "rise_short" else CK - 1) and t < T - 1 and len(rows) < (T - 1) // CK:
            rows.append(sc)      # (rise_short: the same off-by-one in the forward pass - the row is taken a frame early)
    r = Ref()
    r.T, r.L, r.W, r.beam, r.max_move = T, L, max(1, min(beam_size, L)), beam_size, max_move
    r.lo, r.hi, r.moves, r.finite, r.rows = lo, hi, moves, finite, rows
    live = np.nonzero(finite[T - 1])[0]
    if live.size == 0:
        raise ValueError("attempt to get argmax of an empty sequence")
    r.end = int(lo[T - 1] + live[-1])
    r.total = prev[pad + r.end]
    path = np.empty(T, np.int32)
    p = r.end
    for t in range(T - 1, -1, -1):
        path[t] = p
        p -= int(moves[t, p - lo[t]])
    r.path = path
    r.labels = ext[path].astype(np.int32)
    r.scores = lp[np.arange(T), r.labels]      # (stale_label: the labels and scores of the positions, as the output gather reads them)
    r.te = chunk_last_frames(T)
    r.entries = path[r.te].astype(np.int32)
    r.super_entries = path[super_last_frames(T)].astype(np.int32)
    r.rise, r.reachable = [None], [None]
    if not maps:
        return r
    short = 1 if fault == "rise_short" else 0
    for c in range(1, len(r.te)):
        te = int(r.te[c])
        pos = np.arange(lo[te], hi[te], dtype=np.int64)
        q = pos.copy()
        for t in range(te, int(r.te[c - 1]) + short, -1):
            k = q - lo[t]
            inside = (k >= 0) & (k < hi[t] - lo[t])      # (a cell outside the band is unreachable: every candidate ties, move 0)
            q = q - np.where(inside, moves[t, np.clip(k, 0, wmax - 1)], 0)
        r.rise.append((pos - q).astype(np.int32))
        r.reachable.append(finite[te, :hi[te] - lo[te]].copy())
    return r


# ---- the map rows as the kernels lay them out: a byte per position, R bytes per chunk ----
def ring_of(T, S, beam, form):
    """(R, ring): bytes per map row and whether position p lies at p & (R - 1) (else at p), restated from plan_tiles'
    checkpoint row (the tiled forms) and the one-wavefront form's 1024 slots."""
    L = 2 * S + 1
    if form == "wave":
        return WAVE_RING, True
    W = max(1, min(beam, L))
    ring = 1024
    while ring < W + 512:
        ring *= 2
    whole = (L + 255) // 256 * 256
    return (whole, False) if whole <= ring else (ring, True)


def map_index(p, R, ring, fault=None):
    return p & (R - 1) if ring and fault != "no_ring_mask" else p


def pack_maps(ref, R, ring):
    """The reference's rises stored the way chunk_map_kernel stores them (flat, chunk c at c R); 255 where nothing is stored."""
    m0 = np.full(len(ref.te) * R, 255, np.uint8)
    for c in range(1, len(ref.te)):
        te = int(ref.te[c])
        pos = np.arange(ref.lo[te], ref.hi[te], dtype=np.int64)
        m0[c * R + map_index(pos, R, ring)] = ref.rise[c]
    return m0


def read_maps(m0, ref, R, ring, fault=None):
    """Per chunk c >= 1 the map bytes of the band of its last frame, read back from a flat image (255 past its end)."""
    out = [None]
    for c in range(1, len(ref.te)):
        te = int(ref.te[c])
        idx = c * R + map_index(np.arange(ref.lo[te], ref.hi[te], dtype=np.int64), R, ring, fault)
        out.append(np.where(idx < m0.size, m0[np.minimum(idx, m0.size - 1)], 255).astype(np.int32))
    return out


def differs(ref, other):
    """Does `other` (a faulted reference of the same lattice) differ from `ref` in an entry, a super-chunk entry or the rise
    of a cell that `ref` can reach?  Positions are compared by their absolute index: the faulted band may lie elsewhere."""
    if not (np.array_equal(ref.entries, other.entries) and np.array_equal(ref.super_entries, other.super_entries)):
        return True
    for c in range(1, len(ref.te)):
        te = int(ref.te[c])
        k = np.arange(ref.lo[te], ref.hi[te]) - other.lo[te]
        ok = (k >= 0) & (k < other.hi[te] - other.lo[te])
        theirs = np.where(ok, other.rise[c][np.clip(k, 0, len(other.rise[c]) - 1)], -1)
        if np.any((theirs != ref.rise[c]) & ref.reachable[c]):
            return True
    return False


# ---- the cases: the smallest shapes that reach each edge of the map geometry ----
# name: (T, S, V, beam, max_move, seed, quantised to halves, transcript with label 0, forms)
ALL = ("wave", "tiled/256", "tiled/128")
TILED = ("tiled/256", "tiled/128")
CASES = {
    # frames against chunks (32) and super-chunks (1024), small bands
    "t1": (1, 3, 5, 7, 4, 11, False, False, ALL),
    "t31_unbanded": (31, 3, 5, 1000, 4, 12, True, False, ALL),
    "t32_w7": (32, 20, 39, 7, 4, 13, False, False, ALL),
    "t33_w7_zero": (33, 40, 39, 7, 4, 14, True, True, ALL),
    "t1024_w7_gentle_m2": (1024, 51, 5, 7, 2, 15, True, False, ALL),
    "t1025_w400_m3_zero": (1025, 500, 39, 400, 3, 16, False, True, ALL),
    "t65_s0_m1": (65, 0, 5, 7, 1, 17, False, False, ALL),
    "t33_s0": (33, 0, 64, 1000, 4, 18, False, False, ALL),
    "t1025_w401_unbanded_m2": (1025, 200, 39, 1000, 2, 19, False, False, ALL),
    "t2049_w205_gentle": (2049, 102, 64, 1000, 4, 20, True, False, ALL),
    # both sides of the switch from 8 to 18 cells per lane (W + 7 <= 408), on a band that crosses the rings' wraps
    "w401_wrap": (2049, 1000, 64, 401, 4, 21, True, False, ALL),
    "w402_wrap_m3_zero": (2049, 1000, 39, 402, 3, 22, False, True, ALL),
    # the widest band of the one-wavefront form; tiled: the whole axis as the row (1280 slots), and a ring of 2048
    "w1009_whole": (2049, 600, 64, 1009, 4, 23, True, False, ALL),
    "w1009_ring_zero": (2049, 2500, 39, 1009, 4, 24, False, True, ALL),
    # one 18-cell segment delivers 1048 positions from a multiple of 8: W + 7 <= 1048, then two segments, then three
    "w1041": (2049, 800, 39, 1041, 4, 25, False, False, TILED),
    "w1042": (2049, 800, 64, 1042, 4, 26, True, False, TILED),
    "w1048_zero": (2049, 1400, 39, 1048, 4, 27, False, True, TILED),
    "w1049": (2049, 1400, 5, 1049, 4, 28, False, False, TILED),
    "w2200": (4500, 2250, 39, 2200, 4, 29, True, False, TILED),
    # L / T near 2.9: the rise reaches 96 a chunk
    "steep_w7": (1025, 1486, 39, 7, 4, 30, False, False, ALL),
    "steep_w400": (2049, 2960, 64, 400, 4, 31, True, False, ALL),
    "steep_w402_zero": (2049, 2960, 39, 402, 4, 32, False, True, ALL),
    # the launch's widest band picks cells per lane and segment count for all its lattices: a narrow band beside a wide one
    "w401_beside_w1000": (1025, 200, 39, 1000, 4, 33, True, False, ALL),
    "w7_beside_w2200": (1025, 3, 39, 2200, 4, 34, False, False, ALL),      # (one-wavefront form: the wide one runs in the generic kernels)
}
# (T, S) of the shorter lattices that share the case's launch, where they are not the default of companions()
BESIDE = {"w401_beside_w1000": [(1000, 800), (300, 40)], "w7_beside_w2200": [(1000, 1100), (300, 40)]}
NAMES = tuple(CASES)


def inputs(T, S, V, seed, quantised, zero):
    lp = O.hash_logprobs(T, V, seed)
    if quantised:
        lp = (np.round(lp * 2) / 2).astype(np.float32)      # real ties
    lab = O.hash_labels(S, V, seed) if S else np.zeros(0, np.int32)
    if zero and S:
        lab = lab.copy()
        lab[_zero_at(S, seed)] = 0
    return lp, lab


def _zero_at(S, seed):
    return np.random.default_rng(seed).random(S) < 0.2


@functools.lru_cache(maxsize=None)
def case(name):
    """(log_probs, labels, beam, max_move) of a case; shared and never written to."""
    T, S, V, beam, mm, seed, quantised, zero, _ = CASES[name]
    lp, lab = inputs(T, S, V, seed, quantised, zero)
    lp.setflags(write=False)
    lab.setflags(write=False)
    return lp, lab, beam, mm


def companions(name):
    """Two shorter lattices of other T and S that share a launch with the case: the case stays descriptor 0 (the longest),
    which is the one ka_debug_chunk_entries reports.  Their bands are no wider than the case's, except in BESIDE."""
    T, S, V, beam, mm, seed, quantised, zero, _ = CASES[name]
    shapes = BESIDE.get(name, [(max(1, T * 2 // 3), S // 2), (max(1, T // 3), S // 5)])
    return [inputs(t, s, V, seed + 100 * (i + 1), quantised, zero) for i, (t, s) in enumerate(shapes)]


@functools.lru_cache(maxsize=None)
def reference(name):
    lp, lab, beam, mm = case(name)
    return best_path_with_moves(lp, lab, beam, mm)


def geometry(name):
    """The classes of the map kernels' geometry a case belongs to."""
    T, S, V, beam, mm, _, quantised, zero, forms = CASES[name]
    L = 2 * S + 1
    W = max(1, min(beam, L))
    out = CM_OUT if W + 7 <= CM_OUT else CM_OUT_WIDE
    tags = {f"cells{8 if out == CM_OUT else 18}", f"segments{(W + 7 + out - 1) // out}", f"max_move{mm}", f"V{V}"}
    tags.add("banded" if L > beam else "unbanded")
    if W in (7, 400, 401, 402, 1009, 1041, 1042, 1048, 1049):
        tags.add(f"W{W}")
    if T in (1, 31, 32, 33, 1024, 1025, 2049):
        tags.add(f"T{T}")
    if "wave" in forms and L > WAVE_RING:
        tags.add("wave_wrap")
    R, ring = ring_of(T, S, beam, "tiled")
    tags.add("tiled_ring" if ring and L > R else "tiled_whole")
    if ring and L > 2 * R:
        tags.add("tiled_ring_twice")
    slope = L / T
    for tag, a, b in (("gentle", 0.0, 0.15), ("unit", 0.8, 1.25), ("steep", 2.85, 3.0)):
        if T > CK and a <= slope <= b:
            tags.add(tag)
    wide = max([W] + [min(beam, 2 * s + 1) for _, s in BESIDE.get(name, [])])
    if (wide + 7 <= CM_OUT) != (W + 7 <= CM_OUT):
        tags.add("cells18_for_a_narrow_band")
    if wide + 7 > 2 * CM_OUT_WIDE and W + 7 <= CM_OUT_WIDE:
        tags.add("three_segments_for_a_narrow_band")
    tags.update(t for t, on in (("zero_label", zero), ("quantised", quantised), ("S0", S == 0), ("tiled_only", "wave" not in forms)) if on)
    return tags


GEOMETRY = {"cells8", "cells18", "segments1", "segments2", "segments3", "max_move1", "max_move2", "max_move3", "max_move4",
            "V5", "V39", "V64", "banded", "unbanded", "W7", "W400", "W401", "W402", "W1009", "W1041", "W1042", "W1048", "W1049",
            "T1", "T31", "T32", "T33", "T1024", "T1025", "T2049", "wave_wrap", "tiled_ring", "tiled_whole", "tiled_ring_twice",
            "gentle", "unit", "steep", "zero_label", "quantised", "S0", "tiled_only", "cells18_for_a_narrow_band",
            "three_segments_for_a_narrow_band"}


def excluded_share(ref):
    """(unreachable, all) map cells of a lattice: the band positions of the last frame of every chunk c >= 1."""
    cells = sum(len(x) for x in ref.reachable[1:])
    return cells - sum(int(x.sum()) for x in ref.reachable[1:]), cells
