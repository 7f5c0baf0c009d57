"""Inputs of the banded best-path tests (tests/test_banded_cpu.py asserts on tests/band_ref.py that they do what their names
say; tests/test_banded_gpu.py runs them through the kernels).  A case is (log_probs, labels, band_lo, beam, max_move).

Log-probs are quantised to 1/8 so that ties between moves are common; labels hold the value 0; one family has -inf entries.
"""
import numpy as np

import band_ref as R

V = 8


def ext_of(labels):
    ext = np.zeros(2 * len(labels) + 1, np.int32)
    ext[1::2] = labels
    return ext


def random_lattice(seed, T, S, V=V, ninf=False):
    rng = np.random.default_rng(seed)
    lp = (np.round(rng.standard_normal((T, V)) * 16) / 8).astype(np.float32)
    if ninf:
        lp = np.where(rng.random((T, V)) < 0.15, -np.inf, lp).astype(np.float32)
    labels = rng.integers(0, V, size=S).astype(np.int32)
    return lp, labels


def planted_lattice(seed, T, S, true_path, V=V):
    """Every frame likes the label of `true_path[t]` (-1/8) and dislikes the others (-4 .. -6, in eighths); labels 1 .. V-1 with
    a few zeros."""
    rng = np.random.default_rng(seed)
    labels = rng.integers(1, V, size=S).astype(np.int32)
    labels[rng.random(S) < 0.1] = 0
    ext = ext_of(labels)
    lp = (np.round((-4 - 2 * rng.random((T, V))) * 8) / 8).astype(np.float32)
    lp[np.arange(T), ext[np.asarray(true_path)]] = -0.125
    return lp, labels


def flat_with_step(T, at, step, base=0):
    lo = np.full(T, base, np.int64)
    lo[at:] += step
    return lo


def _const0():
    lp, lab = random_lattice(11, 64, 60)
    return lp, lab, np.zeros(64, np.int64), 40, 4


def _staircase():
    T = 90
    lp, lab = random_lattice(12, T, 150)
    lo = np.where(np.arange(T) < 30, 0, (np.arange(T) - 30) * 4).astype(np.int64)
    return lp, lab, lo, 64, 4


def _ride_hi():
    # the fastest path, 3 t + 3, is planted and lies on hi - 1 = lo + 15 from frame 4 on: lo steps by max_move - 1 every frame
    T, S, beam = 64, 100, 16
    true = 3 * np.arange(T) + 3
    lp, lab = planted_lattice(13, T, S, true)
    return lp, lab, np.maximum(0, true - (beam - 1)).astype(np.int64), beam, 4


def _ride_lo():
    # lo = 3 t + 3 for 32 frames: only the fastest path survives, on lo itself; then the band stays put and fills
    T, S, beam = 64, 100, 16
    lo = np.minimum(3 * np.arange(T) + 3, 3 * 31 + 3).astype(np.int64)
    lp, lab = random_lattice(14, T, S)
    return lp, lab, lo, beam, 4


def _shifted():
    # a band around the unbanded best path shifted up by beam / 2 - 2: the path lies 2 above lo
    T, S, beam = 120, 80, 32
    lp, lab = random_lattice(15, T, S)
    L = 2 * S + 1
    full = R.best_path_banded(lp, lab, np.zeros(T, np.int64), 2 * L, 4)[0]
    lo = np.clip(full.astype(np.int64) + (beam // 2 - 2) - beam // 2, 0, L - 1)
    return lp, lab, lo, beam, 4


def _ninf():
    T, S, beam = 100, 70, 24
    lp, lab = random_lattice(16, T, S, ninf=True)
    L = 2 * S + 1
    rng = np.random.default_rng(160)
    lo = np.clip(np.cumsum(rng.integers(0, 4, T)) - 8, 0, L - 1).astype(np.int64)
    return lp, lab, lo, beam, 4


def _better_outside():
    # the planted path, a new label every frame (no zeros among them: move 2 must stay open), runs ONE position above hi - 1:
    # the band must not see it
    T, S, beam = 80, 100, 12
    true = 2 * np.arange(T) + 1
    rng = np.random.default_rng(17)
    lab = rng.integers(1, V, size=S).astype(np.int32)
    lp = (np.round((-4 - 2 * rng.random((T, V))) * 8) / 8).astype(np.float32)
    lp[np.arange(T), ext_of(lab)[true]] = -0.125
    return lp, lab, np.maximum(0, true - beam).astype(np.int64), beam, 4


def _no_overlap():
    T, beam, mm = 64, 160, 4
    lp, lab = random_lattice(18, T, 600)
    return lp, lab, flat_with_step(T, 56, beam + mm), beam, mm


def _ring_wrap():
    # L = 1401 on a ring of 1024 slots: the band of 300 straddles slot 1023 -> 0 around frame 330
    T, S, beam = 520, 700, 300
    L = 2 * S + 1
    lp, lab = random_lattice(19, T, S)
    pts = [(0, 0), (100, 100), (300, 900), (T, L)]
    lo = np.zeros(T, np.int64)
    for (f0, p0), (f1, p1) in zip(pts[:-1], pts[1:]):
        t = np.arange(f0, f1)
        lo[f0:f1] = p0 + (p1 - p0) * (t - f0) // (f1 - f0) - beam // 2
    return lp, lab, np.clip(lo, 0, L - 1), beam, 4


def _slow_table(T, L, every=2):
    return np.minimum(np.arange(T) // every, L - 1).astype(np.int64)


def _small(T, S, beam, seed, mm=4):
    def make():
        lp, lab = random_lattice(seed, T, S)
        return lp, lab, _slow_table(T, 2 * S + 1), beam, mm
    return make


STEPS = (1, 15, 16, 17, 63, 64, 65, 500, 159, 1100)   # 159 = beam - 1; 1100 = more than the whole ring


def _step(step):
    def make():
        T, beam = 64, 160
        lp, lab = random_lattice(200 + step, T, 600)
        return lp, lab, flat_with_step(T, 56, step), beam, 4
    return make


def _step1009():
    # lo goes from 15 to 1024 in one frame with a band of 1009: all 64 lanes of the ring are re-labelled at once, and the old
    # band's top cells (positions 1021 .. 1023, live by then) are the only predecessors of the new band's first three
    T, S, beam = 360, 600, 1009
    lp, lab = random_lattice(20, T, S)
    lo = np.full(T, 15, np.int64)
    lo[:5] = 0
    lo[350:] = 1024
    return lp, lab, lo, beam, 4


CASES = {
    "const0": _const0, "staircase": _staircase, "ride_hi": _ride_hi, "ride_lo": _ride_lo, "shifted": _shifted, "ninf": _ninf,
    "better_outside": _better_outside, "no_overlap": _no_overlap, "ring_wrap": _ring_wrap, "step1009": _step1009,
    "T1": _small(1, 5, 8, 31), "T2": _small(2, 5, 8, 32), "T3": _small(3, 5, 8, 33), "S0": _small(9, 0, 4, 34),
    "T5": _small(5, 10, 8, 35), "T6": _small(6, 10, 8, 36), "T7": _small(7, 10, 8, 37),
    "beam_ge_L": _small(30, 10, 50, 38), "beam1": _small(20, 10, 1, 39), "mm2": _small(40, 20, 8, 40, mm=2),
    "mm3": _small(40, 20, 8, 41, mm=3), "mm1": _small(10, 20, 8, 42, mm=1),
}
CASES.update({f"step{s}": _step(s) for s in STEPS})
NAMES = list(CASES)
_made, _want = {}, {}


def case(name):
    if name not in _made:
        _made[name] = CASES[name]()
    return _made[name]


def want(name):
    """band_ref's answer (path, labels, scores, total), or None where it raises ValueError: computed once."""
    if name not in _want:
        lp, lab, lo, beam, mm = case(name)
        try:
            _want[name] = R.best_path_banded(lp, lab, lo, beam, mm, return_total=True)
        except ValueError:
            _want[name] = None
    return _want[name]


def rescue(seed):
    """The issue's case: T = 240, S = 60, V = 8, beam 24; the planted path waits at position 0 for 96 frames, then crosses
    the text.  Returns (lp, labels, L, beam, pre)."""
    rng = np.random.default_rng(seed)
    T, S, beam, pre = 240, 60, 24, 96
    labels = rng.integers(1, V, S).astype(np.int32)
    ext = ext_of(labels)
    L = 2 * S + 1
    true = np.zeros(T, np.int64)
    true[pre:] = (np.arange(T - pre) * (L - 1)) // (T - pre - 1)
    lp = (-4 - 2 * rng.random((T, V))).astype(np.float32)
    lp[np.arange(T), ext[true]] = -0.1
    lp = (np.round(lp * 8) / 8).astype(np.float32)
    return lp, labels, L, beam, pre
