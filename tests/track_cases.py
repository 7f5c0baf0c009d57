"""Inputs of the tracking best-path tests (tests/test_tracking_cpu.py asserts on tests/track_ref.py that they do what their
names say; tests/test_tracking_gpu.py runs them through the kernels).  A case is (log_probs, labels, beam, max_move, period,
end_rule).  Log-probs are quantised to 1/8 so that ties are common; labels hold the value 0; one family has -inf entries.
"""
import numpy as np

import band_cases as C
import track_ref as R

V = C.V


def planted(seed, T, S, true_path, gate=None):
    """band_cases.planted_lattice with labels 1 .. V-2 (no label 0: a move of 2 onto every label stays open).  `gate`: an odd
    position whose label, V-1, no other position has - every path but the planted one pays for the frame spent there."""
    rng = np.random.default_rng(seed)
    labels = rng.integers(1, V - 1, size=S).astype(np.int32)
    if gate is not None:
        labels[(gate - 1) // 2] = V - 1
    ext = C.ext_of(labels)
    lp = (np.round((-4 - 2 * rng.random((T, V))) * 8) / 8).astype(np.float32)
    lp[np.arange(T), ext[np.asarray(true_path)]] = -0.125
    return lp, labels


def climb_to(T, top):
    """(path, gate): 3 positions a frame up to the gate, the odd position at or just below `top`, one frame there, then `top`
    for good.  With the gate's label unique, the planted path is the only one without a bad frame, and once it rests on `top`
    the first maximum of the scores is `top` (where `top` is a blank, the blank two above ties with it, and is higher)."""
    gate = top if top % 2 else top - 1
    path = np.minimum(3 * (np.arange(T) + 1), gate)
    arrive = int(np.argmax(path == gate))
    path[arrive + 1:] = top
    return path, gate


# ---- one retarget (period <= T - 1 < 2 period) that moves lo by a chosen step: the planted path rests on beam // 2 + step
# two frames before it.  A single retarget cannot move lo by more than beam - 1 - beam // 2 (its arg-max cell lies in the
# band): "step504" takes that maximum at the widest band of the one-wavefront form, 1009, with the arg-max in the band's top
# cell - 31 of the ring's 64 lanes are re-labelled at once; no retarget can re-label all 64.  Where the path rests on a blank
# (an even beam // 2 + step) the blank two above ties with it: the first maximum is the lower one ----
def _step(step, beam=160, period=64, T=100):
    def make():
        S = (beam + step) // 2 + 100
        true, gate = climb_to(T, beam // 2 + step)
        lp, lab = planted(300 + step, T, S, true, gate)
        return lp, lab, beam, 4, period, "highest"
    return make


STEPS = {"step0": _step(0), "step1": _step(1), "step16": _step(16), "step70": _step(70),
         "step504": _step(504, beam=1009, period=400, T=440)}
STEP_OF = {"step0": (0, 64), "step1": (1, 64), "step16": (16, 64), "step70": (70, 64), "step504": (504, 400)}   # (step, at frame)


def _tie():
    # every log-prob is -1: all live cells tie at every frame, the first maximum is position 0 and the band never moves
    T, S = 40, 30
    lab = np.random.default_rng(50).integers(1, V, size=S).astype(np.int32)
    return np.full((T, V), -1.0, np.float32), lab, 16, 4, 8, "highest"


def _random(seed, T, S, beam, mm, period, end_rule="highest", ninf=False):
    def make():
        lp, lab = C.random_lattice(seed, T, S, ninf=ninf)
        return lp, lab, beam, mm, period, end_rule
    return make


def _ninf_list(end_rule):
    # rows 13 .. 17 are all -inf: the live list of frame 14, which the retarget of frame 16 reads, holds only -inf (positions 7,
    # 9, 10, 11; the band's low end, 6, is dead), and so does the last frame's
    def make():
        rng = np.random.default_rng(48)
        T, S, V5 = 18, 26, 5
        lp = (np.round(rng.standard_normal((T, V5)) * 16) / 8).astype(np.float32)
        lp = np.where(rng.random((T, V5)) < 0.4, -np.inf, lp).astype(np.float32)
        lp[13:] = -np.inf
        lab = rng.integers(0, V5, size=S).astype(np.int32)
        return lp, lab, 8, 3, 4, end_rule
    return make


def _rescue(seed, period):
    def make():
        lp, lab, L, beam, pre = C.rescue(seed)
        return lp, lab, beam, 4, period, "highest"
    return make


def _short_audio(end_rule):
    # the audio ends in the middle of the text: the planted path stops at position 40 of 121
    def make():
        T, S = 64, 60
        true = np.clip(np.arange(T), 0, 41)
        lp, lab = planted(60, T, S, true, 41)
        return lp, lab, 24, 4, 8, end_rule
    return make


CASES = dict(STEPS)
CASES.update({
    "tie": _tie, "ninf_list": _ninf_list("highest"), "ninf_list_best": _ninf_list("best"),
    "ninf": _random(70, 100, 70, 24, 4, 8, ninf=True), "ninf_best": _random(71, 90, 70, 24, 4, 4, "best", ninf=True),
    "T1": _random(31, 1, 5, 8, 4, 4), "T2": _random(32, 2, 5, 8, 4, 4), "T3": _random(33, 3, 5, 8, 4, 4),
    "T5": _random(35, 5, 10, 8, 4, 4), "T5_best": _random(35, 5, 10, 8, 4, 4, "best"), "T9_p8": _random(36, 9, 10, 4, 4, 8),
    "S0": _random(34, 9, 0, 4, 4, 4), "S0_best": _random(34, 9, 0, 4, 4, 4, "best"),
    "beam1": _random(39, 20, 10, 1, 4, 4), "beam2": _random(43, 40, 30, 2, 4, 4), "beam_ge_2L": _random(38, 30, 10, 50, 4, 4),
    "mm1": _random(42, 20, 20, 8, 1, 4), "mm2": _random(40, 60, 40, 8, 2, 4), "mm3": _random(41, 60, 40, 8, 3, 8),
    "mm4_best": _random(44, 80, 60, 12, 4, 8, "best"),
    # L = 1401 on a ring of 1024 slots: the planted path takes a label a frame, the band of 300 follows it across slot 1023 -> 0
    "wrap": lambda: planted(45, 640, 700, np.minimum(2 * np.arange(640) + 1, 1399)) + (300, 4, 16, "highest"),
    "short_highest": _short_audio("highest"), "short_best": _short_audio("best"),
    # the three shapes that pick the generic form
    "gen_V65": lambda: C.random_lattice(46, 60, 40, V=65) + (12, 4, 8, "highest"),
    "gen_mm5": _random(47, 60, 40, 12, 5, 8), "gen_mm5_best": _random(47, 60, 40, 12, 5, 4, "best"),
    "gen_band1010": lambda: planted(48, 420, 700, *climb_to(420, 1009)) + (1010, 4, 400, "highest"),
})
CASES.update({f"rescue{s}_p{p}": _rescue(s, p) for s in range(6) for p in (4, 8)})
NAMES = list(CASES)
_made, _want = {}, {}


def case(name):
    if name not in _made:
        _made[name] = CASES[name]()
    return _made[name]


def want(name):
    """track_ref's answer (path, labels, scores, table, total, cells), or None where it raises ValueError: computed once."""
    if name not in _want:
        lp, lab, beam, mm, period, end_rule = case(name)
        try:
            _want[name] = R.best_path_tracking(lp, lab, beam, mm, period, end_rule, return_total=True, return_cells=True)
        except ValueError:
            _want[name] = None
    return _want[name]
