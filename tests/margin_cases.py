"""Inputs of the path-margin tests (tests/test_margins_cpu.py asserts on tests/margin_ref.py that they do what their names say
and that every planted fault shows on them; tests/test_margins_gpu.py runs them through the kernels).

A case is a dict: lp float32 [T, V], labels int32 [S], path int32 [T], beam, mm, band_lo (int32 [T] or None: the diagonal) and
catches, the faults of margin_ref.FAULTS the case is meant to notice.  Log-probs are multiples of 1/8 in a narrow range, so
that every float64 sum is exact and ties are common; labels hold the value 0, which arms the veto.
"""
import numpy as np

import margin_ref as R

V = 6


def eighths(seed, T, S, V=V, ninf=0.0, zero=0.15):
    """(lp, labels): log-probs in {-2, -1.875, ..., 0}, a share `ninf` of them -inf; a share `zero` of the labels 0."""
    rng = np.random.default_rng(seed)
    lp = (-rng.integers(0, 17, size=(T, V)) / 8.0).astype(np.float32)
    if ninf:
        lp = np.where(rng.random((T, V)) < ninf, -np.inf, lp).astype(np.float32)
    labels = rng.integers(1, V, size=S).astype(np.int32)
    labels[rng.random(S) < zero] = 0
    return lp, labels


def best_or_random_path(lp, labels, beam, mm, band_lo, seed):
    """The arg-max path to the highest reachable terminal; where no terminal is reachable, any path."""
    p = R.argmax_path(lp, labels, beam, mm, band_lo)
    if p is None:
        L = 2 * len(labels) + 1
        p = np.random.default_rng(seed).integers(0, L, size=lp.shape[0])
    return p.astype(np.int32)


def _case(lp, labels, beam, mm, band_lo=None, path=None, catches=(), seed=0):
    if band_lo is not None:
        band_lo = np.ascontiguousarray(band_lo, np.int32)
    if path is None:
        path = best_or_random_path(lp, labels, beam, mm, band_lo, seed)
    return dict(lp=lp, labels=labels, path=np.ascontiguousarray(path, np.int32), beam=beam, mm=mm, band_lo=band_lo,
                catches=tuple(catches))


ALL = R.FAULTS
CORE = ("keep_group", "seed_all")     # what every lattice with two live cells in a frame notices


def _rand(seed, T, S, beam, mm, catches=CORE, **kw):
    def make():
        lp, labels = eighths(seed, T, S, **{k: v for k, v in kw.items() if k in ("V", "ninf", "zero")})
        return _case(lp, labels, beam, mm, catches=catches, seed=seed)
    return make


def _off_path(seed, T, S, beam, mm, kind):
    """A path the lattice did not choose: `outside` leaves its frame's band at some frames (and returns for the last),
    `disconnected` jumps at random inside [0, L)."""
    def make():
        lp, labels = eighths(seed, T, S)
        L = 2 * S + 1
        best = best_or_random_path(lp, labels, beam, mm, None, seed)
        rng = np.random.default_rng(seed + 1)
        if kind == "outside":
            path = best.copy()
            lo, hi = R.band_of(T, L, beam)
            for t in range(1, T - 1, 3):
                path[t] = (hi[t] + 1) if hi[t] + 1 < L else max(0, lo[t] - 2)
        else:
            path = rng.integers(0, L, size=T).astype(np.int32)
            path[T - 1] = best[T - 1]
        return _case(lp, labels, beam, mm, path=path, catches=CORE)
    return make


def _table(name):
    """A lattice of the tracking tests (tests/track_cases.py) under a table with the single step its name says, 0, 1, 16, 70 or
    504 positions at the frame the tracking call would retarget: the planted path rests inside the band on either side."""
    def make():
        import band_cases as BC
        import track_cases as TC
        lp, labels, beam, mm, _, _ = TC.case(name)
        step, at = TC.STEP_OF[name]
        table = BC.flat_with_step(lp.shape[0], at, step).astype(np.int32)
        return _case(lp, labels, beam, mm, band_lo=table, catches=("keep_group",), seed=7)
    return make


def _stairs(seed, T, S, beam, step_every, step):
    """A table that steps by `step` every `step_every` frames: the backward pass's band t+1 differs from band t."""
    def make():
        lp, labels = eighths(seed, T, S)
        L = 2 * S + 1
        table = np.minimum((np.arange(T) // step_every) * step, L - 1)
        return _case(lp, labels, beam, 4, band_lo=table, catches=CORE + ("band_same_frame",), seed=seed)
    return make


def _ninf_rows(seed, T, S, beam, mm):
    """Rows in which only the best path's label is finite: at those frames (nearly) no other state is alive, so alt is -inf
    there, and the frames around them lose most of their alternatives too."""
    def make():
        lp, labels = eighths(seed, T, S, ninf=0.04)
        path = best_or_random_path(lp, labels, beam, mm, None, seed)
        ext = R.expand(labels)
        lp = lp.copy()
        for t in range(5, T - 1, 7):
            keep = lp[t, ext[path[t]]]
            lp[t] = -np.inf
            lp[t, ext[path[t]]] = keep if np.isfinite(keep) else -1.0
        return _case(lp, labels, beam, mm, catches=("keep_group",), seed=seed)
    return make


def _wrap():
    # L = 1201 on a ring of 1024 slots: the diagonal band of 64 slides across slot 1023 -> 0 near frame 1100
    lp, labels = eighths(90, 1300, 600)
    return _case(lp, labels, 64, 4, catches=CORE, seed=90)


def _flat_ties():
    # every log-prob is -1: all complete paths tie, so every frame's margin is 0.0 and the runner-up is decided by the tie rule
    T, S = 40, 12
    labels = np.random.default_rng(5).integers(1, V, size=S).astype(np.int32)
    lp = np.full((T, V), -1.0, np.float32)
    return _case(lp, labels, 12, 4, catches=("tie_highest", "keep_group"), seed=5)


CASES = {
    # the 32-frame block borders, and a last block of one frame
    "T1": _rand(1, 1, 3, 8, 4, catches=()), "T2": _rand(2, 2, 4, 8, 4), "T3": _rand(3, 3, 5, 8, 4), "T5": _rand(5, 5, 6, 8, 4),
    "T31": _rand(31, 31, 10, 10, 4), "T32": _rand(32, 32, 10, 10, 4), "T33": _rand(33, 33, 10, 10, 4),
    "T64": _rand(64, 64, 20, 12, 4), "T65": _rand(65, 65, 20, 12, 4),
    "S0": _rand(70, 9, 0, 4, 4, catches=()),
    "beam1": _rand(71, 20, 10, 1, 4, catches=()), "beam2": _rand(72, 40, 30, 2, 4, catches=("keep_group",)),
    "beam_ge_2L": _rand(73, 30, 10, 50, 4, catches=CORE + ("open_start",)),
    "mm1": _rand(74, 20, 1, 8, 1, catches=()), "mm2": _rand(75, 60, 20, 8, 2), "mm3": _rand(76, 60, 40, 8, 3),
    "mm4_zeros": _rand(77, 60, 30, 16, 4, catches=CORE + ("veto_on_source",), zero=0.4),
    "ninf": _rand(78, 70, 30, 12, 4, ninf=0.04), "ninf_heavy": _ninf_rows(79, 50, 20, 6, 3),
    "ties": _flat_ties,
    "units": _rand(80, 48, 20, 10, 4, catches=CORE + ("ignore_unit",)),
    "outside": _off_path(81, 50, 30, 8, 4, "outside"), "disconnected": _off_path(82, 50, 30, 16, 4, "disconnected"),
    "wrap": _wrap,
    "stairs": _stairs(83, 70, 60, 12, 4, 6),
    "step0": _table("step0"), "step1": _table("step1"), "step16": _table("step16"), "step70": _table("step70"), "step504": _table("step504"),
    # the three shapes that pick the generic form
    "gen_V65": _rand(84, 60, 40, 12, 4, V=65), "gen_mm5": _rand(85, 60, 40, 12, 5),
    "gen_band1010": _rand(86, 400, 505, 1010, 4, catches=CORE + ("open_start",)),
}
NAMES = list(CASES)
_made, _want = {}, {}


def case(name):
    if name not in _made:
        _made[name] = CASES[name]()
    return _made[name]


def want(name, unit, **fault):
    """margin_ref's answer for a case and a unit, computed once (planted faults are not kept)."""
    c = case(name)
    if fault:
        return R.margins_ref(c["lp"], c["labels"], c["path"], c["beam"], c["mm"], unit, c["band_lo"], **fault)
    if (name, unit) not in _want:
        _want[name, unit] = R.margins_ref(c["lp"], c["labels"], c["path"], c["beam"], c["mm"], unit, c["band_lo"])
    return _want[name, unit]


def fast_form(c):
    return c["lp"].shape[1] <= 64 and c["mm"] <= 4 and min(c["beam"], 2 * len(c["labels"]) + 1) <= 1009


def same(a, b):
    """Do two answers (margin_ref's dicts) agree bit for bit?"""
    return a["status"] == b["status"] and np.array_equal(R.bits(a["through"]), R.bits(b["through"])) and \
        np.array_equal(R.bits(a["alt"]), R.bits(b["alt"])) and np.array_equal(a["runner_up"], b["runner_up"]) and \
        R.bits([a["score"]])[0] == R.bits([b["score"]])[0]


# ---- the family of the exact identities (test_margins_cpu.py) and of the batch tests: T 12..70, S 4..40, beams 6..40,
# max_move 2..4, V = 6, the arg-max path to the highest reachable terminal ----
def identity_family(n, seed=1000):
    rng = np.random.default_rng(seed)
    out = []
    while len(out) < n:
        T, S = int(rng.integers(12, 71)), int(rng.integers(4, 41))
        beam, mm = int(rng.integers(6, 41)), int(rng.integers(2, 5))
        lp, labels = eighths(int(rng.integers(1 << 30)), T, S)
        p = R.argmax_path(lp, labels, beam, mm)
        if p is not None:
            out.append(_case(lp, labels, beam, mm, path=p))
    return out
