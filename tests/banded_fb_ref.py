"""Float64 references of the forward-backward calls over a caller-given band.

The references of the diagonal calls - posterior_ref.forward_backward, occupancy_ref.occupancy, duration_ref.durations - take
their windows from posterior_ref.windows(T, L, beam) and nothing else about the band.  Here that one function is swapped for
the table's rule while a reference runs and put back afterwards:

    lo_t = band_lo[t]        hi_t = min(lo_t + beam, L)

so every banded reference IS the diagonal one on other windows, and with the diagonal as the table it reproduces it exactly
(tests/test_banded_posteriors_cpu.py).  ``enumerate_gamma`` is independent of all of them: every path of a tiny lattice.

Plantable faults (FAULTS), each a mistake a kernel's table walk could make:
    late_table     the table read one frame late: lo_t = band_lo[max(t - 1, 0)]
    past_end_zero  a walk that fetches a frame ahead from a copy shifted by one and does not clamp at its end: the entry past
                   the end reads 0, and it is the last frame's: lo_{T-1} = 0
    hi_unclamped   hi_t = lo_t + beam without the min with L.  The lattice is then run with blank positions behind the text (a
                   kernel would read past the labels).  Paths only move up, so nothing a path can do above L - 1 changes gamma
                   inside [0, L): what this fault moves is the windows' width and the live terminals, which reach past L - 1.
"""
import contextlib
import itertools

import numpy as np

import duration_ref as D
import occupancy_ref as O
import posterior_ref as R

FAULTS = ("late_table", "past_end_zero", "hi_unclamped")


def table_windows(band_lo, L, beam, fault=None):
    """(lo, hi) of every frame under the table."""
    assert fault is None or fault in FAULTS, fault
    lo = np.asarray(band_lo, np.int64).reshape(-1).copy()
    if fault == "late_table":
        lo = np.concatenate([lo[:1], lo[:-1]])
    if fault == "past_end_zero":
        lo[-1] = 0
    hi = lo + beam if fault == "hi_unclamped" else np.minimum(lo + beam, L)
    return lo, hi


@contextlib.contextmanager
def under_table(band_lo, fault=None):
    """posterior_ref.windows answers with the table while the block runs."""
    saved = R.windows

    def windows(T, L, beam):
        assert len(np.asarray(band_lo).reshape(-1)) == T, "a table has one entry per frame"
        return table_windows(band_lo, L, beam, fault)
    R.windows = windows
    try:
        yield
    finally:
        R.windows = saved


def _labels_for(labels, beam, fault):
    """The labels a reference runs on: the caller's, or under hi_unclamped with blanks behind them for the windows to reach."""
    labels = np.asarray(labels, np.int64).reshape(-1)
    return np.concatenate([labels, np.zeros((int(beam) + 1) // 2, np.int64)]) if fault == "hi_unclamped" else labels


def forward_backward(lp, labels, path, band_lo, beam, mm, full=False, fault=None):
    with under_table(band_lo, fault):
        return R.forward_backward(lp, _labels_for(labels, beam, fault), path, beam, mm, full=full)


def ref_at(lp, labels, terminal, band_lo, beam, mm, fault=None):
    """forward_backward(full=True) of the band's paths that end at ``terminal``."""
    return forward_backward(lp, labels, np.full(np.asarray(lp).shape[0], int(terminal), np.int64), band_lo, beam, mm, True, fault)


def occupancy(lp, labels, terminal, band_lo, beam, mm, fault=None):
    with under_table(band_lo, fault):
        return O.occupancy(lp, _labels_for(labels, beam, fault), terminal, beam, mm)


def durations(lp, labels, terminal, band_lo, beam, mm, fault=None):
    """duration_ref.durations of ref_at's result (None for a lattice without one), and that result."""
    ref = ref_at(lp, labels, terminal, band_lo, beam, mm, fault)
    L = 2 * len(_labels_for(labels, beam, fault)) + 1
    return (D.durations(ref, L) if ref["status"] == R.OK else None), ref


def live_terminals(lp, labels, band_lo, beam, mm, fault=None):
    with under_table(band_lo, fault):
        return R.live_terminals(lp, _labels_for(labels, beam, fault), beam, mm)


def enumerate_gamma(lp, labels, terminal, band_lo, beam, mm):
    """(gamma float64 [T, L], ll) from every path of a tiny lattice that stays inside the table's windows and ends at the
    terminal; gamma is all NaN and ll -inf if there is none."""
    lp = np.asarray(lp, np.float64)
    T = lp.shape[0]
    lab = R.expand(labels)
    L = len(lab)
    lo, hi = table_windows(band_lo, L, beam)
    total, gamma = 0.0, np.zeros((T, L))
    for moves in itertools.product(range(mm), repeat=T):
        s, score, states = 0, 0.0, []
        for t, j in enumerate(moves):
            s += j
            if not (lo[t] <= s < hi[t]) or (j >= 2 and j % 2 == 0 and lab[s] == 0):
                break
            score += lp[t, lab[s]]
            states.append(s)
        if len(states) != T or states[-1] != terminal:
            continue
        p = np.exp(score)
        total += p
        gamma[np.arange(T), states] += p
    if total == 0.0:
        return np.full((T, L), np.nan), -np.inf
    return gamma / total, float(np.log(total))


def dense_gamma(ref, L):
    """forward_backward(full=True)'s gamma as [T, L], 0 outside the windows (what a faulty window holds past L is dropped)."""
    out = np.zeros((len(ref["gamma"]), L))
    for t, (lo, g) in enumerate(ref["gamma"]):
        w = min(len(g), L - lo)
        out[t, lo:lo + w] = g[:w]
    return out


def random_table(rng, T, L, max_step, lo0=0):
    """A valid table: non-decreasing from lo0, steps in [0, max_step], clipped to L - 1."""
    steps = rng.integers(0, max_step + 1, size=T)
    steps[0] = 0
    return np.minimum(lo0 + np.cumsum(steps), L - 1).astype(np.int64)
