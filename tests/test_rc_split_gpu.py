"""The two phases of a recomputed chunk (backtrace_rc_body with max_move = 4, ka_wave_backtrace.hpp)
at the shapes where the change of layout can go wrong.  Frames 0 .. SPLIT-1 of a 32-frame chunk are recomputed two cells per
lane on the window [wlo, wlo+123], frames SPLIT .. 31 one cell per lane on [w2, w2+60] with p - w2 = 59 or 60; the walk starts
in the second window's codes and changes to the first's at frame SPLIT-1.  So the cases are about WHERE the path is around
frame SPLIT and how far it falls:

  steep     a path that drops about 3 positions per frame over whole chunks (at least 80 positions inside one chunk): the
            walk ends up at the very bottom of what either window leaves exact
  around    moves at chunk frames SPLIT-1, SPLIT and SPLIT+1, with and without a change of the two-cell lane at SPLIT-1
  still     no move at all across the split (S = 0, S = 1)
  tail      a last chunk of SPLIT-1, SPLIT, SPLIT+1 and 31 frames, and T = 1
  bottom    p <= 59 (w2 = 0) and 60 <= p <= 96 (w2 > 0 while wlo = 0); L < 61 and 61 <= L < 124
  zero      a transcript with label 0 (the other kernel instance), V = 39 and 64, a label-0 cell directly under the path at a
            frame of the second phase
  banded    a band narrower than L whose low edge and whose high edge each fall inside the one-cell window at a frame of the
            second phase (beam 48 and 260)
  control   max_move 2 and 3: their code has no second phase

Each case runs through the checkpointed one-wavefront form with the serial and with the chunk-parallel backtrace; path, labels,
scores and total are compared with the C oracle bit for bit.  The tests without the gpu mark assert from the oracle's paths
that the cases do what their names say; they need no GPU.
"""
import functools
import os

import numpy as np
import pytest

from oracle import oracle as O

CK = 32        # frames per chunk of the recomputing backtrace
SPLIT = 16     # kRcSplit: first chunk frame of the one-cell form
BACK = 59      # kRc1Back: p - w2 is 59 or 60
LANES1 = 61    # kRc1Lanes: live lanes of the one-cell window

# name: (T, S, V, beam, max_move, seed, every k-th label renamed to 0 or None[, pull])
# pull = ("low", t): every column but the blank's is lowered by 20 in the frames before t, so the path stays behind and is pushed along
# by the band's low edge; ("high", t): likewise in the frames from t on, so the path runs ahead along the band's high edge to sit
# on the last blank by then.  (With the hash generator's emissions alone a path keeps to the middle of a 260-wide band.)
CASES = {
    "steep_T64_S81": (64, 81, 39, 1000, 4, 1, None),
    "steep_T64_S95": (64, 95, 64, 1000, 4, 2, None),
    "steep_T96_S121": (96, 121, 64, 1000, 4, 3, None),
    "steep_T96_S140": (96, 140, 39, 1000, 4, 4, None),
    "steep_T96_S140_zero": (96, 140, 39, 1000, 4, 5, 3),
    "around_a": (96, 14, 39, 1000, 4, 101, None),
    "around_b": (96, 18, 39, 1000, 4, 102, None),
    "around_c": (96, 24, 39, 1000, 4, 103, None),
    "around_d": (96, 30, 39, 1000, 4, 104, None),
    "around_e": (96, 36, 39, 1000, 4, 105, None),
    "around_f": (96, 44, 39, 1000, 4, 106, None),
    "still_S1": (100, 1, 39, 1000, 4, 11, None),
    "still_S0": (100, 0, 39, 1000, 4, 12, None),
    "tail_T1": (1, 1, 39, 1000, 4, 21, None),
    "tail_T15": (15, 12, 39, 1000, 4, 22, None),
    "tail_T16": (16, 12, 39, 1000, 4, 23, None),
    "tail_T17": (17, 12, 39, 1000, 4, 24, None),
    "tail_T47": (47, 50, 39, 1000, 4, 25, None),
    "tail_T48": (48, 50, 64, 1000, 4, 26, None),
    "tail_T49": (49, 50, 39, 1000, 4, 27, None),
    "tail_T63": (63, 80, 64, 1000, 4, 28, None),
    "bottom_w2_zero": (100, 25, 39, 1000, 4, 31, None),
    "bottom_wlo_zero": (128, 45, 39, 1000, 4, 32, None),
    "short_L": (70, 29, 64, 1000, 4, 33, None),
    "mid_L": (70, 58, 39, 1000, 4, 34, None),
    "zero_label_V39": (130, 70, 39, 1000, 4, 41, 3),
    "zero_label_V64": (130, 70, 64, 1000, 4, 42, 4),
    "banded_260_low": (352, 300, 39, 260, 4, 51, None, ("low", 150)),
    "banded_260_high": (352, 300, 64, 260, 4, 54, None, ("high", 200)),
    "banded_48": (300, 150, 39, 48, 4, 52, None),
    "banded_48_zero": (300, 150, 64, 48, 4, 53, 3),
    "max_move_2": (161, 40, 39, 1000, 2, 44, None),
    "max_move_3": (161, 90, 39, 1000, 3, 45, None),
}
NAMES = tuple(CASES)
FORMS = ("serial", "parallel")
AROUND = tuple(n for n in NAMES if n.startswith("around_"))


@functools.lru_cache(maxsize=None)
def case(name):
    """(log_probs, labels) of a case: the hash generators of the other GPU tests; shared and never written to."""
    T, S, V, beam, mm, seed, zero = CASES[name][:7]
    lp = O.hash_logprobs(T, V, seed)
    lab = O.hash_labels(S, V, seed)
    if zero:
        lab = np.where(np.arange(S) % zero == 1, 0, lab).astype(np.int32)
    if len(CASES[name]) > 7:
        side, t = CASES[name][7]
        lp = lp.copy()
        lp[(slice(None, t) if side == "low" else slice(t, None)), 1:] -= np.float32(20.0)
    lp.setflags(write=False)
    lab.setflags(write=False)
    return lp, lab


@functools.lru_cache(maxsize=None)
def want(name):
    """(path, labels, scores, total, end) of the C oracle, computed once per case."""
    lp, lab = case(name)
    return O.ctc_best_path_c(lp, lab, CASES[name][3], CASES[name][4], return_total=True)


def moves(name):
    """move[t] = path[t] - path[t - 1]: what the walk decodes at frame t (frame 0 comes from the virtual state at position 0)."""
    path = want(name)[0].astype(np.int64)
    return np.diff(path, prepend=0)


def chunks(name):
    """(t0, n, p, wlo, w2) of every chunk: first frame, frames, position at its last frame, the two windows."""
    T = CASES[name][0]
    path = want(name)[0]
    out = []
    for t0 in range(0, T, CK):
        n = min(CK, T - t0)
        p = int(path[t0 + n - 1])
        out.append((t0, n, p, max(p - 96, 0) & ~1, (p - BACK) & ~1 if p > BACK else 0))
    return out


def band(name, t):
    """[lo, hi) of frame t (align.py:66-68)."""
    T, S, _, beam = CASES[name][:4]
    L = 2 * S + 1
    lo = max(L * t // T - beam // 2, 0)
    return lo, (L if L - lo < beam else lo + beam)


# ---- the cases do what their names say (no GPU) ----
def test_the_second_window_holds_the_walk_in_every_chunk_of_every_case():
    """p - w2 is 59 or 60 (or w2 = 0), and the path of the frames SPLIT .. 31 lies on lanes 0 .. 60 of it."""
    for name in NAMES:
        path = want(name)[0]
        for t0, n, p, wlo, w2 in chunks(name):
            assert w2 % 2 == 0 and wlo <= w2 and (w2 == 0 or p - w2 in (BACK, BACK + 1)), (name, t0, p, w2)
            for f in range(SPLIT, n):
                assert 0 <= path[t0 + f] - w2 < LANES1, (name, t0, f)


@pytest.mark.parametrize("name", [n for n in NAMES if n.startswith("steep_")])
def test_steep_cases_drop_80_positions_inside_one_chunk(name):
    path, mv = want(name)[0], moves(name)
    T = CASES[name][0]
    assert mv[1:].mean() > 2.5, mv[1:].mean()
    drops = [int(path[t0 + CK - 1]) - (int(path[t0 - 1]) if t0 else 0) for t0 in range(0, T, CK)]
    assert max(drops) >= 80, drops
    # a full chunk above the first with wlo > 0 among them: both windows have unknown cells below them
    assert any(d >= 80 and wlo > 0 for d, (t0, n, p, wlo, w2) in zip(drops, chunks(name))), (drops, chunks(name))


def test_steep_cases_cover_the_shapes():
    steep = [CASES[n] for n in NAMES if n.startswith("steep_")]
    assert {c[0] for c in steep} == {64, 96} and {c[2] for c in steep} == {39, 64}
    assert any(73 <= c[1] <= 95 for c in steep) and any(110 <= c[1] <= 140 for c in steep)


def test_around_cases_move_on_both_sides_of_the_split():
    def at(n, f):
        return [t for t in range(f, CASES[n][0], CK) if moves(n)[t] != 0]
    for f in (SPLIT - 1, SPLIT, SPLIT + 1):
        assert any(at(n, f) for n in AROUND), f"no case moves at chunk frame {f}"
    # pairs within one chunk of one lattice
    for a, b in ((SPLIT - 1, SPLIT), (SPLIT, SPLIT + 1)):
        assert any(set(t - a for t in at(n, a)) & set(t - b for t in at(n, b)) for n in AROUND), f"no case moves at chunk frames {a} and {b}"
    # the move at SPLIT-1 is the first that the walk decodes on the two-cell window: with and without a change of lane there
    kinds = set()
    for n in AROUND:
        path = want(n)[0]
        for t in at(n, SPLIT - 1):
            kinds.add((path[t] >> 1) != (path[t - 1] >> 1))
    assert kinds == {True, False}, kinds
    # and a chunk that stays on one position from SPLIT-1 to SPLIT+1
    assert any(not moves(n)[t0 + SPLIT - 1:t0 + SPLIT + 2].any() for n in AROUND for t0 in range(0, CASES[n][0], CK))


@pytest.mark.parametrize("name", ["still_S1", "still_S0"])
def test_still_cases_do_not_move_across_the_split(name):
    mv = moves(name)
    T = CASES[name][0]
    quiet = [c for c in range(T // CK) if not mv[max(c * CK, 1):(c + 1) * CK].any()]
    assert len(quiet) >= 2, quiet


def test_tail_cases_cover_the_partial_chunks():
    tails = [CASES[n][0] for n in NAMES if n.startswith("tail_")]
    assert {T % CK for T in tails if T > CK} >= {SPLIT - 1, SPLIT, SPLIT + 1, 31}
    assert {1, SPLIT - 1, SPLIT, SPLIT + 1} <= set(tails)      # a single partial chunk as well


def test_bottom_cases_sit_where_the_windows_start_at_zero():
    assert all(p <= BACK and w2 == 0 for t0, n, p, wlo, w2 in chunks("bottom_w2_zero"))
    assert any(60 <= p <= 96 and w2 > 0 and wlo == 0 and n == CK for t0, n, p, wlo, w2 in chunks("bottom_wlo_zero"))
    L = 2 * CASES["short_L"][1] + 1
    assert L < LANES1 and want("short_L")[4] == L - 1
    L = 2 * CASES["mid_L"][1] + 1
    assert LANES1 <= L < 124 and want("mid_L")[4] == L - 1


def test_zero_label_cases_put_label_zero_directly_under_the_path_in_the_second_phase():
    for n in NAMES:
        assert (case(n)[1] == 0).any() == (CASES[n][6] is not None), n
    assert {CASES[n][2] for n in NAMES if CASES[n][6] is not None and CASES[n][4] == 4} == {39, 64}
    for name in ("zero_label_V39", "zero_label_V64"):
        path, lab = want(name)[0], case(name)[1]
        hits = 0
        for t in range(CASES[name][0]):
            q = int(path[t])
            under = q - 1 if q % 2 == 0 else q - 2           # the label cell next below position q
            if t % CK >= SPLIT and under >= 1 and lab[under >> 1] == 0:
                hits += 1
        assert hits >= 3, (name, hits)


def test_banded_cases_have_both_band_edges_inside_the_one_cell_window():
    for name in ("banded_260_low", "banded_260_high", "banded_48", "banded_48_zero"):
        L = 2 * CASES[name][1] + 1
        assert CASES[name][3] < L
        low = high = 0
        for t0, n, p, wlo, w2 in chunks(name):
            for f in range(SPLIT, n):
                lo, hi = band(name, t0 + f)
                low += 0 < lo - w2 < LANES1
                high += 0 < hi - w2 < LANES1 and hi < L
        if name.startswith("banded_260"):    # 260 wide: one edge at a time
            assert (low if name.endswith("low") else high) >= 4, (name, low, high)
        else:
            assert low > 0 and high > 0, (name, low, high)
    assert {CASES[n][3] for n in NAMES if n.startswith("banded_")} == {48, 260}


def test_controls_are_the_other_max_moves():
    assert {CASES[n][4] for n in NAMES} == {2, 3, 4}


# ---- the kernels ----
@pytest.fixture(scope="module")
def env():
    import torch
    assert torch.cuda.is_available()
    import kokoro_align_amd as ka
    from kokoro_align_amd import _lib
    assert os.path.exists(ka.library_path()), "HIP library not built"
    eng = _lib.default_engine(torch.cuda.current_device())
    eng.set_mode("wave")
    eng.set_tile_width(0)
    yield ka, eng
    eng.set_mode("auto")
    eng.set_backtrace("auto")


def differs(got, total, name):
    path, labels, scores, wtotal, _ = want(name)
    for g, w, field in zip(got, (path, labels, scores), ("path", "labels", "scores")):
        g = np.asarray(g)
        if g.shape != w.shape:
            return f"{field} has shape {g.shape}"
        bad = np.nonzero(g.view(np.int32) != w.view(np.int32))[0]
        if bad.size:
            t = int(bad[0])
            return f"{field} differs at {bad.size} frames, first at frame {t} (frame {t % CK} of its chunk): got {g[t]}, want {w[t]}"
    if np.float32(total).view(np.int32) != np.float32(wtotal).view(np.int32):
        return f"total {total!r}, want {wtotal!r}"
    return None


@pytest.mark.gpu
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("name", NAMES)
def test_split_gives_the_oracle_s_path_labels_scores_and_total(env, name, form):
    ka, eng = env
    eng.set_backtrace(form)
    lp, lab = case(name)
    beam, mm = CASES[name][3:5]
    res, status, total = ka.ctc_best_path_batch([lp], [lab], beam, mm, return_status=True)
    assert list(status) == [0], (name, form, status)
    why = differs(res[0], total[0], name)
    assert why is None, f"{name} [{form}]: {why}"


@pytest.mark.gpu
@pytest.mark.parametrize("form", FORMS)
def test_split_in_one_launch_of_all_cases_of_a_kind(env, form):
    """All cases that share (V, beam, max_move) in one launch: lattices of both kernel instances and of every T side by side."""
    ka, eng = env
    eng.set_backtrace(form)
    groups = {}
    for n in NAMES:
        groups.setdefault((CASES[n][2], CASES[n][3], CASES[n][4]), []).append(n)
    for (V, beam, mm), names in groups.items():
        res, status, total = ka.ctc_best_path_batch([case(n)[0] for n in names], [case(n)[1] for n in names], beam, mm, return_status=True)
        assert list(status) == [0] * len(names), (names, status)
        for i, n in enumerate(names):
            why = differs(res[i], total[i], n)
            assert why is None, f"{n} [{form}] in a launch of {len(names)}: {why}"
