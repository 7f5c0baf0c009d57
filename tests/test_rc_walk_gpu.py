"""The walk of the recomputing backtrace (rc_walk_out, ka_wave_backtrace.hpp) at the shapes where it
can go wrong.  The walk keeps the code words and the label of the path's lane in scalar registers and reads them again only
when the lane changes, records moves as two bit masks from which lane f counts its position after the walk, and fetches the
labels once per 32-frame chunk; only the score is read per frame.  So the cases are about WHEN the path moves:

  fast      a move in every frame, a new lane in almost every frame (T = 40 and T = 33: a 1-frame last chunk)
  still     no move across whole chunks (S = 1, and S = 0: blank only)
  edges     short transcripts over T = 96, several seeds: together they move at frames 7, 8, 31, 32 and 33, i.e. on both
            sides of an 8-frame code word's end and of a chunk's end
  tail      T = 1, 31, 32, 33 (mod 32): partial last chunks, T = 1 and T = 31 a single partial chunk
  window    the window at the bottom (path within the first 96 positions) and the path ending on L - 1 with L < 124
  instance  a transcript with label 0, V = 39 and 64, max_move 2, 3, 4
  banded    a band narrower than L whose chunks are partly masked and partly open

Each case runs through the checkpointed one-wavefront form with the serial and with the chunk-parallel backtrace; path,
labels, scores and total are compared with the C oracle bit for bit.  The tests without the gpu mark assert from the oracle's
paths that the cases do what their names say; they need no GPU.
"""
import functools
import os

import numpy as np
import pytest

from oracle import oracle as O

CK = 32      # frames per chunk of the recomputing backtrace
EDGE_FRAMES = (7, 8, 31, 32, 33)

# name: (T, S, V, beam, max_move, seed, every k-th label renamed to 0 or None)
CASES = {
    "fast_T40": (40, 55, 39, 1000, 4, 1, None),
    "fast_T33": (33, 55, 39, 1000, 4, 2, None),
    "still_S1": (200, 1, 39, 1000, 4, 3, None),
    "still_S0": (200, 0, 39, 1000, 4, 4, None),
    "edges_a": (96, 14, 39, 1000, 4, 139, None),
    "edges_b": (96, 18, 39, 1000, 4, 131, None),
    "edges_c": (96, 18, 39, 1000, 4, 134, None),
    "edges_d": (96, 24, 39, 1000, 4, 110, None),
    "edges_e": (96, 24, 39, 1000, 4, 107, None),
    "edges_f": (96, 30, 39, 1000, 4, 103, None),
    "tail_T1": (1, 1, 39, 1000, 4, 21, None),
    "tail_T31": (31, 9, 39, 1000, 4, 22, None),
    "tail_T32": (32, 9, 39, 1000, 4, 23, None),
    "tail_T33": (33, 9, 39, 1000, 4, 24, None),
    "tail_T63": (63, 20, 64, 1000, 4, 25, None),
    "tail_T64": (64, 20, 64, 1000, 4, 26, None),
    "tail_T65": (65, 20, 64, 1000, 4, 27, None),
    "tail_T97": (97, 60, 39, 1000, 4, 28, None),
    "window_bottom": (120, 45, 39, 1000, 4, 31, None),
    "window_top": (100, 40, 39, 1000, 4, 32, None),
    "window_moving": (300, 150, 39, 1000, 4, 33, None),
    "zero_label_V39": (130, 70, 39, 1000, 4, 41, 3),
    "zero_label_V64": (130, 70, 64, 1000, 4, 42, 4),
    "V64": (130, 70, 64, 1000, 4, 43, None),
    "max_move_2": (161, 40, 39, 1000, 2, 44, None),
    "max_move_3": (161, 90, 39, 1000, 3, 45, None),
    "max_move_3_zero": (161, 90, 64, 1000, 3, 46, 5),
    "banded": (352, 300, 39, 260, 4, 51, None),
    "banded_narrow": (300, 150, 39, 48, 4, 52, None),
}
NAMES = tuple(CASES)
FORMS = ("serial", "parallel")


@functools.lru_cache(maxsize=None)
def case(name):
    """(log_probs, labels) of a case: the hash generators of the other GPU tests; shared and never written to."""
    T, S, V, beam, mm, seed, zero = CASES[name]
    lp = O.hash_logprobs(T, V, seed)
    lab = O.hash_labels(S, V, seed)
    if zero:
        lab = np.where(np.arange(S) % zero == 1, 0, lab).astype(np.int32)
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


def open_chunks(name):
    """Per full chunk above the first whether backtrace_rc_body recomputes it unmasked (`open`): the band does not cut into
    [wlo, p] at any of its frames."""
    T, S, V, beam, mm, _, _ = CASES[name]
    L = 2 * S + 1
    path = want(name)[0]
    out = []
    for t0 in range(CK, T - CK + 1, CK):
        p = int(path[t0 + CK - 1])
        wlo = max(p - 96, 0) & ~1
        dl_last = L * (t0 + CK - 1) // T - beam // 2
        lo1 = max(L * (t0 - 1) // T - beam // 2, 0)
        hi1 = L if L - lo1 < beam else lo1 + beam
        out.append(wlo > 0 and dl_last <= wlo and p < hi1)
    return out


# ---- the cases do what their names say (no GPU) ----
@pytest.mark.parametrize("name", ["fast_T40", "fast_T33"])
def test_fast_cases_move_in_every_frame_and_change_lane(name):
    path, mv = want(name)[0], moves(name)
    # T = 40: 110 positions in 40 frames leave room for a handful of smaller moves; T = 33: the path ends on the highest
    # position that 33 moves of 3 can reach at all
    assert np.mean(mv[1:] >= 1) >= (0.95 if name == "fast_T40" else 1.0), mv
    assert mv[1:].mean() > 2.5, mv[1:].mean()            # nearly 3 positions per frame
    assert np.mean(np.diff(path >> 1) != 0) >= 0.9


@pytest.mark.parametrize("name", ["still_S1", "still_S0"])
def test_still_cases_stay_across_whole_chunks(name):
    mv = moves(name)
    T = CASES[name][0]
    quiet = [c for c in range(T // CK) if not mv[max(c * CK, 1):(c + 1) * CK].any()]
    assert len(quiet) >= 3, quiet


def test_edge_cases_move_on_both_sides_of_a_code_word_s_and_a_chunk_s_end():
    names = [n for n in NAMES if n.startswith("edges_")]
    for t in EDGE_FRAMES:
        assert any(moves(n)[t] != 0 for n in names), f"no case moves at frame {t}"
    # the pairs themselves: a move at 7 and at 8, at 31 and at 32, at 32 and at 33 within one lattice
    for a, b in ((7, 8), (31, 32), (32, 33)):
        assert any(moves(n)[a] != 0 and moves(n)[b] != 0 for n in names), f"no case moves at frames {a} and {b}"


def test_tail_cases_cover_the_residues():
    assert {CASES[n][0] % CK for n in NAMES if n.startswith("tail_")} == {1, 31, 0}
    assert {1, 31} <= {CASES[n][0] for n in NAMES if n.startswith("tail_")}


def test_window_cases_sit_at_the_bottom_and_at_the_top():
    path = want("window_bottom")[0]
    assert path.max() < 96                                   # wlo == 0 in every chunk
    path, _, _, _, end = want("window_top")
    L = 2 * CASES["window_top"][1] + 1
    assert L < 124 and end == L - 1 and path[-1] == L - 1
    assert want("window_moving")[0].max() > 200              # wlo > 0 in most chunks


def test_banded_case_has_masked_chunks_next_to_open_ones():
    kinds = open_chunks("banded")
    assert any(kinds) and not all(kinds), kinds
    assert any(a != b for a, b in zip(kinds, kinds[1:])), kinds
    assert not any(open_chunks("banded_narrow"))
    assert CASES["banded"][3] < 2 * CASES["banded"][1] + 1 and CASES["banded_narrow"][3] < 2 * CASES["banded_narrow"][1] + 1


def test_zero_label_cases_contain_label_zero():
    for n in ("zero_label_V39", "zero_label_V64", "max_move_3_zero"):
        assert (case(n)[1] == 0).any()
    for n in NAMES:
        if CASES[n][6] is None:
            assert not (case(n)[1] == 0).any()


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
def test_walk_gives_the_oracle_s_path_labels_scores_and_total(env, name, form):
    ka, eng = env
    eng.set_backtrace(form)
    lp, lab = case(name)
    _, _, _, beam, mm, _, _ = CASES[name]
    res, status, total = ka.ctc_best_path_batch([lp], [lab], beam, mm, return_status=True)
    assert list(status) == [0], (name, form, status)
    why = differs(res[0], total[0], name)
    assert why is None, f"{name} [{form}]: {why}"


@pytest.mark.gpu
@pytest.mark.parametrize("form", FORMS)
def test_walk_in_one_launch_of_all_cases_of_a_kind(env, form):
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
