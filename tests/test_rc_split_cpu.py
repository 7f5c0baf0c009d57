"""A NumPy model of the two-phase recompute of backtrace_rc_body (max_move = 4; ka_wave_backtrace.hpp),
checked against a plain full DP.  No GPU.

A chunk of 32 frames is entered at position p (the path's position at its last frame).  Frames 0 .. SPLIT-1 are recomputed from
the checkpoint on the window [wlo, wlo+123], wlo = max(p-96, 0) & ~1; frames SPLIT .. 31 on the window [w2, w2+LANES1-1],
w2 = (p-BACK) & ~1 (0 while p <= BACK), which takes its first scores from the first window.  What lies below a window is not
known to the kernel: the model puts ANYTHING there, drawn afresh in every frame from -inf .. 1e30 (below position 0 there is
nothing: -inf).  The walk decodes frames 31 .. SPLIT in the second window and the others in the first.  The claim is that the
path of the chunk and the position at which the chunk below is entered are those of the full DP, whatever was put below the
windows - for the shipped constants, on paths that drop 80 and more positions inside the chunk, which is where the walk comes
nearest to the cells that the unknown ones have spoilt.  A window that starts too high, or a split that comes too early, must
fail the same check: the model has teeth.
"""
import functools
import os
import re

import numpy as np
import pytest

CK = 32
SPLIT = 16      # kRcSplit
BACK = 59       # kRc1Back
LANES1 = 61     # kRc1Lanes
WIDTH = 124     # 2 * kRcLanes: cells of the first window
NINF = np.float32(-np.inf)
JUNK = np.array([-np.inf, -1e30, -50.0, 0.0, 1e30], dtype=np.float32)
HOT = np.array([1e30], dtype=np.float32)

# (T, S, V, seed): L = 2S+1 is just under 3T, so the path has to fall nearly 3 positions per frame all the way
LATTICES = [(96, 125, 39, s) for s in range(6)] + [(96, 140, 64, s) for s in range(6)] + [(64, 90, 39, s) for s in range(3)]


def test_constants_are_the_header_s():
    src = open(os.path.join(os.path.dirname(__file__), "..", "kokoro-align_amd", "csrc", "ka_wave_backtrace.hpp")).read()
    for name, value in (("kRcSplit", SPLIT), ("kRc1Back", BACK), ("kRc1Lanes", LANES1), ("kRcLanes", WIDTH // 2)):
        m = re.search(r"constexpr int %s = (\d+);" % name, src)
        assert m and int(m.group(1)) == value, name


def frame(prev_ext, e, veto):
    """One frame on a window.  prev_ext: last frame's scores of the 3 positions below the window, then of the window.
    -> (scores, moves): float32 sums as the kernels form them, the FIRST best move (np.argmax, align.py:83)."""
    c = np.stack([prev_ext[3:] + e, prev_ext[2:-1] + e, np.where(veto, NINF, prev_ext[1:-2] + e), prev_ext[:-3] + e])
    return c.max(axis=0), c.argmax(axis=0)


@functools.lru_cache(maxsize=None)
def lattice(T, S, V, seed):
    """(emissions [T, L+WIDTH], veto [L+WIDTH], alpha [T+1, L+WIDTH] with alpha[t+1] = scores after frame t, moves [T, L+WIDTH],
    path [T]) of a seeded lattice, by the plain full DP.  Positions past L-1 are padding that no path enters."""
    rng = np.random.RandomState(1000 * S + seed)
    lp = np.log(rng.dirichlet(np.ones(V), size=T)).astype(np.float32)
    lab = rng.randint(1, V, size=S)
    if seed % 2:
        lab[1::3] = 0                                      # label 0: its move 2 is vetoed as a blank's is
    L, W = 2 * S + 1, 2 * S + 1 + WIDTH
    pos = np.arange(W)
    col = np.where((pos % 2 == 1) & (pos < L), lab[np.minimum(pos >> 1, S - 1)], 0)
    em = lp[:, col]
    veto = (pos % 2 == 0) | (col == 0)
    alpha = np.full((T + 1, W), NINF, dtype=np.float32)
    alpha[0, 0] = 0.0                                      # the virtual state before frame 0 (align.py:57-58)
    mv = np.zeros((T, W), dtype=np.int64)
    for t in range(T):
        alpha[t + 1], mv[t] = frame(np.concatenate([np.full(3, NINF, np.float32), alpha[t]]), em[t], veto)
        alpha[t + 1, L:] = NINF
    q = L - 1 if alpha[T, L - 1] >= alpha[T, L - 2] else L - 2
    path = np.zeros(T, dtype=np.int64)
    for t in range(T - 1, -1, -1):
        path[t] = q
        q -= mv[t, q]
    assert q == 0
    for a in (em, veto, alpha, mv, path):
        a.setflags(write=False)
    return em, veto, alpha, mv, path


def two_phase(lat, t0, split, back, lanes1, junk, rng):
    """The chunk [t0, t0+32) as backtrace_rc_body recomputes and walks it -> (path of the chunk, entry position of the chunk
    below), or None where the walk leaves the second window."""
    em, veto, alpha, _, path = lat
    p = int(path[t0 + CK - 1])
    wlo = max(p - 96, 0) & ~1
    w2 = (p - back) & ~1 if p > back else 0

    def below(lo):
        return np.full(3, NINF, np.float32) if lo == 0 else rng.choice(junk, 3)

    s = alpha[t0, wlo:wlo + WIDTH].copy()
    mv1 = np.zeros((split, WIDTH), dtype=np.int64)
    for f in range(split):
        s, mv1[f] = frame(np.concatenate([below(wlo), s]), em[t0 + f, wlo:wlo + WIDTH], veto[wlo:wlo + WIDTH])
    s = s[w2 - wlo:w2 - wlo + lanes1]                      # the relayout
    mv2 = np.zeros((CK, lanes1), dtype=np.int64)
    for f in range(split, CK):
        s, mv2[f] = frame(np.concatenate([below(w2), s]), em[t0 + f, w2:w2 + lanes1], veto[w2:w2 + lanes1])
    q = p
    out = np.zeros(CK, dtype=np.int64)
    for f in range(CK - 1, -1, -1):
        out[f] = q
        if f >= split:
            if not 0 <= q - w2 < lanes1:
                return None
            q -= mv2[f, q - w2]
        else:
            if not 0 <= q - wlo < WIDTH:
                return None
            q -= mv1[f, q - wlo]
    return out, q


def steep_chunks():
    """(lattice, t0) of every full chunk in which the path drops at least 80 positions."""
    out = []
    for key in LATTICES:
        path = lattice(*key)[4]
        for t0 in range(0, key[0], CK):
            if int(path[t0 + CK - 1]) - (int(path[t0 - 1]) if t0 else 0) >= 80:
                out.append((key, t0))
    return out


def agrees(key, t0, split, back, lanes1, junk, seed):
    lat = lattice(*key)
    got = two_phase(lat, t0, split, back, lanes1, junk, np.random.RandomState(seed))
    want_entry = int(lat[4][t0 - 1]) if t0 else 0
    return got is not None and np.array_equal(got[0], lat[4][t0:t0 + CK]) and got[1] == want_entry


def test_there_are_enough_steep_chunks_of_every_kind():
    chunks = steep_chunks()
    assert len({key for key, _ in chunks}) >= 10, len(chunks)
    ps = [int(lattice(*key)[4][t0 + CK - 1]) for key, t0 in chunks]
    assert sum(p > 96 for p in ps) >= 10                      # both windows have unknown cells below them
    assert any(BACK < p <= 96 for p in ps)                    # only the second has
    assert {int(lattice(*key)[4][t0 + CK - 1]) % 2 for key, t0 in chunks} == {0, 1}   # p - w2 = 59 and 60
    assert any(lattice(*key)[1][1:2 * key[1]:2].any() for key, _ in chunks)           # label 0 among them


@pytest.mark.parametrize("split", sorted({13, SPLIT}))
def test_two_phases_give_the_full_dp_s_path_and_entry(split):
    """The shipped window with the shipped split, and with the earliest split the proof allows."""
    for key, t0 in steep_chunks():
        for seed, junk in ((1, JUNK), (2, HOT), (3, JUNK[:1])):
            assert agrees(key, t0, split, BACK, LANES1, junk, seed), (key, t0, split, junk)


def test_every_chunk_of_every_lattice_agrees_with_the_shipped_constants():
    for key in LATTICES:
        for t0 in range(0, key[0], CK):
            assert agrees(key, t0, SPLIT, BACK, LANES1, JUNK, 4), (key, t0)


def test_an_undersized_window_fails():
    """A second window that starts 40 instead of 60 positions below p (its unknown cells reach the path before the chunk's
    last frame), and a split at frame 6 (13 is the earliest the proof allows): the same check must not pass."""
    chunks = [(key, t0) for key, t0 in steep_chunks() if int(lattice(*key)[4][t0 + CK - 1]) > 96]
    narrow = [agrees(key, t0, SPLIT, 39, 41, HOT, 5) for key, t0 in chunks]
    early = [agrees(key, t0, 6, BACK, LANES1, HOT, 6) for key, t0 in chunks]
    assert not any(narrow), narrow
    assert not any(early), early
    # and one frame before the earliest split that the proof allows, some chunk already goes wrong
    assert not all(agrees(key, t0, 12, BACK, LANES1, HOT, 7) for key, t0 in chunks)
