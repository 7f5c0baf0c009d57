"""The keyed frames of the recomputing backtrace (rc_frame4_keyed / rc_frame1_keyed, ka_wave_backtrace.hpp; DESIGN.md
section 4.2) and their routing, at the smallest shapes at which they can go wrong.

A lattice whose log-probs all have the sign bit set is flagged by the checkpointed forward kernel (bit 3 of the flag word,
read back with ka_debug_meta_flags) and walked by backtrace_rc_kernel<4, false, false, true>, which takes every cell's maximum
and first arg-max from 64-bit minima; every other lattice keeps the compare form.  Outputs are compared with the C oracle bit
for bit, serial backtrace.

  ties      T = 70, S = 40, unbanded: two full chunks and one of 6 frames; log-probs quantised to multiples of 0.25, so that
            most cells have tied candidates - the path itself passes through tied cells in both phases of a chunk
  plain     the same lattice with one element +0.0, and with one element positive (first row, middle, last row - the last
            row lies in the partial row block of the V = 64 forward pass): the flag is clear, the result is the oracle's
  veto      the path crosses cells with one, two and three -inf candidates
  mixed     all-negative, not-all-negative and label-0 lattices in one launch
  drop      the steep and tail recipes of test_rc_split_gpu.py (80 and more positions inside one chunk, both sides of the split;
            last chunks of 15, 16 and 17 frames)

The tests without the gpu mark assert from a NumPy DP (checked against the oracle's path) that the cases do what their names
say; they need no GPU.
"""
import functools
import os

import numpy as np
import pytest

import test_rc_split_gpu as R
from oracle import oracle as O

CK, SPLIT = R.CK, R.SPLIT
FLAG_ZERO_LABEL, FLAG_ALL_NEG = 1, 8
T, S, BEAM, MM = 70, 40, 1000, 4
SEED = 27      # a seed whose path has three tied cells in each phase and cells with 1, 2 and 3 absent candidates, V = 39 and 64
NINF = np.float32(-np.inf)
SPOTS = ("first", "middle", "last")


@functools.lru_cache(maxsize=None)
def tied(V, spoil=None, spot=None, zero_label=False):
    """(log_probs, labels): hash log-probs rounded to multiples of 0.25, zero as -0.0; `spoil`: one element +0.0 or +0.5."""
    lp = -np.abs(np.round(O.hash_logprobs(T, V, SEED) * np.float32(4.0)) / np.float32(4.0)).astype(np.float32)
    assert np.signbit(lp).all()
    lab = O.hash_labels(S, V, SEED)
    if zero_label:
        lab = np.where(np.arange(S) % 3 == 1, 0, lab).astype(np.int32)
    if spoil is not None:
        t, c = {"first": (0, 0), "middle": (35, 5), "last": (T - 1, V - 1)}[spot]
        lp[t, c] = np.float32(0.0) if spoil == "zero" else np.float32(0.5)
    lp.setflags(write=False)
    lab.setflags(write=False)
    return lp, lab


@functools.lru_cache(maxsize=None)
def want(V, spoil=None, spot=None, zero_label=False):
    lp, lab = tied(V, spoil, spot, zero_label)
    return O.ctc_best_path_c(lp, lab, BEAM, MM, return_total=True)


@functools.lru_cache(maxsize=None)
def path_cells(V):
    """Per frame the four candidate sums (float32, -inf where absent or vetoed) of the cell the oracle's path is on, by a plain
    NumPy DP of the unbanded lattice whose back-trace is checked against the oracle's path."""
    lp, lab = tied(V)
    L = 2 * S + 1
    pos = np.arange(L)
    col = np.where(pos % 2 == 1, lab[np.minimum(pos >> 1, S - 1)], 0)
    veto = (pos % 2 == 0) | (col == 0)
    alpha = np.full(L + 3, NINF, np.float32)       # three absent positions below 0
    alpha[3] = np.float32(0.0)                     # the virtual state before frame 0 (align.py:57-58)
    cands, moves = [], []
    for t in range(T):
        e = lp[t, col]
        c = np.stack([alpha[3:] + e, alpha[2:-1] + e, np.where(veto, NINF, alpha[1:-2] + e), alpha[:-3] + e])
        cands.append(c)
        moves.append(c.argmax(axis=0))
        alpha = np.concatenate([np.full(3, NINF, np.float32), c.max(axis=0)])
    path = want(V)[0]
    q = int(path[-1])
    out = []
    for t in range(T - 1, -1, -1):
        assert q == path[t], (t, q, path[t])
        out.append(cands[t][:, q])
        q -= int(moves[t][q])
    assert q == 0
    return out[::-1]


# ---- the cases do what their names say (no GPU) ----
@pytest.mark.parametrize("V", [39, 64])
def test_the_path_takes_tied_cells_in_both_phases(V):
    cells = path_cells(V)
    first, second = [], []
    for t, c in enumerate(cells):
        m = c.max()
        if m > NINF and (c == m).sum() >= 2:
            (first if t % CK < SPLIT else second).append(t)
    assert len(first) >= 3 and len(second) >= 3, (first, second)
    # and a tie in which the first maximum is not candidate 0: the order of the candidates matters
    assert any(int(np.argmax(cells[t])) > 0 for t in first + second)
    # both full chunks and the 6-frame one
    assert T % CK == 6 and {t // CK for t in first + second} >= {0, 1}


@pytest.mark.parametrize("V", [39, 64])
def test_the_path_crosses_cells_with_one_two_and_three_absent_candidates(V):
    counts = {int((c == NINF).sum()) for c in path_cells(V)}
    assert counts >= {1, 2, 3}, counts


def test_spoilt_lattices_are_not_all_negative():
    for spoil in ("zero", "positive"):
        for spot in SPOTS:
            lp = tied(64, spoil, spot)[0]
            assert (~np.signbit(lp)).sum() == 1


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
    eng.set_backtrace("serial")
    yield ka, eng
    eng.set_mode("auto")
    eng.set_backtrace("auto")


def flags_of(eng, n):
    out = np.full(n, -1, np.int32)
    assert eng.lib.ka_debug_meta_flags(eng.handle, out.ctypes.data, n) == n
    return out


def differs(got, total, ref):
    path, labels, scores, wtotal, _ = ref
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
@pytest.mark.parametrize("V", [39, 64])
def test_tied_lattice_takes_the_keyed_frames_and_gives_the_oracle_s_result(env, V):
    ka, eng = env
    lp, lab = tied(V)
    res, status, total = ka.ctc_best_path_batch([lp], [lab], BEAM, MM, return_status=True)
    assert list(status) == [0]
    assert flags_of(eng, 1)[0] == FLAG_ALL_NEG
    why = differs(res[0], total[0], want(V))
    assert why is None, why


@pytest.mark.gpu
@pytest.mark.parametrize("spot", SPOTS)
@pytest.mark.parametrize("spoil", ["zero", "positive"])
@pytest.mark.parametrize("V", [39, 64])
def test_one_element_that_is_not_negative_sends_the_lattice_to_the_plain_frames(env, V, spoil, spot):
    ka, eng = env
    lp, lab = tied(V, spoil, spot)
    res, status, total = ka.ctc_best_path_batch([lp], [lab], BEAM, MM, return_status=True)
    assert list(status) == [0]
    assert flags_of(eng, 1)[0] == 0
    why = differs(res[0], total[0], want(V, spoil, spot))
    assert why is None, why


@pytest.mark.gpu
@pytest.mark.parametrize("V", [39, 64])
def test_mixed_launch(env, V):
    """All-negative, not-all-negative and label-0 lattices side by side: three kernel instances share the launch."""
    ka, eng = env
    keys = [(V,), (V, "zero", "middle"), (V, None, None, True), (V, "positive", "last"), (V,), (V, "positive", "first", True)]
    res, status, total = ka.ctc_best_path_batch([tied(*k)[0] for k in keys], [tied(*k)[1] for k in keys], BEAM, MM, return_status=True)
    assert list(status) == [0] * len(keys)
    assert list(flags_of(eng, len(keys))) == [FLAG_ALL_NEG, 0, FLAG_ALL_NEG | FLAG_ZERO_LABEL, 0, FLAG_ALL_NEG, FLAG_ZERO_LABEL]
    for i, k in enumerate(keys):
        why = differs(res[i], total[i], want(*k))
        assert why is None, f"lattice {i} {k}: {why}"


DROP = ("steep_T64_S81", "steep_T64_S95", "steep_T96_S121", "steep_T96_S140", "tail_T15", "tail_T16", "tail_T17", "tail_T47", "tail_T48",
        "tail_T49", "banded_48")


def test_drop_cases_are_all_negative_and_cover_the_partial_chunks():
    for name in DROP:
        assert np.signbit(R.case(name)[0]).all() and not (R.case(name)[1] == 0).any(), name
    assert {R.CASES[n][0] % CK for n in DROP if n.startswith("tail_")} == {SPLIT - 1, SPLIT, SPLIT + 1}


@pytest.mark.gpu
@pytest.mark.parametrize("name", DROP)
def test_drop_and_partial_chunk_on_the_keyed_frames(env, name):
    ka, eng = env
    lp, lab = R.case(name)
    beam, mm = R.CASES[name][3:5]
    res, status, total = ka.ctc_best_path_batch([lp], [lab], beam, mm, return_status=True)
    assert list(status) == [0]
    assert flags_of(eng, 1)[0] == FLAG_ALL_NEG
    why = R.differs(res[0], total[0], name)
    assert why is None, f"{name}: {why}"
