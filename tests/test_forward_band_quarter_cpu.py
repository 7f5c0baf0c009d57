"""A NumPy model of forward_ck's score ring with its mask schedule (max_move = 4; ka_wave_forward.hpp),
checked against a plain banded DP.  No GPU.

The ring has 1024 slots, position p in cell p & 15 of lane (p >> 4) & 63.  Every frame computes all sixteen cells of every lane
from the lane's own cells and three halos (cells 13..15 of the lane below, taken at the end of the frame before); the band mask
is applied only (i) in the frame in front of a band step, all sixteen cells; (ii) in the first frame of a new band: where lo
went ONE further, only the quarter of the cells that holds the position that left, lo_old & 15 - anything else all sixteen;
(iii) periodically, every 8th or 4th frame, or on checkpoint frames only where the steps alone bound the distance between two
full masks (steps_mask); and once behind the last frame.  A step that leaves lo where it was (clamped at 0) leaves the whole
band where it was - hi is a function of lo - and owes no pass (ii).

Cells at or above hi pick up leaked scores between two full masks, three positions further per frame.  The model puts ANYTHING
there instead, -inf .. 1e30 drawn afresh in every frame, over the whole stretch a leak can have reached since the last full mask.
The claim: every in-band cell of every frame equals the plain DP's bit for bit, the ring is clean on checkpoint frames and at
the end, whatever was put there.  A quarter chosen one off, or a last quarter that leaves the halos as they were, must fail the
same check: the cases have teeth.
"""
import functools

import numpy as np
import pytest

RING, LANES, CELLS, M, CK = 1024, 64, 16, 4, 32
NINF = np.float32(-np.inf)
JUNK = np.array([-np.inf, -1e30, -50.0, 0.0, 1e30], dtype=np.float32)
HOT = np.array([1e30], dtype=np.float32)

# (T, S, V, beam): lo leaves 0 after beam/2 * T/L frames
CASES = {
    "every_5th": (1000, 100, 64, 40),         # L = 201: a step every 4.98 frames, lo & 15 through all sixteen values six times
    "every_2nd": (400, 100, 39, 24),
    "every_frame": (201, 100, 64, 24),        # dq = 1: every frame steps, every mask is a full one
    "two_per_frame": (150, 150, 39, 30),      # dq = 2: lo moves by two
    "relabel_5th": (6007, 600, 64, 1000),     # L = 1201 > 1024: lanes are re-labelled (lo & 15: 15 -> 0), cfg2's rhythm
    "relabel_fast": (1300, 600, 64, 1000),    # 0.92 positions per frame
    "narrow_gap": (3000, 600, 39, 1006),      # 18 dead slots: period 4
    "slow": (2000, 60, 39, 30),               # a step every 16.5 frames: no steps_mask, the periodic pass every 8th frame
    "hi_at_L": (500, 40, 64, 30),             # the last 15 positions of lo's way: hi stays at L
    "zero_label": (1000, 100, 64, 40),
    "blank_heavy": (1000, 100, 64, 40),       # blanks cheap, labels dear: the best scores sit at the lo edge, where a stale cell wins
}


def _ends_behind_a_step(S, beam, around):
    """The T nearest `around` whose last frame is the first of a new band."""
    L = 2 * S + 1
    for T in sorted(range(around - 20, around + 21), key=lambda x: abs(x - around)):
        lo = [max(0, L * t // T - beam // 2) for t in (T - 2, T - 1)]
        if lo[1] == lo[0] + 1:
            return T
    raise AssertionError("no such T")


CASES["ends_behind_step"] = (_ends_behind_a_step(100, 40, 300), 100, 64, 40)


@functools.lru_cache(maxsize=None)
def lattice(name):
    T, S, V, beam = CASES[name]
    rng = np.random.RandomState(sum(map(ord, name)))
    weight = np.ones(V)
    if name == "blank_heavy":
        weight[0] = 20.0 * V
    lp = np.log(rng.dirichlet(weight, size=T)).astype(np.float32)
    lab = rng.randint(1, V, size=S)
    if name == "zero_label":
        lab[1::3] = 0
    L = 2 * S + 1
    ext = np.zeros(L + 2 * RING, np.int64)        # positions past L - 1: the zero padding of the label buffer
    ext[1:L:2] = lab
    t = np.arange(T, dtype=np.int64)
    lo = np.maximum(0, L * t // T - beam // 2)
    hi = np.minimum(lo + beam, L)
    for a in (lp, ext, lo, hi):
        a.setflags(write=False)
    return T, L, beam, lp, ext, lo, hi


@functools.lru_cache(maxsize=None)
def plain_dp(name):
    """alpha[t]: scores after frame t over all positions, -inf outside the band (align.py:64-99)."""
    T, L, beam, lp, ext, lo, hi = lattice(name)
    veto = ext[:L] == 0
    alpha = np.full((T, L), NINF, np.float32)
    prev = np.full(L + 3, NINF, np.float32)
    prev[3] = 0.0
    for t in range(T):
        e = lp[t, ext[:L]]
        c = np.maximum(np.maximum(prev[3:], prev[2:-1]), np.maximum(np.where(veto, NINF, prev[1:-2]), prev[:-3])) + e
        a, b = int(lo[t]), int(hi[t])
        alpha[t, a:b] = c[a:b]
        prev[3:] = alpha[t]
    alpha.setflags(write=False)
    return alpha


def ring_model(name, junk, seed, quarter_off=0, halos="always"):
    """The ring as the kernel runs it.  -> None where every check holds, else (frame, what).
    halos: when a visit of the rare block takes the halos again - "always" (the kernel), "last_quarter" (only where cells 12..15
    were masked: all that is needed), "full_only" (the fault: a last quarter alone leaves them)."""
    T, L, beam, lp, ext, lo_ref, hi_ref = lattice(name)
    alpha = plain_dp(name)
    rng = np.random.RandomState(seed)
    dq, dr = L // T, L % T
    thr_real = 0 if dq else T
    width = min(beam, L)
    p_static = 8 if RING - width >= 8 * (M - 1) else 4
    steps_mask = dq != 0 or (p_static - 1) * dr >= T
    mask_bits = (CK - 1) & ~3 if steps_mask else (p_static - 1) & ~3
    cell = np.arange(CELLS)
    P = np.full((LANES, CELLS), NINF, np.float32)
    P[0, 0] = 0.0
    H = np.full((LANES, 3), NINF, np.float32)     # cells 13, 14, 15 of the lane below
    blk = np.arange(LANES)
    blo, q, rem, lo, hi = 0, 0, 0, 0, width
    thr, quarter = thr_real, 15
    since_full = 0                                # frames computed since the last full mask

    def inside():
        pos = blk[:, None] * CELLS + cell
        return pos, (pos >= lo) & (pos < hi)

    def take_halos():
        H[:] = np.roll(P[:, 13:], 1, axis=0)

    for t in range(T):
        assert (lo, hi) == (int(lo_ref[t]), int(hi_ref[t]))
        pos, band = inside()
        e = lp[t, ext[pos]]
        X = np.concatenate([H, P], axis=1)
        veto = ext[pos] == 0
        P = np.maximum(np.maximum(X[:, 3:], X[:, 2:-1]), np.maximum(np.where(veto, NINF, X[:, 1:-2]), X[:, :-3])) + e
        since_full += 1
        # anything where a leak can be: the positions from hi up that (M - 1) cells per frame have reached since the last full mask
        leak = (pos >= hi) & (pos < hi + (M - 1) * since_full)
        P[leak] = rng.choice(junk, int(leak.sum()))
        got, want = P[band], alpha[t, pos[band]]
        if not np.array_equal(got.view(np.int32), want.view(np.int32)):
            return t, "an in-band cell differs"
        static = t % 4 == 3 and (~(t - 3) & mask_bits) == 0
        if static:
            P[~band] = NINF
            since_full = 0
            if t % CK == CK - 1 and not np.all(P[~band] == NINF):
                return t, "checkpoint row not clean"
        take_halos()
        rem += dr
        if rem >= thr:
            thr = thr_real
            sel = 15 if rem >= thr_real else quarter
            if static:
                sel = 0
            for g in range(4):
                if sel >> g & 1:
                    part = ~band & ((cell >> 2) == g)
                    P[part] = NINF
            if sel == 15:
                since_full = 0
            if halos == "always" or (halos == "last_quarter" and sel & 8) or (halos == "full_only" and sel == 15):
                take_halos()
            if rem >= thr_real:
                q += dq
                if rem >= T:
                    rem -= T
                    q += 1
                if t + 1 != T:
                    nlo = max(q - beam // 2, 0)
                    nhi = L if L - nlo < beam else nlo + beam
                    if nlo >> 4 != blo:
                        blo = nlo >> 4
                        nb = blo + ((np.arange(LANES) - blo) & 63)
                        reset = nb != blk
                        blk = nb
                        H[reset & np.roll(reset, 1)] = NINF
                        P[reset] = NINF
                    if nlo != lo:
                        quarter = 1 << (((lo >> 2) + quarter_off) & 3) if nlo - lo == 1 else 15
                        lo, hi = nlo, nhi
                        thr = 0
                    else:
                        assert nhi == hi          # hi is a function of lo
    pos, band = inside()
    P[~band] = NINF
    if not np.array_equal(P[band].view(np.int32), alpha[T - 1, pos[band]].view(np.int32)):
        return T, "the last row differs"
    return None


def situations(name):
    """What the case's band does, from the band arithmetic alone."""
    T, L, beam, lp, ext, lo, hi = lattice(name)
    step = np.nonzero(lo[1:] != lo[:-1])[0]                       # frames t after which lo moves
    by = lo[step + 1] - lo[step]
    dq, dr = L // T, L % T
    width = min(beam, L)
    p_static = 8 if RING - width >= 8 * (M - 1) else 4
    return dict(step=step, by=by, left=lo[step] & 15, steps_mask=dq != 0 or (p_static - 1) * dr >= T, p_static=p_static,
                q_moves=np.nonzero((L * np.arange(1, T) // T) != (L * np.arange(T - 1) // T))[0], lo=lo, hi=hi, L=L, T=T)


def test_the_cases_are_what_their_names_say():
    s = situations("every_5th")
    assert s["steps_mask"] and set(s["by"]) == {1} and set(s["left"]) == set(range(16)) and 4 <= np.diff(s["step"]).min() and np.diff(s["step"]).max() == 5
    # lo stays at 0 while floor(L t / T) already moves: those steps change nothing, hi included
    early = s["q_moves"][s["q_moves"] < s["step"][0]]
    assert early.size >= 10 and not s["lo"][early + 1].any() and np.all(s["hi"][early + 1] == s["hi"][0])
    s = situations("every_2nd")
    assert s["steps_mask"] and set(s["by"]) == {1} and set(s["left"]) == set(range(16)) and set(np.diff(s["step"])) == {1, 2}
    s = situations("every_frame")
    assert set(s["by"]) == {1} and set(np.diff(s["step"])) == {1} and set(s["left"]) == set(range(16))
    assert set(situations("two_per_frame")["by"]) >= {2}
    for name in ("relabel_5th", "relabel_fast"):
        s = situations(name)
        assert s["L"] > RING and np.any((s["left"] == 15) & (s["by"] == 1)) and s["steps_mask"]
    assert 5 in np.diff(situations("relabel_5th")["step"])
    s = situations("narrow_gap")
    assert s["p_static"] == 4 and s["steps_mask"] and s["L"] > RING
    s = situations("slow")
    assert not s["steps_mask"] and s["p_static"] == 8 and set(s["by"]) == {1} and np.diff(s["step"]).min() > 8
    s = situations("hi_at_L")
    late = s["step"][s["hi"][s["step"]] == s["L"]]
    assert late.size >= 10 and np.all(s["hi"][late + 1] == s["L"]) and set(s["by"]) == {1}
    # a pass (ii) frame that is a checkpoint frame, one that is the last frame, one in front of every residue of t mod 8
    s = situations("every_5th")
    assert np.any((s["step"] + 1) % CK == CK - 1) and {int(x) for x in (s["step"] + 1) % 8} == set(range(8))
    assert lattice("zero_label")[4][1::2][:100].min() == 0


@pytest.mark.parametrize("name", sorted(CASES))
@pytest.mark.parametrize("halos", ["always", "last_quarter"])
def test_the_ring_equals_the_plain_dp_whatever_lies_above_hi(name, halos):
    for seed, junk in ((1, JUNK), (2, HOT), (3, JUNK[:1])):
        assert ring_model(name, junk, seed, halos=halos) is None, (name, seed)


def test_the_last_frame_right_behind_a_step():
    """Frame T - 1 is the first of a new band: its pass (ii) and the mask behind the loop fall together."""
    s = situations("ends_behind_step")
    assert s["step"][-1] + 1 == s["T"] - 1 and s["by"][-1] == 1
    assert ring_model("ends_behind_step", JUNK, 5) is None


def test_a_quarter_one_off_fails():
    wrong = [ring_model(name, JUNK[:1], 7, quarter_off=1) for name in ("every_5th", "every_2nd", "relabel_5th", "hi_at_L", "blank_heavy")]
    assert all(w is not None for w in wrong), wrong


def test_a_last_quarter_that_leaves_the_halos_fails():
    assert ring_model("blank_heavy", JUNK[:1], 8, halos="full_only") is not None
    # ... and it is the last quarter that it takes: with the halos taken there, the same lattices pass (the test above)
