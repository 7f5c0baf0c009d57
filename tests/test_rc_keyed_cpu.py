"""A NumPy model of the keyed cell of the recomputing backtrace (rc_frame4_keyed / rc_frame1_keyed, ka_wave_backtrace.hpp;
DESIGN.md section 4.2), run on the CPU.

The kernel takes a cell's maximum and its first index from one 64-bit minimum per candidate: candidate j is the register pair
(high word |s_j| as f32 bits, low word j), read as a double, and v_min_f64 over the pairs returns the pair of the largest sum
and, among equal sums, of the smallest j.  That is exact while every sum is -0.0 or below, or -inf.  The model builds the
doubles from the bits exactly as the registers hold them and takes np.minimum; the reference is np.argmax over the float32 sums
(align.py:83 takes the first maximum).

A label cell has the four candidates of max_move 4, a blank cell the candidates of moves 0, 1 and 3 (move 2 would skip from
blank to blank: vetoed); an absent or vetoed candidate is -inf, as in the kernel.
"""
import itertools

import numpy as np
import pytest

NINF = np.float32(-np.inf)
NZERO = np.float32(-0.0)
TINY = np.frombuffer(np.uint32(0x80000001).tobytes(), np.float32)[0]      # the smallest negative f32 denormal
DENORM = np.frombuffer(np.uint32(0x807FFFFF).tobytes(), np.float32)[0]    # the largest negative f32 denormal
HUGE = np.float32(-np.finfo(np.float32).max)                              # the largest finite magnitude
MOVES = {"label": (0, 1, 2, 3), "blank": (0, 1, 3)}


def keyed(sums, moves):
    """(bits of the maximum, move) as the keyed cell finds them: the minimum of the doubles (|s_j| bits << 32 | j)."""
    s = np.asarray(sums, np.float32)
    key_hi = s.view(np.uint32).astype(np.uint64) & np.uint64(0x7FFFFFFF)          # the abs modifier clears bit 63 of the pair
    pairs = (key_hi << np.uint64(32)) | np.asarray(moves, np.uint64)
    d = pairs.view(np.float64)
    assert np.isfinite(d).all()                                                  # f32 exponent 0xFF is f64 exponent 0x7F8
    best = d[0]
    for x in d[1:]:                                                              # the chain of v_min_f64
        best = np.minimum(best, x)
    bits = int(np.float64(best).view(np.uint64))
    return np.uint32(bits >> 32) | np.uint32(0x80000000), bits & 0xFFFFFFFF       # the score is kept as |s|: its sign is known


def reference(sums, moves):
    s = np.asarray(sums, np.float32)
    j = int(np.argmax(s))
    return s[j].view(np.uint32), moves[j]


def check(sums, kind):
    moves = MOVES[kind]
    got, want = keyed(sums, moves), reference(sums, moves)
    assert (int(got[0]), got[1]) == (int(want[0]), want[1]), (kind, [float(x) for x in sums], got, want)


@pytest.mark.parametrize("kind", ["label", "blank"])
def test_random_negative_sums(kind):
    rng = np.random.default_rng(20240 + len(kind))
    n = len(MOVES[kind])
    for _ in range(4000):
        s = -np.exp(rng.uniform(-100.0, 80.0, n)).astype(np.float32)            # from denormals to 1e34
        s[rng.random(n) < 0.15] = NINF
        if rng.random() < 0.3:                                                   # a tie between two random positions
            a, b = rng.integers(0, n, 2)
            s[a] = s[b]
        check(s, kind)


@pytest.mark.parametrize("kind", ["label", "blank"])
def test_equal_sums_in_every_subset_of_positions(kind):
    n = len(MOVES[kind])
    for r in range(2, n + 1):
        for subset in itertools.combinations(range(n), r):
            for tied, other in ((-3.25, -7.5), (-3.25, -1.0), (float(NZERO), -1.0), (float(DENORM), -2.0), (float(HUGE), -np.inf)):
                s = np.full(n, other, np.float32)
                s[list(subset)] = tied
                check(s, kind)


@pytest.mark.parametrize("kind", ["label", "blank"])
def test_minus_infinity_in_every_subset_and_everywhere(kind):
    n = len(MOVES[kind])
    base = np.array([-4.0, -2.5, -2.5, -9.0], np.float32)[:n]
    for r in range(0, n + 1):
        for subset in itertools.combinations(range(n), r):
            s = base.copy()
            s[list(subset)] = NINF
            check(s, kind)
    got = keyed(np.full(n, NINF), MOVES[kind])
    assert got == (np.uint32(0xFF800000), 0)                                     # the all -inf cell: move 0, as np.argmax


@pytest.mark.parametrize("kind", ["label", "blank"])
def test_minus_zero_denormals_and_the_largest_magnitude(kind):
    n = len(MOVES[kind])
    specials = [NZERO, TINY, DENORM, np.float32(-1.1754944e-38), np.float32(-1.0), HUGE, NINF]
    for s in itertools.product(specials, repeat=n):
        check(np.array(s, np.float32), kind)
    # -0.0 and the denormals are f64 denormals (or zero) as keys: a minimum that flushed them would tie them all at move 0
    assert keyed([DENORM, TINY, NZERO, TINY], MOVES["label"])[1] == 2
    assert keyed([DENORM, TINY, DENORM], MOVES["blank"])[1] == 1


def test_a_positive_sum_and_plus_zero_go_wrong():
    """Why the keyed frames run only on lattices whose log-probs all have the sign bit set: the key is |s|."""
    s = np.array([-1.0, 2.0, -3.0, -4.0], np.float32)
    assert reference(s, MOVES["label"])[1] == 1 and keyed(s, MOVES["label"])[1] == 0
    s = np.array([0.5, 2.0, -3.0, -4.0], np.float32)
    assert reference(s, MOVES["label"])[1] == 1 and keyed(s, MOVES["label"])[1] == 0
    # +0.0 against -0.0: equal as floats (the first wins), but the keyed cell cannot tell the maximum's sign
    s = np.array([NZERO, np.float32(0.0), -1.0, -1.0], np.float32)
    want, got = reference(s, MOVES["label"]), keyed(s, MOVES["label"])
    assert want[1] == got[1] == 0 and int(want[0]) == 0x80000000
    s = np.array([np.float32(0.0), NZERO, -1.0, -1.0], np.float32)
    want, got = reference(s, MOVES["label"]), keyed(s, MOVES["label"])
    assert int(want[0]) == 0x00000000 and int(got[0]) == 0x80000000               # wrong bits of the maximum
    # and +0.0 next to a negative sum it should beat: it does, but a positive denormal next to -0.0 does not
    s = np.array([NZERO, np.float32(1e-45), -1.0, -1.0], np.float32)
    assert reference(s, MOVES["label"])[1] == 1 and keyed(s, MOVES["label"])[1] == 0


def test_the_flag_of_the_forward_kernel():
    """kFlagAllNeg is the sign bit of the AND of all log-prob bits: -0.0 and -inf keep it, +0.0 and anything positive clear it."""
    def all_neg(a):
        return bool(np.bitwise_and.reduce(np.asarray(a, np.float32).view(np.uint32)) & np.uint32(0x80000000))
    assert all_neg([-1.0, NZERO, NINF, TINY, HUGE])
    assert not all_neg([-1.0, 0.0, -2.0])
    assert not all_neg([-1.0, 1e-45, -2.0])
    assert not all_neg([-1.0, np.inf])
