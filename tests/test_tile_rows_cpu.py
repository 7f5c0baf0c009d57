"""What tests/test_tile_rows_gpu.py stands on, without a GPU: the cases of tests/tile_rows_cases.py end where their names say,
run in the tiled form at both tile widths, and a copy of the last block of rows that stops at its last whole 16-byte piece
(clamped_tail, the fault model) moves the total's bits of every case named as sensitive and nothing of the controls - and
loses exactly the non-finite cells named as hidden.  Conditions on the oracle and on the host's tile plan, not measurements."""
import ctypes

import numpy as np
import pytest

import tile_rows_cases as C
from oracle import oracle as O


def same(a, b):
    return (a is not None and b is not None and all(np.array_equal(x.view(np.int32), y.view(np.int32)) for x, y in zip(a[:3], b[:3]))
            and C.bits(a[3]) == C.bits(b[3]) and a[4] == b[4])


def faulted(lp, lab, beam):
    try:
        return O.ctc_best_path_c(C.clamped_tail(lp), lab, beam, C.MM, return_total=True)
    except ValueError:
        return None


def test_the_tail_is_what_the_block_s_bytes_say():
    assert [C.tail(T, 39) for T in (32, 33, 34, 35, 36, 65, 66, 67, 99)] == [0, 3, 2, 1, 0, 3, 2, 1, 1]
    assert all(C.tail(T, V) == 0 for T in C.RESIDUE_T for V in (64, 40))
    assert {T % 4 for T in C.RESIDUE_T} == {0, 1, 2, 3}
    assert {1, 2, 3} <= set(C.RESIDUE_T)                              # below one block
    assert {31, 32, 33, 63, 64, 65} <= set(C.RESIDUE_T)               # a block ends on the checkpoint frames 31 and 63
    assert {T % 4 for T in C.NONFINITE_T} == {1, 2, 3}
    lp = O.hash_logprobs(34, 39, 1)
    f = C.clamped_tail(lp)
    assert np.array_equal(f[:33], lp[:33]) and np.array_equal(f[33, :37], lp[33, :37]) and np.array_equal(f[33, 37:], lp[33, 33:35])


@pytest.mark.parametrize("T", C.RESIDUE_T)
def test_residue_cases_end_on_a_label_cell_and_only_the_sensitive_ones_move(T):
    S, beam = C.residue_shape(T)
    assert T <= 99 and S <= 150
    for V in C.VS:
        for k in C.TERMS:
            name, lp, lab, b = C.residue(T, V, k)
            w = C.want(name, lp, lab, b)
            assert w is not None and w[4] == C.residue_end(T) and w[4] % 2 == 1 and w[4] < 2 * S, name
            assert w[1][-1] == V - k, name                           # the terminal reads column V - k of row T - 1
            f = faulted(lp, lab, b)
            if C.sensitive(T, V, V - k):
                assert V == 39 and T % 4 != 0 and k <= 3
                assert np.array_equal(f[0], w[0]) and f[4] == w[4], name      # the path never moves ..
                assert C.bits(f[3]) != C.bits(w[3]), name                     # .. the total does
            else:
                assert same(f, w), name
    # every tail length meets a terminal inside and outside it
    assert [C.sensitive(T, 39, 39 - k) for k in C.TERMS] == [C.tail(T, 39) >= k for k in C.TERMS[:3]] + [False]


def test_even_frame_counts_need_the_band_to_cap_the_end():
    for T in (34, 66):
        S, beam = C.residue_shape(T)
        lp, lab = C.constant_lattice(T, S, 39, 38)
        assert O.ctc_best_path_c(lp, lab, C.WIDE_BEAM, C.MM, return_total=True)[4] % 2 == 0      # no band: 3 T, a blank
        assert O.ctc_best_path_c(lp, lab, beam + 2, C.MM, return_total=True)[4] == 2 * S          # a wider band reaches L - 1
        L, q = 2 * S + 1, (2 * S + 1) * (T - 1) // T
        assert min(max(q - beam // 2, 0) + beam, L) - 1 == C.residue_end(T)                       # hi(T - 1) - 1 (align.py:64-65)


@pytest.mark.parametrize("T", C.TWO_TILE_T)
def test_two_tile_cases_end_below_the_highest_tile_alive(T):
    for k in C.TERMS:
        name, lp, lab, beam = C.two_tile(T, 39, k)
        w = C.want(name, lp, lab, beam)
        assert w[4] == 3 * T and w[1][-1] == 39 - k
        f = faulted(lp, lab, beam)
        assert (C.bits(f[3]) != C.bits(w[3])) == C.sensitive(T, 39, 39 - k), name
        assert same(f, w) != C.sensitive(T, 39, 39 - k), name
    assert 2 * C.TWO_TILE_S + 1 > 256
    assert {3 * T // 128 for T in C.TWO_TILE_T} == {1, 2}              # 65, 67: the middle one of three 128-position tiles
    assert {3 * T // 256 for T in C.TWO_TILE_T} == {0, 1}


@pytest.mark.parametrize("T", C.RESIDUE_T)
def test_blank_cases_end_on_the_last_blank_and_nothing_moves(T):
    for V in C.VS:
        name, lp, lab, beam = C.blank(T, V)
        w = C.want(name, lp, lab, beam)
        assert w is not None and w[4] == 2 * len(lab) and w[1][-1] == 0, name
        assert same(faulted(lp, lab, beam), w), name


def test_every_shape_runs_tiled_at_both_widths():
    from kokoro_align_amd import _lib
    L = _lib.load_library()
    shapes = {(T,) + C.residue_shape(T) for T in C.RESIDUE_T} | {(T, C.TWO_TILE_S, C.WIDE_BEAM) for T in C.TWO_TILE_T}
    shapes |= {(T,) + C.blank_shape(T) for T in C.RESIDUE_T} | {C.WIDE}
    for T, S, beam in sorted(shapes):
        for V in C.VS:
            for width in (128, 256):
                n = L.ka_debug_plan_tiles_width(T, S, V, beam, C.MM, width, None, None, 0, None)
                assert n >= 1, (T, S, V, beam, width, n)             # 0: the shape would not run tiled
    # the two-tile cases: every tile is alive in frame T - 1 (no band), three of 128 positions and two of 256
    for T in C.TWO_TILE_T:
        for width, n_want in ((128, 3), (256, 2)):
            t_in, t_end = np.zeros(8, np.int32), np.zeros(8, np.int32)
            n = L.ka_debug_plan_tiles_width(T, C.TWO_TILE_S, 39, C.WIDE_BEAM, C.MM, width, t_in.ctypes.data, t_end.ctypes.data, 8, None)
            assert n == n_want and list(t_in[:n]) == [0] * n and list(t_end[:n]) == [T] * n
    T, S, beam = C.WIDE
    assert min(beam, 2 * S + 1) > 1009


@pytest.mark.parametrize("T", C.NONFINITE_T)
def test_the_fault_model_loses_the_hidden_cells_and_only_those(T):
    cells = C.nonfinite_cells(T)
    assert [C.hidden(T, c) for c in cells] == [False] + [39 - c[1] <= C.tail(T, 39) for c in cells[1:4]] + [False]
    for cell in cells:
        for value in C.VALUES:
            name, lp, lab, beam = C.nonfinite(T, cell, value)
            assert np.sum(~np.isfinite(lp) | (np.abs(lp) >= 1e30)) == 1, name
            lost = np.all(np.abs(C.clamped_tail(lp)) < 1e30)            # (a NaN compares false)
            assert lost == C.hidden(T, cell), name
            if value != "nan":
                # the reference takes -inf and -3e31 as they are: a result, or its ValueError
                w = C.want(name, lp, lab, beam)
                assert w is None or len(w[0]) == T
                if cell == (T - 1, 38) and value == "huge":
                    assert w[4] == C.residue_end(T) and w[2][-1] == C.VALUES["huge"], name      # read as the terminal
    for case in C.neighbours(T):
        assert C.want(*case) is not None and case[3] == C.residue_shape(T)[1]


def test_the_wide_case():
    for value in ("ninf", "huge"):
        lp, lab, beam = C.wide(value)
        w = C.want(("wide", value), lp, lab, beam)
        assert w is not None and len(w[0]) == C.WIDE[0]
    assert w[4] == 99 and w[2][-1] == C.VALUES["huge"]
