"""Inputs for the last, partial 32-row block of the tiled forms (ka_tiled.hpp: stage_rows, sum_rows).

When a launch's rows are contiguous (V = 39 or 64, row pitch V, 16-byte aligned base, or host memory) a tile copies a block
of 32 rows into LDS as it lies in memory, in 16-byte pieces.  A block of r rows of V = 39 floats ends on a 16-byte border only
when r % 4 == 0; otherwise its last piece holds tail(T) = 3, 2 or 1 floats - the last columns of row T - 1 - and bytes that
are not the lattice's.  Two things can then go wrong, and neither moves the path (a last-frame emission is the same for every
predecessor of a cell) or the scores (gathered from global memory): the TOTAL, which is the tile's own score of the terminal
cell, when the terminal's label value lies in those columns; and the finiteness flags, which are summed from the same LDS
bytes - a NaN there must be KA_ERR_NAN, a -inf or a magnitude of 1e30 or more must reach the exact kernels, and whatever lies
behind row T - 1 in the caller's allocation must not count.

Every other best-path test ends its path on L - 1, a blank (column 0), so none reads those columns as a terminal.  Here:

  residues    T with every T % 4, below one block, and block ends on and off the checkpoint frames; the audio is too short for
              the text, so the path ends on a LABEL cell: 3 T for odd T (no band: L > 3 T + 1), and for even T - where 3 T is a
              blank - the band's highest cell of frame T - 1 (beam 6 is the widest that does it: hi(T-1) < L needs
              beam / 2 < ceil(L / T) <= 4).  The transcript is one label value throughout, V - 1, V - 2, V - 3 in turn and
              V - 5 as the control, so that the terminal reads column `term` of row T - 1.  V = 39 is the subject, V = 64
              the same pipeline without a tail, V = 40 always goes row by row.
  two tiles   the same with L = 301: the terminal lies in a lower tile than the highest one alive in frame T - 1
  blank       the text finishes: the terminal is L - 1 (hash labels), same T
  nonfinite   one cell of lp[T-1, V-4 .. V-1] or lp[T-2, V-1] made NaN, -inf or -3e31, for T % 4 = 1, 2, 3
  wide        once with a band of 1011 positions: too wide for the exact kernels

clamped_tail() is the fault model the CPU file tries the cases on: row T - 1's last tail(T) columns read 4 columns lower, which
is what a copy that stops at the block's last whole 16-byte piece delivers.  No product file imports this module.
"""
import functools

import numpy as np

from oracle import oracle as O

MM = 4
SEED = 7
VS = (39, 64, 40)
RESIDUE_T = (1, 2, 3, 4, 5, 31, 32, 33, 34, 35, 36, 37, 63, 64, 65, 66, 67, 97, 98, 99)
TERMS = (1, 2, 3, 5)                    # the transcript's label value is V - k
EVEN_BEAM, WIDE_BEAM = 6, 1000          # the launch's beam for even and for odd T
TWO_TILE_T = (65, 67, 97, 99)           # with S = 150 (L = 301); (98, 147, 6) of the residues has two tiles too
TWO_TILE_S = 150
NONFINITE_T = (33, 34, 35)              # T % 4 = 1, 2, 3: tails of 3, 2 and 1 columns
VALUES = {"nan": np.float32(np.nan), "ninf": np.float32(-np.inf), "huge": np.float32(-3e31)}
WIDE = (33, 505, 2100)                  # T, S, beam: lo(T - 1) = 0 and a band of L = 1011 positions, more than the 1009 of the exact kernels

FORMS = ("tiled/128", "tiled/256", "tiled/128+parallel", "auto", "wave_exact")
TILED = ("tiled/128", "tiled/256", "tiled/128+parallel")
LAYOUTS = ("host", "aligned", "off4", "ld64", "fenced", "mixed")


def tail(T, V):
    """Floats of row T - 1 in the last, partly filled 16-byte piece of the last block of rows (0: the block ends on a border)."""
    return ((4 * V * (T % 32)) % 16) // 4


def residue_shape(T):
    """(S, beam) of the residue case of T: its path ends on a label cell."""
    if T % 2:
        return (3 * T + 3) // 2, WIDE_BEAM          # L = 2 S + 1 >= 3 T + 3: the frontier 3 T is a label cell below L - 1
    return 3 * T // 2, EVEN_BEAM                    # L = 3 T + 1, band of 6: hi(T - 1) - 1 = 3 T - 1


def residue_end(T):
    return 3 * T if T % 2 else 3 * T - 1


def blank_shape(T):
    return T - 1, WIDE_BEAM                         # L - 1 = 2 T - 2: the text finishes (T = 1: no text, one blank)


@functools.lru_cache(maxsize=None)
def constant_lattice(T, S, V, term):
    lp = O.hash_logprobs(T, V, SEED)
    lab = np.full(S, term, np.int32)
    lp.setflags(write=False)
    lab.setflags(write=False)
    return lp, lab


@functools.lru_cache(maxsize=None)
def hash_lattice(T, S, V, seed):
    lp, lab = O.hash_logprobs(T, V, seed), O.hash_labels(S, V, seed)
    lp.setflags(write=False)
    lab.setflags(write=False)
    return lp, lab


def residue(T, V, k):
    """(name, lp, labels, beam) of the residue case: transcript of V - k throughout."""
    S, beam = residue_shape(T)
    return (f"T{T}_V{V}_term{V - k}",) + constant_lattice(T, S, V, V - k) + (beam,)


def two_tile(T, V, k):
    return (f"two_T{T}_V{V}_term{V - k}",) + constant_lattice(T, TWO_TILE_S, V, V - k) + (WIDE_BEAM,)


def blank(T, V):
    S, beam = blank_shape(T)
    return (f"blank_T{T}_V{V}",) + hash_lattice(T, S, V, 300 + T) + (beam,)


def sensitive(T, V, term):
    """Does the terminal of a lattice that ends on a cell of label `term` read one of the tail columns?"""
    return term >= V - tail(T, V)


def clamped_tail(lp):
    """The fault model: row T - 1's last tail(T) columns hold what lies 4 columns lower."""
    T, V = lp.shape
    out = np.array(lp, dtype=np.float32)
    n = tail(T, V)
    if n:
        out[T - 1, V - n:] = lp[T - 1, V - n - 4:V - 4]
    return out


def nonfinite_cells(T, V=39):
    """(row, column) of the cells tried one at a time"""
    return [(T - 1, c) for c in (V - 4, V - 3, V - 2, V - 1)] + [(T - 2, V - 1)]


def nonfinite(T, cell, value, V=39):
    """(name, lp, labels, beam): the residue case of T that ends on label V - 1, with one cell replaced."""
    _, lp, lab, beam = residue(T, V, 1)
    lp = lp.copy()
    lp[cell] = VALUES[value]
    return f"T{T}_{value}_at_{cell[0]}_{cell[1]}", lp, lab, beam


def hidden(T, cell, V=39):
    """Does the fault model lose the cell?"""
    return cell[0] == T - 1 and cell[1] >= V - tail(T, V)


def neighbours(T, V=39):
    """Two residue cases of other T, the launch's beam theirs too: a faulty lattice runs as the middle one of three."""
    a, b = (37, 5) if T % 2 else (36, 4)
    return residue(a, V, 5), residue(b, V, 2)


def wide(value):
    T, S, beam = WIDE
    lp, lab = constant_lattice(T, S, 39, 38)
    lp = lp.copy()
    lp[T - 1, 38] = VALUES[value]
    return lp, lab, beam


_want = {}


def want(name, lp, lab, beam):
    """The C oracle's (path, labels, scores, total, end), once per name; None where the reference raises (empty beam)."""
    if name not in _want:
        try:
            _want[name] = O.ctc_best_path_c(lp, lab, beam, MM, return_total=True)
        except ValueError:
            _want[name] = None
    return _want[name]


def bits(x):
    return int(np.float32(x).view(np.int32))
