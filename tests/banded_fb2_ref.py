"""Float64 references of the state visits, the boundary quantiles, the sampled paths and the MEA path over a caller-given
band, beside tests/banded_fb_ref.py and by its one device: visit_ref, quantile_ref, sample_ref and
mea_ref take their windows from posterior_ref.windows(T, L, beam) through the module attribute, so ``under_table`` around them
IS the banded reference, and with the diagonal as the table it reproduces the unwrapped one exactly
(tests/test_banded_posteriors2_cpu.py).  That holds for the integer definitions the kernels are held to bit for bit as well:
quantile_ref.integer_quantiles and mea_ref.replay on the rows of ka_ctc_state_posteriors_banded at every frame.

Plantable faults (FAULTS), each a mistake one of the walks could make under a table; each is shown on a named case:
    mea_late_table     the MEA forward walk takes lo one frame late: the code of frame t is decoded at offset
                       p - lo_{max(t-1, 0)}, another cell's code wherever the table stepped into frame t
    start_gt           a cut's start frame as the first t with lo_t > c in place of >= c: the frames at which the band's low end
                       stands on the cut are lost (F reads 0 there)
    start_zero_only    start frame 0 for c <= lo_0 only when c = 0: a cut in (0, lo_0] is never given a start and reads T
    prev_band          sample_ref's: the draw into frame t - 1 is confined to the band of frame t as well
"""
import numpy as np

import banded_fb_ref as B
import mea_ref as M
import posterior_ref as R
import quantile_ref as Q
import sample_ref as SR
import visit_ref as VR

FAULTS = ("mea_late_table", "start_gt", "start_zero_only", "prev_band")
under_table = B.under_table


def visits(lp, labels, terminal, band_lo, beam, mm):
    """visit_ref.visits under the table (the lattice must have mass at the terminal)."""
    with under_table(band_lo):
        return VR.visits(lp, labels, terminal, beam, mm)


def quantiles(lp, labels, terminal, band_lo, beam, mm, cuts, levels, gamma=None):
    """quantile_ref.quantiles under the table: the float64 frames, their margins and the unsafe pairs."""
    with under_table(band_lo):
        return Q.quantiles(lp, labels, terminal, beam, mm, cuts, levels, gamma=gamma)


def integer_quantiles(rows, band_lo, cuts, levels, L, beam, fault=None):
    """quantile [K, M] int32 from the rows of the banded state-posterior call at every frame (its band_lo output is the
    table): quantile_ref.integer_quantiles under the table.  ``fault``: start_gt or start_zero_only, applied to F before the
    levels are read off it."""
    assert fault in (None, "start_gt", "start_zero_only"), fault
    table = np.asarray(band_lo, np.int64).reshape(-1)
    cuts = np.asarray(cuts, np.int64).reshape(-1)
    with under_table(table):
        if fault is None:
            return Q.integer_quantiles(rows, table, cuts, levels, L, beam)
        F = Q.integer_sums(rows, table, cuts, L, beam)
    if fault == "start_gt":
        F[table[:, None] == cuts[None, :]] = 0
    else:
        F[:, (cuts > 0) & (cuts <= table[0])] = 0
    T = F.shape[0]
    thr = Q.thresholds(levels)
    out = np.full((len(cuts), len(thr)), T, np.int32)
    for m, x in enumerate(thr):
        hit = F >= np.uint64(x)
        any_hit = hit.any(axis=0)
        out[any_hit, m] = np.argmax(hit, axis=0)[any_hit]
    return out


def mea_reference(ref, labels, terminal, band_lo, beam, mm, fault=None):
    """mea_ref.reference (float64 gamma of banded_fb_ref.ref_at) under the table; ``fault``: one of mea_ref.FAULTS."""
    with under_table(band_lo):
        return M.reference(ref, labels, terminal, beam, mm, fault)


def mea_replay(rows, band_lo, labels, terminal, beam, mm, fault=None):
    """mea_ref.replay on the rows of the banded state-posterior call at every frame: what ka_ctc_mea_path_banded must return
    bit for bit.  ``fault``: mea_late_table, the forward walk re-done with lo one frame late (status mea_ref.LEFT_BAND and -1
    from there on if that leaves the codes' row)."""
    assert fault in (None, "mea_late_table"), fault
    table = np.asarray(band_lo, np.int64).reshape(-1)
    with under_table(table):
        got = M.replay(rows, table, labels, terminal, beam, mm)
    if fault is None or got["status"] != R.OK:
        return got
    T = len(table)
    path = np.full(T, -1, np.int64)
    path[0] = got["path"][0]
    for t in range(T - 1):
        o = int(path[t] - table[max(t - 1, 0)])
        if not 0 <= o < len(got["code"][t]):
            return dict(got, status=M.LEFT_BAND, path=path)
        path[t + 1] = path[t] + got["code"][t][o]
    return dict(got, path=path)


def windows(band_lo, L, beam):
    return B.table_windows(band_lo, L, beam)


def sample_lattice(lp, labels, band_lo, beam, mm):
    """sample_ref.Lattice under the table: alpha over the table's windows, and the draws on it."""
    with under_table(band_lo):
        return SR.Lattice(lp, labels, beam, mm)


def sample_paths(lp, labels, terminal, K, seed, band_lo, beam, mm, fault=None, lattice=None):
    lat = lattice or sample_lattice(lp, labels, band_lo, beam, mm)
    return SR.sample_paths(lp, labels, terminal, K, seed, beam, mm, fault=fault, lattice=lat)


def held_positions(band_lo, L, beam):
    """The positions that some frame's band holds."""
    lo, hi = B.table_windows(band_lo, L, beam)
    held = np.zeros(L, bool)
    for a, b in zip(lo, hi):
        held[int(a):int(b)] = True
    return held


# the tables of the GPU tests beyond tests/band_cases.py: T = 70, a step of 5 at a block's last frame, its first and the one
# behind it, and a flat table that starts at 2 (section 4.30's four)
def _flat70(at, step, base=0):
    import band_cases as C

    def make():
        lp, labels = C.random_lattice(300 + at + base, 70, 40)
        return lp, labels, C.flat_with_step(70, at, step, base), 24, 4
    return make


EXTRA = {"step5_at31": _flat70(31, 5), "step5_at32": _flat70(32, 5), "step5_at33": _flat70(33, 5), "lo2": _flat70(70, 0, base=2)}
NO_PATH = ("no_overlap", "step500", "step1100", "mm1")
_made = {}


def case(name):
    """(lp, labels, table, beam, mm) of a band_cases name or one of EXTRA: made once."""
    import band_cases as C
    if name in EXTRA:
        if name not in _made:
            _made[name] = EXTRA[name]()
        return _made[name]
    return C.case(name)


def names_with_path():
    import band_cases as C
    return [n for n in C.NAMES if n not in NO_PATH]


_live = {}


def live(name):
    if name not in _live:
        lp, labels, table, beam, mm = case(name)
        _live[name] = B.live_terminals(lp, labels, table, beam, mm)
    return _live[name]


SAMPLER_K, SAMPLER_SEED = 64, 20240
MAX_UNDECIDABLE_PER_CASE, MAX_UNDECIDABLE_SHARE = 3, 1e-5


def sampler_inputs():
    """[(name, terminal)]: the band_cases tables that have a path, two terminals each (live[0], live[-1]: the one with the most
    mass and the one with the least; one where only one is live) - the inputs the sampler's caps are stated on, for the CPU test
    of the reference and the GPU test of the kernels alike."""
    return [(n, t) for n in names_with_path() for t in dict.fromkeys((live(n)[0], live(n)[-1]))]
