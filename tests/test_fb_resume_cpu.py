"""The float64 reference of the resumed forward-backward (tests/fb_resume_ref.py) against the uncut references, against path
enumeration and against its own planted faults; and what of ka_ctc_posteriors_resume needs no device: the symbols, the
workspace figure and the Python argument checks."""
import ctypes
import os
import re

import numpy as np
import pytest

import banded_fb_ref as B
import fb_resume_ref as F
import posterior_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("ka_ctc_posteriors_resume_f32", "ka_ctc_posteriors_resume_batch_f32", "ka_posteriors_resume_workspace_bytes")
SMALL = [(s, t) for s, t in F.all_cases() if s != F.WIDE_SHAPE]      # (the widest band runs once, below)

_built = {}


def case(shape, table):
    if (shape, table) not in _built:
        _built[shape, table] = F.build(shape, table)
    return _built[shape, table]


def uncut(shape, table):
    """(gamma [T, L], ll) of the uncut lattice: banded_fb_ref's, or for a lattice with a start row of its own the resumed
    reference in one piece (checked on every other case against banded_fb_ref)."""
    lp, labels, band, term, beam, mm, alpha0, _ = case(shape, table)
    if alpha0 is None:
        ref = B.ref_at(lp, labels, term, band, beam, mm)
        assert ref["status"] == R.OK
        return B.dense_gamma(ref, 2 * len(labels) + 1), ref["ll"]
    one = F.resume(lp, labels, band, beam, mm, alpha0, term)
    assert one["status"] == R.OK
    return one["gamma"], one["ll"]


@pytest.mark.parametrize("shape,table", SMALL, ids=[F.case_name(s, t) for s, t in SMALL])
def test_cut_and_resume_is_the_uncut_lattice(shape, table):
    """Claim 4 in the reference: chunked gamma and every chunk's Z within 1e-9 of the uncut reference (the worst over these cases
    and cuts is printed: 5.7e-13), and logsumexp(alpha_in + beta_out) over a chunk's start row is its Z."""
    lp, labels, band, term, beam, mm, alpha0, cut_sets = case(shape, table)
    gamma, ll = uncut(shape, table)
    worst = 0.0
    for cuts in cut_sets:
        got = F.chunked(lp, labels, band, beam, mm, cuts, term, alpha0=alpha0)
        assert got["status"] == R.OK, cuts
        worst = max(worst, float(np.max(np.abs(got["gamma"] - gamma))), max(abs(z - ll) for z in got["ll"]))
        for c in got["chunks"]:
            if c["alpha_in"] is not None:
                z0 = float(R._lse((c["alpha_in"] + c["beta_out"])[:, None])[0])
                worst = max(worst, abs(z0 - c["ll"]))
    print("worst", worst)
    assert worst <= 1e-9


def test_the_widest_band_cut_in_the_middle():
    for table in F.TABLES:
        lp, labels, band, term, beam, mm, alpha0, cut_sets = case(F.WIDE_SHAPE, table)
        assert cut_sets == [(350,)] and R.fast_form(F.WIDE_SHAPE[1], F.WIDE_SHAPE[2], beam, mm)
        gamma, ll = uncut(F.WIDE_SHAPE, table)
        got = F.chunked(lp, labels, band, beam, mm, (350,), term)
        assert np.max(np.abs(got["gamma"] - gamma)) <= 1e-9 and max(abs(z - ll) for z in got["ll"]) <= 1e-9
        lo, hi = got["chunks"][1]["windows"]
        if table == "diagonal":
            assert hi[0] - max(lo[0] - (mm - 1), 0) == 1012, "the start window of the second chunk fills 1012 slots"


def test_the_uncut_resumed_reference_is_banded_fb_ref():
    """One piece, virtual start, a terminal: the reference this file adds is the one the banded calls are tested against."""
    for shape, table in SMALL:
        lp, labels, band, term, beam, mm, alpha0, _ = case(shape, table)
        if alpha0 is not None:
            continue
        ref = B.ref_at(lp, labels, term, band, beam, mm)
        one = F.resume(lp, labels, band, beam, mm, None, term)
        assert np.max(np.abs(one["gamma"] - B.dense_gamma(ref, 2 * len(labels) + 1))) <= 1e-12
        assert abs(one["ll"] - ref["ll"]) <= 1e-9


def test_cases_are_what_they_say():
    forms = {s: R.fast_form(s[1], s[2], s[3], s[4]) for s, _ in F.all_cases()}
    assert forms[(97, 40, 39, 16, 4)] and forms[(200, 280, 39, 7, 4)] and forms[F.WIDE_SHAPE] and forms[F.FAR_SHAPE]
    assert not forms[(100, 40, 80, 16, 4)] and not forms[(120, 50, 39, 12, 6)]
    for shape, table in F.all_cases():
        lp, labels, band, term, beam, mm, alpha0, cut_sets = case(shape, table)
        assert cut_sets == ([(350,)] if shape == F.WIDE_SHAPE else F.cuts_of(shape[0])), (shape, "the issue's cut list")
        if table == "random":      # a valid table whose steps reach max_move-1
            steps = np.diff(band)
            assert steps.min() >= 0 and steps.max() == mm - 1 and set(range(mm)) <= set(steps.tolist()), (shape, np.bincount(steps))
    for table in F.TABLES:
        lp, labels, band, term, beam, mm, alpha0, _ = case(F.FAR_SHAPE, table)
        assert band[0] == F.FAR_LO > 1024 and alpha0 is not None
        assert np.any(np.asarray(labels) == 0), "label value 0: the veto is in play"
    # a vetoed cell lies on a cut: some cut frame's band holds an odd position whose label value is 0
    lp, labels, band, term, beam, mm, _, cut_sets = case((97, 40, 39, 16, 4), "diagonal")
    lab = R.expand(labels)
    odd0 = np.flatnonzero((lab == 0) & (np.arange(len(lab)) % 2 == 1))
    assert any(np.any((odd0 >= band[c[0]]) & (odd0 < band[c[0]] + beam)) for c in cut_sets)


def test_brute_force_on_a_tiny_resumed_lattice():
    """Path enumeration with a non-trivial start row and end row, a label 0 and a table that starts above 0."""
    rng = np.random.default_rng(5)
    for trial in range(6):
        T, S, V, beam, mm = int(rng.integers(2, 7)), 4, 5, int(rng.integers(3, 6)), int(rng.integers(2, 5))
        L = 2 * S + 1
        lp = np.log(rng.dirichlet(np.ones(V), size=T))
        labels = rng.integers(1, V, size=S)
        labels[trial % S] = 0
        band = B.random_table(rng, T, L, mm - 1, lo0=1 + trial % 2)
        alpha_in = np.where(rng.random(L) < 0.7, -2.0 * rng.random(L), -np.inf)
        end_row = np.where(rng.random(L) < 0.7, -2.0 * rng.random(L), -np.inf)
        want_g, want_ll = F.enumerate_resumed(lp, labels, band, beam, mm, alpha_in, end_row)
        got = F.resume(lp, labels, band, beam, mm, alpha_in, end_row)
        if not np.isfinite(want_ll):
            assert got["status"] == R.ZERO_MASS
            continue
        assert got["status"] == R.OK
        assert abs(got["ll"] - want_ll) <= 1e-12 and np.max(np.abs(got["gamma"] - want_g)) <= 1e-12
        # and cut in two: the rows carry everything
        if T >= 2:
            two = F.chunked(lp, labels, band, beam, mm, (T // 2,), end_row, alpha0=alpha_in)
            assert np.max(np.abs(two["gamma"] - want_g)) <= 1e-12 and max(abs(z - want_ll) for z in two["ll"]) <= 1e-12


@pytest.mark.parametrize("fault", F.FAULTS)
def test_every_planted_fault_moves_the_occupancy(fault):
    """... by more than 8 x R.label_tolerance on some cell of some case.  Over all cases and cuts (printed) the weakest fault, cut_no_veto_fwd,
    moves a cell by 1.9e6 x; runs that a fault leaves without any mass are counted beside it."""
    worst, no_mass = 0.0, 0
    for shape, table in SMALL:
        lp, labels, band, term, beam, mm, alpha0, cut_sets = case(shape, table)
        gamma, _ = uncut(shape, table)
        clean = F.chunked(lp, labels, band, beam, mm, cut_sets[0], term, alpha0=alpha0)
        lo, hi = B.table_windows(band, 2 * len(labels) + 1, beam)
        tol = R.label_tolerance(F.gamma_list(gamma, lo, hi), labels, lp.shape[1])
        for cuts in cut_sets:
            got = F.chunked(lp, labels, band, beam, mm, cuts, term, alpha0=alpha0, fault=fault)
            if got["status"] != R.OK:       # (a fault that leaves a chunk without mass: counted, not measured)
                no_mass += 1
                continue
            with np.errstate(divide="ignore", invalid="ignore"):
                r = np.abs(got["occ"] - clean["occ"]) / tol
            worst = max(worst, float(np.nanmax(np.where(tol > 0, r, 0.0))))
    print(fault, worst, "runs without mass:", no_mass)
    assert worst > 8.0, fault


def test_symbols_in_header_and_binding_table():
    with open(os.path.join(ROOT, "include", "kokoro_align_amd.h")) as f:
        header = f.read()
    with open(os.path.join(ROOT, "kokoro-align_amd", "_lib.py")) as f:
        binding = f.read()
    exports = re.search(r"EXPORTS = \[(.*?)\]", binding, re.S).group(1)
    for sym in SYMBOLS:
        assert re.search(r"\b%s\(" % sym, header), sym
        assert f'"{sym}"' in exports, sym
    assert "const double *alpha_in" in header and "section 4.37" in header


def test_workspace_figure_without_a_gpu():
    from kokoro_align_amd import _lib
    L = _lib.load_library()
    T, S = (ctypes.c_int64 * 2)(97, 700), (ctypes.c_int64 * 2)(40, 600)
    for mem in (_lib.KA_MEM_HOST, _lib.KA_MEM_DEVICE):
        own = L.ka_posteriors_resume_workspace_bytes(2, T, S, 39, 1009, 4, mem)
        sibling = L.ka_label_posterior_workspace_bytes(2, T, S, 39, 1009, 4, mem)
        assert own > sibling > 0
    host, dev = (L.ka_posteriors_resume_workspace_bytes(2, T, S, 39, 1009, 4, m) for m in (_lib.KA_MEM_HOST, _lib.KA_MEM_DEVICE))
    assert host - dev >= 4 * 8 * (81 + 1201), "the staged rows"
    assert L.ka_posteriors_resume_workspace_bytes(2, T, S, 39, 1009, 0, _lib.KA_MEM_HOST) == 0      # max_move 0
    assert L.ka_posteriors_resume_workspace_bytes(2, (ctypes.c_int64 * 2)(97, 0), S, 39, 16, 4, _lib.KA_MEM_HOST) == 0   # no frames
    assert L.ka_posteriors_resume_workspace_bytes(2, T, S, 39, 16, 4, 7) == 0                       # no such memory mode
    assert L.ka_posteriors_resume_workspace_bytes(-1, T, S, 39, 16, 4, _lib.KA_MEM_HOST) == 0


def test_python_argument_checks():
    import kokoro_align_amd as ka
    lp = np.zeros((8, 5), np.float32)
    labels = np.array([1, 2, 3], np.int32)
    band = np.zeros(8, np.int64)
    assert ka.free_end_scores(7).tolist() == [0.0] * 7 and ka.free_end_scores(7).dtype == np.float64
    with pytest.raises(ValueError, match="2S\\+1"):
        ka.ctc_posteriors_resume(lp, labels, band, alpha_in=np.zeros(6), end=6)
    with pytest.raises(ValueError, match="2S\\+1"):
        ka.ctc_posteriors_resume(lp, labels, band, end=np.zeros(8))
    with pytest.raises(ValueError, match="end"):
        ka.ctc_posteriors_resume(lp, labels, band)
    with pytest.raises(ValueError, match="one position per frame"):
        ka.ctc_posteriors_resume(lp, labels, band, end=6, path=np.zeros(7, np.int32))
    with pytest.raises(ValueError, match="one entry per frame"):
        ka.ctc_posteriors_resume(lp, labels, band[:5], end=6)
    with pytest.raises(ValueError, match="rows"):
        ka.ctc_posteriors_resume(lp, labels, band, end=6, rows="gamma")
    with pytest.raises(ValueError):
        ka.ctc_label_posteriors_chunked(lp, labels, band, 0, 6)
    with pytest.raises(ValueError):
        ka.ctc_label_posteriors_chunked(lp, labels, band, 4, 6, path=np.zeros(3, np.int32))
    # a ragged push: rows of unequal length, or no rows at all
    for bad in ([[0.0, -1.0], [0.0]], np.zeros(5, np.float32), np.zeros((0, 5), np.float32)):
        with pytest.raises(ValueError):
            ka.StreamingAligner(labels, beam_size=4, confidence=True).push(bad)
    a = ka.StreamingAligner(labels, beam_size=4, confidence=True)
    assert a.confidence and not ka.StreamingAligner(labels).confidence
    a._ragged = True          # (what a chunk of a ragged length leaves behind)
    with pytest.raises(ValueError, match="must be the last"):
        a.push(lp)
