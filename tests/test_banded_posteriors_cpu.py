"""The forward-backward calls over a caller-given band, without a GPU: the float64 references under a table
(tests/banded_fb_ref.py), what they say about the rescue case, the tables that leave no path, the planted faults, and the new
symbols and keywords."""
import ctypes

import numpy as np
import pytest

import band_cases as C
import band_ref
import banded_fb_ref as B
import duration_ref as D
import occupancy_ref as O
import posterior_ref as R
from fb_harness import assert_declared_exported_bound

import kokoro_align_amd as ka

CALLS = ("path_posteriors", "label_posteriors", "state_posteriors", "state_durations")
NEW_SYMBOLS = tuple(f"ka_ctc_{c}_banded{f}_f32" for c in CALLS for f in ("", "_batch")) + ("ka_band_table_workspace_bytes",)
ZERO_MASS_TABLES = ("no_overlap", "step500", "step1100", "mm1")


def _same(a, b):
    if isinstance(a, np.ndarray):
        return a.shape == b.shape and a.tobytes() == b.tobytes()
    if isinstance(a, (list, tuple)):
        return len(a) == len(b) and all(_same(x, y) for x, y in zip(a, b))
    return a == b or (a != a and b != b)


# ---------------------------------------------------------------------------------------
# the wrapped references are the originals on other windows
# ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("T,S,V,beam,mm,seed", [(70, 40, 8, 24, 4, 1), (33, 40, 8, 24, 5, 2), (1, 5, 8, 8, 4, 3), (90, 12, 8, 1000, 3, 4),
                                                (64, 150, 8, 7, 4, 5)])
def test_diagonal_table_reproduces_the_diagonal_references_exactly(T, S, V, beam, mm, seed):
    lp, labels = C.random_lattice(seed, T, S, V)
    L = 2 * S + 1
    diag = ka.diagonal_band(T, L, beam)
    assert _same(B.table_windows(diag, L, beam), R.windows(T, L, beam))
    live = R.live_terminals(lp, labels, beam, mm)
    assert B.live_terminals(lp, labels, diag, beam, mm) == live
    for term in live[:2] + [0]:
        want = R.ref_at(lp, labels, term, beam, mm)
        got = B.ref_at(lp, labels, term, diag, beam, mm)
        assert want.keys() == got.keys() and all(_same(want[k], got[k]) for k in want), term
        wo, go = O.occupancy(lp, labels, term, beam, mm), B.occupancy(lp, labels, term, diag, beam, mm)
        assert _same(wo["occ"], go["occ"]) and _same(wo["ll"], go["ll"]) and wo["status"] == go["status"]
        if want["status"] == R.OK:
            wd, gd = D.durations(want, L), B.durations(lp, labels, term, diag, beam, mm)[0]
            assert all(_same(wd[k], gd[k]) for k in wd)
    assert R.windows(T, L, beam)[0].tolist() == np.asarray(diag).tolist()          # (windows is back in place)


def test_windows_are_restored_after_a_failure():
    saved = R.windows
    with pytest.raises(AssertionError):
        B.ref_at(np.zeros((5, 4), np.float32), [1, 2], 4, np.zeros(4, np.int64), 3, 4)     # a table of the wrong length
    assert R.windows is saved


# ---------------------------------------------------------------------------------------
# path enumeration on tiny lattices under random monotone tables
# ---------------------------------------------------------------------------------------
def _tiny_cases():
    rng = np.random.default_rng(2024)
    cases = []
    for i in range(60):
        T, S, beam, mm = int(rng.integers(1, 7)), int(rng.integers(0, 4)), int(rng.integers(2, 6)), int(rng.integers(2, 5))
        L = 2 * S + 1
        lo0 = int(rng.integers(1, 4)) if i % 3 == 0 else 0                      # every third table starts above 0
        table = B.random_table(rng, T, L, max_step=3, lo0=min(lo0, L - 1))
        cases.append((i, T, S, beam, mm, table))
    # a step that leaves no live predecessor: the band jumps by more than beam + max_move
    cases.append((100, 5, 3, 2, 3, np.array([0, 0, 0, 6, 6], np.int64)))
    cases.append((101, 6, 3, 2, 2, np.array([0, 0, 1, 1, 5, 5], np.int64)))
    return cases


def test_tables_against_path_enumeration():
    seen_lo0, seen_dead, seen_live = 0, 0, 0
    for i, T, S, beam, mm, table in _tiny_cases():
        lp, labels = _tiny_lattice(900 + i, T, S)
        L = 2 * S + 1
        lo, hi = B.table_windows(table, L, beam)
        seen_lo0 += int(table[0] > 0)
        for term in range(int(lo[-1]), int(hi[-1])):
            gamma, ll = B.enumerate_gamma(lp, labels, term, table, beam, mm)
            ref = B.ref_at(lp, labels, term, table, beam, mm)
            what = (i, term, table.tolist(), beam, mm)
            if ll == -np.inf:
                assert ref["status"] == R.ZERO_MASS and ref["ll"] == -np.inf, what
                assert B.occupancy(lp, labels, term, table, beam, mm)["status"] == R.ZERO_MASS, what
                seen_dead += 1
                continue
            seen_live += 1
            assert ref["status"] == R.OK and abs(ref["ll"] - ll) < 1e-12 * max(1.0, abs(ll)), what
            np.testing.assert_allclose(B.dense_gamma(ref, L), gamma, rtol=0, atol=1e-12, err_msg=str(what))
            # the path call's posterior is gamma at the path, whatever the path does inside or outside the windows
            path = np.minimum(np.arange(T), L - 1)
            path[-1] = term
            got = B.forward_backward(lp, labels, path, table, beam, mm)
            np.testing.assert_allclose(got["post"], gamma[np.arange(T), path], rtol=0, atol=1e-12, err_msg=str(what))
            occ = np.zeros((T, lp.shape[1]))
            for t in range(T):
                np.add.at(occ[t], R.expand(labels), gamma[t])
            np.testing.assert_allclose(B.occupancy(lp, labels, term, table, beam, mm)["occ"], occ, rtol=0, atol=1e-12, err_msg=str(what))
            dref = B.durations(lp, labels, term, table, beam, mm)[0]
            np.testing.assert_allclose(dref["D"], gamma.sum(0), rtol=0, atol=1e-12, err_msg=str(what))
            np.testing.assert_allclose(dref["B"], (np.arange(T)[:, None] * gamma).sum(0), rtol=0, atol=1e-11, err_msg=str(what))
            held = np.zeros(L, bool)
            for t in range(T):
                held[lo[t]:hi[t]] = True
            assert np.all(dref["D"][~held] == 0.0) and np.all(dref["n"][~held] == 0), what
    # the two hand-made tables leave no path at all; the random ones exercise both outcomes and tables that start above 0
    for i, T, S, beam, mm, table in _tiny_cases()[-2:]:
        lp, labels = _tiny_lattice(900 + i, T, S)
        assert B.live_terminals(lp, labels, table, beam, mm) == [], i
    assert seen_lo0 >= 10 and seen_dead >= 10 and seen_live >= 40, (seen_lo0, seen_dead, seen_live)


def _tiny_lattice(seed, T, S, V=5):
    rng = np.random.default_rng(seed)
    lp = np.log(rng.dirichlet(np.ones(V), size=T)).astype(np.float32)
    labels = rng.integers(0, V, size=S).astype(np.int32)           # (label 0 among them: the veto is live)
    return lp, labels


# ---------------------------------------------------------------------------------------
# the rescue case: the diagonal band's posteriors describe the wrong lattice
# ---------------------------------------------------------------------------------------
_rescue = {}


def rescue_refs(seed):
    """The rescue case under the diagonal and the anchored band: computed once per seed."""
    if seed not in _rescue:
        lp, labels, L, beam, pre = C.rescue(seed)
        T = lp.shape[0]
        out = {}
        for name, table in (("diagonal", ka.diagonal_band(T, L, beam)), ("anchored", ka.anchored_band(T, L, [(pre, 0)], beam))):
            path = band_ref.best_path_banded(lp, labels, table, beam, 4)[0]
            post = B.forward_backward(lp, labels, path, table, beam, 4)
            dref, ref = B.durations(lp, labels, L - 1, table, beam, 4)
            out[name] = dict(path=path, post=post, z=ref["ll"], D=dref["D"])
        _rescue[seed] = (out, T, L, pre)
    return _rescue[seed]


@pytest.mark.parametrize("seed", range(6))
def test_rescue_case(seed):
    out, T, L, pre = rescue_refs(seed)
    anchored, diagonal = out["anchored"], out["diagonal"]
    assert anchored["post"]["status"] == R.OK and diagonal["post"]["status"] == R.OK
    assert anchored["post"]["post"].mean() >= 0.95
    assert diagonal["post"]["post"].mean() <= 0.6
    assert anchored["z"] - diagonal["z"] > 100.0                   # log-likelihood of terminal L-1, nats
    assert abs(anchored["D"][0] - pre) < 3.0
    assert abs(anchored["D"].sum() - T) < 1e-9 * T


# ---------------------------------------------------------------------------------------
# the tables on which the best-path reference finds no path leave no mass at any terminal
# ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ZERO_MASS_TABLES)
def test_tables_without_a_best_path_are_zero_mass_for_every_terminal(name):
    assert C.want(name) is None
    lp, labels, table, beam, mm = C.case(name)
    L = 2 * len(labels) + 1
    assert B.live_terminals(lp, labels, table, beam, mm) == []
    lo, hi = B.table_windows(table, L, beam)
    for term in (int(lo[-1]), int(hi[-1]) - 1, 0, L - 1):
        ref = B.ref_at(lp, labels, term, table, beam, mm)
        assert ref["status"] == R.ZERO_MASS and ref["ll"] == -np.inf, (name, term)
        assert B.occupancy(lp, labels, term, table, beam, mm)["status"] == R.ZERO_MASS


# ---------------------------------------------------------------------------------------
# each planted fault shows on a named case
# ---------------------------------------------------------------------------------------
def _outputs_moved(lp, labels, term, table, beam, mm, fault):
    """Worst |faulty - right| / tolerance over gamma (per cell, M_STATE x its model), the occupancy rows (M_LABEL) and Z (M_Z);
    inf if the faulty pass fails where the right one does not."""
    L = 2 * len(labels) + 1
    right = B.ref_at(lp, labels, term, table, beam, mm)
    wrong = B.ref_at(lp, labels, term, table, beam, mm, fault)
    assert right["status"] == R.OK
    if wrong["status"] != R.OK:
        return np.inf
    g, h = B.dense_gamma(right, L), B.dense_gamma(wrong, L)
    with np.errstate(divide="ignore", invalid="ignore"):
        state = np.nanmax(np.where(g >= R.TINY, np.abs(h - g) / (R.M_STATE * R.state_error_model(np.where(g >= R.TINY, g, 1.0))), 0.0))
    z = abs(wrong["ll"] - right["ll"]) / (R.M_Z * R.z_error_model(right))
    occ_r, occ_w = B.occupancy(lp, labels, term, table, beam, mm), B.occupancy(lp, labels, term, table, beam, mm, fault)
    E = R.M_LABEL * R.label_error_model(right["gamma"], labels, lp.shape[1])
    with np.errstate(divide="ignore", invalid="ignore"):
        lab = np.nanmax(np.where(E > 0, np.abs(occ_w["occ"] - occ_r["occ"]) / E, 0.0))
    return max(state, z, lab)


def test_fault_late_table_moves_the_staircase():
    lp, labels, table, beam, mm = C.case("staircase")
    term = int(C.want("staircase")[0][-1])
    assert _outputs_moved(lp, labels, term, table, beam, mm, "late_table") > 1.0


def test_fault_past_end_zero_moves_the_staircase():
    lp, labels, table, beam, mm = C.case("staircase")
    term = int(C.want("staircase")[0][-1])
    assert _outputs_moved(lp, labels, term, table, beam, mm, "past_end_zero") > 1.0       # (the last band no longer holds the terminal)


def test_fault_hi_unclamped_widens_the_last_windows_of_beam_ge_L():
    # Paths only move up, so what a band does above L - 1 cannot change gamma inside [0, L) (asserted); the fault shows in what
    # the tests draw from the band itself: its windows reach past L, and there are live terminals past L - 1.
    lp, labels, table, beam, mm = C.case("beam_ge_L")
    L = 2 * len(labels) + 1
    lo, hi = B.table_windows(table, L, beam, "hi_unclamped")
    assert hi.max() > L and B.table_windows(table, L, beam)[1].max() == L
    right, wrong = B.live_terminals(lp, labels, table, beam, mm), B.live_terminals(lp, labels, table, beam, mm, "hi_unclamped")
    assert max(right) <= L - 1 < max(wrong)
    assert len(B.ref_at(lp, labels, right[0], table, beam, mm, "hi_unclamped")["last"][1]) > L - int(lo[-1])
    assert _outputs_moved(lp, labels, right[0], table, beam, mm, "hi_unclamped") < 1e-3


def test_faults_are_refused_by_name():
    with pytest.raises(AssertionError):
        B.table_windows(np.zeros(3, np.int64), 5, 2, "no_such_fault")


# ---------------------------------------------------------------------------------------
# symbols, workspace, and the Python keyword
# ---------------------------------------------------------------------------------------
def test_new_symbols_are_declared_exported_and_bound():
    assert_declared_exported_bound(NEW_SYMBOLS)


def test_banded_argtypes_are_the_siblings_with_a_table_behind_max_move():
    from kokoro_align_amd import _lib
    L = _lib.load_library()
    for call in CALLS:
        for form, at, kind in (("", 9, ctypes.c_void_p), ("_batch", 10, ctypes.POINTER(ctypes.c_void_p))):
            sib = getattr(L, f"ka_ctc_{call}{form}_f32").argtypes
            ban = getattr(L, f"ka_ctc_{call}_banded{form}_f32").argtypes
            assert list(ban[:at]) == list(sib[:at]) and ban[at] is kind and list(ban[at + 1:]) == list(sib[at:]), (call, form)
    assert _lib.load_library().ka_version() == 104


def test_band_table_workspace_bytes():
    from kokoro_align_amd import _lib
    L = _lib.load_library()
    arr = lambda xs: (ctypes.c_int64 * len(xs))(*xs)
    ws = lambda n, Ts, mem: L.ka_band_table_workspace_bytes(n, arr(Ts) if Ts is not None else None, mem)
    desc = lambda n: (n * 144 + 255) // 256 * 256                     # the widest derived descriptor, 256-byte granules
    assert ws(1, [240], _lib.KA_MEM_DEVICE) == desc(1)
    assert ws(1, [240], _lib.KA_MEM_HOST) == desc(1) + 1024          # 960 bytes of table, rounded up
    assert ws(3, [1, 64, 65], _lib.KA_MEM_HOST) == desc(3) + 256 + 256 + 512
    assert ws(768, [10000] * 768, _lib.KA_MEM_DEVICE) == desc(768)
    assert ws(2, [5, 0], 0) == 0 and ws(-1, [5], 0) == 0 and ws(1, [5], 7) == 0 and ws(1, None, 0) == 0
    assert ws(0, None, 0) == 0


class _Recorder:
    """Stands in for ``eng.lib``: every symbol answers KA_OK and is written down with its arguments."""

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        def call(*args):
            self.calls.append((name, args))
            return 0
        return call


def _recorded(run):
    """The (symbol, arguments) a front-end function sends, on a stand-in engine."""
    from kokoro_align_amd import posteriors as P
    rec = _Recorder()
    saved = P._host_lattices

    def host_lattices(*args):
        lat = saved(*args)
        lat.engine = lambda: type("Engine", (), dict(lib=rec, handle=None))()
        return lat
    P._host_lattices = host_lattices
    try:
        run(P)
    finally:
        P._host_lattices = saved
    (call,) = rec.calls
    return call


@pytest.mark.parametrize("call", CALLS)
def test_band_lo_none_reaches_the_old_symbol_and_a_table_the_new(call):
    lp, labels = C.random_lattice(7, 12, 4)
    T, L, beam = 12, 9, 4
    own = dict(path_posteriors=lambda P, kw: P.ctc_path_posteriors_batch([lp], [labels], [np.zeros(T, np.int32)], beam, 4, **kw),
               label_posteriors=lambda P, kw: P.ctc_label_posteriors_batch([lp], [labels], [L - 1], beam, 4, **kw),
               state_posteriors=lambda P, kw: P.ctc_state_posteriors_batch([lp], [labels], [L - 1], [[0, 3]], beam, 4, **kw),
               state_durations=lambda P, kw: P.ctc_state_durations_batch([lp], [labels], [L - 1], beam, 4, **kw))[call]
    name, args = _recorded(lambda P: own(P, {}))
    assert name == f"ka_ctc_{call}_batch_f32"
    name_none, args_none = _recorded(lambda P: own(P, dict(band_lo=None)))
    assert name_none == name and len(args_none) == len(args)
    table = ka.diagonal_band(T, L, beam)
    assert table.dtype == np.int64
    name_b, args_b = _recorded(lambda P: own(P, dict(band_lo=[table])))
    assert name_b == f"ka_ctc_{call}_banded_batch_f32" and len(args_b) == len(args) + 1
    assert args_b[8:10] == args[8:10] == (beam, 4)                          # the table sits directly behind max_move
    sent = np.ctypeslib.as_array(ctypes.cast(ctypes.c_void_p(args_b[10][0]), ctypes.POINTER(ctypes.c_int32)), shape=(T,))
    assert np.array_equal(sent, table)                                      # int64 in, int32 out
    with pytest.raises(ValueError):
        _recorded(lambda P: own(P, dict(band_lo=[table[:-1]])))
    with pytest.raises(ValueError):
        _recorded(lambda P: own(P, dict(band_lo=[table, table])))


def test_single_lattice_functions_take_one_table():
    import inspect
    from kokoro_align_amd import posteriors as P
    for name in ("ctc_path_posteriors", "ctc_label_posteriors", "ctc_state_posteriors", "ctc_state_durations"):
        for form in ("", "_batch", "_device"):
            params = list(inspect.signature(getattr(P, name + form)).parameters.values())
            assert params[-1].name == "band_lo" and params[-1].default is None, name + form
    params = list(inspect.signature(P.lattice_log_likelihood).parameters.values())
    assert params[-1].name == "band_lo" and params[-1].default is None
