"""State visits, boundary quantiles, sampled paths and the MEA path over a caller-given band: the
float64 references of tests/banded_fb2_ref.py held against path enumeration, their plantable faults, the rescue case, the new
symbols, the two workspace figures and the ``band_lo=`` keyword of the Python front end.  No GPU."""
import ctypes
import inspect

import numpy as np
import pytest

import band_cases as C
import band_ref
import banded_fb2_ref as B2
import banded_fb_ref as B
import mea_ref as M
import posterior_ref as R
import quantile_ref as Q
import sample_ref as SR
import visit_ref as VR
from fb_harness import assert_declared_exported_bound

import kokoro_align_amd as ka

CALLS = ("state_visits", "boundary_quantiles", "sample_paths", "mea_path")
NEW_SYMBOLS = [f"ka_ctc_{c}_banded{f}_f32" for c in CALLS for f in ("", "_batch")] + ["ka_boundary_quantile_band_table_workspace_bytes"]
LEVELS = (0.05, 0.5, 0.95)


# ---------------------------------------------------------------------------------------
# the diagonal as the table: the unwrapped references, exactly
# ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("T,S,V,beam,mm,seed", [(1, 3, 6, 4, 4, 1), (33, 20, 8, 9, 4, 2), (70, 40, 8, 24, 3, 3), (40, 6, 8, 1000, 5, 4)])
def test_diagonal_table_reproduces_the_diagonal_references_exactly(T, S, V, beam, mm, seed):
    lp, labels = C.random_lattice(seed, T, S, V)
    L = 2 * S + 1
    table = ka.diagonal_band(T, L, beam)
    term = R.live_terminals(lp, labels, beam, mm)[-1]
    cuts = np.arange(0, L + 1)
    plain, wrapped = VR.visits(lp, labels, term, beam, mm), B2.visits(lp, labels, term, table, beam, mm)
    for k in ("V", "X", "E_V", "E_X", "D", "B"):
        assert plain[k].tobytes() == wrapped[k].tobytes(), k
    qp, qw = Q.quantiles(lp, labels, term, beam, mm, cuts, LEVELS), B2.quantiles(lp, labels, term, table, beam, mm, cuts, LEVELS)
    assert np.array_equal(qp["q"], qw["q"]) and qp["F"].tobytes() == qw["F"].tobytes() and np.array_equal(qp["unsafe"], qw["unsafe"])
    ref = R.ref_at(lp, labels, term, beam, mm)
    W = max(1, min(beam, L))
    rows, lo = Q.float32_rows(ref["gamma"], W)
    assert np.array_equal(Q.integer_quantiles(rows, lo, cuts, LEVELS, L, beam), B2.integer_quantiles(rows, table, cuts, LEVELS, L, beam))
    mp, mw = M.reference(ref, labels, term, beam, mm), B2.mea_reference(ref, labels, term, table, beam, mm)
    assert np.array_equal(mp["path"], mw["path"]) and mp["value"] == mw["value"]
    rp, rw = M.replay(rows, lo, labels, term, beam, mm), B2.mea_replay(rows, table, labels, term, beam, mm)
    assert np.array_equal(rp["path"], rw["path"]) and rp["value"] == rw["value"]
    assert np.array_equal(SR.sample_paths(lp, labels, term, 7, 5, beam, mm), B2.sample_paths(lp, labels, term, 7, 5, table, beam, mm))
    assert R.windows(T, L, beam)[0].tolist() == table.tolist()


# ---------------------------------------------------------------------------------------
# every path of tiny lattices under random monotone tables
# ---------------------------------------------------------------------------------------
def _tiny_lattice(seed, T, S, V=5):
    rng = np.random.default_rng(seed)
    lp = np.log(rng.dirichlet(np.ones(V), size=T)).astype(np.float32)
    labels = rng.integers(0, V, size=S).astype(np.int32)           # (label 0 among them: the veto is live)
    return lp, labels


def _tiny_cases():
    rng = np.random.default_rng(4031)
    cases = []
    for i in range(36):
        T, S, beam, mm = int(rng.integers(1, 7)), int(rng.integers(0, 4)), int(rng.integers(2, 6)), int(rng.integers(2, 5))
        L = 2 * S + 1
        lo0 = int(rng.integers(1, 4)) if i % 3 == 0 else 0                      # every third table starts above 0
        cases.append((i, T, S, beam, mm, B.random_table(rng, T, L, max_step=3, lo0=min(lo0, L - 1))))
    return cases


def test_tables_against_path_enumeration():
    seen_lo0 = seen_live = seen_dead = seen_sampled = 0
    for i, T, S, beam, mm, table in _tiny_cases():
        lp, labels = _tiny_lattice(700 + i, T, S)
        L = 2 * S + 1
        lo, hi = B.table_windows(table, L, beam)
        cuts = np.arange(0, L + 1)
        seen_lo0 += int(table[0] > 0)
        for term in range(int(lo[-1]), int(hi[-1])):
            what = (i, term, table.tolist(), beam, mm)
            with B.under_table(table):
                V, X = VR.sequential(lp, labels, term, beam, mm)
                F = Q.enumerate_cdf(lp, labels, term, beam, mm, cuts)
            if V is None:
                assert F is None and term not in B.live_terminals(lp, labels, table, beam, mm), what
                seen_dead += 1
                continue
            seen_live += 1
            v = B2.visits(lp, labels, term, table, beam, mm)
            np.testing.assert_allclose(v["V"], V, rtol=0, atol=1e-12, err_msg=str(what))
            np.testing.assert_allclose(v["X"], X, rtol=0, atol=1e-11, err_msg=str(what))
            held = B2.held_positions(table, L, beam)
            assert np.all(v["V"][~held] == 0.0) and np.all(v["V"][:int(table[0])] == 0.0) and abs(v["V"][term] - 1.0) < 1e-12, what
            q = B2.quantiles(lp, labels, term, table, beam, mm, cuts, LEVELS, gamma=v["gamma"])
            np.testing.assert_allclose(q["F"], F, rtol=0, atol=1e-12, err_msg=str(what))
            assert np.all(q["F"][:, cuts <= table[0]] == 1.0), what                # a cut at or below lo_0: crossed from frame 0 on
            gamma = [g for _, g in v["gamma"]]
            m = B2.mea_reference(v["ref"], labels, term, table, beam, mm)
            value, path = M.brute_force(gamma, lo, hi, labels, term, mm)
            assert m["status"] == R.OK and np.array_equal(m["path"], path) and abs(m["value"] - value) < 1e-12, what
            assert M.validity(m["path"], lo, hi, labels, term, mm) is None and m["path"][0] >= table[0], what
            if i % 4 == 0 and term == int(hi[-1]) - 1:                               # sample frequencies: a quarter of the tables
                with B.under_table(table):
                    want = SR.path_probabilities(lp, labels, term, beam, mm)
                lat = B2.sample_lattice(lp, labels, table, beam, mm)
                counts, n = {}, 0
                for seed in range(80):                                               # 80 x 64 = 5120 samples
                    for row in B2.sample_paths(lp, labels, term, 64, 9000 + seed, table, beam, mm, lattice=lat):
                        key = tuple(int(x) for x in row)
                        counts[key] = counts.get(key, 0) + 1
                        n += 1
                assert set(counts) <= set(want), (what, "a sampled path is not a path of the table's band")
                for p_, pr in want.items():                                          # five standard errors of a binomial share
                    assert abs(counts.get(p_, 0) / n - pr) <= 5.0 * np.sqrt(pr * (1.0 - pr) / n) + 1e-12, (what, p_)
                seen_sampled += 1
    assert seen_lo0 >= 10 and seen_live >= 40 and seen_dead >= 5 and seen_sampled >= 4, (seen_lo0, seen_live, seen_dead, seen_sampled)


# ---------------------------------------------------------------------------------------
# the plantable faults, each on its case
# ---------------------------------------------------------------------------------------
def _rows_of(name, term):
    lp, labels, table, beam, mm = B2.case(name)
    L = 2 * len(labels) + 1
    ref = B.ref_at(lp, labels, term, table, beam, mm)
    assert ref["status"] == R.OK
    with B.under_table(table):
        rows, lo = Q.float32_rows(ref["gamma"], max(1, min(beam, L)))
    assert np.array_equal(lo, table)
    return rows


def test_fault_mea_late_table_moves_the_staircase_and_a_step_at_a_block_edge():
    for name in ("staircase", "step5_at32"):
        lp, labels, table, beam, mm = B2.case(name)
        term = B2.live(name)[0]                                              # (the terminal with the most mass)
        rows = _rows_of(name, term)
        good = B2.mea_replay(rows, table, labels, term, beam, mm)
        bad = B2.mea_replay(rows, table, labels, term, beam, mm, fault="mea_late_table")
        lo, hi = B.table_windows(table, 2 * len(labels) + 1, beam)
        assert good["status"] == R.OK and M.validity(good["path"], lo, hi, labels, term, mm) is None, name
        assert bad["status"] != R.OK or not np.array_equal(bad["path"], good["path"]), name


def test_faults_of_the_quantile_start_frame_show_on_lo2_and_the_staircase():
    for name, cut in (("lo2", 2), ("staircase", None)):
        lp, labels, table, beam, mm = B2.case(name)
        L = 2 * len(labels) + 1
        term = B2.live(name)[-1]
        rows = _rows_of(name, term)
        cuts = np.arange(0, L + 1)
        good = B2.integer_quantiles(rows, table, cuts, LEVELS, L, beam)
        gt = B2.integer_quantiles(rows, table, cuts, LEVELS, L, beam, fault="start_gt")
        assert not np.array_equal(good, gt), name
        assert np.all(good[cuts <= table[0]] == 0), name
        if cut is not None:                                                  # lo = 2 throughout: cut 2 is crossed at frame 0, and never with >
            assert good[cut].tolist() == [0, 0, 0] and gt[cut].tolist() == [70, 70, 70]
    lp, labels, table, beam, mm = B2.case("lo2")
    L = 2 * len(labels) + 1
    rows = _rows_of("lo2", B2.live("lo2")[-1])
    cuts = np.arange(0, L + 1)
    zero_only = B2.integer_quantiles(rows, table, cuts, LEVELS, L, beam, fault="start_zero_only")
    assert zero_only[0].tolist() == [0, 0, 0] and zero_only[1].tolist() == [70, 70, 70] and zero_only[2].tolist() == [70, 70, 70]
    assert np.array_equal(zero_only[3:], B2.integer_quantiles(rows, table, cuts, LEVELS, L, beam)[3:])


def test_fault_prev_band_moves_a_draw_at_a_blocks_first_frame():
    lp, labels, table, beam, mm = B2.case("step5_at32")                      # lo: 0 up to frame 31, 5 from frame 32, a block's first
    assert table[31] == 0 and table[32] == 5 and 32 % R.CK == 0
    term = B2.live("step5_at32")[-1]
    assert term == 5                                                         # every path stands at 5 at frame 32, the band's low end
    lat = B2.sample_lattice(lp, labels, table, beam, mm)
    good = B2.sample_paths(lp, labels, term, 64, B2.SAMPLER_SEED, table, beam, mm, lattice=lat)
    bad = B2.sample_paths(lp, labels, term, 64, B2.SAMPLER_SEED, table, beam, mm, fault="prev_band", lattice=lat)
    assert all(SR.valid_path(lat, row, term) is None for row in good)
    assert np.array_equal(good[:, 32:], bad[:, 32:]) and not np.array_equal(good[:, 31], bad[:, 31])
    assert np.all(bad[:, 31] >= 5) and np.any(good[:, 31] < 5)               # the faulty draw never leaves the band of frame 32
    wrong, _ = SR.check_draws(lat, bad, B2.SAMPLER_SEED, term)
    assert any(f == 31 for _, f, _, _ in wrong)


def test_faults_are_refused_by_name():
    rows = np.zeros((3, 2), np.float32)
    with pytest.raises(AssertionError):
        B2.integer_quantiles(rows, np.zeros(3, np.int64), [0], LEVELS, 3, 2, fault="nope")
    with pytest.raises(AssertionError):
        B2.mea_replay(rows, np.zeros(3, np.int64), np.array([1], np.int32), 0, 2, 4, fault="nope")


# ---------------------------------------------------------------------------------------
# the rescue case: quantiles and the MEA path from a band that does not hold the path
# ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", range(6))
def test_rescue_case(seed):
    lp, labels, L, beam, pre = C.rescue(seed)
    T = lp.shape[0]
    true = np.zeros(T, np.int64)
    true[pre:] = (np.arange(T - pre) * (L - 1)) // (T - pre - 1)
    anchored, diagonal = ka.anchored_band(T, L, [(pre, 0)], beam), ka.diagonal_band(T, L, beam)
    ref = B.ref_at(lp, labels, L - 1, anchored, beam, 4)
    q = B2.quantiles(lp, labels, L - 1, anchored, beam, 4, [1], LEVELS, gamma=ref["gamma"])
    assert q["q"][0].tolist() == [98, 98, 98] and not q["unsafe"].any()
    m = B2.mea_reference(ref, labels, L - 1, anchored, beam, 4)
    assert m["status"] == R.OK and np.array_equal(m["path"], true)                       # all 240 frames
    assert np.array_equal(band_ref.best_path_banded(lp, labels, anchored, beam, 4)[0], true)
    dref = B.ref_at(lp, labels, L - 1, diagonal, beam, 4)
    qd = B2.quantiles(lp, labels, L - 1, diagonal, beam, 4, [1], LEVELS, gamma=dref["gamma"])
    assert qd["q"][0, 1] < 10                                                            # the median of cut 1 under the diagonal
    md = B2.mea_reference(dref, labels, L - 1, diagonal, beam, 4)
    assert int(np.sum(md["path"] == true)) < 60


# ---------------------------------------------------------------------------------------
# tables that leave no path
# ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", B2.NO_PATH)
def test_tables_without_a_best_path_are_zero_mass_for_every_terminal(name):
    lp, labels, table, beam, mm = C.case(name)
    L = 2 * len(labels) + 1
    assert B2.live(name) == []
    lat = B2.sample_lattice(lp, labels, table, beam, mm)
    assert not np.any(np.isfinite(lat.alpha[-1]))                                        # no terminal for the sampler to start from
    lo, hi = B.table_windows(table, L, beam)
    for term in (int(lo[-1]), int(hi[-1]) - 1, 0, L - 1):
        assert B.ref_at(lp, labels, term, table, beam, mm)["status"] == R.ZERO_MASS, (name, term)


# ---------------------------------------------------------------------------------------
# the sampler's caps: conditions, stated on the reference's own paths over the inputs the GPU test uses
# ---------------------------------------------------------------------------------------
def test_the_references_own_paths_stay_within_the_undecidable_caps():
    total = draws = 0
    for name, term in B2.sampler_inputs():
        lp, labels, table, beam, mm = B2.case(name)
        lat = B2.sample_lattice(lp, labels, table, beam, mm)
        paths = B2.sample_paths(lp, labels, term, B2.SAMPLER_K, B2.SAMPLER_SEED, table, beam, mm, lattice=lat)
        wrong, ties = SR.check_draws(lat, paths, B2.SAMPLER_SEED, term)
        assert wrong == [] and ties <= B2.MAX_UNDECIDABLE_PER_CASE, (name, term, ties)
        assert all(SR.valid_path(lat, row, term) is None for row in paths[:4]), (name, term)
        total += ties
        draws += B2.SAMPLER_K * (lat.T - 1)
    print("undecidable draws of the reference:", total, "of", draws)
    assert draws == 268224 and total <= B2.MAX_UNDECIDABLE_SHARE * draws


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
    assert L.ka_version() == 104


def test_the_two_workspace_figures():
    from kokoro_align_amd import _lib
    L = _lib.load_library()
    arr = lambda xs: (ctypes.c_int64 * len(xs))(*xs)
    up = lambda x: (x + 255) // 256 * 256
    for fn, per in ((L.ka_band_table_workspace_bytes, 144), (L.ka_boundary_quantile_band_table_workspace_bytes, 160)):
        ws = lambda n, Ts, mem: fn(n, arr(Ts) if Ts is not None else None, mem)
        assert ws(1, [240], _lib.KA_MEM_DEVICE) == up(per)
        assert ws(1, [240], _lib.KA_MEM_HOST) == up(per) + 1024
        assert ws(3, [1, 64, 65], _lib.KA_MEM_HOST) == up(3 * per) + 256 + 256 + 512
        assert ws(768, [10000] * 768, _lib.KA_MEM_DEVICE) == up(768 * per)
        assert ws(2, [5, 0], 0) == 0 and ws(-1, [5], 0) == 0 and ws(1, [5], 7) == 0 and ws(1, None, 0) == 0 and ws(0, None, 0) == 0
    # the sibling's figure for the banded quantile call: it uploads cuts only, so the sibling's bytes still bound it
    assert L.ka_boundary_quantile_band_table_workspace_bytes(16, arr([100] * 16), 0) > L.ka_band_table_workspace_bytes(16, arr([100] * 16), 0)


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
    own = dict(state_visits=lambda P, kw: P.ctc_state_visits_batch([lp], [labels], [L - 1], beam, 4, **kw),
               boundary_quantiles=lambda P, kw: P.ctc_boundary_quantiles_batch([lp], [labels], [L - 1], [[0, 3]], LEVELS, beam, 4, **kw),
               sample_paths=lambda P, kw: P.ctc_sample_paths_batch([lp], [labels], [L - 1], 5, 9, beam, 4, **kw),
               mea_path=lambda P, kw: P.ctc_mea_path_batch([lp], [labels], [L - 1], beam, 4, **kw))[call]
    name, args = _recorded(lambda P: own(P, {}))
    assert name == f"ka_ctc_{call}_batch_f32"
    name_none, args_none = _recorded(lambda P: own(P, dict(band_lo=None)))
    assert name_none == name and len(args_none) == len(args)
    table = ka.diagonal_band(T, L, beam)
    name_b, args_b = _recorded(lambda P: own(P, dict(band_lo=[table])))
    assert name_b == f"ka_ctc_{call}_banded_batch_f32" and len(args_b) == len(args) + 1
    assert args_b[8:10] == args[8:10] == (beam, 4)                          # the table sits directly behind max_move
    sent = np.ctypeslib.as_array(ctypes.cast(ctypes.c_void_p(args_b[10][0]), ctypes.POINTER(ctypes.c_int32)), shape=(T,))
    assert np.array_equal(sent, table)                                      # int64 in, int32 out
    with pytest.raises(ValueError):
        _recorded(lambda P: own(P, dict(band_lo=[table[:-1]])))
    with pytest.raises(ValueError):
        _recorded(lambda P: own(P, dict(band_lo=[table, table])))


def test_the_twelve_functions_take_band_lo_last():
    from kokoro_align_amd import posteriors as P
    for name in ("ctc_state_visits", "ctc_boundary_quantiles", "ctc_sample_paths", "ctc_mea_path"):
        for form in ("", "_batch", "_device"):
            params = list(inspect.signature(getattr(P, name + form)).parameters.values())
            assert params[-1].name == "band_lo" and params[-1].default is None, name + form
