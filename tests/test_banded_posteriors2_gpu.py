"""State visits, boundary quantiles, sampled paths and the MEA path over a caller-given band on the GPU (DESIGN.md section
4.31), through the raw C ABI (tests/banded_fb2_harness.py) and, at the end, through the Python front end.

1. with the diagonal as the table every banded call returns its sibling's bits; 2. tables: the visits against the float64
reference of tests/banded_fb2_ref.py within the diagonal call's model and margin, the quantiles and the MEA path bit for bit
against their integer definitions on the rows of ka_ctc_state_posteriors_banded, every sampled draw against the reference's
choice on the kernel's own states; 3. zero-mass, invalid and NULL tables; 4. more lattices than slots; 5. Python."""
import numpy as np
import pytest

import band_cases as C
import banded_fb2_harness as H2
import banded_fb2_ref as B2
import banded_fb_harness as BH
import banded_fb_ref as B
import fb_harness as H
import mea_ref as M
import posterior_ref as R
import sample_ref as SR
import visit_ref as VR

pytestmark = pytest.mark.gpu

KINDS = H2.KINDS
LEVELS = H2.LEVELS
OK, BAD_ARGS, ZERO_MASS = 0, -2, -9
GENERIC_V = 65                      # above 64 columns the kernels take their generic form
SEED = B2.SAMPLER_SEED


@pytest.fixture(scope="module")
def env():
    return H.engine()


def _generic(lp):
    return R.pad_vocabulary(lp, GENERIC_V)


def _own(kind, terms, Ls, K=64, seed=SEED):
    """The own input of a batch, as H2.run takes it: every cut of [0, L] for the quantiles."""
    terms = [int(t) for t in terms]
    if kind == "boundary_quantiles":
        return (terms, [np.arange(0, L + 1) for L in Ls])
    if kind == "sample_paths":
        return (terms, [K] * len(terms), [seed] * len(terms))
    return terms


def _assert_failed(got, i, kind, status, what=None):
    assert got.st[i] == status, (kind, i, what)
    assert got.ll[i] == -np.inf if status == ZERO_MASS else np.isnan(got.ll[i]), (kind, i, what)
    for out in got.outs[i]:
        assert np.all(out == -1) if out.dtype == np.int32 else np.all(np.isnan(out)), (kind, i, what)
    if kind == "mea_path":
        assert np.isnan(got.ea[i]), (kind, i, what)


# ---------------------------------------------------------------------------------------
# 1. the diagonal as the table: the sibling's bits
# ---------------------------------------------------------------------------------------
def _identity_lattice(name):
    if name == "ring_wrap":
        lp, labels, _, beam, mm = C.case("ring_wrap")
        return lp, labels, beam
    if name == "zero_ninf":
        lp, labels = H.tiny(np.random.default_rng(77), 70, 40, 8, zero_label=True, ninf=True)
        return lp, labels, 24
    lp, labels = C.random_lattice(50 + int(name[1:]), int(name[1:]), 40)
    return lp, labels, 24


IDENTITY = [(n, form, 4) for n in ("T1", "T32", "T33", "T70", "ring_wrap", "zero_ninf") for form in ("fast", "generic")] + [("T70", "fast", 5)]


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
@pytest.mark.parametrize("name,form,mm", IDENTITY)
def test_diagonal_table_gives_the_siblings_bits(env, name, form, mm, device):
    import kokoro_align_amd as ka
    _, _lib, eng = env
    lp, labels, beam = _identity_lattice(name)
    T, L = lp.shape[0], 2 * len(labels) + 1
    live = R.live_terminals(lp, labels, beam, mm)
    assert live, name
    term = live[0]
    table = ka.diagonal_band(T, L, beam)
    x = _generic(lp) if form == "generic" else lp
    assert R.fast_form(len(labels), x.shape[1], beam, mm) == (form == "fast" and mm <= 4)
    for kind in KINDS:
        for K in ((1, 7, 64) if kind == "sample_paths" else (64,)):
            own = _own(kind, [term], [L], K=K)
            plain = H2.run(eng, _lib, kind, [x], [labels], own, beam, mm, device=device)
            banded = H2.run(eng, _lib, kind, [x], [labels], own, beam, mm, tables=[table], device=device)
            assert plain.rc == OK and plain.st[0] == OK, (kind, plain.rc)
            assert banded.same_bits(plain), (kind, K)
            assert banded.guards_intact() and plain.guards_intact(), kind


# ---------------------------------------------------------------------------------------
# 2. tables
# ---------------------------------------------------------------------------------------
GENERIC_AGAIN = ("staircase", "ninf", "ring_wrap", "step1009", "step159")
TABLE_CASES = [(n, "fast") for n in B2.names_with_path() + list(B2.EXTRA)] + [(n, "generic") for n in GENERIC_AGAIN]
_terms, _vrefs, _lats, _sampled = {}, {}, {}, {}


def terminals(name):
    """Two terminals of a case (the one with the most mass and the one with the least; one where only one is live)."""
    if name not in _terms:
        live = B2.live(name)
        assert live, name
        _terms[name] = list(dict.fromkeys((live[0], live[-1])))
    return _terms[name]


def visit_ref(name, term):
    if (name, term) not in _vrefs:
        lp, labels, table, beam, mm = B2.case(name)
        _vrefs[name, term] = B2.visits(lp, labels, term, table, beam, mm)
    return _vrefs[name, term]


def sample_lattice(name):
    if name not in _lats:
        lp, labels, table, beam, mm = B2.case(name)
        _lats[name] = B2.sample_lattice(lp, labels, table, beam, mm)
    return _lats[name]


def sampled(env, name, form, term):
    """(paths [64, T] of the banded sampler, wrong draws, undecidable draws) of one input: run and checked once."""
    key = (name, form, term)
    if key not in _sampled:
        _, _lib, eng = env
        lp, labels, table, beam, mm = B2.case(name)
        x = _generic(lp) if form == "generic" else lp
        got = H2.run(eng, _lib, "sample_paths", [x], [labels], ([term], [B2.SAMPLER_K], [SEED]), beam, mm, tables=[table])
        assert got.rc == OK and got.guards_intact(), key
        paths = got.outs[0][0]
        wrong, ties = SR.check_draws(sample_lattice(name), paths, SEED, term)
        _sampled[key] = (paths, wrong, ties, got.ll[0])
    return _sampled[key]


@pytest.mark.parametrize("name,form", TABLE_CASES)
def test_tables(env, name, form):
    _, _lib, eng = env
    lp, labels, table, beam, mm = B2.case(name)
    T, L = lp.shape[0], 2 * len(labels) + 1
    x = _generic(lp) if form == "generic" else lp
    assert R.fast_form(len(labels), x.shape[1], beam, mm) == (form == "fast")
    terms = terminals(name)
    n = len(terms)
    xs, labs, tabs, Ls = [x] * n, [labels] * n, [table] * n, [L] * n
    lo, hi = B.table_windows(table, L, beam)
    held = B2.held_positions(table, L, beam)
    cuts = np.arange(0, L + 1)
    what = (name, form)
    every = np.arange(T, dtype=np.int64)
    st = BH.run(eng, _lib, "state_posteriors", xs, labs, (terms, [every] * n), beam, mm, tables=tabs)
    du = BH.run(eng, _lib, "state_durations", xs, labs, terms, beam, mm, tables=tabs)
    assert st.rc == OK and du.rc == OK, what

    vi = H2.run(eng, _lib, "state_visits", xs, labs, _own("state_visits", terms, Ls), beam, mm, tables=tabs)
    assert vi.rc == OK and vi.guards_intact(), what
    for i, term in enumerate(terms):
        ref = visit_ref(name, term)
        visit, exit_time = vi.outs[i]
        dur, tsum = du.outs[i]
        H.record("banded_visit", VR.visit_ratio(visit, ref["V"], ref["E_V"], what), VR.M_VISIT)
        H.record("banded_exit_time", VR.visit_ratio(exit_time, ref["X"], ref["E_X"], what), VR.M_VISIT)
        assert np.all(visit <= dur) and np.all(exit_time <= tsum), what
        assert visit[term] == 1.0, what
        for out in (visit, exit_time):
            dead = ~held | (np.arange(L) > term) | (np.arange(L) < int(table[0]))
            assert np.all(out[dead] == 0.0) and not np.any(np.signbit(out[dead])), what
        assert vi.ll[i].tobytes() == du.ll[i].tobytes(), what

    qu = H2.run(eng, _lib, "boundary_quantiles", xs, labs, _own("boundary_quantiles", terms, Ls), beam, mm, tables=tabs)
    assert qu.rc == OK and qu.guards_intact(), what
    for i, term in enumerate(terms):
        rows, blo = st.outs[i]
        assert np.array_equal(blo, np.asarray(table, np.int64)), what
        want = B2.integer_quantiles(rows, table, cuts, LEVELS, L, beam)
        got = qu.outs[i][0]
        assert np.array_equal(got, want), (what, term, np.argwhere(got != want)[:5].tolist())
        assert np.all(got[cuts <= table[0]] == 0), what                          # c <= lo_0 reads 0 at every level
        never = cuts >= hi[-1]                                                   # above every band: never crossed
        assert np.all(got[never] == T), what
        first = np.searchsorted(np.asarray(table), cuts, side="left")            # the first t with lo_t >= c, T if none
        assert np.all(got <= first[:, None]), what
        assert qu.ll[i].tobytes() == du.ll[i].tobytes(), what
        ref = visit_ref(name, term)
        q = B2.quantiles(lp, labels, term, table, beam, mm, cuts, LEVELS, gamma=ref["gamma"])
        safe = ~q["unsafe"]                                                      # (pairs within the margin are left out)
        assert np.array_equal(got[safe], q["q"][safe]), what

    me = H2.run(eng, _lib, "mea_path", xs, labs, _own("mea_path", terms, Ls), beam, mm, tables=tabs)
    assert me.rc == OK and me.guards_intact(), what
    for i, term in enumerate(terms):
        rows, _ = st.outs[i]
        want = B2.mea_replay(rows, table, labels, term, beam, mm)
        path = me.outs[i][0]
        assert want["status"] == R.OK and np.array_equal(path, want["path"]), (what, term)
        assert np.float64(me.ea[i]).tobytes() == np.float64(want["value"]).tobytes(), (what, term)
        assert M.validity(path, lo, hi, labels, term, mm) is None, (what, term)
        assert me.ll[i].tobytes() == du.ll[i].tobytes(), what

    lat = sample_lattice(name)
    for i, term in enumerate(terms):
        paths, wrong, ties, z = sampled(env, name, form, term)
        assert wrong == [], (what, term, wrong[:5])
        assert ties <= B2.MAX_UNDECIDABLE_PER_CASE, (what, term, ties)
        for k, row in enumerate(paths):
            assert SR.valid_path(lat, row, term) is None, (what, term, k)
        assert np.float64(z).tobytes() == du.ll[i].tobytes(), what


def test_the_samplers_undecidable_draws_stay_within_the_caps(env):
    total = draws = 0
    for name, term in B2.sampler_inputs():
        paths, wrong, ties, _ = sampled(env, name, "fast", term)
        assert wrong == [] and ties <= B2.MAX_UNDECIDABLE_PER_CASE, (name, term, ties)
        total += ties
        draws += paths.shape[0] * (paths.shape[1] - 1)
    print("undecidable draws of the kernels:", total, "of", draws)
    assert draws == 268224 and total <= B2.MAX_UNDECIDABLE_SHARE * draws


@pytest.mark.parametrize("form", ["fast", "generic"])
def test_a_sample_has_the_same_bits_alone_in_a_batch_and_for_any_n_samples(env, form):
    _, _lib, eng = env
    names = ("staircase", "step5_at32", "lo2")
    cases = [B2.case(n) for n in names]
    assert len({(c[3], c[4]) for c in cases[1:]}) == 1
    full = {}
    for name, (lp, labels, table, beam, mm) in zip(names, cases):
        x = _generic(lp) if form == "generic" else lp
        term = terminals(name)[0]
        full[name] = sampled(env, name, form, term)[0]
        for K in (1, 7):
            got = H2.run(eng, _lib, "sample_paths", [x], [labels], ([term], [K], [SEED]), beam, mm, tables=[table])
            assert got.rc == OK and got.guards_intact() and np.array_equal(got.outs[0][0], full[name][:K]), (name, K)
        one = H2.single(eng, _lib, "sample_paths", x, labels, (term, 7, SEED), beam, mm, table)
        assert one[2] == OK and np.array_equal(one[0][0], full[name][:7]), name
    # the two T = 70 lattices (one beam and max_move) in one batch, with n_samples of their own
    (lp1, lab1, tab1, beam, mm), (lp2, lab2, tab2, _, _) = cases[1], cases[2]
    xs = [_generic(lp) if form == "generic" else lp for lp in (lp1, lp2, lp1)]
    t1, t2 = terminals(names[1])[0], terminals(names[2])[0]
    got = H2.run(eng, _lib, "sample_paths", xs, [lab1, lab2, lab1], ([t1, t2, t1], [64, 7, 1], [SEED] * 3), beam, mm, tables=[tab1, tab2, tab1])
    assert got.rc == OK and got.guards_intact()
    assert np.array_equal(got.outs[0][0], full[names[1]]) and np.array_equal(got.outs[1][0], full[names[2]][:7])
    assert np.array_equal(got.outs[2][0], full[names[1]][:1])


# ---------------------------------------------------------------------------------------
# 3. failures
# ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", ["fast", "generic"])
@pytest.mark.parametrize("name", B2.NO_PATH)
def test_tables_that_leave_no_path_are_zero_mass(env, name, form):
    _, _lib, eng = env
    lp, labels, table, beam, mm = C.case(name)
    L = 2 * len(labels) + 1
    term = min(int(table[-1]) + beam, L) - 1
    x = _generic(lp) if form == "generic" else lp
    for kind in KINDS:
        got = H2.run(eng, _lib, kind, [x], [labels], _own(kind, [term], [L]), beam, mm, tables=[table])
        assert got.rc == ZERO_MASS and got.guards_intact(), (name, kind)
        _assert_failed(got, 0, kind, ZERO_MASS, name)


def _invalid(table, L, how):
    bad = np.asarray(table, np.int64).copy()
    T = len(bad)
    if how == "decreasing":
        assert bad[T // 2 - 1] > 0
        bad[T // 2] = bad[T // 2 - 1] - 1                                     # (one step down, inside [0, L))
    elif how == "negative":
        bad[0] = -1
    else:
        bad[-1] = L
    return bad


INVALID = ("decreasing", "negative", "too_high")


@pytest.mark.parametrize("form", ["fast", "generic"])
def test_invalid_tables_alone_and_in_a_batch(env, form):
    import kokoro_align_amd as ka
    _, _lib, eng = env
    T, S, beam, mm = 70, 40, 24, 4
    L = 2 * S + 1
    n = 15
    lats = [C.random_lattice(400 + i, T, S) for i in range(n)]
    xs = [_generic(lp) if form == "generic" else lp for lp, _ in lats]
    labs = [lab for _, lab in lats]
    good = [np.minimum(ka.diagonal_band(T, L, beam) + i % 3, L - 1) for i in range(n)]
    terms = [B.live_terminals(lp, lab, tb, beam, mm)[0] for (lp, lab), tb in zip(lats, good)]
    tabs = list(good)
    for i in range(0, n, 7):                                                 # every seventh lattice: 0, 7, 14
        tabs[i] = _invalid(good[i], L, INVALID[(i // 7) % 3])
        assert tabs[i].min() < 0 or tabs[i].max() >= L or np.any(np.diff(tabs[i]) < 0)
    for kind in KINDS:
        batch = H2.run(eng, _lib, kind, xs, labs, _own(kind, terms, [L] * n, K=5), beam, mm, tables=tabs)
        assert batch.rc == BAD_ARGS and batch.guards_intact(), kind
        for i in range(n):
            alone = H2.run(eng, _lib, kind, [xs[i]], [labs[i]], _own(kind, [terms[i]], [L], K=5), beam, mm, tables=[tabs[i]])
            assert alone.guards_intact(), (kind, i)
            if i % 7 == 0:
                assert alone.rc == BAD_ARGS, (kind, i)
                _assert_failed(alone, 0, kind, BAD_ARGS)
                _assert_failed(batch, i, kind, BAD_ARGS)
            else:                                                            # the neighbours are answered, with their own bits
                assert alone.rc == OK and batch.st[i] == OK, (kind, i)
                assert batch.ll[i].tobytes() == alone.ll[0].tobytes(), (kind, i)
                assert all(a.tobytes() == b.tobytes() for a, b in zip(batch.outs[i], alone.outs[0])), (kind, i)
                assert kind != "mea_path" or batch.ea[i].tobytes() == alone.ea[0].tobytes(), i


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
def test_null_table_fails_before_launch(env, device):
    _, _lib, eng = env
    lp, labels = C.random_lattice(9, 40, 12)
    table = np.zeros(40, np.int64)
    for kind in KINDS:
        own = _own(kind, [24, 24], [25, 25], K=3)
        for null in ("array", 1):
            got = H2.run(eng, _lib, kind, [lp, lp], [labels, labels], own, 16, 4, tables=[table, table], device=device, null_table=null)
            assert got.rc == BAD_ARGS and np.all(got.st == 99) and np.all(got.ll == 0.0), (kind, null)
            assert got.guards_intact(), (kind, null)
            for outs in got.outs:                                            # nothing was written at all
                assert all(np.all(o == BH.SENTINEL) for o in outs), (kind, null)
            assert got.ea is None or np.all(got.ea == BH.SENTINEL), (kind, null)


# ---------------------------------------------------------------------------------------
# 4. more lattices than slots, each with a table of its own
# ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("form,n", [("fast", 1030), ("generic", 520)])     # kOccFastSlots = 1024, kOccGenericSlots = 512
def test_more_lattices_than_slots(env, form, n):
    _, _lib, eng = env
    T, S, beam, mm = 40, 12, 8, 4
    L = 2 * S + 1
    rng = np.random.default_rng(5)
    # seven distinct (lattice, table, terminal) triples, lattice i the triple i mod 7: a slot's second lattice (i + slots) is
    # another triple than its first, since neither 1024 nor 512 is a multiple of 7
    triples = []
    for k in range(7):
        lp, labels = C.random_lattice(600 + k, T, S)
        table = B.random_table(rng, T, L, max_step=1, lo0=k % 3)
        live = B.live_terminals(lp, labels, table, beam, mm)
        assert live, k
        triples.append((_generic(lp) if form == "generic" else lp, labels, table, live[0]))
    pick = [triples[i % 7] for i in range(n)]
    for kind in KINDS:
        singles = [H2.run(eng, _lib, kind, [p[0]], [p[1]], _own(kind, [p[3]], [L], K=3), beam, mm, tables=[p[2]]) for p in triples]
        assert all(s.rc == OK for s in singles), kind
        batch = H2.run(eng, _lib, kind, [p[0] for p in pick], [p[1] for p in pick], _own(kind, [p[3] for p in pick], [L] * n, K=3), beam, mm,
                       tables=[p[2] for p in pick])
        assert batch.rc == OK and batch.guards_intact(), kind
        for i in range(n):
            one = singles[i % 7]
            assert batch.ll[i].tobytes() == one.ll[0].tobytes(), (kind, i)
            assert all(a.tobytes() == b.tobytes() for a, b in zip(batch.outs[i], one.outs[0])), (kind, i)
            assert kind != "mea_path" or batch.ea[i].tobytes() == one.ea[0].tobytes(), i


def test_the_siblings_figure_plus_the_add_on_keeps_a_call_free_of_allocations(env):
    import ctypes
    import torch
    _, _lib, eng = env
    lp, labels, table, beam, mm = B2.case("staircase")
    T, S, L, V = lp.shape[0], len(labels), 2 * len(labels) + 1, lp.shape[1]
    arr = lambda xs: (ctypes.c_int64 * len(xs))(*xs)
    term = terminals("staircase")[0]
    lib = eng.lib
    for mem, device in ((_lib.KA_MEM_HOST, False), (_lib.KA_MEM_DEVICE, True)):
        add_on = lib.ka_band_table_workspace_bytes(1, arr([T]), mem)
        add_on_q = lib.ka_boundary_quantile_band_table_workspace_bytes(1, arr([T]), mem)
        assert add_on_q >= add_on > 0
        figure = dict(state_visits=lib.ka_state_visit_workspace_bytes(1, arr([T]), arr([S]), V, beam, mm, mem) + add_on,
                      boundary_quantiles=lib.ka_boundary_quantile_workspace_bytes(1, arr([T]), arr([S]), arr([L + 1]), 3, V, beam, mm, mem) + add_on_q,
                      sample_paths=lib.ka_sample_paths_workspace_bytes(1, arr([T]), arr([S]), (ctypes.c_int32 * 1)(64), V, beam, mm, mem) + add_on,
                      mea_path=lib.ka_mea_path_workspace_bytes(1, arr([T]), arr([S]), V, beam, mm, mem) + add_on)
        for kind in KINDS:
            assert figure[kind] > add_on_q, kind
            own = _own(kind, [term], [L])
            # (once on the shared engine: the kernels' code is on the device, and torch holds the harness's tensors, before memory is counted)
            want = H2.run(eng, _lib, kind, [lp], [labels], own, beam, mm, tables=[table], device=device)
            fresh = _lib.Engine(torch.cuda.current_device())
            try:
                fresh.reserve(figure[kind])
                torch.cuda.synchronize()
                free0 = torch.cuda.mem_get_info()[0]
                got = H2.run(fresh, _lib, kind, [lp], [labels], own, beam, mm, tables=[table], device=device)
                assert got.rc == OK and torch.cuda.mem_get_info()[0] == free0, (kind, mem)
                assert got.same_bits(want), (kind, mem)
            finally:
                fresh.close()


# ---------------------------------------------------------------------------------------
# 5. Python
# ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", range(6))
def test_rescue_case_through_python(env, seed):
    ka, _, _ = env
    lp, labels, L, beam, pre = C.rescue(seed)
    T = lp.shape[0]
    anchored = ka.anchored_band(T, L, [(pre, 0)], beam)
    best = ka.ctc_best_path_banded(lp, labels, anchored, beam, 4)[0]
    quant, z_q = ka.ctc_boundary_quantiles(lp, labels, L - 1, [1], LEVELS, beam, 4, band_lo=anchored)
    assert quant[0].tolist() == [98, 98, 98]
    path, ea, z_m = ka.ctc_mea_path(lp, labels, L - 1, beam, 4, band_lo=anchored)
    assert np.array_equal(path, best) and ea > 0.9 * T and z_m == z_q
    paths, z_s = ka.ctc_sample_paths(lp, labels, L - 1, 64, 1, beam, 4, band_lo=anchored)
    lat = B2.sample_lattice(lp, labels, anchored, beam, 4)
    assert all(SR.valid_path(lat, row, L - 1) is None for row in paths) and z_s == z_q
    visit, exit_time, z_v = ka.ctc_state_visits(lp, labels, L - 1, beam, 4, band_lo=anchored)
    assert visit[0] == 1.0 or visit[0] > 0.99
    assert z_v == z_q
    plain, _ = ka.ctc_boundary_quantiles(lp, labels, L - 1, [1], LEVELS, beam, 4)
    diag, _ = ka.ctc_boundary_quantiles(lp, labels, L - 1, [1], LEVELS, beam, 4, band_lo=ka.diagonal_band(T, L, beam))
    assert np.array_equal(plain, diag) and plain[0, 1] < 10


def test_batch_and_device_forms_equal_the_raw_call(env):
    import torch
    ka, _lib, eng = env
    lp, labels, L, beam, pre = C.rescue(1)
    T = lp.shape[0]
    table = ka.anchored_band(T, L, [(pre, 0)], beam)
    term = L - 1
    cuts = np.arange(0, L + 1, 7)
    d_lp, d_lab, d_tab = torch.from_numpy(lp).cuda(), torch.from_numpy(labels).cuda(), torch.from_numpy(table).cuda()
    raw = {k: H2.run(eng, _lib, k, [lp], [labels], own, beam, 4, tables=[table])
           for k, own in (("state_visits", [term]), ("boundary_quantiles", ([term], [cuts])), ("sample_paths", ([term], [9], [3])), ("mea_path", [term]))}
    assert all(r.rc == OK for r in raw.values())
    host = dict(state_visits=ka.ctc_state_visits_batch([lp], [labels], [term], beam, 4, band_lo=[table])[0],
                boundary_quantiles=ka.ctc_boundary_quantiles_batch([lp], [labels], [term], [cuts], LEVELS, beam, 4, band_lo=[table])[0],
                sample_paths=ka.ctc_sample_paths_batch([lp], [labels], [term], 9, 3, beam, 4, band_lo=[table])[0],
                mea_path=ka.ctc_mea_path_batch([lp], [labels], [term], beam, 4, band_lo=[table])[0])
    dev = dict(state_visits=ka.ctc_state_visits_device([d_lp], [d_lab], [term], beam, 4, band_lo=[d_tab])[0],
               boundary_quantiles=ka.ctc_boundary_quantiles_device([d_lp], [d_lab], [term], [cuts], LEVELS, beam, 4, band_lo=[d_tab])[0],
               sample_paths=ka.ctc_sample_paths_device([d_lp], [d_lab], [term], 9, 3, beam, 4, band_lo=[d_tab])[0],
               mea_path=ka.ctc_mea_path_device([d_lp], [d_lab], [term], beam, 4, band_lo=[d_tab])[0])
    for kind in KINDS:
        outs = raw[kind].outs[0]
        for res in (host[kind], dev[kind]):
            for a, b in zip(outs, res):
                b = b.cpu().numpy() if torch.is_tensor(b) else np.asarray(b)
                assert a.tobytes() == b.tobytes(), kind
            assert res[-1] == raw[kind].ll[0], kind
        if kind == "mea_path":
            assert host[kind][1] == dev[kind][1] == raw[kind].ea[0]
    one = ka.ctc_mea_path(d_lp, d_lab, term, beam, 4, band_lo=d_tab)          # a single tensor call goes to the device form
    assert np.array_equal(one[0].cpu().numpy(), raw["mea_path"].outs[0][0])
    with pytest.raises(ValueError):
        ka.ctc_state_visits(lp, labels, term, beam, 4, band_lo=table[::-1].copy())        # a decreasing table
