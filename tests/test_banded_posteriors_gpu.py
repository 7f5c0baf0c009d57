"""The forward-backward calls over a caller-given band on the GPU, through the raw C ABI
(tests/banded_fb_harness.py) and, at the end, through the Python front end.

1. with the diagonal as the table every banded call returns its sibling's bits; 2. tables against the float64 references of
tests/banded_fb_ref.py, per cell, with the diagonal calls' error models and multipliers; 3. relations that hold exactly under a
table; 4. invalid tables; 5. more lattices than slots; 6. Python."""
import numpy as np
import pytest

import band_cases as C
import banded_fb_harness as BH
import banded_fb_ref as B
import duration_ref as DR
import fb_harness as H
import posterior_ref as R

pytestmark = pytest.mark.gpu

KINDS = BH.KINDS
OK, BAD_ARGS, ZERO_MASS = 0, -2, -9
GENERIC_V = 65                      # above 64 columns the kernels take their generic form


@pytest.fixture(scope="module")
def env():
    return H.engine()


def _own(kind, T, terminal, frames, path=None):
    """One lattice's own input of a call, as BH.run takes them (lists)."""
    if kind == "path_posteriors":
        return [np.full(T, terminal, np.int32) if path is None else path]
    if kind == "state_posteriors":
        return ([terminal], [frames])
    return [terminal]


def _owns(kind, items):
    """The own input of a batch from per-lattice (T, terminal, frames, path)."""
    if kind == "path_posteriors":
        return [np.full(T, term, np.int32) if path is None else path for T, term, _, path in items]
    if kind == "state_posteriors":
        return ([term for _, term, _, _ in items], [fr for _, _, fr, _ in items])
    return [term for _, term, _, _ in items]


def _generic(lp):
    return R.pad_vocabulary(lp, GENERIC_V)


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
    lo, hi = R.windows(T, L, beam)
    path = np.clip(lo + (hi - lo) // 2, 0, L - 1).astype(np.int32)
    path[-1] = term
    frames = R.query_frames(T)
    x = _generic(lp) if form == "generic" else lp
    assert R.fast_form(len(labels), x.shape[1], beam, mm) == (form == "fast" and mm <= 4)
    for kind in KINDS:
        own = _own(kind, T, term, frames, path)
        plain = BH.run(eng, _lib, kind, [x], [labels], own, beam, mm, device=device)
        banded = BH.run(eng, _lib, kind, [x], [labels], own, beam, mm, tables=[table], device=device)
        assert plain.rc == OK and plain.st[0] == OK, (kind, plain.rc)
        assert banded.same_bits(plain), kind
        assert banded.guards_intact() and plain.guards_intact(), kind


# ---------------------------------------------------------------------------------------
# 2. tables against float64
# ---------------------------------------------------------------------------------------
def _flat70(at, step, base=0):
    def make():
        lp, labels = C.random_lattice(300 + at + base, 70, 40)
        return lp, labels, C.flat_with_step(70, at, step, base), 24, 4
    return make


EXTRA = {"step5_at31": _flat70(31, 5), "step5_at32": _flat70(32, 5), "step5_at33": _flat70(33, 5), "lo2": _flat70(70, 0, base=2)}
WITH_PATH = [n for n in C.NAMES if n not in ("no_overlap", "step500", "step1100", "mm1")]
GENERIC_AGAIN = ("staircase", "ninf", "ring_wrap", "step1009", "step159")
TABLE_CASES = [(n, "fast") for n in WITH_PATH + list(EXTRA)] + [(n, "generic") for n in GENERIC_AGAIN]
_refs = {}


def _case(name):
    return EXTRA[name]() if name in EXTRA else C.case(name)


def table_refs(name):
    """(case, [(terminal, ref, dref, path, path_ref)] for band_ref's path end and one other live terminal): computed once."""
    if name not in _refs:
        lp, labels, table, beam, mm = _case(name)
        L = 2 * len(labels) + 1
        live = B.live_terminals(lp, labels, table, beam, mm)
        assert live, name
        if name in EXTRA:
            terms = live[:2]
        else:
            end = int(C.want(name)[0][-1])
            assert end in live, name
            terms = [end] + [s for s in live if s != end][:1]
        per = []
        for term in terms:
            dref, ref = B.durations(lp, labels, term, table, beam, mm)
            path = R.mixed_path(ref, B.table_windows(table, L, beam), term)
            per.append((term, ref, dref, path, B.forward_backward(lp, labels, path, table, beam, mm)))
        _refs[name] = ((lp, labels, table, beam, mm), per)
    return _refs[name]


def query_frames_of(table):
    """(the frames at and before the table's first and last steps, with 0 and T-1; the frames of the first step's block only,
    so that every block above it is skipped, across the later steps)."""
    T = len(table)
    steps = np.flatnonzero(np.diff(table) != 0) + 1
    pick = np.concatenate([steps[:4], steps[-4:]]) if len(steps) else np.zeros(0, np.int64)
    around = sorted({0, T - 1} | {int(t) for t in pick} | {int(t) - 1 for t in pick})
    first = int(steps[0]) if len(steps) else 0
    block = [t for t in range((first // R.CK) * R.CK, min((first // R.CK + 1) * R.CK, T)) if t % 5 == 0 or abs(t - first) <= 1]
    return np.array(around, np.int64), np.array(sorted(set(block)), np.int64)


@pytest.mark.parametrize("name,form", TABLE_CASES)
def test_tables_against_float64(env, name, form):
    _, _lib, eng = env
    (lp, labels, table, beam, mm), per = table_refs(name)
    T, L = lp.shape[0], 2 * len(labels) + 1
    x = _generic(lp) if form == "generic" else lp
    assert R.fast_form(len(labels), x.shape[1], beam, mm) == (form == "fast")
    n = len(per)
    terms = [p[0] for p in per]
    xs, labs, tabs = [x] * n, [labels] * n, [table] * n
    what = (name, form)

    got = BH.run(eng, _lib, "path_posteriors", xs, labs, [p[3].astype(np.int32) for p in per], beam, mm, tables=tabs)
    assert got.rc == OK and got.guards_intact(), what
    for i, (term, ref, _, _, pref) in enumerate(per):
        H.record("banded_path", R.path_ratio(got.outs[i][0], pref, what), R.M_PATH)
        H.record("banded_path_z", R.z_ratio(got.ll[i], ref), R.M_Z)
    z_path = got.ll.copy()

    got = BH.run(eng, _lib, "label_posteriors", xs, labs, terms, beam, mm, tables=tabs)
    assert got.rc == OK and got.guards_intact(), what
    for i, (term, ref, _, _, _) in enumerate(per):
        H.record("banded_label", R.label_ratio(got.outs[i][0], ref, labels, what), R.M_LABEL)
        H.record("banded_label_z", R.z_ratio(got.ll[i], ref), R.M_Z)
    z_label = got.ll.copy()

    for frames in query_frames_of(table):
        got = BH.run(eng, _lib, "state_posteriors", xs, labs, (terms, [frames] * n), beam, mm, tables=tabs)
        assert got.rc == OK and got.guards_intact(), what
        for i, (term, ref, _, _, _) in enumerate(per):
            rows, lo = got.outs[i]
            assert np.array_equal(lo, np.asarray(table, np.int64)[frames]), what      # band_lo is the table at the query frames
            H.record("banded_state", R.state_ratio(rows, frames, ref, what), R.M_STATE)
            for k, f in enumerate(frames):
                width = min(int(table[f]) + beam, L) - int(table[f])
                assert np.all(rows[k, width:] == 0.0), (what, int(f))
            assert got.ll[i].tobytes() == z_label[i].tobytes(), what

    got = BH.run(eng, _lib, "state_durations", xs, labs, terms, beam, mm, tables=tabs)
    assert got.rc == OK and got.guards_intact(), what
    for i, (term, ref, dref, _, _) in enumerate(per):
        dur, tsum = got.outs[i]
        H.record("banded_duration", DR.duration_ratio(dur, dref["D"], dref["E_D"], dref["n"], what), DR.M_DURATION)
        # (a position that only frame 0's band holds has B = 0 g exactly and a model of 0: it is held to 0.0 like the unheld ones)
        timed = np.where(dref["E_B"] > 0.0, dref["n"], 0)
        H.record("banded_time_sum", DR.duration_ratio(tsum, dref["B"], dref["E_B"], timed, what), DR.M_DURATION)
        assert got.ll[i].tobytes() == z_label[i].tobytes(), what
    # the path call's Z for a path that ends at the same terminal: the bits of the terminal calls
    assert z_path.tobytes() == z_label.tobytes(), what


@pytest.mark.parametrize("form", ["fast", "generic"])
@pytest.mark.parametrize("name", ["no_overlap", "step500", "step1100", "mm1"])
def test_tables_that_leave_no_path_are_zero_mass(env, name, form):
    _, _lib, eng = env
    lp, labels, table, beam, mm = C.case(name)
    T, L = lp.shape[0], 2 * len(labels) + 1
    term = min(int(table[-1]) + beam, L) - 1
    x = _generic(lp) if form == "generic" else lp
    for kind in KINDS:
        got = BH.run(eng, _lib, kind, [x], [labels], _own(kind, T, term, np.array([0, T - 1], np.int64)), beam, mm, tables=[table])
        assert got.rc == ZERO_MASS and got.st[0] == ZERO_MASS and got.ll[0] == -np.inf, (name, kind)
        assert got.guards_intact(), (name, kind)
        for out in got.outs[0]:
            assert np.all(out == -1) if out.dtype == np.int64 else np.all(np.isnan(out)), (name, kind)


# ---------------------------------------------------------------------------------------
# 3. relations that hold exactly under a table
# ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", ["fast", "generic"])
@pytest.mark.parametrize("name", ["staircase", "step1009", "lo2"])
def test_exact_relations_under_a_table(env, name, form):
    _, _lib, eng = env
    (lp, labels, table, beam, mm), per = table_refs(name)
    term = per[0][0]
    T, L = lp.shape[0], 2 * len(labels) + 1
    x = _generic(lp) if form == "generic" else lp
    every = np.arange(T, dtype=np.int64)
    run = lambda kind, own: BH.run(eng, _lib, kind, [x], [labels], own, beam, mm, tables=[table])
    st = run("state_posteriors", ([term], [every]))
    du = run("state_durations", [term])
    la = run("label_posteriors", [term])
    pa = run("path_posteriors", [np.full(T, term, np.int32)])
    assert st.rc == du.rc == la.rc == pa.rc == OK
    rows, lo = st.outs[0]
    dur, tsum = du.outs[0]
    occ = la.outs[0][0]
    assert np.array_equal(lo, np.asarray(table, np.int64))
    # the durations are the state rows added one frame at a time, T-1 first
    want_D, want_B = DR.sequential_sums(rows, lo, L)
    assert dur.tobytes() == want_D.tobytes() and tsum.tobytes() == want_B.tobytes()
    assert abs(dur.sum() - T) <= 1e-5 * T
    held = np.zeros(L, bool)
    for t in range(T):
        held[int(table[t]):min(int(table[t]) + beam, L)] = True
    assert name != "lo2" or (not held[:2].any() and not held[26:].any())       # (below lo_0 = 2 and above hi = 26: no band)
    for out in (dur, tsum):
        assert np.all(out[~held] == 0.0) and not np.any(np.signbit(out[~held]))
    # the last row is the terminal, exactly
    last = np.zeros(rows.shape[1], np.float32)
    last[term - int(table[-1])] = 1.0
    assert rows[T - 1].tobytes() == last.tobytes()
    # the occupancy is gamma summed by label
    lab = R.expand(labels)
    by_label = np.zeros((T, occ.shape[1]))
    for t in range(T):
        w = min(int(table[t]) + beam, L) - int(table[t])
        np.add.at(by_label[t], lab[int(table[t]):int(table[t]) + w], rows[t, :w].astype(np.float64))
    assert np.max(np.abs(by_label - occ)) <= 1e-5
    # one Z, the same bits, from all four
    assert st.ll.tobytes() == du.ll.tobytes() == la.ll.tobytes() == pa.ll.tobytes()


# ---------------------------------------------------------------------------------------
# 4. invalid tables
# ---------------------------------------------------------------------------------------
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


def _assert_failed(got, i, kind):
    assert got.st[i] == BAD_ARGS and np.isnan(got.ll[i]), (kind, i)
    for out in got.outs[i]:
        assert np.all(out == -1) if out.dtype == np.int64 else np.all(np.isnan(out)), (kind, i)


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
    frames = np.array([0, 31, 32, 69], np.int64)
    tabs = list(good)
    for i in range(0, n, 7):                                                 # every seventh lattice: 0, 7, 14
        tabs[i] = _invalid(good[i], L, INVALID[(i // 7) % 3])
        assert tabs[i].min() < 0 or tabs[i].max() >= L or np.any(np.diff(tabs[i]) < 0)
    items = [(T, terms[i], frames, None) for i in range(n)]
    for kind in KINDS:
        batch = BH.run(eng, _lib, kind, xs, labs, _owns(kind, items), beam, mm, tables=tabs)
        assert batch.rc == BAD_ARGS and batch.guards_intact(), kind
        for i in range(n):
            alone = BH.run(eng, _lib, kind, [xs[i]], [labs[i]], _owns(kind, [items[i]]), beam, mm, tables=[tabs[i]])
            assert alone.guards_intact(), (kind, i)
            if i % 7 == 0:
                assert alone.rc == BAD_ARGS, (kind, i)
                _assert_failed(alone, 0, kind)
                _assert_failed(batch, i, kind)
            else:                                                            # the neighbours are answered, with their own bits
                assert alone.rc == OK and batch.st[i] == OK, (kind, i)
                assert batch.ll[i].tobytes() == alone.ll[0].tobytes(), (kind, i)
                assert all(a.tobytes() == b.tobytes() for a, b in zip(batch.outs[i], alone.outs[0])), (kind, i)


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
def test_null_table_fails_before_launch(env, device):
    _, _lib, eng = env
    lp, labels = C.random_lattice(9, 40, 12)
    table = np.zeros(40, np.int64)
    for kind in KINDS:
        own = _owns(kind, [(40, 24, np.array([0, 39], np.int64), None)] * 2)
        for null in ("array", 1):
            got = BH.run(eng, _lib, kind, [lp, lp], [labels, labels], own, 16, 4, tables=[table, table], device=device, null_table=null)
            assert got.rc == BAD_ARGS and np.all(got.st == 99) and np.all(got.ll == 0.0), (kind, null)
            assert got.guards_intact(), (kind, null)
            for outs in got.outs:                                            # nothing was written at all
                assert all(np.all(o == (-9 if o.dtype == np.int64 else BH.SENTINEL)) for o in outs), (kind, null)


# ---------------------------------------------------------------------------------------
# 5. more lattices than slots, each with a table of its own
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
    frames = np.array([0, 17, 31, 32, 39], np.int64)
    pick = [triples[i % 7] for i in range(n)]
    items = [(T, p[3], frames, None) for p in pick]
    for kind in KINDS:
        singles = [BH.run(eng, _lib, kind, [p[0]], [p[1]], _owns(kind, [(T, p[3], frames, None)]), beam, mm, tables=[p[2]]) for p in triples]
        assert all(s.rc == OK for s in singles), kind
        batch = BH.run(eng, _lib, kind, [p[0] for p in pick], [p[1] for p in pick], _owns(kind, items), beam, mm, tables=[p[2] for p in pick])
        assert batch.rc == OK and batch.guards_intact(), kind
        for i in range(n):
            one = singles[i % 7]
            assert batch.ll[i].tobytes() == one.ll[0].tobytes(), (kind, i)
            assert all(a.tobytes() == b.tobytes() for a, b in zip(batch.outs[i], one.outs[0])), (kind, i)


# ---------------------------------------------------------------------------------------
# 6. Python
# ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", range(6))
def test_rescue_case_through_python(env, seed):
    ka, _, _ = env
    lp, labels, L, beam, pre = C.rescue(seed)
    T = lp.shape[0]
    anchored = ka.anchored_band(T, L, [(pre, 0)], beam)
    diagonal = ka.diagonal_band(T, L, beam)
    path = ka.ctc_best_path_banded(lp, labels, anchored, beam, 4)[0]
    post, z = ka.ctc_path_posteriors(lp, labels, path, beam, 4, band_lo=anchored)
    dur, tsum, z_d = ka.ctc_state_durations(lp, labels, L - 1, beam, 4, band_lo=anchored)
    path_d = ka.ctc_best_path_banded(lp, labels, diagonal, beam, 4)[0]
    post_d, _ = ka.ctc_path_posteriors(lp, labels, path_d, beam, 4, band_lo=diagonal)
    plain, _ = ka.ctc_path_posteriors(lp, labels, path_d, beam, 4)
    assert post_d.tobytes() == plain.tobytes()
    _, _, z_diag = ka.ctc_state_durations(lp, labels, L - 1, beam, 4)
    assert post.mean() >= 0.95 and post_d.mean() <= 0.6
    assert z_d - z_diag > 100.0
    assert abs(dur[0] - pre) < 3.0 and abs(dur.sum() - T) <= 1e-5 * T
    if int(path[-1]) == L - 1:
        assert z == z_d


def test_likelihood_gradient_is_the_banded_occupancy(env):
    import torch
    ka, _, _ = env
    lp, labels, L, beam, pre = C.rescue(0)
    table = ka.anchored_band(lp.shape[0], L, [(pre, 0)], beam)
    occ, z = ka.ctc_label_posteriors(lp, labels, L - 1, beam, 4, band_lo=table)
    for dev in ("cpu", "cuda"):
        x = torch.from_numpy(lp).to(dev).requires_grad_(True)
        band = torch.from_numpy(table).to(dev) if dev == "cuda" else table
        ll = ka.lattice_log_likelihood(x, torch.from_numpy(labels), L - 1, beam, 4, band_lo=band)
        assert float(ll.detach()) == z
        ll.backward()
        assert np.array_equal(x.grad.cpu().numpy(), occ), dev
    unbanded = ka.lattice_log_likelihood(torch.from_numpy(lp), torch.from_numpy(labels), L - 1, beam, 4)
    assert float(unbanded) < z - 100.0


def test_device_forms_take_the_table_as_a_device_tensor(env):
    import torch
    ka, _, _ = env
    lp, labels, L, beam, pre = C.rescue(1)
    T = lp.shape[0]
    table = ka.anchored_band(T, L, [(pre, 0)], beam)
    d_lp, d_lab, d_tab = torch.from_numpy(lp).cuda(), torch.from_numpy(labels).cuda(), torch.from_numpy(table).cuda()
    frames = [0, pre, T - 1]
    path = ka.ctc_best_path_banded(lp, labels, table, beam, 4)[0]
    host = (ka.ctc_path_posteriors(lp, labels, path, beam, 4, band_lo=table),
            ka.ctc_label_posteriors(lp, labels, L - 1, beam, 4, band_lo=table),
            ka.ctc_state_posteriors(lp, labels, L - 1, frames, beam, 4, band_lo=table),
            ka.ctc_state_durations(lp, labels, L - 1, beam, 4, band_lo=table))
    dev = (ka.ctc_path_posteriors_device([d_lp], [d_lab], [torch.from_numpy(path).cuda()], beam, 4, band_lo=[d_tab])[0],
           ka.ctc_label_posteriors_device([d_lp], [d_lab], [L - 1], beam, 4, band_lo=[d_tab])[0],
           ka.ctc_state_posteriors_device([d_lp], [d_lab], [L - 1], [frames], beam, 4, band_lo=[d_tab])[0],
           ka.ctc_state_durations_device([d_lp], [d_lab], [L - 1], beam, 4, band_lo=[d_tab])[0])
    for h, d in zip(host, dev):
        assert len(h) == len(d)
        for a, b in zip(h, d):
            b = b.cpu().numpy() if torch.is_tensor(b) else b
            assert np.array_equal(np.asarray(a), np.asarray(b))
    assert np.array_equal(host[2][1], table[frames])
    # a single tensor call goes to the device form with its one table
    one = ka.ctc_state_durations(d_lp, d_lab, L - 1, beam, 4, band_lo=d_tab)
    assert np.array_equal(one[0].cpu().numpy(), host[3][0])
    with pytest.raises(ValueError):
        ka.ctc_state_durations(lp, labels, L - 1, beam, 4, band_lo=table[::-1].copy())        # a decreasing table
