"""The forward-backward calls on deep input ("magnitude"): rows 2^k nats below their neighbours, k up to
44, and single cells masked with a large finite constant, through the raw C ABI in the one-wavefront form (V = 39) and the
generic form (the same lattices padded to V = 80).  The inputs, the references and the conditions are tests/posterior_ref.py's
and are asserted on the CPU by tests/test_posterior_deep_cpu.py.

Every (case, call) pair must return KA_OK with finite, legal outputs, its sentinels intact, and, from a ``_banded`` call over
``diagonal_band``, the same bits.  Z is held to m x deep_error_model("z") at every rung and to 2^-40 |Z| where
posterior_ref.z_rel_holds says the float store of the terminal's alpha leaves that within reach.  A pair inside the cap (the
model within 2^-10 of every value >= 2^-20: a condition on the reference) is compared cell by cell with the float64 reference of
the UNSHIFTED lattice; the worst ratio of each call is recorded and held against its multiplier."""
import numpy as np
import pytest

import banded_fb2_harness as H2
import banded_fb_harness as BH
import duration_ref as DR
import fb_harness as H
import fb_resume_harness as RH
import fb_resume_ref as F
import mea_ref as MR
import posterior_ref as R
import quantile_ref as QR
import sample_ref as S
import visit_ref as VR

pytestmark = pytest.mark.gpu

SHAPES = list(R.DEEP_SHAPES)
FORMS = ("one_wavefront", "generic")
N_SAMPLES, SEED = 8, 20240
_cache = {}


@pytest.fixture(scope="module")
def env():
    return H.engine()


def cases(shape):
    if shape not in _cache:
        cs = R.deep_all(shape)
        for c in cs:
            T, L = len(c["lp"]), 2 * len(c["labels"]) + 1
            c["lo"], c["hi"] = R.windows(T, L, c["beam"])
            c["caps"] = R.deep_caps(c)
            c["cost"] = R.deep_cost(c["shift"])
            c["wide"] = R.pad_vocabulary(c["lp"], 80)
        _cache[shape] = cs
    return _cache[shape]


def inputs(cs, form):
    c = cs[0]
    V = 39 if form == "one_wavefront" else 80
    assert R.fast_form(len(c["labels"]), V, c["beam"], c["mm"]) == (form == "one_wavefront")
    return [x["lp"] if form == "one_wavefront" else x["wide"] for x in cs], [x["labels"] for x in cs], c["beam"], c["mm"]


def both(env, run, kind, cs, form, own):
    """The call on every case of a shape in one batch, and its ``_banded`` sibling over the diagonal: the same bits."""
    ka, _lib, eng = env
    lps, labs, beam, mm = inputs(cs, form)
    plain = run(eng, _lib, kind, lps, labs, own, beam, mm)
    tables = [np.asarray(ka.diagonal_band(len(x), 2 * len(y) + 1, beam), np.int32) for x, y in zip(lps, labs)]
    band = run(eng, _lib, kind, lps, labs, own, beam, mm, tables=tables)
    bad = [(c["name"], int(s)) for c, s in zip(cs, plain.st) if s != 0]
    assert plain.rc == 0 and not bad, (kind, form, plain.rc, bad[:12], len(bad))
    assert plain.guards_intact() and band.guards_intact(), (kind, form)
    assert band.same_bits(plain), (kind, form, "the banded call over diagonal_band differs")
    return plain


def z_check(c, z, ref, problems):
    """Z against the reference: its ratio to the model, and 2^-40 |Z| where that is within reach."""
    E = R.deep_error_model("z", ref, c["shift"])
    if not np.isfinite(z):
        problems.append((c["name"], "Z", z))
        return 0.0
    if R.z_rel_holds(ref, c["shift"]) and abs(z - c["z"]) > R.Z_DEEP_REL * abs(c["z"]):
        problems.append((c["name"], "Z beyond 2^-40", z, c["z"]))
    return abs(z - c["z"]) / E


def finish(call, form, worst, m, problems):
    for name, ratio in worst.items():
        H.record("deep_" + name, ratio, m[name] if isinstance(m, dict) else m)
    assert not problems, (call, form, problems[:10], len(problems))


def terms_of(cs):
    return [c["terminal"] for c in cs]


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("shape", SHAPES)
def test_state_posteriors_at_every_frame(env, shape, form):
    cs = cases(shape)
    res = both(env, BH.run, "state_posteriors", cs, form, (terms_of(cs), [np.arange(len(c["lp"])) for c in cs]))
    worst, problems = dict(state=0.0, z=0.0), []
    for i, c in enumerate(cs):
        rows, blo = res.outs[i]
        if not (np.all(np.isfinite(rows)) and np.all((rows >= 0.0) & (rows <= 1.0)) and np.array_equal(blo, c["lo"])):
            problems.append((c["name"], "rows outside [0, 1] or band_lo"))
            continue
        worst["z"] = max(worst["z"], z_check(c, res.ll[i], c["ref"], problems))
        E = R.deep_error_model("state", c["ref"], c["shift"])
        for t, (_, rg) in enumerate(c["ref"]["gamma"]):
            if np.any(rows[t, len(rg):] != 0.0):
                problems.append((c["name"], "a column past the band is not 0", t))
            if c["caps"]["state"]:
                worst["state"] = max(worst["state"], R.cells_ratio(rows[t, :len(rg)], rg, E[t], (c["name"], t)))
    finish("state", form, worst, dict(state=R.M_DEEP_STATE, z=R.M_DEEP_Z), problems)


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("shape", SHAPES)
def test_label_posteriors(env, shape, form):
    cs = cases(shape)
    res = both(env, BH.run, "label_posteriors", cs, form, terms_of(cs))
    worst, problems = dict(label=0.0, z=0.0), []
    for i, c in enumerate(cs):
        occ = res.outs[i][0]
        if not (np.all(np.isfinite(occ)) and np.all((occ >= 0.0) & (occ <= 1.0))):
            problems.append((c["name"], "occupancy outside [0, 1]", float(np.nanmax(occ))))
            continue
        assert np.all(occ[:, 39:] == 0.0), c["name"]
        worst["z"] = max(worst["z"], z_check(c, res.ll[i], c["ref"], problems))
        if c["caps"]["label"]:
            want = np.zeros((len(occ), 39))
            lab = R.expand(c["labels"])
            for t, (lo, g) in enumerate(c["ref"]["gamma"]):
                np.add.at(want[t], lab[lo:lo + len(g)], g)
            E = R.deep_error_model("label", c["ref"], c["shift"], c["labels"], 39)
            worst["label"] = max(worst["label"], R.cells_ratio(occ[:, :39], want, E, c["name"]))
    finish("label", form, worst, dict(label=R.M_DEEP_LABEL, z=R.M_DEEP_Z), problems)


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("shape", SHAPES)
def test_path_posteriors_along_a_mixed_path(env, shape, form):
    cs = cases(shape)
    res = both(env, BH.run, "path_posteriors", cs, form, [c["path"] for c in cs])
    worst, problems = dict(path=0.0, z=0.0), []
    for i, c in enumerate(cs):
        post = res.outs[i][0]
        if not (np.all(np.isfinite(post)) and np.all((post >= 0.0) & (post <= 1.0)) and post[-1] == 1.0):
            problems.append((c["name"], "posteriors outside [0, 1]"))
            continue
        outside = (c["path"] < c["lo"]) | (c["path"] >= c["hi"])
        if np.any(post[outside] != 0.0):
            problems.append((c["name"], "a path cell outside the band is not 0"))
        worst["z"] = max(worst["z"], z_check(c, res.ll[i], c["pref"], problems))
        if c["caps"]["path"]:
            worst["path"] = max(worst["path"], R.cells_ratio(post, c["pref"]["post"], R.deep_error_model("path", c["pref"], c["shift"]), c["name"]))
    finish("path", form, worst, dict(path=R.M_DEEP_PATH, z=R.M_DEEP_Z), problems)


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("shape", SHAPES)
def test_durations(env, shape, form):
    cs = cases(shape)
    res = both(env, BH.run, "state_durations", cs, form, terms_of(cs))
    worst, problems = dict(duration=0.0, time_sum=0.0), []
    for i, c in enumerate(cs):
        D, B = res.outs[i]
        T, L = len(c["lp"]), len(D)
        if "dref" not in c:
            c["dref"] = DR.durations(c["ref"], L)
        d = c["dref"]
        if not (np.all(np.isfinite(D)) and np.all(np.isfinite(B)) and np.all((D >= 0.0) & (D <= d["n"])) and np.all((B >= 0.0) & (B <= T * d["n"]))):
            problems.append((c["name"], "durations not finite or outside [0, frames that hold the position]"))
            continue
        if c["caps"]["state"]:
            eD, eB = np.zeros(L), np.zeros(L)
            for t, (lo, g) in enumerate(c["ref"]["gamma"]):
                eD[lo:lo + len(g)] += g * c["cost"][t]
                eB[lo:lo + len(g)] += t * g * c["cost"][t]
            worst["duration"] = max(worst["duration"], DR.duration_ratio(D, d["D"], d["E_D"] + eD, d["n"], c["name"]))
            worst["time_sum"] = max(worst["time_sum"], DR.duration_ratio(B, d["B"], d["E_B"] + eB, d["n"], c["name"]))
    finish("durations", form, worst, R.M_DEEP_STATE, problems)


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("shape", SHAPES)
def test_visits(env, shape, form):
    """visit and exit_time are sums of gamma r over the frames and are not clamped: a sum of probabilities of disjoint events
    stays below 1 only as far as its terms are accurate.  At every rung a visit lies in [0, 1 + m E] (E its model) and below the
    number of frames that hold the position; inside the cap both outputs are compared with the reference."""
    cs = cases(shape)
    res = both(env, H2.run, "state_visits", cs, form, terms_of(cs))
    worst, problems = dict(visit=0.0, exit_time=0.0), []
    for i, c in enumerate(cs):
        Vs, X = res.outs[i]
        T, L = len(c["lp"]), len(Vs)
        key = ("vref", c["shape"], c["pattern"], R.deep_ref_key(c["k"]))
        if key not in _cache:
            _cache[key] = VR.visits(c["plain"], c["labels"], c["terminal"], c["beam"], c["mm"])
        v = _cache[key]
        # gamma moves by cost_t of itself, and r, a difference of two cells of frame t + 1's column, by 6 roundings for every
        # deep frame behind t (3 on either cell): no more than cost_t again
        eV, eX = np.zeros(L), np.zeros(L)
        for t, (lo, g) in enumerate(c["ref"]["gamma"]):
            eV[lo:lo + len(g)] += 2.0 * g * c["cost"][t]
            eX[lo:lo + len(g)] += 2.0 * t * g * c["cost"][t]
        top = np.minimum(v["n"], 1.0 + R.M_DEEP_VISIT * (v["E_V"] + eV))
        if not (np.all(np.isfinite(Vs)) and np.all(np.isfinite(X)) and np.all((Vs >= 0.0) & (Vs <= top)) and np.all((X >= 0.0) & (X <= T * top))):
            problems.append((c["name"], "visits not finite or outside [0, 1 + m E]", float(np.nanmax(Vs - top))))
            continue
        if c["caps"]["state"]:
            worst["visit"] = max(worst["visit"], VR.visit_ratio(Vs, v["V"], v["E_V"] + eV, c["name"]))
            worst["exit_time"] = max(worst["exit_time"], VR.visit_ratio(X, v["X"], v["E_X"] + eX, c["name"]))
    finish("visits", form, worst, R.M_DEEP_VISIT, problems)


def _state_rows(env, cs, form):
    ka, _lib, eng = env
    lps, labs, beam, mm = inputs(cs, form)
    res = BH.run(eng, _lib, "state_posteriors", lps, labs, (terms_of(cs), [np.arange(len(x)) for x in lps]), beam, mm)
    assert res.rc == 0 and not np.any(res.st), res.st
    return res


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("shape", SHAPES)
def test_boundary_quantiles_are_the_integer_definition_on_the_state_rows(env, shape, form):
    cs = cases(shape)
    cuts = [np.arange(1, c["terminal"] + 1, 3) for c in cs]                      # every path crosses a cut at or below its terminal
    res = both(env, H2.run, "boundary_quantiles", cs, form, (terms_of(cs), cuts))
    rows = _state_rows(env, cs, form)
    problems = []
    for i, c in enumerate(cs):
        q = res.outs[i][0]
        T, L = len(c["lp"]), 2 * len(c["labels"]) + 1
        if not np.all((q >= 0) & (q < T)) or np.any(np.diff(q, axis=1) < 0):
            problems.append((c["name"], "a quantile frame outside [0, T) or levels out of order"))
            continue
        want = QR.integer_quantiles(rows.outs[i][0], rows.outs[i][1], cuts[i], H2.LEVELS, L, c["beam"])
        if not np.array_equal(q, want):
            problems.append((c["name"], "not the integer definition on the state call's rows"))
        if res.ll[i] != rows.ll[i]:
            problems.append((c["name"], "Z differs from the state call's"))
    assert not problems, (form, problems[:10], len(problems))


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("shape", SHAPES)
def test_mea_path_is_a_band_path_and_the_replay_of_the_state_rows(env, shape, form):
    cs = cases(shape)
    res = both(env, H2.run, "mea_path", cs, form, terms_of(cs))
    rows = _state_rows(env, cs, form)
    problems = []
    for i, c in enumerate(cs):
        path, T = res.outs[i][0], len(c["lp"])
        why = MR.validity(path, c["lo"], c["hi"], c["labels"], c["terminal"], c["mm"])
        if why is not None or not (np.isfinite(res.ea[i]) and 0.0 <= res.ea[i] <= T):
            problems.append((c["name"], why, res.ea[i]))
            continue
        want = MR.replay(rows.outs[i][0], rows.outs[i][1], c["labels"], c["terminal"], c["beam"], c["mm"])
        if want["status"] != R.OK or not np.array_equal(path, want["path"]) or np.float64(res.ea[i]).tobytes() != np.float64(want["value"]).tobytes():
            problems.append((c["name"], "not the replay of the state call's rows"))
    assert not problems, (form, problems[:10], len(problems))


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("shape", SHAPES)
def test_sampled_paths_are_legal_and_every_decidable_draw_is_the_references(env, shape, form):
    """The conditional-draw check of tests/test_sample_paths_gpu.py with its caps (at most 3 undecidable draws a case, 1e-5 of
    all), on the cases whose deep cost stays below a quarter of sample_ref.DELTA = 2^-26 - a draw's weights are ratios of two
    cells of one column, which the shift moves by no more than that cost; every other case: legal band paths to the terminal."""
    cs = cases(shape)
    n = len(cs)
    res = both(env, H2.run, "sample_paths", cs, form, (terms_of(cs), [N_SAMPLES] * n, [SEED + i for i in range(n)]))
    problems, draws, ties, compared = [], 0, 0, 0
    for i, c in enumerate(cs):
        paths = res.outs[i][0]
        key = ("lat", c["shape"], c["pattern"], R.deep_ref_key(c["k"]))
        if key not in _cache:
            _cache[key] = S.Lattice(c["plain"], c["labels"], c["beam"], c["mm"])
        lat = _cache[key]
        bad = [S.valid_path(lat, row, c["terminal"]) for row in paths]
        if any(b is not None for b in bad):
            problems.append((c["name"], [b for b in bad if b is not None][:2]))
            continue
        if float(np.max(c["cost"])) <= S.DELTA / 4.0:
            wrong, t = S.check_draws(lat, paths, SEED + i, c["terminal"])
            compared += 1
            draws += paths.shape[0] * (paths.shape[1] - 1)
            ties += t
            if wrong or t > 3:
                problems.append((c["name"], wrong[:3], len(wrong), t))
    print("cases compared draw by draw:", compared, "of", n, "- undecidable draws:", ties, "of", draws)
    assert compared >= 9 and ties <= 1e-5 * draws
    assert not problems, (form, problems[:10], len(problems))


# ---- ka_ctc_posteriors_resume ----
RESUME_CASES = [(s, p, k) for s in ("T40_S12_B16_M4", "T70_S20_B16_M4") for p in ("f30_34", "pad8", "all") for k in (17, 30, 37, 44)]


def _resume_cuts(c):
    """No cut; a cut at either edge of the deep frames and one inside them, where that is a frame in (0, T); all of them at once."""
    T = len(c["lp"])
    deep = np.flatnonzero(c["shift"] > 0)
    at = sorted({int(x) for x in (deep[0], deep[len(deep) // 2], deep[-1] + 1) if 0 < x < T})
    return [()] + [(x,) for x in at] + ([tuple(at)] if len(at) > 1 else [])


@pytest.mark.parametrize("form", FORMS)
def test_resume_rows_and_posteriors_cut_inside_and_at_the_edge_of_the_deep_frames(env, form):
    """alpha_out and beta_out against the reference's rows less the shifts they carry; occupancy and path posteriors of the cut
    lattice against the uncut reference where the pair is inside the cap; finite and legal everywhere."""
    ka, _lib, eng = env
    worst, problems = dict(alpha_out=0.0, beta_out=0.0, label=0.0, state=0.0), []
    for shape, pattern, k in RESUME_CASES:
        c = [x for x in cases(shape) if x["pattern"] == pattern and x["k"] == k][0]
        lp = c["lp"] if form == "one_wavefront" else c["wide"]
        T, L = len(lp), 2 * len(c["labels"]) + 1
        band = np.asarray(ka.diagonal_band(T, L, c["beam"]), np.int32)
        post_ref = c["pref"]["post"]
        for cuts in _resume_cuts(c):
            key = ("chunks", shape, pattern, R.deep_ref_key(k), cuts)
            if key not in _cache:
                _cache[key] = F.chunked(c["plain"], c["labels"], band, c["beam"], c["mm"], cuts, c["terminal"], c["path"])
            ref = _cache[key]
            assert ref["status"] == R.OK
            bounds = F.chunk_bounds(T, cuts)
            one = lambda a, b, a_in, end, want=None, path=True: RH.run(
                eng, _lib, [lp[a:b]], [c["labels"]], [band[a:b]], c["beam"], c["mm"], [a_in], [end if F.is_row(end) else None],
                [-1 if F.is_row(end) else end], [c["path"][a:b]] if path else None, want)
            starts, row = [], None
            for a, b in bounds[:-1]:
                starts.append(row)
                got = one(a, b, row, np.zeros(L), dict(occ=False, path_post=False, beta_out=False), path=False)
                assert got.rc == 0 and got.st[0] == 0 and got.guards_intact(), (c["name"], cuts, a)
                row = got.outs[0][2]
            starts.append(row)
            outs, end = [None] * len(bounds), c["terminal"]
            for j in range(len(bounds) - 1, -1, -1):
                a, b = bounds[j]
                got = one(a, b, starts[j], end)
                assert got.rc == 0 and got.st[0] == 0 and got.guards_intact(), (c["name"], cuts, a)
                outs[j] = got
                end = got.outs[0][3]
            occ = np.concatenate([o.outs[0][0] for o in outs])
            post = np.concatenate([o.outs[0][1] for o in outs])
            legal = all(np.all(np.isfinite(x)) and np.all((x >= 0.0) & (x <= 1.0)) for x in (occ, post))
            rows_ok = all(not np.isnan(o.outs[0][j]).any() and not np.isposinf(o.outs[0][j]).any() for o in outs for j in (2, 3))
            if not (legal and rows_ok and all(np.isfinite(o.ll[0]) for o in outs)):
                problems.append((c["name"], cuts, "outputs not finite or outside [0, 1]"))
                continue
            before = np.concatenate([np.zeros(1), np.cumsum(c["shift"])])
            for (a, b), o, r in zip(bounds, outs, ref["chunks"]):
                sh = c["shift"][a:b]
                for j, name, carried, moved in ((2, "alpha_out", before[a], before[b]), (3, "beta_out", before[-1] - before[b], before[-1] - before[a])):
                    want = r[name] - moved
                    got = o.outs[0][j]
                    dead = np.isneginf(want)
                    if not np.all(np.isneginf(got[dead])):
                        problems.append((c["name"], cuts, a, name, "a cell without mass came out finite"))
                        continue
                    E = R.deep_row_model(want, sh, name, carried)
                    worst[name] = max(worst[name], float(np.max(np.abs(got[~dead] - want[~dead]) / E[~dead])))
            if c["caps"]["label"]:
                want = np.zeros((T, 39))
                lab = R.expand(c["labels"])
                for t, (lo, g) in enumerate(c["ref"]["gamma"]):
                    np.add.at(want[t], lab[lo:lo + len(g)], g)
                worst["label"] = max(worst["label"], R.cells_ratio(occ[:, :39], want, R.deep_error_model("label", c["ref"], c["shift"], c["labels"], 39), (c["name"], cuts)))
            if c["caps"]["state"]:
                E = R.state_error_model(post_ref) + post_ref * c["cost"]
                worst["state"] = max(worst["state"], R.cells_ratio(post, post_ref, E, (c["name"], cuts)))
    finish("resume", form, worst, dict(alpha_out=R.M_DEEP_ROW, beta_out=R.M_DEEP_ROW, label=R.M_DEEP_LABEL, state=R.M_DEEP_STATE), problems)


# ---- masked cells ----
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("value", R.MASK_VALUES, ids=["1e9", "1e30", "float_min"])
def test_masked_cells_are_cells_without_mass(env, value, form):
    """A cell at -1e9, -1e30 or float32's lowest finite value beside live alternatives: the reference is the lattice with -inf
    there, the existing models and multipliers apply, and a cell below 2^-120 comes out in [0, 2^-119)."""
    ka, _lib, eng = env
    worst = dict(state=0.0, label=0.0, path=0.0, z=0.0)
    for shape in SHAPES:
        lp, ninf, mask, labels, term, beam, mm = R.masked_case(shape, value)
        T, L = lp.shape[0], 2 * len(labels) + 1
        ref = R.ref_at(ninf, labels, term, beam, mm)
        path = R.mixed_path(ref, R.windows(T, L, beam), term)
        pref = R.forward_backward(ninf, labels, path, beam, mm)
        x = lp if form == "one_wavefront" else R.pad_vocabulary(lp, 80)
        (rows,), (blo,), z_s, st, rc = H.state_call(eng, _lib, [x], [labels], [term], [np.arange(T)], beam, mm)
        assert rc == 0 and st[0] == 0
        (occ,), z_l, st, rc = H.label_call(eng, _lib, [x], [labels], [term], beam, mm)
        assert rc == 0 and st[0] == 0
        (post,), z_p, st, rc = H.path_call(eng, _lib, [x], [labels], [path], beam, mm)
        assert rc == 0 and st[0] == 0
        worst["state"] = max(worst["state"], R.state_ratio(rows, np.arange(T), ref, (shape, value)))
        worst["label"] = max(worst["label"], R.label_ratio(occ[:, :39], ref, labels, (shape, value)))
        worst["path"] = max(worst["path"], R.path_ratio(post, pref, (shape, value)))
        worst["z"] = max(worst["z"], R.z_ratio(z_s[0], ref), R.z_ratio(z_l[0], ref), R.z_ratio(z_p[0], pref))
    for call, m in (("state", R.M_STATE), ("label", R.M_LABEL), ("path", R.M_PATH), ("z", R.M_Z)):
        H.record(call, worst[call], m)


def test_a_lattice_beyond_float32s_range_reports_zero_mass(env):
    """The contract of include/kokoro_align_amd.h: the zero-mass test is made on the float that Z is reported from, the terminal's
    alpha relative to its block's offset, so a lattice whose every path lies beyond float32's range below that offset reports
    KA_ERR_ZERO_MASS with Z = -inf and NaN outputs, as a lattice without a path does, in the path call and the others alike."""
    ka, _lib, eng = env
    lp = np.full((3, 39), -3.0e38, np.float32)
    labels = np.array([1, 2], np.int32)
    (rows,), _, z_s, st_s, rc_s = H.state_call(eng, _lib, [lp], [labels], [4], [np.arange(3)], 16, 4)
    (post,), z_p, st_p, rc_p = H.path_call(eng, _lib, [lp], [labels], [np.array([1, 3, 4], np.int32)], 16, 4)
    assert st_s[0] == st_p[0] == _lib.KA_ERR_ZERO_MASS and np.isneginf(z_s[0]) and np.isneginf(z_p[0])
    assert np.all(np.isnan(rows)) and np.all(np.isnan(post))
    lp[:] = -1.0e37                                                  # three frames of it stay inside: an ordinary lattice
    (rows,), _, z_s, st_s, rc_s = H.state_call(eng, _lib, [lp], [labels], [4], [np.arange(3)], 16, 4)
    assert rc_s == 0 and st_s[0] == 0 and np.isfinite(z_s[0]) and abs(z_s[0] / -3.0e37 - 1.0) < 1e-6


# ---- a deep lattice between two ordinary ones on one slot ----
@pytest.mark.parametrize("form,slots", [("one_wavefront", 1024), ("generic", 512)])
def test_neighbours_on_a_shared_slot_keep_the_bits_they_have_alone(env, form, slots):
    """launch_fb_ck runs lattice i on workgroup i mod slots (tests/test_posterior_slots_gpu.py): lattices s, s + slots and
    s + 2 slots share a slot's checkpoints, slab and offsets.  An ordinary lattice before and one behind a deep one (2^44, every
    frame) come out with the bits they have when sent alone, in the label and the state call."""
    ka, _lib, eng = env
    deep = [c for c in cases("T70_S20_B16_M4") if c["pattern"] == "all" and c["k"] == 44][0]
    beam, mm = deep["beam"], deep["mm"]
    V = 39 if form == "one_wavefront" else 80
    wide = lambda x: x if V == 39 else R.pad_vocabulary(x, V)
    a = R.sloped(90, 18, 39, 7, alpha=0.5, zero_every=5)
    b = R.sloped(50, 25, 39, 8, alpha=0.5, zero_every=5)
    fill = R.sloped(20, 4, 39, 9, alpha=0.5, zero_every=5)
    lats = {k: (wide(x[0]), x[1], R.live_terminals(x[0], x[1], beam, mm)[0]) for k, x in (("a", a), ("b", b), ("fill", fill))}
    lats["deep"] = (wide(deep["lp"]), deep["labels"], deep["terminal"])
    s = 5
    order = ["fill"] * (2 * slots + s + 1)
    order[s], order[s + slots], order[s + 2 * slots] = "a", "deep", "b"
    lps, labs, terms = ([lats[k][j] for k in order] for j in range(3))
    frs = [np.arange(len(x)) for x in lps]
    gs, los, z_s, st_s, rc_s = H.state_call(eng, _lib, lps, labs, terms, frs, beam, mm)
    occs, z_l, st_l, rc_l = H.label_call(eng, _lib, lps, labs, terms, beam, mm)
    assert rc_s == rc_l == 0 and not np.any(st_s) and not np.any(st_l)
    for i in (s, s + slots, s + 2 * slots):
        (g1,), (lo1,), z1, st, rc = H.state_call(eng, _lib, [lps[i]], [labs[i]], [terms[i]], [frs[i]], beam, mm)
        (o1,), zl1, st2, rc2 = H.label_call(eng, _lib, [lps[i]], [labs[i]], [terms[i]], beam, mm)
        assert rc == rc2 == 0 and st[0] == st2[0] == 0
        assert gs[i].tobytes() == g1.tobytes() and np.array_equal(los[i], lo1) and occs[i].tobytes() == o1.tobytes(), (form, order[i])
        assert z_s[i:i + 1].tobytes() == z1.tobytes() and z_l[i:i + 1].tobytes() == zl1.tobytes(), (form, order[i])
