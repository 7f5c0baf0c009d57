"""The path margins' definition and test inputs, checked without a GPU: tests/margin_ref.py against brute-force path
enumeration, its exact identities, the conditions that keep the GPU tests (tests/test_margins_gpu.py) from passing vacuously,
the planted faults on the GPU case list, and the agreement with the C oracle's best path."""
import numpy as np
import pytest

import margin_cases as C
import margin_ref as R


# ---- 1. brute force ----
def _paths(lab, lo, hi, mm):
    """Every band path as a tuple of positions: from the virtual state 0, moves j in [0, mm), the veto on the target's label."""
    T, out = len(lo), []

    def ok(j, p):
        return not (j >= 2 and j % 2 == 0 and lab[p] == 0)

    def walk(prefix, last):
        t = len(prefix)
        if t == T:
            out.append(tuple(prefix))
            return
        for j in range(mm):
            p = last + j
            if lo[t] <= p < hi[t] and ok(j, p):
                walk(prefix + [p], p)

    walk([], 0)
    return out


def _brute(lp, labels, path, beam, mm, unit, band_lo):
    lab = R.expand(labels)
    T, L = lp.shape[0], len(lab)
    lo, hi = R.band_of(T, L, beam, band_lo)
    lpd = lp.astype(np.float64)
    sstar = int(path[-1])
    scored = [(sum(lpd[t, lab[p]] for t, p in enumerate(ps)), ps) for ps in _paths(lab, lo, hi, mm) if ps[-1] == sstar]
    score = max((s for s, _ in scored), default=-np.inf)
    if score == -np.inf:
        return None
    through, alt = np.full(T, -np.inf), np.full(T, -np.inf)
    for t in range(T):
        for s, ps in scored:
            if ps[t] == path[t]:
                through[t] = max(through[t], s)
            if (ps[t] >> unit) != (int(path[t]) >> unit):
                alt[t] = max(alt[t], s)
    return through, alt, score


def test_reference_equals_brute_force_enumeration():
    rng = np.random.default_rng(2024)
    checked = zero_mass = 0
    for k in range(1200):
        T, S = int(rng.integers(1, 7)), int(rng.integers(0, 4))
        beam, mm, unit = int(rng.integers(1, 10)), int(rng.integers(1, 5)), k % 2
        lp, labels = C.eighths(int(rng.integers(1 << 30)), T, S, V=4, ninf=0.15, zero=0.3)
        L = 2 * S + 1
        band_lo = None
        if k % 3 == 0:
            band_lo = np.sort(rng.integers(0, L, size=T)).astype(np.int32)
        path = rng.integers(0, L, size=T)
        lo, hi = R.band_of(T, L, beam, band_lo)
        if k % 4:       # mostly a terminal inside the last band
            path[-1] = int(rng.integers(lo[-1], hi[-1]))
        got = R.margins_ref(lp, labels, path, beam, mm, unit, band_lo, cells=True)
        want = _brute(lp, labels, path, beam, mm, unit, band_lo)
        if want is None:
            assert got["status"] == R.ZERO_MASS and got["score"] == -np.inf, k
            zero_mass += 1
            continue
        assert got["status"] == R.OK, k
        assert np.array_equal(got["through"], want[0]) and np.array_equal(got["alt"], want[1]) and got["score"] == want[2], k
        for t in range(T):      # the runner-up attains alt, lies in the band and outside the group, and is the lowest such
            r = got["runner_up"][t]
            assert (r == -1) == (want[1][t] == -np.inf)
            if r >= 0:
                others = [p for p in range(lo[t], hi[t]) if (p >> unit) != (int(path[t]) >> unit) and got["m"][t, p] == want[1][t]]
                assert others and r == others[0], (k, t)
        checked += 1
    assert checked >= 500 and zero_mass >= 10, (checked, zero_mass)


# ---- 2. exact identities, 3. family conditions ----
@pytest.fixture(scope="module")
def family():
    return C.identity_family(40)


def _shares(answers):
    frames = sum(len(a["alt"]) for a in answers)
    none = sum(int(np.sum(a["alt"] == -np.inf)) for a in answers)
    ties = sum(int(np.sum(R.margin_of(a["through"], a["alt"]) == 0.0)) for a in answers)
    return none / frames, ties / frames


def test_exact_identities_on_eighths(family):
    answers = {0: [], 1: []}
    for c in family:
        r0 = R.margins_ref(c["lp"], c["labels"], c["path"], c["beam"], c["mm"], 0, cells=True)
        r1 = R.margins_ref(c["lp"], c["labels"], c["path"], c["beam"], c["mm"], 1)
        assert r0["status"] == r1["status"] == R.OK
        T = len(c["path"])
        lo, hi = r0["lo"], r0["hi"]
        assert all(r0["m"][t, lo[t]:hi[t]].max() == r0["score"] for t in range(T))
        m0, m1 = R.margin_of(r0["through"], r0["alt"]), R.margin_of(r1["through"], r1["alt"])
        for r, m, unit in ((r0, m0, 0), (r1, m1, 1)):
            assert np.all(r["through"] == r["score"]) and np.all(m >= 0)
            ru = r["runner_up"]
            have = ru >= 0
            assert np.all((ru[have] >= lo[have]) & (ru[have] < hi[have]) & ((ru[have] >> unit) != (c["path"][have] >> unit)))
            answers[unit].append(r)
        assert np.all(m1 >= m0)
    for unit in (0, 1):     # the family conditions: at most a quarter of the frames without an alternative, 2 % exact ties
        none, ties = _shares(answers[unit])
        print(f"identity family, unit {unit}: no alternative {none:.3f}, exact ties {ties:.3f}")
        assert none <= 0.25 and ties >= 0.02, (unit, none, ties)


def test_gpu_case_list_meets_the_family_conditions():
    for unit in (0, 1):
        answers = [C.want(n, unit) for n in C.NAMES]
        assert all(a["status"] == R.OK for a in answers), [n for n, a in zip(C.NAMES, answers) if a["status"] != R.OK]
        none, ties = _shares(answers)
        print(f"GPU case list, unit {unit}: no alternative {none:.3f}, exact ties {ties:.3f}")
        assert none <= 0.25 and ties >= 0.02, (unit, none, ties)
    # what the names promise
    assert all(C.fast_form(C.case(n)) == (not n.startswith("gen_")) for n in C.NAMES)
    assert np.any(C.want("ninf", 0)["alt"] == -np.inf) and np.any(C.want("ninf_heavy", 0)["alt"] == -np.inf)
    assert np.any(C.want("outside", 0)["through"] == -np.inf)
    assert np.any(R.margin_of(C.want("disconnected", 0)["through"], C.want("disconnected", 0)["alt"]) < 0)
    assert np.all(R.margin_of(C.want("ties", 0)["through"], C.want("ties", 0)["alt"])[:-1] == 0.0)     # (the last frame has no alternative)
    w = C.case("wrap")
    lo, hi = R.band_of(len(w["path"]), 2 * len(w["labels"]) + 1, w["beam"])
    assert np.any((lo < 1024) & (hi > 1024)) and lo[-1] > 1024
    steps = {n: int(np.diff(C.case(n)["band_lo"].astype(np.int64)).max()) for n in ("step0", "step1", "step16", "step70", "step504")}
    assert steps == {"step0": 0, "step1": 1, "step16": 16, "step70": 70, "step504": 504}


# ---- 4. planted faults ----
def test_every_planted_fault_shows_on_the_gpu_case_list():
    caught = {f: [] for f in R.FAULTS}
    for n in C.NAMES:
        c = C.case(n)
        hit = [f for f in c["catches"] if any(not C.same(C.want(n, u), C.want(n, u, **{f: True})) for u in (0, 1))]
        assert hit == list(c["catches"]), (n, "meant to catch", c["catches"], "catches", hit)
        for f in hit:
            caught[f].append(n)
    assert all(caught.values()), caught
    assert all(C.case(n)["catches"] for n in C.NAMES if n not in ("S0", "beam1", "T1", "mm1")), "a case that catches nothing"


# ---- 5. agreement with the best path ----
def test_the_oracles_best_path_has_through_equal_to_its_total_score():
    from oracle import oracle as O
    O.build()
    rng = np.random.default_rng(77)
    done = 0
    for _ in range(12):
        T, S = int(rng.integers(12, 71)), int(rng.integers(4, 41))
        beam, mm = int(rng.integers(6, 41)), int(rng.integers(2, 5))
        lp, labels = C.eighths(int(rng.integers(1 << 30)), T, S)
        try:
            path, _, scores = O.ctc_best_path_c(lp, labels, beam, mm)
        except ValueError:
            continue
        total = float(np.sum(scores.astype(np.float64)))     # eighths, |total| < 2^20: exact in float32 and float64 alike
        for unit in (0, 1):
            r = R.margins_ref(lp, labels, path, beam, mm, unit)
            assert r["status"] == R.OK and r["score"] == total
            assert np.all(r["through"] == total) and np.all(R.margin_of(r["through"], r["alt"]) >= 0)
        done += 1
    assert done >= 8
