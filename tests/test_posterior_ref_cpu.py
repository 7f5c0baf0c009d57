"""The float64 posterior reference and its input families, without a GPU: every family meets the
condition it was built for (mass at the band's edges, a band that slides several positions a frame, cells far below any
flat tolerance); the reference agrees with a brute-force enumeration on tiny lattices of those families, where the band's
edges are reached; and each of eight deliberate faults, applied to the reference, moves some family's result by at least
five times the tolerance derived from the kernels' own roundings (posterior_ref.*_tolerance)."""
import numpy as np
import pytest

import occupancy_ref as OR
import posterior_ref as R

CASES = R.edge_cases()


def _built(name):
    lp, labels, term, beam, mm = CASES[name]()
    ref = R.ref_at(lp, labels, term, beam, mm)
    assert ref["status"] == R.OK, name
    return lp, labels, term, beam, mm, ref


@pytest.mark.parametrize("name", [n for n in CASES if n.startswith("edge")])
def test_edge_hugging_puts_mass_on_both_edges(name):
    lp, labels, term, beam, mm, ref = _built(name)
    lower, upper = R.edge_mass(ref)
    print(name, "frames with >= 0.5 of gamma on the two lowest / highest cells:", lower, upper)
    assert lower >= 0.2 and upper >= 0.2, (name, lower, upper)
    T, L = lp.shape[0], 2 * len(labels) + 1
    lo, _ = R.windows(T, L, beam)
    if beam >= 1000:                                    # the wide bands: the low edge is hugged while it moves, not only at 0
        moving = [t for t in range(T // 2) if lo[t] > 0 and ref["gamma"][t][1][:2].sum() >= 0.5]
        assert L > 2 * beam and len(moving) >= 0.1 * T, (name, len(moving))


def test_edge_hugging_covers_the_required_forms():
    shapes = R.EDGE_SHAPES
    assert any(1000 <= min(b, 2 * s + 1) <= 1009 and v <= 64 and m <= 4 and 2 * s + 1 > 2 * b for _, s, v, b, m in shapes)
    assert any(min(b, 2 * s + 1) >= 1010 for _, s, v, b, m in shapes)
    assert any(v == 80 for _, s, v, b, m in shapes) and any(m > 4 for _, s, v, b, m in shapes)


@pytest.mark.parametrize("name", [n for n in CASES if n.startswith(("steep", "flat"))])
def test_steep_and_flat_bands(name):
    lp, labels, term, beam, mm, ref = _built(name)
    T, S = lp.shape[0], len(labels)
    two, any_ = R.band_steps(T, S, beam)
    slope = (2 * S + 1) / T
    if name.startswith("steep"):
        assert mm - 1.3 <= slope <= mm - 1, (name, slope)
        assert (two >= 0.7) if mm >= 3 else (any_ >= 0.8), (name, two, any_)
        # in a narrow band the cells that just entered carry mass: the label ring's newest entries decide a result
        top = np.mean([g[-1] >= 1e-6 for _, g in ref["gamma"]])
        assert top >= 0.1 or beam > 9, (name, top)
    else:
        assert slope <= 0.1 and any_ <= 0.1, (name, slope, any_)
    assert np.isfinite(ref["ll"])


def test_beams_one_two_three_and_odd_are_there():
    beams = {sh[3] for sh in R.STEEP_SHAPES + R.FLAT_SHAPES}
    assert {1, 2, 3} <= beams and any(b % 2 == 1 and b > 3 for b in beams)


@pytest.mark.parametrize("name", [n for n in CASES if n.startswith("peaked")])
def test_peaked_emissions_have_a_wide_range(name):
    lp, labels, term, beam, mm, ref = _built(name)
    fin = lp[np.isfinite(lp)]
    assert fin.min() <= -55.0 and np.median(lp.max(1)) >= -1e-6, (name, fin.min())
    assert np.isneginf(lp).all(0).sum() >= lp.shape[1] // 2 - 1          # whole -inf columns
    assert labels[0] == 0 and labels[-1] == 0 and np.any((labels[1:] == 0) & (labels[:-1] == 0))
    assert np.any((labels[1:] == labels[:-1]) & (labels[1:] != 0)) or lp.shape[1] // 2 <= 2
    g = np.concatenate([g for _, g in ref["gamma"]])
    assert np.mean((g > 0) & (g < 2.0 ** -30)) >= 0.05, name           # cells that only a relative check sees


def test_geometry_covers_the_boundaries():
    sh = R.GEOMETRY_SHAPES
    assert {1, 2, 31, 32, 33, 63, 64, 65, 97} <= {s[0] for s in sh} and {0, 1, 2} <= {s[1] for s in sh}
    assert {32, 33, 64, 65, 161} <= {s[0] for s in sh if min(s[3], 2 * s[1] + 1) < 2 * s[1] + 1}   # ... under a sliding window
    assert {63, 65, 1023, 1025} <= {2 * s[1] + 1 for s in sh}
    assert {63, 64, 65, 1008, 1009, 1010} <= {min(s[3], 2 * s[1] + 1) for s in sh}
    assert {1, 63, 64, 65} <= {s[2] for s in sh} and {1, 2, 3, 4, 5, 6} <= {s[4] for s in sh}
    for n in CASES:
        if n.startswith("geom"):
            _built(n)
    assert {31, 32, 33} <= set(R.query_frames(700).tolist()) and set(range(672, 700)) <= set(R.query_frames(700).tolist())


# ---- tiny lattices of the families against a brute-force enumeration ----
def _tiny_cases():
    out = []
    for T, S, V, beam, mm, seed in [(6, 3, 5, 2, 4, 1), (6, 3, 5, 3, 3, 2), (7, 2, 4, 2, 4, 3), (5, 4, 6, 3, 4, 4)]:
        lp, labels = R.edge_hugging(T, S, V, beam, seed, boost=3.0)
        out.append((f"edge{seed}", lp, labels, beam, mm))
    for T, S, V, beam, mm, seed in [(5, 6, 5, 3, 4, 5), (4, 5, 5, 2, 4, 6), (7, 1, 4, 1, 4, 7), (7, 2, 4, 2, 2, 8), (6, 5, 5, 5, 3, 9)]:
        lp, labels = R.sloped(T, S, V, seed, zero_every=2)
        out.append((f"sloped{seed}", lp, labels, beam, mm))
    for T, S, V, beam, mm, seed in [(7, 4, 6, 3, 3, 10), (6, 5, 8, 4, 4, 11)]:
        lp, labels, _ = R.peaked(T, S, V, beam, mm, seed, floor=-40.0)
        out.append((f"peaked{seed}", lp, labels, beam, mm))
    return out


@pytest.mark.parametrize("case", _tiny_cases(), ids=lambda c: c[0])
def test_reference_equals_brute_force_where_the_band_edges_are_reached(case):
    name, lp, labels, beam, mm = case
    T, L = lp.shape[0], 2 * len(labels) + 1
    lo, hi = R.windows(T, L, beam)
    live = R.live_terminals(lp, labels, beam, mm)
    assert live, name
    edge_reached = False
    for term in live[:3]:
        ref = R.ref_at(lp, labels, term, beam, mm)
        edge_reached |= any(g[0] > 1e-3 or g[-1] > 1e-3 for (_, g), t in zip(ref["gamma"], range(T)) if hi[t] - lo[t] < L)
        occ = OR.occupancy(lp, labels, term, beam, mm)
        want, z = OR.brute_force(lp, labels, term, beam, mm)
        assert np.max(np.abs(occ["occ"] - want)) <= 1e-12 and abs(occ["ll"] - z) <= 1e-12, (name, term)
        path = R.mixed_path(ref, (lo, hi), term)
        got = R.forward_backward(lp, labels, path, beam, mm, full=True)
        post, z2 = R.brute_force(lp, labels, path, beam, mm)
        assert np.max(np.abs(got["post"] - post)) <= 1e-12 and abs(got["ll"] - z2) <= 1e-12, (name, term)
        for t, (rlo, g) in enumerate(got["gamma"]):                  # gamma at the path is the path posterior
            if rlo <= path[t] < rlo + len(g):
                assert abs(g[path[t] - rlo] - post[t]) <= 1e-12
    assert edge_reached or min(beam, L) == L, name


# ---- faults: what a subtly wrong kernel would compute ----
FAULT_FAMILIES = ["edge_T400_S150_V39_B16_M4_back0", "edge_T400_S150_V39_B64_M4_back1", "steep_T200_S280_V39_B7_M4",
                  "peaked_T200_S60_V39_B16_M4", "geom_T150_S100_V39_B64_M4"]
_CLEAN = {}


def _clean(name):
    if name not in _CLEAN:
        lp, labels, term, beam, mm, ref = _built(name)
        T, L = lp.shape[0], 2 * len(labels) + 1
        lo, hi = R.windows(T, L, beam)
        path = R.mixed_path(ref, (lo, hi), term)
        pref = R.forward_backward(lp, labels, path, beam, mm)
        _CLEAN[name] = (lp, labels, term, beam, mm, ref, path, pref, lo, hi)
    return _CLEAN[name]


def _where(kind, T, lo, hi):
    """The frame (or block) a fault is applied at: one place, as a kernel's slip at one boundary would be."""
    if kind == "lo_high":
        return T // 4
    if kind == "hi_low":
        return 3 * T // 4
    if kind == "bwd_drop_move":
        return (T // 2) // R.CK * R.CK + R.CK - 1
    if kind == "stale_row":
        return (T // 2) // R.CK * R.CK
    if kind == "late_label":
        t = 3 * T // 4
        while t < T - 1 and hi[t] <= hi[t - 1]:
            t += 1
        return t
    if kind == "short_offset":
        return (T // 2) // R.CK
    return None


def _margin(name, kind):
    """The largest distance the fault moves any output of the three calls, in units of that output's tolerance."""
    lp, labels, term, beam, mm, ref, path, pref, lo, hi = _clean(name)
    T, V = lp.shape
    at = _where(kind, T, lo, hi)
    bad = R.ref_at(lp, labels, term, beam, mm, fault=(kind, at))
    pbad = R.forward_backward(lp, labels, path, beam, mm, fault=(kind, at))
    if bad["status"] != R.OK or pbad["status"] != R.OK:
        return np.inf                                   # the fault kills the lattice: a status no test lets pass
    best = abs(bad["ll"] - ref["ll"]) / R.z_tolerance(ref)
    for t in range(T):
        (l0, g0), (l1, g1) = ref["gamma"][t], bad["gamma"][t]
        a = np.zeros(hi[t] - lo[t] + 2)
        a[l1 - lo[t]:l1 - lo[t] + len(g1)] = g1         # a moved window: compare at absolute positions
        b = np.zeros_like(a)
        b[:len(g0)] = g0
        tol = np.maximum(R.state_tolerance(b), R.M_STATE * R.TINY)
        best = max(best, float(np.max(np.abs(a - b) / tol)))
    lab = R.expand(labels)
    occ0, occ1 = np.zeros((T, V)), np.zeros((T, V))
    for t in range(T):
        for occ, r in ((occ0, ref), (occ1, bad)):
            l, g = r["gamma"][t]
            np.add.at(occ[t], lab[l:l + len(g)], g)
    tol = R.label_tolerance(ref["gamma"], labels, V)
    ok = tol > 0
    best = max(best, float(np.max(np.abs(occ1 - occ0)[ok] / tol[ok])))
    tol = np.maximum(R.path_tolerance(pref), R.M_PATH * R.TINY)
    best = max(best, float(np.max(np.abs(pbad["post"] - pref["post"]) / tol)))
    return best


@pytest.mark.parametrize("kind", R.FAULTS)
def test_every_fault_moves_some_family_by_five_tolerances(kind):
    margins = {name: _margin(name, kind) for name in FAULT_FAMILIES}
    print(kind, {k: float(f"{v:.3g}") for k, v in margins.items()})
    assert max(margins.values()) >= 5.0, (kind, margins)
    # the band-edge faults must be seen by an edge-hugging family, not only by chance elsewhere
    # (by a comparison of numbers: a fault that kills the lattice counts as infinite above, but proves nothing here)
    if kind in ("lo_high", "hi_low"):
        assert max(v for k, v in margins.items() if k.startswith("edge") and np.isfinite(v)) >= 5.0, (kind, margins)


def test_error_models_are_what_the_design_says():
    # gamma = 1: the exp2f ulp alone; gamma = 2^-100: half a float32 ulp of 100 (2^-18) in the exponent dominates
    assert R.state_error_model(np.array([1.0]))[0] == 2.0 ** -23
    e = R.state_error_model(np.array([2.0 ** -100]))[0] / 2.0 ** -100
    assert abs(e - (R.LN2 * 2.0 ** -18 + 2.0 ** -23)) < 1e-12
    assert R.state_error_model(np.array([0.0]))[0] == 0.0
    # the label model's floor: 2^-32 per band cell of the bin
    lp, labels, term, beam, mm, ref = _built("geom_T40_S2_V39_B1000_M4")
    E = R.label_error_model(ref["gamma"], labels, lp.shape[1])
    lab = R.expand(labels)
    assert np.all(E[:, [v for v in range(lp.shape[1]) if v not in lab]] == 0.0)
    assert np.all(E[5, 0] >= 3 * 2.0 ** -32)
    # the block offsets: 0 for block 0, the largest alpha of frame 31 for block 1
    assert np.all(R.block_offsets(ref)[:32] == 0.0) and R.block_offsets(ref)[32] == ref["fmax"][31] * R.LOG2E
