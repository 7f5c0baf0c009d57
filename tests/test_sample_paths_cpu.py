"""The float64 reference of the path sampler (tests/sample_ref.py) against brute force, against the closed forms it must
agree with, and against its own seeded faults; the new symbols; the host helpers.  No GPU."""
import numpy as np
import pytest

import posterior_ref as R
import sample_ref as S
from fb_harness import assert_declared_exported_bound, tiny

# one case of every family that tests/test_sample_paths_gpu.py runs (all of them run there)
FAMILY_CASES = ("edge_T400_S150_V39_B16_M4_back0", "steep_T200_S280_V39_B7_M4", "flat_T300_S10_V39_B2_M4", "flat_T300_S10_V39_B5_M3",
                "peaked_T200_S60_V39_B16_M4", "peaked_T300_S40_V80_B9_M4", "peaked_T129_S30_V39_B7_M2", "geom_T65_S5_V39_B1000_M4",
                "geom_T120_S40_V39_B1000_M3", "geom_T65_S40_V39_B16_M4")
SEED = 20240


def _case(name):
    return R.edge_cases()[name]()


def test_the_reference_repeats_posterior_refs_forward_pass():
    for name in FAMILY_CASES[:3]:
        lp, labels, term, beam, mm = _case(name)
        ref = R.ref_at(lp, labels, term, beam, mm)
        lo, hi, al = S.alphas(lp, labels, beam, mm)
        assert np.array_equal(np.array([np.max(a) for a in al]), ref["fmax"])
        assert al[-1][term - lo[-1]] == ref["ll"]


FIVE_SIGMA = 5.7e-7      # the two-sided tail of a normal variable beyond 5 standard deviations


def _binomial_tail(c, n, q):
    """min(1, 2 min(P(X <= c), P(X >= c))) for X ~ Binomial(n, q).  "Within 5 standard errors" is a statement about a
    normal variable; a cell expected to hold fewer than 25 of the samples is not one (a single sample in a cell of posterior
    1e-5 lies 5.5 'standard errors' out and happens in 2 % of the runs), so such a cell is held to the same tail probability
    on its exact distribution instead.  The line between the two, n g (1 - g) >= 25, is chosen, not derived: there 5 standard
    errors are 25 samples, and the normal tail is within a small factor of the binomial one."""
    from math import exp, lgamma, log
    if q <= 0.0 or q >= 1.0:
        return 1.0 if c == (0 if q <= 0.0 else n) else 0.0
    pmf = lambda i: exp(lgamma(n + 1) - lgamma(i + 1) - lgamma(n - i + 1) + i * log(q) + (n - i) * log(1.0 - q))
    below = sum(pmf(i) for i in range(0, c + 1))
    return min(1.0, 2.0 * min(below, 1.0 - below + pmf(c)))


def _tiny_lattices():
    rng = np.random.default_rng(11)
    out = []
    for T, Sn, V, beam, mm, zero in ((5, 2, 4, 1000, 4, False), (6, 2, 4, 1000, 4, True), (7, 3, 3, 3, 3, False), (7, 3, 4, 2, 4, True),
                                     (4, 1, 3, 1000, 2, False)):
        lp, labels = tiny(rng, T, Sn, V, zero_label=zero)
        live = R.live_terminals(lp, labels, beam, mm)
        out.append((lp, labels, live[0], beam, mm))
        if len(live) > 1:
            out.append((lp, labels, live[-1], beam, mm))
    return out


def test_path_frequencies_match_brute_force():
    for lp, labels, term, beam, mm in _tiny_lattices():
        want = S.path_probabilities(lp, labels, term, beam, mm)
        lat = S.Lattice(lp, labels, beam, mm)
        counts, n = {}, 0
        for seed in range(320):                                     # 320 x 64 = 20 480 samples
            for row in S.sample_paths(lp, labels, term, 64, SEED + seed, beam, mm, lattice=lat):
                counts[tuple(int(x) for x in row)] = counts.get(tuple(int(x) for x in row), 0) + 1
                n += 1
        assert n >= 20000 and set(counts) <= set(want), "a sampled path is not a path of the band"
        for path, p in want.items():
            se = np.sqrt(p * (1.0 - p) / n)
            assert abs(counts.get(path, 0) / n - p) <= 5.0 * se + 1e-12, (path, counts.get(path, 0) / n, p, se)


@pytest.mark.parametrize("name", ["steep_T200_S280_V39_B7_M4", "geom_T120_S40_V39_B1000_M4"])
def test_occupancy_and_crossing_frames_match_the_closed_forms(name):
    import kokoro_align_amd as ka
    lp, labels, term, beam, mm = _case(name)
    ref = R.ref_at(lp, labels, term, beam, mm)
    lat = S.Lattice(lp, labels, beam, mm)
    T, L, n = lat.T, len(lat.lab), 2048
    paths = np.concatenate([S.sample_paths(lp, labels, term, 64, SEED + i, beam, mm, lattice=lat) for i in range(n // 64)])
    dur = np.zeros(L)
    cuts = np.arange(0, L + 1, max(1, L // 16))
    below = np.zeros((T, len(cuts)))                              # P(state_t < c) = P(tau_c > t)
    for t, (lo, g) in enumerate(ref["gamma"]):
        count = np.bincount(paths[:, t] - lo, minlength=len(g))
        g = np.minimum(g, 1.0)
        se = np.sqrt(g * (1.0 - g) / n)
        common = n * g * (1.0 - g) >= 25.0
        assert np.all(np.abs(count / n - g)[common] <= 5.0 * se[common]), t
        for c, q in zip(count[~common], g[~common]):
            assert _binomial_tail(int(c), n, float(q)) >= FIVE_SIGMA, (t, int(c), float(q))
        dur[lo:lo + len(g)] += g
        below[t] = np.minimum(np.concatenate([np.zeros(1), np.cumsum(g)])[np.clip(cuts - lo, 0, len(g))], 1.0)
    tau = ka.sampled_crossing_frames(paths, cuts).astype(np.float64)
    want = ka.expected_crossing_frames(dur, cuts)
    # the standard error is the true one, from the float64 reference (E tau^2 = sum_t (2t + 1) P(tau > t): in float64 the
    # sum that drowns in float32 holds), not the samples' own: 2048 samples that all agree estimate a deviation of zero
    second = np.sum((2.0 * np.arange(T)[:, None] + 1.0) * below, axis=0)
    se = np.sqrt(np.maximum(second - np.sum(below, axis=0) ** 2, 0.0) / n)
    assert np.allclose(np.sum(below, axis=0), want, rtol=0, atol=1e-9)
    assert np.all(np.abs(tau.mean(axis=0) - want) <= 5.0 * se + 1e-9), (tau.mean(axis=0), want, se)


def test_every_seeded_fault_shows_in_every_family():
    """The four faults of the walk change a path under the suite's own seeds, each in some case of every family.  cdf_not_strict cannot show that way - it needs
    U tot == c_j exactly, an event of probability 2^-53 per draw under hashed uniforms - so it is shown on the draw: with
    u = 0 and a first predecessor of weight 0, '>=' takes that predecessor, which no path of the band passes through."""
    shown = {}
    # (peaked inputs keep nearly all their mass off the band's edges: prev_band shows there on one case at one seed in ten)
    for name, seed in [(n, SEED) for n in FAMILY_CASES] + [("peaked_T300_S40_V80_B9_M4", SEED + 7)]:
        family = name.split("_")[0]
        lp, labels, term, beam, mm = _case(name)
        lat = S.Lattice(lp, labels, beam, mm)
        good = S.sample_paths(lp, labels, term, 64, seed, beam, mm, lattice=lat)
        assert S.check_draws(lat, good, seed, term)[0] == []
        for fault in S.FAULTS[1:]:
            bad = S.sample_paths(lp, labels, term, 64, seed, beam, mm, fault=fault, lattice=lat)
            if np.any(bad != good):
                shown.setdefault(family, set()).add(fault)
                assert S.check_draws(lat, bad, seed, term)[0] != [], (name, fault)     # ... and the draw-by-draw check sees it
        t = np.repeat(np.arange(1, lat.T), [lat.hi[t] - lat.lo[t] for t in range(1, lat.T)])
        p = np.concatenate([np.arange(lat.lo[t], lat.hi[t]) for t in range(1, lat.T)])
        w = lat.weights(t, p)
        pick = np.nonzero((w[:, 0] == 0) & (w.sum(axis=1) > 0))[0]
        assert len(pick), name
        i = pick[0]
        strict, loose = lat.step(t[i:i + 1], p[i:i + 1], np.zeros(1)), lat.step(t[i:i + 1], p[i:i + 1], np.zeros(1), "cdf_not_strict")
        assert loose[0] == p[i] and strict[0] < p[i], (name, int(t[i]), int(p[i]))
    for family in ("edge", "steep", "flat", "peaked", "geom"):
        assert shown.get(family, set()) == set(S.FAULTS[1:]), (family, shown.get(family))


def test_undecidable_draws_are_rare_on_the_references_own_paths():
    """DELTA = 2^-26: the kernel's float64 columns add a few ulp of a value in the hundreds per frame (<~ 2e-13 in log2), over
    the <= 640 frames of these shapes (the 3000-frame edge cases: five times that) <~ 1.5e-10 on a normalised sum; DELTA is
    100 x that.  U is a 53-bit uniform: a draw is undecidable with probability ~ 2 DELTA (M - 1) ~ 1e-7."""
    total, ties = 0, 0
    for name, build in R.edge_cases().items():
        lp, labels, term, beam, mm = build()
        lat = S.Lattice(lp, labels, beam, mm)
        for K in (1, 7, 64):
            paths = S.sample_paths(lp, labels, term, K, SEED + K, beam, mm, lattice=lat)
            n = S.undecidable_draws(lat, paths, SEED + K)
            assert n <= 3, (name, K, n)
            ties += n
            total += K * (lat.T - 1)
    print("undecidable draws:", ties, "of", total)
    assert ties <= 1e-5 * total


def test_the_three_symbols_are_declared_exported_and_bound():
    assert_declared_exported_bound(["ka_ctc_sample_paths_f32", "ka_ctc_sample_paths_batch_f32", "ka_sample_paths_workspace_bytes"])


def test_sampled_crossing_frames_on_hand_made_paths():
    import kokoro_align_amd as ka
    paths = np.array([[0, 0, 1, 2, 2], [0, 1, 1, 1, 2], [0, 0, 0, 0, 0]], np.int32)
    got = ka.sampled_crossing_frames(paths, [0, 1, 2, 3])
    assert got.dtype == np.int64 and np.array_equal(got, [[0, 2, 3, 5], [0, 1, 4, 5], [0, 5, 5, 5]])
    assert ka.sampled_crossing_frames(paths, []).shape == (3, 0)
    with pytest.raises(ValueError):
        ka.sampled_crossing_frames(paths[0], [1])


def test_segment_boundary_spread_on_hand_made_paths():
    import kokoro_align_amd as ka
    best = np.array([0, 1, 1, 2, 3, 4, 4, 4], np.int32)           # S = 2, L = 5
    # boundary frames 0, 3 (seg_ends 3, 8): cuts 2 min(0 // 2, 2) = 0 and 2 min(2 // 2, 2) = 2
    paths = np.array([[0, 1, 2, 2, 3, 4, 4, 4], [0, 0, 1, 2, 3, 4, 4, 4], [0, 1, 1, 1, 2, 3, 4, 4], [0, 0, 0, 1, 1, 2, 4, 4]], np.int32)
    tau2 = np.array([2.0, 3.0, 4.0, 5.0])                         # first frame with state >= 2
    sq, ss, eq, es = ka.segment_boundary_spread(paths, best, [3, 8], 2, q=(0.0, 0.5, 1.0))
    assert sq.shape == eq.shape == (2, 3) and ss.shape == es.shape == (2,)
    assert np.array_equal(sq[0], [0.0, 0.0, 0.0]) and ss[0] == 0.0                    # cut 0 is crossed at frame 0 by every path
    assert np.array_equal(eq[0], [2.0, 3.5, 5.0]) and es[0] == pytest.approx(np.std(tau2))
    assert np.array_equal(sq[1], eq[0]) and ss[1] == es[0]                             # segment 1 starts where segment 0 ends
    assert np.array_equal(eq[1], [8.0, 8.0, 8.0]) and es[1] == 0.0                     # its end lies at T
    # the same cuts as segment_boundary_shift: the mean of tau is its expected crossing frame
    dur = np.array([np.mean(np.sum(paths == s, axis=1)) for s in range(5)])
    start, end = ka.segment_boundary_shift(dur, best, [3, 8], 2)
    assert end[0] == pytest.approx(tau2.mean() - 3.0) and start[0] == 0.0
