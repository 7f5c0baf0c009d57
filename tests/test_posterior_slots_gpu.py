"""Workspace slots that a second lattice inherits dirty.  launch_fb_ck runs lattice i of a form on
workgroup i mod grid with at most 1024 one-wavefront and 512 generic workgroups, and a workgroup's lattices share its slot:
checkpoint columns, slab, offsets, LDS columns and label ring.  One batch of more than 1024 one-wavefront lattices and one
of more than 512 generic ones (V = 80) go through the label and the state call, ordered so that a slot's second lattice
follows a longer one, a wider one, one that failed (NaN, bad label, zero mass) and, in the state call, one that recomputed
none of the blocks it asks for, or all but those.  Every lattice's outputs and Z must have the bits of the same lattice
sent alone, and one lattice of every kind must match the float64 reference per cell (posterior_ref.*_ratio).

The path-posterior launch walks no slots: posterior_kernel<Form> takes lats[blockIdx.x], one workgroup per lattice, and plan::posterior_workspace carves offsets and columns per lattice.  The same batches go through
it all the same, so that more than 1024 workgroups of it have run once, and are held to the same bit-equality."""
import numpy as np
import pytest

import posterior_ref as R
from fb_harness import band_width, engine, label_call, path_call, record, state_call

pytestmark = pytest.mark.gpu

BEAM, MM = 64, 4
KINDS = ("after_longer", "after_wider", "after_nan", "after_bad_label", "after_zero_mass", "asks_blocks_not_recomputed",
         "asks_none_of_the_recomputed", "after_no_query")


@pytest.fixture(scope="module")
def env():
    return engine()


def _lattice(rng, T, S, V_used, V):
    lp, labels = R.sloped(T, S, V_used, int(rng.integers(1 << 30)), alpha=0.5, zero_every=5)
    return R.pad_vocabulary(lp, V) if V != V_used else lp, labels


def _frames(rng, T, blocks=None):
    if blocks is None:
        return np.sort(rng.choice(T, min(T, 12), replace=False)).astype(np.int64)
    f = np.concatenate([np.arange(b * R.CK, min(T, (b + 1) * R.CK)) for b in blocks])
    return f[::3].astype(np.int64)


def _batch(V, slots, pairs, seed):
    """[(lp, labels, terminal, frames, kind)] of slots + pairs lattices: lattice slots + k runs on slot k after lattice k."""
    rng = np.random.default_rng(seed)
    first, second = [], []
    for k in range(pairs):
        kind = KINDS[k % len(KINDS)]
        T2, S2 = int(rng.integers(40, 130)), int(rng.integers(3, 25))
        T1, S1 = T2, S2
        f1 = f2 = None
        if kind == "after_longer":
            T1 = T2 + int(rng.integers(33, 120))
        elif kind == "after_wider":
            T1 = T2 = int(rng.integers(80, 130))
            S1, S2 = int(rng.integers(40, 70)), int(rng.integers(2, 12))         # band 64 before band 5 ... 25
        elif kind in ("asks_blocks_not_recomputed", "asks_none_of_the_recomputed"):
            T1 = T2 = int(rng.integers(130, 200))                                # five to seven blocks
            nb = (T2 - 1) // R.CK + 1
            if kind == "asks_blocks_not_recomputed":
                f1, f2 = [0, 2], [1] + list(range(3, nb))
            else:
                f1, f2 = list(range(1, nb)), [0]
        a = _lattice(rng, T1, S1, 39, V)
        b = _lattice(rng, T2, S2, 39, V)
        ta = R.live_terminals(a[0], a[1], BEAM, MM)[0]
        tb = R.live_terminals(b[0], b[1], BEAM, MM)[0]
        lp1, lab1 = a
        if kind == "after_nan":
            lp1 = lp1.copy()
            lp1[T1 // 2, 3] = np.nan
        elif kind == "after_bad_label":
            lab1 = lab1.copy()
            lab1[S1 // 2] = V
        elif kind == "after_zero_mass":
            lp1 = lp1.copy()
            lp1[:, 0] = -np.inf                          # the last blank is reached only through -inf emissions
            ta = 2 * S1
        fr1 = np.zeros(0, np.int64) if kind == "after_no_query" else _frames(rng, T1, f1)
        first.append((lp1, lab1, ta, fr1, "first_of_" + kind))
        second.append((b[0], b[1], tb, _frames(rng, T2, f2), kind))
    pool = []
    for _ in range(16):                                  # the slots nobody inherits: a few small lattices in turn
        lp, labels = _lattice(rng, int(rng.integers(20, 60)), int(rng.integers(1, 12)), 39, V)
        pool.append((lp, labels, R.live_terminals(lp, labels, BEAM, MM)[0], _frames(rng, lp.shape[0]), "filler"))
    return first + [pool[i % len(pool)] for i in range(slots - pairs)] + second


def _bits(a):
    return np.ascontiguousarray(a).view(np.int32 if a.dtype == np.float32 else np.int64)


def _path_of(lat):
    lp, labels, term = lat[:3]
    T, L = lp.shape[0], 2 * len(labels) + 1
    p = np.minimum(L - 1, (L * np.arange(T)) // T).astype(np.int32)
    p[-1] = term
    return p


@pytest.mark.parametrize("V,slots,pairs", [(39, 1024, 136), (80, 512, 72)], ids=["one_wavefront_1160", "generic_584"])
def test_a_reused_slot_gives_the_bits_of_a_lattice_sent_alone(env, V, slots, pairs):
    ka, _lib, eng = env
    lats = _batch(V, slots, pairs, seed=V)
    n = len(lats)
    assert n > slots and all(R.fast_form(len(x[1]), V, BEAM, MM) == (V <= 64) for x in lats)
    lps, labs, terms, frs = ([x[i] for x in lats] for i in range(4))
    paths = [_path_of(x) for x in lats]
    gs, los, z_s, st_s, _ = state_call(eng, _lib, lps, labs, terms, frs, BEAM, MM)
    occs, z_l, st_l, _ = label_call(eng, _lib, lps, labs, terms, BEAM, MM)
    posts, z_p, st_p, _ = path_call(eng, _lib, lps, labs, paths, BEAM, MM)
    want_status = {"first_of_after_nan": _lib.KA_ERR_NAN, "first_of_after_bad_label": _lib.KA_ERR_BAD_LABEL,
                   "first_of_after_zero_mass": _lib.KA_ERR_ZERO_MASS}
    seen = {}
    for i, (lp, labels, term, fr, kind) in enumerate(lats):
        assert st_s[i] == st_l[i] == st_p[i] == want_status.get(kind, 0), (i, kind, st_s[i], st_l[i], st_p[i])
        if kind == "filler" and id(lp) in seen:          # a filler sent alone once: its later copies must equal the first
            j = seen[id(lp)]
            g1, lo1, zs1, occ1, zl1, post1, zp1 = gs[j], los[j], z_s[j:j + 1], occs[j], z_l[j:j + 1], posts[j], z_p[j:j + 1]
        else:
            seen[id(lp)] = i
            (g1,), (lo1,), zs1, s1, _ = state_call(eng, _lib, [lp], [labels], [term], [fr], BEAM, MM)
            (occ1,), zl1, s2, _ = label_call(eng, _lib, [lp], [labels], [term], BEAM, MM)
            (post1,), zp1, s3, _ = path_call(eng, _lib, [lp], [labels], [paths[i]], BEAM, MM)
            assert s1[0] == s2[0] == s3[0] == st_s[i], (i, kind)
        assert np.array_equal(_bits(gs[i]), _bits(g1)) and np.array_equal(los[i], lo1), ("state", i, kind)
        assert np.array_equal(_bits(occs[i]), _bits(occ1)), ("label", i, kind)
        assert np.array_equal(_bits(posts[i]), _bits(post1)), ("path", i, kind)
        assert _bits(z_s[i:i + 1])[0] == _bits(zs1)[0] and _bits(z_l[i:i + 1])[0] == _bits(zl1)[0] \
            and _bits(z_p[i:i + 1])[0] == _bits(zp1)[0], ("Z", i, kind)
    # one lattice of every kind against the reference: the last of it, which ran on an inherited slot
    worst = dict(state=0.0, label=0.0, path=0.0, z=0.0)
    for kind in KINDS:
        i = max(k for k, x in enumerate(lats) if x[4] == kind)
        assert i >= slots
        lp, labels, term, fr, _ = lats[i]
        ref = R.ref_at(lp, labels, term, BEAM, MM)
        assert ref["status"] == R.OK
        lo, hi = R.windows(lp.shape[0], 2 * len(labels) + 1, BEAM)
        assert np.array_equal(los[i], lo[fr]) and gs[i].shape == (len(fr), band_width(len(labels), BEAM))
        for k, f in enumerate(fr):
            assert np.all(gs[i][k, hi[f] - lo[f]:] == 0.0), (kind, f)
        worst["state"] = max(worst["state"], R.state_ratio(gs[i], fr, ref, kind))
        worst["label"] = max(worst["label"], R.label_ratio(occs[i], ref, labels, kind))
        pref = R.forward_backward(lp, labels, paths[i], BEAM, MM)
        worst["path"] = max(worst["path"], R.path_ratio(posts[i], pref, kind))
        worst["z"] = max(worst["z"], R.z_ratio(z_s[i], ref), R.z_ratio(z_l[i], ref), R.z_ratio(z_p[i], pref))
        assert z_s[i] == z_l[i]
    for call, m in (("state", R.M_STATE), ("label", R.M_LABEL), ("path", R.M_PATH), ("z", R.M_Z)):
        record(call, worst[call], m)
