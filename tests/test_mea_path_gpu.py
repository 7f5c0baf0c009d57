"""The maximum-expected-accuracy alignment on the GPU: ka_ctc_mea_path replayed exactly from the rows
of ka_ctc_state_posteriors on the input families of posterior_ref.edge_cases() and round the 32-frame block edges, held
against the float64 reference within the derived 2 E, every path checked for validity, failed lattices, memory modes and
argument errors, reused workspace slots and the Python layer.  Every figure held against the model is printed through
fb_harness.record."""
import ctypes
import functools
import os
import tempfile

import numpy as np
import pytest

import mea_ref as MR
import posterior_ref as R
from fb_harness import engine, label_call, record, state_call
from mea_harness import EA_SENTINEL, GUARD, SENTINEL, mea_call, mea_call_one

pytestmark = pytest.mark.gpu

CASES = R.edge_cases()
SHAPES = R.case_shapes()
NAMES = list(SHAPES)
SMALL = [k for k, sh in SHAPES.items() if sh[0] <= 700]            # against the float64 reference (whose Python loops the two 3000-frame cases would spend seconds in)
FAST = [k for k in NAMES if R.fast_form(*SHAPES[k][1:])]          # every one-wavefront case, run again in the generic form
NAN64 = 0x7ff8000000000000
ctypes_p64 = ctypes.POINTER(ctypes.c_int64)


@pytest.fixture(scope="module")
def env():
    return engine()


def _bits(x):
    return np.float64(x).tobytes()


@functools.lru_cache(maxsize=None)
def _case(name):
    return CASES[name]()


@functools.lru_cache(maxsize=None)
def _reference(name):
    lp, labels, terminal, beam, mm = _case(name)
    ref = R.ref_at(lp, labels, terminal, beam, mm)
    assert ref["status"] == R.OK, name
    return ref, MR.reference(ref, labels, terminal, beam, mm)


def _checked(what, path, ea, labels, terminal, beam, mm):
    """A returned path buffer: nothing past T, every frame written, a band path that ends at the terminal."""
    T = len(path) - GUARD
    assert np.all(path[T:] == SENTINEL), what
    lo, hi = R.windows(T, 2 * len(labels) + 1, beam)
    assert MR.validity(path[:T], lo, hi, labels, terminal, mm) is None, (what, MR.validity(path[:T], lo, hi, labels, terminal, mm))
    assert 0.0 <= ea <= T, (what, ea)
    return path[:T]


def _replayed(env, what, lp, labels, terminal, beam, mm):
    """One lattice: the kernel's path and value against mea_ref on the state call's rows at every frame, bit for bit."""
    _, _lib, eng = env
    T = lp.shape[0]
    (rows,), (blo,), z_s, st, rc = state_call(eng, _lib, [lp], [labels], [terminal], [np.arange(T)], beam, mm)
    assert rc == 0 and st[0] == 0, (what, rc, st)
    want = MR.replay(rows, blo, labels, terminal, beam, mm)
    assert want["status"] == R.OK, what
    (path,), ea, z, st, rc = mea_call(eng, _lib, [lp], [labels], [terminal], beam, mm)
    assert rc == 0 and st[0] == 0, (what, rc, st)
    path = _checked(what, path, ea[0], labels, terminal, beam, mm)
    assert np.array_equal(path, want["path"]), (what, np.flatnonzero(path != want["path"])[:8])
    assert _bits(ea[0]) == _bits(want["value"]), (what, ea[0], want["value"])
    assert _bits(z[0]) == _bits(z_s[0]), what
    return path, ea[0], z[0]


def test_the_cases_cover_both_forms_and_every_family():
    forms = {(k.split("_")[0], R.fast_form(*SHAPES[k][1:])) for k in NAMES}
    assert forms == {(f, x) for f in ("edge", "steep", "flat", "peaked", "geom") for x in (True, False)}
    assert len(FAST) >= 40


_results = {}


@pytest.mark.parametrize("name", NAMES)
def test_exact_replay_of_the_state_rows(env, name):
    lp, labels, terminal, beam, mm = _case(name)
    _results[name] = _replayed(env, name, lp, labels, terminal, beam, mm)


@pytest.mark.parametrize("name", FAST)
def test_exact_replay_again_in_the_generic_form(env, name):
    lp, labels, terminal, beam, mm = _case(name)
    assert not R.fast_form(len(labels), 80, beam, mm)
    _replayed(env, name, R.pad_vocabulary(lp, 80), labels, terminal, beam, mm)


def _edge_lattice(T, mm, beam, seed):
    """A lattice whose band steps every frame (L / T about 2.9, or as steep as max_move allows) under a transcript with label
    value 0 at every third place, and a live terminal below L - 1 where there is one."""
    slope = {1: 0.0, 2: 0.9, 3: 1.3}.get(mm, 2.9)
    S = int(slope * T / 2)
    lp, labels = R.sloped(T, max(S, 1), 39, seed, alpha=1.0, zero_every=3)
    labels = labels[:S]
    live = R.live_terminals(lp, labels, beam, mm)
    assert live, (T, mm, beam)
    below = [s for s in live if s < 2 * S]
    return lp, labels, (below[0] if below else live[0])


@pytest.mark.parametrize("beam", [7, 1000], ids=["band7", "whole"])
@pytest.mark.parametrize("mm", [1, 2, 3, 4, 6])
@pytest.mark.parametrize("T", [1, 2, 31, 32, 33, 64, 65])
def test_block_edges_by_exact_replay(env, T, mm, beam):
    lp, labels, terminal = _edge_lattice(T, mm, beam, seed=1000 * T + 10 * mm + (beam > 7))
    L = 2 * len(labels) + 1
    assert R.fast_form(len(labels), 39, beam, mm) == (mm <= 4)
    if T >= 31 and mm >= 4:
        assert L / T > 2.7 and (beam > L or (R.band_steps(T, len(labels), beam)[1] > 0.9 and beam < L))   # the band steps every frame
        assert np.any(labels == 0) and terminal < L - 1
    _replayed(env, (T, mm, beam), lp, labels, terminal, beam, mm)


@pytest.mark.parametrize("name", SMALL)
def test_against_the_float64_reference(env, name):
    """Guards against an error shared with the state-posterior call: from the kernel's own states, the chosen successor is
    within 2 E_{t+1} of the best allowed one in the reference's W, and the path's sum of the reference's gamma within 2 E_0 of
    the reference's optimum (mea_ref.choice_ratio)."""
    _, _lib, eng = env
    lp, labels, terminal, beam, mm = _case(name)
    ref, mref = _reference(name)
    if name not in _results:
        (path,), ea, z, st, rc = mea_call(eng, _lib, [lp], [labels], [terminal], beam, mm)
        assert rc == 0 and st[0] == 0
        _results[name] = (_checked(name, path, ea[0], labels, terminal, beam, mm), ea[0], z[0])
    path, ea, z = _results[name]
    step, total = MR.choice_ratio(path, ref, mref, labels, mm)
    E0 = MR.error_bounds(ref)[0]
    record("mea", step, MR.M_MEA)
    record("mea_total", total, MR.M_MEA)
    record("mea_value", abs(ea - mref["value"]) / E0, MR.M_MEA)
    record("z", R.z_ratio(z, ref), R.M_Z)


def _small(rng, V, T=None, S=None):
    T, S = T or int(rng.integers(30, 60)), S or int(rng.integers(3, 20))
    lp, labels = R.sloped(T, S, 39, int(rng.integers(1 << 30)), alpha=0.5, zero_every=5)
    lp = R.pad_vocabulary(lp, V) if V != 39 else lp
    return lp, labels, R.live_terminals(lp, labels, 64, 4)[0]


@pytest.mark.parametrize("V", [39, 80], ids=["one_wavefront", "generic"])
@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
def test_failed_lattices_beside_good_ones(env, V, device):
    _, _lib, eng = env
    rng = np.random.default_rng(41 + V)
    good = _small(rng, V)
    lats, want = [good], [0]
    lp, labels, term = _small(rng, V)
    bad = labels.copy()
    bad[len(bad) // 2] = V
    lats.append((lp, bad, term)); want.append(_lib.KA_ERR_BAD_LABEL)
    for value, code in ((np.nan, _lib.KA_ERR_NAN), (np.inf, _lib.KA_ERR_NONFINITE)):
        lp, labels, term = _small(rng, V)
        lp = lp.copy()
        lp[lp.shape[0] // 2, 3] = value
        lats.append((lp, labels, term)); want.append(code)
    lp, labels, term = _small(rng, V)
    lats.append((lp, labels, 2 * len(labels) + 1)); want.append(_lib.KA_ERR_BAD_ARGS)
    lats.append((lp, labels, -1)); want.append(_lib.KA_ERR_BAD_ARGS)
    lp, labels, term = _small(rng, V)
    lp = lp.copy()
    lp[:, 0] = -np.inf                                    # the last blank is reached only through -inf emissions
    lats.append((lp, labels, 2 * len(labels))); want.append(_lib.KA_ERR_ZERO_MASS)
    lats.append(good); want.append(0)
    lps, labs, terms = ([x[i] for x in lats] for i in range(3))
    paths, ea, z, st, rc = mea_call(eng, _lib, lps, labs, terms, 64, 4, device=device)
    assert rc == want[1] and list(st) == want
    for i, (lp, labels, term) in enumerate(lats):
        T = lp.shape[0]
        assert np.all(paths[i][T:] == SENTINEL), i                                             # nothing written beyond [0, T)
        if want[i]:
            assert np.all(paths[i][:T] == -1) and ea[i:i + 1].view(np.uint64)[0] == NAN64, i
            assert (z[i] == -np.inf) if want[i] == _lib.KA_ERR_ZERO_MASS else np.isnan(z[i]), i
    (alone,), ea1, z1, _, _ = mea_call(eng, _lib, [good[0]], [good[1]], [good[2]], 64, 4)
    _checked("alone", alone, ea1[0], good[1], good[2], 64, 4)
    _, z_label, _, _ = label_call(eng, _lib, [good[0]], [good[1]], [good[2]], 64, 4)
    assert _bits(z1[0]) == _bits(z_label[0])                                                   # the label call's bits
    for i in (0, len(lats) - 1):
        assert np.array_equal(paths[i], alone) and _bits(ea[i]) == _bits(ea1[0]) and _bits(z[i]) == _bits(z1[0])


@pytest.mark.parametrize("V", [39, 80], ids=["one_wavefront", "generic"])
def test_strided_rows_argument_errors_and_the_smallest_lattices(env, V):
    _, _lib, eng = env
    rng = np.random.default_rng(87 + V)
    lp, labels, term = _small(rng, V)
    T = lp.shape[0]
    path, ea, z, rc = mea_call_one(eng, _lib, lp, labels, term, 64, 4)
    assert rc == 0
    _checked("one", path, ea, labels, term, 64, 4)
    path1, ea1, z1, rc = mea_call_one(eng, _lib, lp, labels, term, 64, 4, ld=V + 5)             # the other columns hold NaN
    assert rc == 0 and np.array_equal(path1, path) and _bits(ea1) == _bits(ea) and _bits(z1) == _bits(z)
    (pd,), ead, zd, st, rc = mea_call(eng, _lib, [lp], [labels], [term], 64, 4, device=True)
    assert rc == 0 and np.array_equal(pd, path) and _bits(ead[0]) == _bits(ea) and _bits(zd[0]) == _bits(z)
    # argument errors fail the call before anything is launched: nothing is written
    path2, ea2, z2, rc = mea_call_one(eng, _lib, lp, labels, term, 64, 4, ld=V - 1)
    assert rc == _lib.KA_ERR_BAD_ARGS and np.all(path2 == SENTINEL) and ea2 == EA_SENTINEL
    lpc, labc = np.ascontiguousarray(lp, np.float32), np.ascontiguousarray(labels, np.int32)
    buf = np.full(T, SENTINEL, np.int32)
    e1, zz = np.full(1, EA_SENTINEL), np.zeros(1)
    head = (lpc.ctypes.data, T, V, V, labc.ctypes.data, len(labc))
    call = eng.lib.ka_ctc_mea_path_f32
    assert call(eng.handle, *head, 64, 4, term, None, e1.ctypes.data, zz.ctypes.data, _lib.KA_MEM_HOST, None) == _lib.KA_ERR_BAD_ARGS
    assert call(eng.handle, *head, 64, 4, term, buf.ctypes.data, e1.ctypes.data, zz.ctypes.data, 7, None) == _lib.KA_ERR_BAD_ARGS
    assert call(eng.handle, *head, 64, 0, term, buf.ctypes.data, e1.ctypes.data, zz.ctypes.data, _lib.KA_MEM_HOST, None) == _lib.KA_ERR_BAD_ARGS
    assert call(None, *head, 64, 4, term, buf.ctypes.data, e1.ctypes.data, zz.ctypes.data, _lib.KA_MEM_HOST, None) == _lib.KA_ERR_BAD_ARGS
    assert np.all(buf == SENTINEL) and e1[0] == EA_SENTINEL
    assert call(eng.handle, *head, 64, 4, term, buf.ctypes.data, None, None, _lib.KA_MEM_HOST, None) == 0   # both may be NULL
    assert np.array_equal(buf, path[:T])
    Ts, Ss = (np.array([T], np.int64), np.array([len(labc)], np.int64))
    wb = eng.lib.ka_mea_path_workspace_bytes
    host_bytes = wb(1, Ts.ctypes.data_as(ctypes_p64), Ss.ctypes.data_as(ctypes_p64), V, 64, 4, _lib.KA_MEM_HOST)
    dev_bytes = wb(1, Ts.ctypes.data_as(ctypes_p64), Ss.ctypes.data_as(ctypes_p64), V, 64, 4, _lib.KA_MEM_DEVICE)
    assert host_bytes > dev_bytes >= T * (256 if V <= 64 else 1) and wb(1, Ts.ctypes.data_as(ctypes_p64), Ss.ctypes.data_as(ctypes_p64), V, 64, 4, 7) == 0
    # S = 0 (one blank holds every frame) and T = 1
    for T1, S1 in ((1, 0), (1, 2), (37, 0)):
        lp1 = R.sloped(T1, 1, 39, 5 + T1 + S1)[0]
        lp1 = R.pad_vocabulary(lp1, V) if V != 39 else lp1
        labels1 = np.arange(1, S1 + 1, dtype=np.int32)
        term1 = R.live_terminals(lp1, labels1, 64, 4)[0]
        p1, e1v, _, rc = mea_call_one(eng, _lib, lp1, labels1, term1, 64, 4)
        assert rc == 0
        p1 = _checked((T1, S1), p1, e1v, labels1, term1, 64, 4)
        if S1 == 0:
            assert np.all(p1 == 0) and e1v == T1                                               # gamma is 1.0 exactly in every frame
        if T1 == 1:
            assert p1[0] == term1 and e1v == 1.0


@pytest.mark.parametrize("V,slots,pairs", [(39, 1024, 76), (80, 512, 28)], ids=["one_wavefront_1100", "generic_540"])
def test_a_reused_slot_gives_the_bits_of_a_lattice_sent_alone(env, V, slots, pairs):
    """Lattice slots + k runs on slot k after lattice k (launch_fb_ck: lattice i on workgroup i mod grid): after a wider and
    longer one, which every third time failed after its forward pass or before it.  Stale back-pointers or rings would show."""
    _, _lib, eng = env
    rng = np.random.default_rng(V + 1)
    first, second = [], []
    for k in range(pairs):
        lp, labels, term = _small(rng, V, T=int(rng.integers(48, 65)), S=int(rng.integers(24, 40)))        # band 49 ... 64
        if k % 3 == 1:
            lp = lp.copy()
            lp[:, 0] = -np.inf                            # zero mass: found after the forward pass
            term = 2 * len(labels)
        elif k % 6 == 2:
            labels = labels.copy()
            labels[0] = V                                 # a bad label: found before anything runs
        first.append((lp, labels, term))
        second.append(_small(rng, V, T=int(rng.integers(20, 40)), S=int(rng.integers(2, 10))))               # band 5 ... 19
    pool = [_small(rng, V, T=int(rng.integers(16, 33)), S=int(rng.integers(1, 8))) for _ in range(8)]
    lats = first + [pool[i % len(pool)] for i in range(slots - pairs)] + second
    assert len(lats) == slots + pairs and all(R.fast_form(len(x[1]), V, 64, 4) == (V <= 64) for x in lats)
    lps, labs, terms = ([x[i] for x in lats] for i in range(3))
    paths, ea, z, st, rc = mea_call(eng, _lib, lps, labs, terms, 64, 4)
    assert all(st[i] == (_lib.KA_ERR_ZERO_MASS if i % 3 == 1 else _lib.KA_ERR_BAD_LABEL if i % 6 == 2 else 0) for i in range(pairs))
    assert np.all(st[pairs:] == 0)
    alone = {}
    for i in range(pairs, len(lats)):
        lp, labels, term = lats[i]
        if id(lp) not in alone:
            (p1,), e1, z1, st1, _ = mea_call(eng, _lib, [lp], [labels], [term], 64, 4)
            assert st1[0] == 0
            _checked(i, p1, e1[0], labels, term, 64, 4)
            alone[id(lp)] = (p1, e1[0], z1[0])
        p1, e1, z1 = alone[id(lp)]
        assert np.array_equal(paths[i], p1), (i, "reused" if i >= slots else "filler")
        assert _bits(ea[i]) == _bits(e1) and _bits(z[i]) == _bits(z1), i
    # one of those on an inherited slot by exact replay
    lp, labels, term = lats[-1]
    p, e, _ = _replayed(env, "reused", lp, labels, term, 64, 4)
    assert np.array_equal(paths[-1][:len(p)], p) and _bits(ea[-1]) == _bits(e)


def test_python_layer_gives_the_raw_calls_results(env):
    import torch
    ka, _lib, eng = env
    rng = np.random.default_rng(13)
    lats = [_small(rng, 39), _small(rng, 39, T=70, S=30), _small(rng, 39, T=1, S=2)]
    lps, labs, terms = ([x[i] for x in lats] for i in range(3))
    paths, ea, z, st, rc = mea_call(eng, _lib, lps, labs, terms, 64, 4)
    assert rc == 0
    batch = ka.ctc_mea_path_batch(lps, labs, terms, 64, 4)
    dev, dst = ka.ctc_mea_path_device([torch.from_numpy(x).cuda() for x in lps], [torch.from_numpy(x).cuda() for x in labs], terms, 64, 4,
                                      return_status=True)
    assert dst == [0, 0, 0]
    for i in range(3):
        for p, e, ll in (batch[i], ka.ctc_mea_path(lps[i], labs[i], terms[i], 64, 4)):
            assert p.dtype == np.int32 and isinstance(e, float) and isinstance(ll, float)
            assert np.array_equal(p, paths[i][:-GUARD]) and _bits(e) == _bits(ea[i]) and ll == z[i]
        p, e, ll = dev[i]
        assert p.dtype == torch.int32 and p.is_cuda and np.array_equal(p.cpu().numpy(), paths[i][:-GUARD])
        assert _bits(e) == _bits(ea[i]) and ll == z[i]
    p, e, ll = ka.ctc_mea_path(torch.from_numpy(lps[1]).cuda(), labs[1], ka.ctc_best_path(lps[1], labs[1], 64, 4, verbose=False)[0], 64, 4)
    assert p.is_cuda and p[-1].item() == ka.ctc_best_path(lps[1], labs[1], 64, 4, verbose=False)[0][-1]
    # failures raise, or come back as statuses
    bad = lps[0].copy()
    bad[3, 3] = np.nan
    with pytest.raises(ValueError):
        ka.ctc_mea_path(bad, labs[0], terms[0], 64, 4)
    with pytest.raises(ValueError):
        ka.ctc_mea_path(lps[0], labs[0], 2 * len(labs[0]) + 1, 64, 4)
    res, status = ka.ctc_mea_path_batch([bad, lps[1]], [labs[0], labs[1]], [terms[0], terms[1]], 64, 4, return_status=True)
    assert status == [_lib.KA_ERR_NAN, 0] and np.all(res[0][0] == -1) and np.isnan(res[0][1]) and np.isnan(res[0][2])
    assert np.array_equal(res[1][0], paths[1][:-GUARD]) and _bits(res[1][1]) == _bits(ea[1])
    # the caller's tensors
    out = [torch.full((lps[0].shape[0],), -7, dtype=torch.int32, device="cuda")]
    (p, e, ll), = ka.ctc_mea_path_device([torch.from_numpy(lps[0]).cuda()], [labs[0]], [terms[0]], 64, 4, out=out)
    assert p is out[0] and np.array_equal(p.cpu().numpy(), paths[0][:-GUARD])
    assert ka.ctc_mea_path_batch([], [], []) == []


@pytest.mark.parametrize("V", [39, 80], ids=["one_wavefront", "generic"])
def test_on_a_peaked_lattice_the_path_is_the_best_path(env, V):
    ka, _lib, eng = env
    T, S, beam, mm = 150, 30, 16, 4
    lp, labels, states = MR.unique_peaked(T, S, 39, beam, mm, seed=5)
    ref = R.ref_at(lp, labels, int(states[-1]), beam, mm)
    lpk = R.pad_vocabulary(lp, V) if V != 39 else lp
    best = ka.ctc_best_path(lp, labels, beam, mm, verbose=False)[0]
    path, ea, ll = ka.ctc_mea_path(lpk, labels, best, beam, mm)
    assert np.array_equal(best, states) and np.array_equal(path, best)
    on_best = float(sum(g[p - lo] for (lo, g), p in zip(ref["gamma"], best)))
    assert abs(ea - on_best) <= MR.M_MEA * MR.error_bounds(ref)[0] and T - on_best < 1e-6
    shift, share = ka.segment_path_disagreement(best, path, [50, 120, T + 5], S)
    assert np.all(shift == 0) and np.all(share == 0.0)


def test_path_outputs_round_trip_through_align(env):
    """A g4-style round trip: the posterior-decoded path of a transcript's lattice, saved as a best_path.npz, goes through
    align() unchanged and the align.txt it writes parses."""
    from golden_util import g4
    from kokoro_align_amd.align import _host_log_softmax
    from oracle import oracle as O
    ka, _lib, eng = env
    g = g4()
    rt = g["rt_a"]
    T, segs = rt["T"], rt["segments"]
    labels = np.array(g["read_transcript"], np.int64)
    S = labels.shape[0]
    logits = O.hash_logprobs(T, 39, rt["logits_seed"]) + np.float32(4.0)
    ext = np.zeros(2 * S + 1, np.int64)
    ext[1::2] = labels
    logits[np.arange(T), ext[np.arange(T) * (2 * S + 1) // T]] += 4.0
    lp = _host_log_softmax(logits)
    best = ka.ctc_best_path(lp, labels, verbose=False)
    path, ea, ll = ka.ctc_mea_path(lp, labels, best[0])
    triple = ka.path_outputs(lp, labels, path)
    assert [x.dtype for x in triple] == [x.dtype for x in best] and [x.shape for x in triple] == [x.shape for x in best]
    assert np.array_equal(triple[0], path) and np.array_equal(triple[1], ext[path]) and np.array_equal(triple[2], lp[np.arange(T), ext[path]])
    again = ka.path_outputs(lp, labels, best[0])
    assert all(np.array_equal(a, b) for a, b in zip(again, best))                                # the best path's own triple
    with tempfile.TemporaryDirectory() as td:
        voca, bf, mf, af = (os.path.join(td, n) for n in ("x.voca.txt", "x.best_path.npz", "x.mfcc.npz", "x.align.txt"))
        with open(voca, "wt") as f:
            f.write(g["voca_txt"])
        np.savez(bf, best_path=triple[0], best_labels=triple[1], best_scores=triple[2])
        np.savez(mf, indices=np.array(segs, np.int32), data=np.zeros((T, 1), np.float32))
        ka.align(bf, mf, voca, af, True)
        df = ka.pandas_read_align([af])
        assert len(df) == len(segs) and df["audio_end"].tolist() == [int(x) for x in segs]
        assert abs(df["all_score"].sum() - float(triple[2][:min(int(segs[-1]), T)].sum())) < 1e-2
    shift, share = ka.segment_path_disagreement(best[0], path, segs, S)
    assert len(shift) == len(ka.boundary_frames(segs, T)) and len(share) == len(segs) and np.all((share >= 0) & (share <= 1))
    assert 0.0 < ea <= T
