"""The determined prefix on the GPU (ka_ctc_best_path_determined[_batch]_f32, ka_ctc_best_path_tracking_determined[_batch]_f32,
DESIGN.md section 4.36).  Every comparison is exact: ``determined`` against tests/determined_ref.py on every case of
tests/determined_cases.py (tests/test_determined_cpu.py asserts that the reference and the cases do what they say), every other
output against the parent call's bits through the raw C ABI in both memory modes and both kernel forms; batches that mix forms,
zero-label kernels and failing neighbours; a NULL ``determined``; the workspace figure; and finality itself, by ending the path
at every live cell.
"""
import ctypes

import numpy as np
import pytest

import band_cases as C
import determined_cases as K
import determined_ref as DR
import resume_ref as RR

pytestmark = pytest.mark.gpu

MODES = ("host", "device")
SENTINEL = -7777
SYMBOLS = ("ka_ctc_best_path_determined_f32", "ka_ctc_best_path_determined_batch_f32", "ka_ctc_best_path_tracking_determined_f32",
           "ka_ctc_best_path_tracking_determined_batch_f32", "ka_determined_workspace_bytes")


@pytest.fixture(scope="module")
def env():
    import torch
    assert torch.cuda.is_available()
    import kokoro_align_amd as ka
    from kokoro_align_amd import _lib
    lib = _lib.load_library()
    for sym in SYMBOLS:
        assert hasattr(lib, sym), sym
    return ka, _lib.default_engine(torch.cuda.current_device())


def same_bits(a, b):
    return RR.same_bits(np.asarray(a), np.asarray(b))


def widened(lp):
    """72 more columns (that no label names) take V past 64: the generic kernels"""
    return np.concatenate([lp, np.full((lp.shape[0], 72), -1.0, np.float32)], axis=1)


class Buffers:
    """host arrays, or their copies on the device, handed to the C ABI by address"""

    def __init__(self, mode):
        self.mode, self.keep = mode, []

    def put(self, a):
        if a is None:
            return None
        a = np.ascontiguousarray(a)
        if self.mode == "host":
            self.keep.append((a, a))
            return a.ctypes.data
        import torch
        t = torch.from_numpy(a.copy()).cuda() if a.size else torch.empty(0, device="cuda")
        self.keep.append((a, t))
        return t.data_ptr() if a.size else None

    def fetch(self):
        """copy every device buffer back into its host array"""
        if self.mode == "device":
            for a, t in self.keep:
                if a.size:
                    a[...] = t.cpu().numpy()


def raw_batch(eng, cases, mode, determined, final=True, det_ptr=True, probe=None):
    """One raw batch call of the determined entry point or of its parent over cases of one family, beam, max_move, period and V.
    Returns everything the call wrote (outputs preset to a sentinel).  ``probe``: called right before and right after the C
    call, when every buffer exists; its two answers are returned too."""
    from kokoro_align_amd import _lib
    n = len(cases)
    track = "table" not in cases[0]
    c0 = cases[0]
    V = c0["lp"].shape[1]
    assert all(("table" not in c) == track and c["beam"] == c0["beam"] and c["mm"] == c0["mm"] and c["lp"].shape[1] == V for c in cases)
    buf = Buffers(mode)
    Ts = [c["lp"].shape[0] for c in cases]
    Ss = [len(c["lab"]) for c in cases]
    outs = [[np.full(T, SENTINEL, dt) for T in Ts] for dt in ((np.int32, np.int32, np.float32) + ((np.int32,) if track else ()))]
    fins = [np.full(2 * S + 1, SENTINEL, np.float32) for S in Ss]
    arr = lambda ps: (ctypes.c_void_p * n)(*ps)   # noqa: E731
    i64 = lambda xs: (ctypes.c_int64 * n)(*xs)    # noqa: E731
    ends = np.array([c["end"] for c in cases], np.int32)
    entry, nxt, det = np.full(n, SENTINEL, np.int32), np.full(n, SENTINEL, np.int32), np.full(n, SENTINEL, np.int32)
    status, total = np.full(n, SENTINEL, np.int32), np.full(n, SENTINEL, np.float32)
    p_lp = arr([buf.put(c["lp"]) for c in cases])
    p_lab = arr([buf.put(np.asarray(c["lab"], np.int32)) for c in cases])
    p_init = arr([buf.put(c["init"]) for c in cases])
    p_outs = [arr([buf.put(a) for a in o]) for o in outs]
    p_fin = arr([buf.put(a) for a in fins]) if final else None
    head = (eng.handle, n, p_lp, i64(Ts), V, i64([V] * n), p_lab, i64(Ss), c0["beam"], c0["mm"])
    tail = (total.ctypes.data, status.ctypes.data, _lib.KA_MEM_HOST if mode == "host" else _lib.KA_MEM_DEVICE, None)
    more = (det.ctypes.data if det_ptr else None,) if determined else ()
    before = probe() if probe else None
    if track:
        first = np.array([c["first_lo"] for c in cases], np.int32)
        fn = eng.lib.ka_ctc_best_path_tracking_determined_batch_f32 if determined else eng.lib.ka_ctc_best_path_tracking_resume_batch_f32
        rc = fn(*head, c0["period"], first.ctypes.data, p_init, ends.ctypes.data, *p_outs, p_fin, entry.ctypes.data, nxt.ctypes.data, *more, *tail)
    else:
        p_tab = arr([buf.put(np.asarray(c["table"], np.int32)) for c in cases])
        fn = eng.lib.ka_ctc_best_path_determined_batch_f32 if determined else eng.lib.ka_ctc_best_path_resume_batch_f32
        rc = fn(*head, p_tab, p_init, ends.ctypes.data, *p_outs, p_fin, entry.ctypes.data, *more, *tail)
    after = probe() if probe else None
    buf.fetch()
    return dict(rc=rc, status=status, total=total, outs=outs, fins=fins, entry=entry, nxt=nxt, det=det, probe=(before, after))


def same_lattice(a, i, b, j):
    """lattice i of call a and lattice j of call b: every output but ``determined`` has the same bits"""
    ok = a["status"][i] == b["status"][j] and same_bits(a["total"][i:i + 1], b["total"][j:j + 1])
    ok = ok and a["entry"][i] == b["entry"][j] and a["nxt"][i] == b["nxt"][j] and same_bits(a["fins"][i], b["fins"][j])
    return bool(ok and all(same_bits(x[i], y[j]) for x, y in zip(a["outs"], b["outs"])))


def same_call(a, b):
    return a["rc"] == b["rc"] and all(same_lattice(a, k, b, k) for k in range(len(a["status"])))


def forms_of(c):
    """the case in the forms it runs in: as it is, and (a one-wavefront case) widened into the generic form"""
    if c["form"] == "generic":
        return [("generic", c)]
    return [("wave", c), ("generic", dict(c, lp=widened(c["lp"])))]


@pytest.mark.parametrize("name", K.NAMES)
def test_determined_is_the_reference_and_the_rest_is_the_parent(env, name):
    _, eng = env
    want = K.want(name)[0]
    for form, c in forms_of(K.case(name)):
        for mode in MODES:
            got = raw_batch(eng, [c], mode, True)
            parent = raw_batch(eng, [c], mode, False)
            assert got["det"][0] == want, (name, form, mode, int(got["det"][0]), want)
            assert same_call(got, parent), (name, form, mode)
            assert got["status"][0] == K.FAILING.get(name, got["status"][0])
            if want >= 0 and name not in ("dead_end",):
                assert got["status"][0] == 0
        # ... and where the caller wants no last row the engine's own serves
        got = raw_batch(eng, [c], "device", True, final=False)
        assert got["det"][0] == want and np.all(got["fins"][0] == SENTINEL), (name, form)
        got = raw_batch(eng, [c], "host", True, final=False)
        assert got["det"][0] == want and np.all(got["fins"][0] == SENTINEL), (name, form)


def test_dead_end_is_an_empty_beam_with_determined(env):
    _, eng = env
    got = raw_batch(eng, [K.case("dead_end")], "host", True)
    assert got["rc"] == -1 and got["status"][0] == -1 and got["entry"][0] == -1 and got["det"][0] == K.want("dead_end")[0] > 0
    assert np.all(got["outs"][0][0] == SENTINEL)


def test_python_front_doors(env):
    import torch
    ka, _ = env
    c = K.case("hash_small")
    want = K.want("hash_small")[0]
    parent = ka.ctc_best_path_resume(c["lp"], c["lab"], c["table"], None, "highest", c["beam"], c["mm"])
    got = ka.ctc_best_path_determined(c["lp"], c["lab"], c["table"], None, "highest", c["beam"], c["mm"])
    assert len(got) == 6 and got[5] == want and got[3] == parent[3] and all(same_bits(g, w) for g, w in zip(got[:3] + (got[4],), parent[:3] + (parent[4],)))
    dev = ka.ctc_best_path_determined(torch.from_numpy(c["lp"]).cuda(), c["lab"], c["table"], None, "highest", c["beam"], c["mm"])
    assert dev[5] == want and dev[0].is_cuda and same_bits(dev[0].cpu().numpy(), parent[0])
    res, st, tot = ka.ctc_best_path_determined_batch([c["lp"]] * 2, [c["lab"]] * 2, [c["table"]] * 2, None, ["highest", int(K.case("dead_end")["end"])],
                                                     c["beam"], c["mm"], return_status=True)
    assert st == [0, -1] and res[0][5] == res[1][5] == want
    t = K.case("track_hash_p4_b")
    parent = ka.ctc_best_path_tracking_resume(t["lp"], t["lab"], t["first_lo"], t["init"], "highest", t["beam"], t["mm"], t["period"])
    got = ka.ctc_best_path_tracking_determined(t["lp"], t["lab"], t["first_lo"], t["init"], "highest", t["beam"], t["mm"], t["period"])
    assert len(got) == 8 and got[7] == K.want("track_hash_p4_b")[0] and got[4] == parent[4] and got[6] == parent[6]
    assert all(same_bits(g, w) for g, w in zip(got[:4] + (got[5],), parent[:4] + (parent[5],)))
    dev = ka.ctc_best_path_tracking_determined_device([torch.from_numpy(t["lp"]).cuda()], [t["lab"]], t["first_lo"], [t["init"]], "highest", t["beam"],
                                                      t["mm"], t["period"])[0]
    assert dev[7] == got[7] and dev[3].is_cuda and same_bits(dev[3].cpu().numpy(), parent[3])


# ---- batches ----
def mixed_batch(track):
    """lattices of one beam (1010: a lattice of more than 1009 positions takes the generic form, a shorter one the wavefront's),
    max_move and V: both forms, transcripts with and without label 0, S = 0, start rows, and four that fail on their own"""
    V = K.V_HASH
    pad = lambda lp: np.concatenate([lp, np.full((lp.shape[0], V - lp.shape[1]), -9.0, np.float32)], axis=1) if lp.shape[1] < V else lp  # noqa: E731
    names = ["hash_small", "label0", "wide1010", "S0", "wide1010_flat", "ninf_row", "bad_label", "peaked_small", "nan", "ninf_cells", "pinf_row",
             "flat_small", "hash_big", "drift_generic"]
    cases = []
    for name in names:
        table = None
        if name == "drift_generic":   # 2401 positions under a band of 1010 that climbs 2.4 positions a frame: the band's low edge merges the lines
            T, S = 1000, 1200
            lp, lab = C.planted_lattice(83, T, S, np.minimum(np.arange(T) * (2 * S + 1) // T, 2 * S))
            c = dict(lp=lp, lab=lab, init=None)
            table = K.diagonal(T, 2 * S + 1, 1010)
        else:
            c = K.case(name)
        T = c["lp"].shape[0]
        if track:
            cases.append(dict(lp=pad(c["lp"]), lab=c["lab"], first_lo=0, period=8, beam=1010, mm=4, init=c["init"], end=-1))
        else:
            cases.append(dict(lp=pad(c["lp"]), lab=c["lab"], table=np.zeros(T, np.int64) if table is None else table, beam=1010, mm=4,
                              init=c["init"], end=-1))
    if not track:   # a bad table among them
        bad = dict(cases[0], table=np.arange(cases[0]["lp"].shape[0], dtype=np.int64)[::-1].copy())
        cases.append(bad)
    return names + ([] if track else ["bad_table"]), cases


@pytest.mark.parametrize("track", [False, True])
def test_batch_lattices_get_the_bits_they_have_alone(env, track):
    _, eng = env
    names, cases = mixed_batch(track)
    want = [K.reference(c) for c in cases]
    generic = [min(c["beam"], 2 * len(c["lab"]) + 1) > 1009 for c in cases]
    assert any(generic) and not all(generic) and any(np.any(c["lab"] == 0) for c in cases) and any(not np.any(c["lab"] == 0) for c in cases)
    frames = [c["lp"].shape[0] for c in cases]
    assert sum(w == -1 for w in want) >= 4 and any(w == 0 for w in want) and any(w == T for w, T in zip(want, frames))
    assert any(0 < w < T and g for w, T, g in zip(want, frames, generic)) and any(0 < w < T and not g for w, T, g in zip(want, frames, generic))
    for mode in MODES:
        got = raw_batch(eng, cases, mode, True)
        parent = raw_batch(eng, cases, mode, False)
        assert got["det"].tolist() == want, (mode, names, got["det"].tolist(), want)
        assert same_call(got, parent), mode
        assert sorted(set(got["status"].tolist())) == [-6, -5, -2, 0]
        for i, c in enumerate(cases):
            alone = raw_batch(eng, [c], mode, True)
            assert alone["det"][0] == got["det"][i] and same_lattice(alone, 0, got, i), (mode, names[i])


# ---- bad arguments ----
def test_null_determined_is_bad_args_and_writes_nothing(env):
    from kokoro_align_amd import _lib
    _, eng = env
    for name in ("hash_small", "track_hash_p4_b"):
        for mode in MODES:
            got = raw_batch(eng, [K.case(name)], mode, True, det_ptr=False)
            assert got["rc"] == _lib.KA_ERR_BAD_ARGS, (name, mode)
            assert all(np.all(o[0] == SENTINEL) for o in got["outs"]) and np.all(got["fins"][0] == SENTINEL)
            assert got["entry"][0] == got["nxt"][0] == got["status"][0] == SENTINEL and got["total"][0] == SENTINEL


# ---- workspace ----
def test_workspace_bytes_cover_the_call(env):
    import torch
    from kokoro_align_amd import _lib
    lib = _lib.load_library()
    for track in (0, 1):
        for name in ("hash_big", "wide1010"):
            c = K.case(name)
            T, S = c["lp"].shape[0], len(c["lab"])
            L = 2 * S + 1
            if track:
                c = dict(lp=c["lp"], lab=c["lab"], first_lo=0, period=8, beam=c["beam"], mm=c["mm"], init=c["init"], end=-1)
            want = K.reference(c)
            for mode in MODES:
                mem = _lib.KA_MEM_HOST if mode == "host" else _lib.KA_MEM_DEVICE
                Ts, Ss = (ctypes.c_int64 * 1)(T), (ctypes.c_int64 * 1)(S)
                V = c["lp"].shape[1]
                need = lib.ka_determined_workspace_bytes(1, Ts, Ss, V, c["beam"], c["mm"], mem, track)
                parent = (lib.ka_tracking_resume_workspace_bytes if track else lib.ka_resume_workspace_bytes)(1, Ts, Ss, V, c["beam"], c["mm"], mem)
                own = 0 if mode == "host" else 4 * L
                assert parent + 4 + own <= need <= parent + 256 + own + 256
                assert lib.ka_determined_workspace_bytes(1, Ts, Ss, V, c["beam"], 300, mem, track) == 0
                assert lib.ka_determined_workspace_bytes(1, Ts, Ss, V, c["beam"], c["mm"], 7, track) == 0
                raw_batch(_lib.default_engine(torch.cuda.current_device()), [c], mode, True)   # (the kernels' code is on the device before memory is counted)
                eng = _lib.Engine(torch.cuda.current_device())
                try:
                    eng.reserve(need)

                    def free_bytes():
                        torch.cuda.synchronize()
                        return torch.cuda.mem_get_info()[0]
                    got = raw_batch(eng, [c], mode, True, final=False, probe=free_bytes)   # (no last row of the caller's: the engine's own)
                    assert got["rc"] == 0 and got["det"][0] == want and got["probe"][0] == got["probe"][1], (track, name, mode, want)
                finally:
                    eng.close()


# ---- finality ----
@pytest.mark.parametrize("name", ["hash_small", "peaked_small", "T33", "ninf_cells", "flat_wide_null", "one_cell"])
def test_paths_from_every_live_cell_agree_before_determined_and_not_at_it(env, name):
    _, eng = env
    c = K.case(name)
    d = K.want(name)[0]
    T = c["lp"].shape[0]
    live = DR.live_cells(c["lp"], c["lab"], c["table"], c["init"], c["beam"], c["mm"])
    got = raw_batch(eng, [dict(c, end=int(q)) for q in live], "host", True)
    assert got["rc"] == 0 and not got["status"].any() and np.all(got["det"] == d)
    paths = np.array(got["outs"][0])
    assert np.all(paths[:, -1] == live)
    assert np.all(paths[:, :d] == paths[0, :d])
    if d < T:
        assert len(live) > 1 and np.unique(paths[:, d]).size > 1
    else:
        assert len(live) == 1
    if d == 0:
        assert np.unique(got["entry"]).size == 1
