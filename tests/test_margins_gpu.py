"""ka_ctc_path_margins on the GPU against tests/margin_ref.py, bit for bit: every comparison is on the stored bits of the
doubles.  The inputs are tests/margin_cases.py (tests/test_margins_cpu.py shows what they exercise and that each planted fault
would be noticed on them).  The raw caller below goes to the C ABI on host or device buffers whose rows are longer than V and
whose outputs are views into sentinel-filled buffers, and never through the Python front end; the front end has its own test."""
import ctypes

import numpy as np
import pytest

import margin_cases as C
import margin_ref as R

pytestmark = pytest.mark.gpu

GUARD, F_SENT, I_SENT, PAD = 4, -7.0, -9, 3
_ptrs = lambda xs: ctypes.cast((ctypes.c_void_p * len(xs))(*xs), ctypes.POINTER(ctypes.c_void_p))
_i64 = lambda xs: (ctypes.c_int64 * len(xs))(*[int(v) for v in xs])


@pytest.fixture(scope="module")
def env():
    from fb_harness import engine
    return engine()


def margin_call(eng, _lib, lats, unit, mem="host", runner=True, tables=True, statuses=True, score=True):
    """One ka_ctc_path_margins_batch_f32 call on the case dicts `lats`.  Host rows have ld = V + PAD with NaN in the padding;
    every output lies inside a buffer with GUARD sentinels on either side, which must survive.  Returns (rc, [answer dicts in
    margin_ref's form], raw output buffers)."""
    import torch
    n = len(lats)
    V = lats[0]["lp"].shape[1]
    dev = mem == "device"
    keep, addr = [], {k: [] for k in ("lp", "lab", "tab", "path", "thr", "alt", "run")}
    outs = []

    def place(a):
        if dev:
            t = torch.from_numpy(a).cuda()
            keep.append(t)
            return t, t.data_ptr()
        keep.append(a)
        return a, a.ctypes.data

    for c in lats:
        T = c["lp"].shape[0]
        rows = np.full((T, V + PAD), np.nan, np.float32)
        rows[:, :V] = c["lp"]
        addr["lp"].append(place(rows)[1])
        lab = np.ascontiguousarray(c["labels"], np.int32)
        addr["lab"].append(place(lab)[1] if len(lab) else None)
        addr["tab"].append(place(np.ascontiguousarray(c["band_lo"], np.int32))[1] if tables and c["band_lo"] is not None else None)
        addr["path"].append(place(np.ascontiguousarray(c["path"], np.int32))[1])
        o = {}
        for key, dtype, sent in (("thr", np.float64, F_SENT), ("alt", np.float64, F_SENT), ("run", np.int32, I_SENT)):
            buf, base = place(np.full(T + 2 * GUARD, sent, dtype))
            o[key] = buf
            addr[key].append(base + GUARD * np.dtype(dtype).itemsize)
        outs.append(o)
    if any(a is None for a in addr["lab"]):       # S = 0: any non-NULL address will do, nothing is read
        addr["lab"] = [a if a is not None else addr["path"][i] for i, a in enumerate(addr["lab"])]
    sc = np.full(n, F_SENT, np.float64)
    st = np.full(n, 99, np.int32)
    if dev:
        torch.cuda.synchronize()
    rc = eng.lib.ka_ctc_path_margins_batch_f32(
        eng.handle, n, _ptrs(addr["lp"]), _i64([c["lp"].shape[0] for c in lats]), V, _i64([V + PAD] * n), _ptrs(addr["lab"]),
        _i64([len(c["labels"]) for c in lats]), int(lats[0]["beam"]), int(lats[0]["mm"]),
        _ptrs(addr["tab"]) if any(a is not None for a in addr["tab"]) else None, _ptrs(addr["path"]), int(unit), _ptrs(addr["thr"]),
        _ptrs(addr["alt"]), _ptrs(addr["run"]) if runner else None, sc.ctypes.data if score else None,
        st.ctypes.data if statuses else None, _lib.KA_MEM_DEVICE if dev else _lib.KA_MEM_HOST, None)
    answers = []
    for c, o, z, s in zip(lats, outs, sc, st):
        T = c["lp"].shape[0]
        h = {k: (v.cpu().numpy() if dev else v) for k, v in o.items()}
        for k, sent in (("thr", F_SENT), ("alt", F_SENT), ("run", I_SENT)):
            assert np.all(h[k][:GUARD] == sent) and np.all(h[k][GUARD + T:] == sent), ("a guard was written", k)
        answers.append(dict(status=int(s), through=h["thr"][GUARD:GUARD + T], alt=h["alt"][GUARD:GUARD + T],
                            runner_up=h["run"][GUARD:GUARD + T], score=float(z)))
    return rc, answers, outs


def untouched(a):
    return a["status"] == 99 and np.all(a["through"] == F_SENT) and np.all(a["alt"] == F_SENT) and np.all(a["runner_up"] == I_SENT) \
        and a["score"] == F_SENT


def failed_as_specified(a, status):
    nan = np.int64(0x7ff8000000000000)
    z = R.bits([a["score"]])[0]
    return a["status"] == status and np.all(R.bits(a["through"]) == nan) and np.all(R.bits(a["alt"]) == nan) and \
        np.all(a["runner_up"] == -1) and (a["score"] == -np.inf if status == R.ZERO_MASS else z == nan)


# ---- every case, either unit, alone in a call on host buffers ----
@pytest.mark.parametrize("name", C.NAMES)
def test_case_alone_on_host_buffers(env, name):
    ka, _lib, eng = env
    c = C.case(name)
    for unit in (0, 1):
        rc, (got,), _ = margin_call(eng, _lib, [c], unit)
        assert rc == 0 and C.same(got, C.want(name, unit)), (name, unit)


# ---- all cases of one beam and max_move in one call on device buffers: tables beside NULL entries, both forms ----
@pytest.mark.parametrize("unit", [0, 1])
def test_cases_together_on_device_buffers(env, unit):
    ka, _lib, eng = env
    groups = {}
    for n in C.NAMES:
        c = C.case(n)
        groups.setdefault((c["beam"], c["mm"], c["lp"].shape[1]), []).append(n)
    mixed = 0
    for (beam, mm, V), names in groups.items():
        rc, got, _ = margin_call(eng, _lib, [C.case(n) for n in names], unit, mem="device")
        assert rc == 0
        for n, g in zip(names, got):
            assert C.same(g, C.want(n, unit)), (n, unit)
        mixed += len({C.case(n)["band_lo"] is None for n in names}) == 2
    assert mixed >= 1 and len(groups) < len(C.NAMES)


def test_a_null_table_equals_the_diagonal_band_table(env):
    ka, _lib, eng = env
    for name in ("T65", "wrap", "gen_mm5", "beam_ge_2L"):
        c = dict(C.case(name))
        assert c["band_lo"] is None
        T, L = c["lp"].shape[0], 2 * len(c["labels"]) + 1
        c["band_lo"] = ka.diagonal_band(T, L, c["beam"]).astype(np.int32)
        for mem in ("host", "device"):
            rc, (got,), _ = margin_call(eng, _lib, [c], 1, mem=mem)
            assert rc == 0 and C.same(got, C.want(name, 1)), (name, mem)
    # a table next to a NULL entry in one call
    a, b = C.case("T64"), dict(C.case("T65"))
    b["band_lo"] = ka.diagonal_band(65, 2 * len(b["labels"]) + 1, b["beam"]).astype(np.int32)
    rc, got, _ = margin_call(eng, _lib, [a, b, a], 0)
    assert rc == 0 and C.same(got[0], C.want("T64", 0)) and C.same(got[1], C.want("T65", 0)) and C.same(got[2], C.want("T64", 0))


def test_optional_outputs_may_be_null(env):
    ka, _lib, eng = env
    c = C.case("units")
    rc, (got,), _ = margin_call(eng, _lib, [c], 1, runner=False, statuses=False, score=False)
    want = C.want("units", 1)
    assert rc == 0 and np.array_equal(R.bits(got["through"]), R.bits(want["through"])) and np.array_equal(R.bits(got["alt"]), R.bits(want["alt"]))
    assert np.all(got["runner_up"] == I_SENT) and got["score"] == F_SENT and got["status"] == 99


# ---- 150 one-wavefront and 60 generic lattices in one call, with failures among them ----
# V, beam_size and max_move are one per call, so a call mixes the forms through L: under a beam of 1010 a lattice with
# L <= 1009 runs on one wavefront and one with L >= 1010 in the generic form.
@pytest.fixture(scope="module")
def big_batch():
    beam, mm = 1010, 4
    fam = C.identity_family(30, seed=4242)
    wide = [C.eighths(500 + i, T, S) for i, (T, S) in enumerate(((400, 505), (380, 510), (420, 520)))]
    bases = [(c["lp"], c["labels"]) for c in fam]
    lats, paths = [], {}
    for k in range(210):
        lp, labels = bases[k % len(bases)] if k < 150 else wide[k % len(wide)]
        L = 2 * len(labels) + 1
        band_lo = None
        if k % 3 == 1:                               # a table of its own: the diagonal, four positions below it
            band_lo = np.maximum((L * np.arange(lp.shape[0])) // lp.shape[0] - 4, 0).astype(np.int32)
        key = (k % len(bases) if k < 150 else -1 - k % len(wide), band_lo is not None)
        if key not in paths:
            paths[key] = C.best_or_random_path(lp, labels, beam, mm, band_lo, 0)
        path = paths[key]
        kind = "ok"
        if k % 7 == 3:
            labels = labels.copy()
            labels[len(labels) // 2] = lp.shape[1]
            kind = "bad_label"
        elif k in (10, 160):
            lp = lp.copy()
            lp[lp.shape[0] // 2, 2] = np.nan
            kind = "nan"
        elif k in (22, 172):
            band_lo = np.zeros(lp.shape[0], np.int32)
            band_lo[lp.shape[0] // 2] = 1            # steps down again: no band
            kind = "bad_table"
        elif k in (30, 180):
            lp = lp.copy()
            lp[3, 1] = np.inf
            kind = "posinf"
        elif k in (37, 187):
            path = path.copy()
            path[len(path) // 3] = L
            kind = "bad_path"
        lats.append(dict(lp=lp, labels=labels, path=path.astype(np.int32), beam=beam, mm=mm, band_lo=band_lo, kind=kind,
                         key=key if kind == "ok" else k))      # lattices of one key are the same lattice
    return lats


def test_a_mixed_batch_equals_every_lattice_sent_alone_and_the_reference(env, big_batch):
    ka, _lib, eng = env
    assert [C.fast_form(c) for c in big_batch] == [True] * 150 + [False] * 60
    want_status = dict(ok=0, bad_label=R.BAD_LABEL, nan=R.NAN, bad_table=R.BAD_ARGS, posinf=R.NONFINITE, bad_path=R.BAD_ARGS)
    for unit, mem in ((0, "host"), (1, "device")):
        once = {}
        for c in big_batch:
            if c["key"] not in once:
                once[c["key"]] = R.margins_ref(c["lp"], c["labels"], c["path"], c["beam"], c["mm"], unit, c["band_lo"])
        refs = [once[c["key"]] for c in big_batch]
        assert all(r["status"] == want_status[c["kind"]] for r, c in zip(refs, big_batch) if c["kind"] != "ok")
        assert sum(r["status"] == 0 for r in refs) >= 160 and all(r["status"] in (0, R.ZERO_MASS) for r, c in zip(refs, big_batch) if c["kind"] == "ok")
        rc, got, _ = margin_call(eng, _lib, big_batch, unit, mem=mem)
        assert rc == next(r["status"] for r in refs if r["status"] != 0)      # the call returns its first failed lattice's status
        for i, (c, g, ref) in enumerate(zip(big_batch, got, refs)):
            assert (C.same(g, ref) if ref["status"] == 0 else failed_as_specified(g, ref["status"])), (i, unit, c["kind"], g["status"])
            if unit == 0:
                rc1, (alone,), _ = margin_call(eng, _lib, [c], unit, mem=mem)
                assert rc1 == g["status"] and C.same(alone, g), (i, "alone")


# ---- more lattices than slots: a slot's second lattice inherits a dirty slab, dirty columns and a dirty ring ----
@pytest.mark.parametrize("V,slots,pairs", [(6, 1024, 96), (65, 512, 48)], ids=["one_wavefront", "generic"])
def test_a_reused_slot_gives_the_reference_bits(env, V, slots, pairs):
    ka, _lib, eng = env
    beam, mm = 24, 4
    rng = np.random.default_rng(V)
    pool, refs = [], {}

    def lattice(T, S, spoil=None):
        lp, labels = C.eighths(int(rng.integers(1 << 30)), T, S, V=V)
        path = C.best_or_random_path(lp, labels, beam, mm, None, 1)
        if spoil == "nan":
            lp[T // 2, 1] = np.nan
        elif spoil == "bad_label":
            labels[S // 2] = V
        elif spoil == "zero_mass":
            path[-1] = 0                              # position 0 has left the last frame's band
        c = dict(lp=lp, labels=labels, path=path, beam=beam, mm=mm, band_lo=None)
        refs[id(c)] = R.margins_ref(lp, labels, path, beam, mm, 1)
        return c

    kinds = ("longer", "wider", "nan", "bad_label", "zero_mass")
    first, second = [], []
    for k in range(pairs):
        kind = kinds[k % len(kinds)]
        T2, S2 = int(rng.integers(40, 100)), int(rng.integers(14, 25))
        T1, S1 = (T2 + int(rng.integers(33, 70)), S2) if kind == "longer" else (T2, S2)
        if kind == "wider":
            S1, S2 = int(rng.integers(30, 40)), int(rng.integers(3, 9))
        first.append(lattice(T1, S1, kind if kind in ("nan", "bad_label", "zero_mass") else None))
        second.append(lattice(T2, S2))
    fill = [lattice(int(rng.integers(20, 60)), int(rng.integers(3, 12))) for _ in range(8)]
    lats = first + [fill[i % len(fill)] for i in range(slots - pairs)] + second
    assert len(lats) > slots and all(C.fast_form(c) == (V <= 64) for c in lats)
    assert {refs[id(c)]["status"] for c in first} == {0, R.NAN, R.BAD_LABEL, R.ZERO_MASS} and all(refs[id(c)]["status"] == 0 for c in second)
    rc, got, _ = margin_call(eng, _lib, lats, 1, mem="device")
    assert rc == next(refs[id(c)]["status"] for c in lats if refs[id(c)]["status"] != 0)
    for i, (c, g) in enumerate(zip(lats, got)):
        ref = refs[id(c)]
        assert (C.same(g, ref) if ref["status"] == 0 else failed_as_specified(g, ref["status"])), (i, ref["status"], g["status"])


# ---- arguments and statuses ----
def test_a_bad_unit_writes_nothing(env):
    ka, _lib, eng = env
    for unit in (-1, 2, 7):
        rc, (got,), _ = margin_call(eng, _lib, [C.case("T33")], unit)
        assert rc == _lib.KA_ERR_BAD_ARGS and untouched(got), unit
    with pytest.raises(ValueError):
        c = C.case("T33")
        ka.ctc_path_margins(c["lp"], c["labels"], c["path"], c["beam"], c["mm"], unit="word")


def test_zero_mass_and_the_other_statuses(env):
    ka, _lib, eng = env
    base = C.case("T65")
    L = 2 * len(base["labels"]) + 1
    zero = dict(base, path=base["path"].copy())
    zero["path"][-1] = 0                               # left by the last frame's band: no path ends there
    assert R.margins_ref(zero["lp"], zero["labels"], zero["path"], zero["beam"], zero["mm"])["status"] == R.ZERO_MASS
    dead = dict(base, lp=base["lp"].copy())
    dead["lp"][40, :] = -np.inf                        # -inf is legal, and a whole row of it leaves no path at all
    inf = dict(base, lp=base["lp"].copy())
    inf["lp"][64, 5] = np.inf
    nan = dict(base, lp=base["lp"].copy())
    nan["lp"][0, 0] = np.nan
    out = dict(base, path=base["path"].copy())
    out["path"][7] = -1
    tab = dict(base, band_lo=np.full(65, L, np.int32))
    for mem in ("host", "device"):
        rc, got, _ = margin_call(eng, _lib, [base, zero, dead, inf, nan, out, tab, base], 0, mem=mem)
        assert rc == _lib.KA_ERR_ZERO_MASS
        want = [0, _lib.KA_ERR_ZERO_MASS, _lib.KA_ERR_ZERO_MASS, _lib.KA_ERR_NONFINITE, _lib.KA_ERR_NAN, _lib.KA_ERR_BAD_ARGS,
                _lib.KA_ERR_BAD_ARGS, 0]
        assert [g["status"] for g in got] == want
        for g, s in zip(got, want):
            assert (C.same(g, C.want("T65", 0)) if s == 0 else failed_as_specified(g, s)), s
    with pytest.raises(ValueError):
        ka.ctc_path_margins(zero["lp"], zero["labels"], zero["path"], zero["beam"], zero["mm"])
    with pytest.raises(IndexError):
        ka.ctc_path_margins(base["lp"], base["labels"] + 100, base["path"], base["beam"], base["mm"])


def test_a_reserved_workspace_covers_the_call(env):
    import torch
    ka, _lib, eng = env
    lib = _lib.load_library()
    for name in ("T65", "gen_mm5"):
        c = C.case(name)
        T, S, V = c["lp"].shape[0], len(c["labels"]), c["lp"].shape[1]
        for mem, code in (("host", _lib.KA_MEM_HOST), ("device", _lib.KA_MEM_DEVICE)):
            need = lib.ka_path_margin_workspace_bytes(3, _i64([T] * 3), _i64([S] * 3), V, c["beam"], c["mm"], code)
            assert need > 3 * 32 * 8 * min(c["beam"], 2 * S + 1)
            # the same call once on the default engine: the kernels' code and the buffers of this harness are in place before
            # memory is counted
            margin_call(eng, _lib, [c, c, c], 1, mem=mem)
            fresh = _lib.Engine(torch.cuda.current_device())
            try:
                fresh.reserve(need)
                torch.cuda.synchronize()
                free0 = torch.cuda.mem_get_info()[0]
                rc, got, keep = margin_call(fresh, _lib, [c, c, c], 1, mem=mem)
                assert rc == 0 and torch.cuda.mem_get_info()[0] == free0, (name, mem)
                assert all(C.same(g, C.want(name, 1)) for g in got)
            finally:
                fresh.close()
    assert lib.ka_path_margin_workspace_bytes(1, _i64([0]), _i64([3]), 6, 8, 4, 0) == 0
    assert lib.ka_path_margin_workspace_bytes(1, _i64([5]), _i64([3]), 6, 8, 4, 2) == 0


# ---- the Python front end ----
def test_python_front_end(env):
    import torch
    ka, _lib, eng = env
    c, w0, w1 = C.case("units"), C.want("units", 0), C.want("units", 1)
    lp, lab, path, beam, mm = c["lp"], c["labels"], c["path"], c["beam"], c["mm"]
    margin, runner, score = ka.ctc_path_margins(lp, lab, path, beam, mm)
    assert margin.dtype == np.float64 and runner.dtype == np.int32 and isinstance(score, float)
    assert np.array_equal(R.bits(margin), R.bits(R.margin_of(w0["through"], w0["alt"]))) and np.array_equal(runner, w0["runner_up"])
    assert score == w0["score"] and np.all(margin >= 0) and np.isposinf(margin[-1])
    th, al, ru, sc = ka.ctc_path_margins(lp, lab, path, beam, mm, unit="text", raw=True)
    assert np.array_equal(R.bits(th), R.bits(w1["through"])) and np.array_equal(R.bits(al), R.bits(w1["alt"])) and np.array_equal(ru, w1["runner_up"])
    # a table, None beside a table, statuses
    s = C.case("stairs")
    res, st = ka.ctc_path_margins_batch([lp, s["lp"], lp], [lab, s["labels"], lab + 100], [path, s["path"], path], s["beam"], s["mm"],
                                        unit="text", return_status=True, band_lo=[None, s["band_lo"].astype(np.int64), None])
    assert st == [0, 0, _lib.KA_ERR_BAD_LABEL] and np.all(np.isnan(res[2][0])) and np.all(res[2][1] == -1) and np.isnan(res[2][2])
    ws = C.want("stairs", 1)
    assert np.array_equal(R.bits(res[1][0]), R.bits(R.margin_of(ws["through"], ws["alt"]))) and res[1][2] == ws["score"]
    with pytest.raises(ValueError):
        ka.ctc_path_margins(lp, lab, path[:-1], beam, mm)
    with pytest.raises(ValueError):
        ka.ctc_path_margins(s["lp"], s["labels"], s["path"], s["beam"], s["mm"], band_lo=s["band_lo"][::-1].copy())
    assert ka.ctc_path_margins_batch([], [], []) == []
    # tensors in, tensors out
    (dm, dr, dz), = ka.ctc_path_margins_device([torch.from_numpy(lp).cuda()], [torch.from_numpy(lab).cuda()], [torch.from_numpy(path).cuda()],
                                               beam, mm, unit="text")
    assert dm.is_cuda and dm.dtype == torch.float64 and dr.dtype == torch.int32 and dz == w1["score"]
    assert np.array_equal(R.bits(dm.cpu().numpy()), R.bits(R.margin_of(w1["through"], w1["alt"])))
    m1 = ka.ctc_path_margins(torch.from_numpy(lp).cuda(), lab, path, beam, mm, unit="text")[0]
    assert torch.equal(m1, dm)
    # segments: three of them, the last ending at T
    T = len(path)
    mt = R.margin_of(w1["through"], w1["alt"])
    ends = [15, 31, T]
    got = ka.segment_boundary_margin(mt, ends)
    assert np.array_equal(got, [min(mt[0], mt[15]), min(mt[15], mt[31]), mt[31]])
    assert np.array_equal(ka.segment_boundary_margin(dm, ends), got)
    got = ka.segment_min_margin(margin, ends)
    assert np.array_equal(got, [margin[:15].min(), margin[15:31].min(), margin[31:].min()])
    assert np.array_equal(ka.segment_min_margin(margin, [0, T + 5]), [np.inf, margin.min()])
    m0 = R.margin_of(w0["through"], w0["alt"])
    assert np.all(mt >= m0)
