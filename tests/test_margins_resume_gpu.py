"""ka_ctc_margins_resume on the GPU against tests/margin_resume_ref.py and against ka_ctc_path_margins, bit for bit: every
comparison is on the stored bits of the doubles, none has a tolerance.  The inputs are tests/margin_resume_cases.py
(tests/test_margins_resume_cpu.py shows what they exercise and that each planted fault would be noticed on them).  The raw
caller below goes to the C ABI on host or device buffers whose rows are longer than V and whose outputs are views into
sentinel-filled buffers, and never through the Python front end; the front end has its own tests at the end."""
import ctypes

import numpy as np
import pytest

import margin_cases as C
import margin_ref as R
import margin_resume_cases as MC
import margin_resume_ref as RR
from test_margins_gpu import margin_call

pytestmark = pytest.mark.gpu

GUARD, F_SENT, I_SENT, PAD = 4, -7.0, -9, 3
ALL = ("through", "alt", "runner_up", "rows", "d_out", "e_out")
_ptrs = lambda xs: ctypes.cast((ctypes.c_void_p * len(xs))(*xs), ctypes.POINTER(ctypes.c_void_p))
_i64 = lambda xs: (ctypes.c_int64 * len(xs))(*[int(v) for v in xs])


@pytest.fixture(scope="module")
def env():
    from fb_harness import engine
    return engine()


def req(c, lo=0, hi=None, d_in=None, e_in=None, terminal=-1, frames=(), want=ALL, path=True, table=True):
    """Frames [lo, hi) of a case (tests/margin_cases.py's or margin_resume_cases.py's dicts) as one lattice of a call."""
    hi = c["lp"].shape[0] if hi is None else hi
    band = c["band_lo"]
    return dict(lp=c["lp"][lo:hi], labels=c["labels"], beam=c["beam"], mm=c["mm"], band_lo=None if band is None or not table else band[lo:hi],
                path=c["path"][lo:hi] if path else None, d_in=d_in, e_in=e_in, terminal=terminal, frames=np.asarray(frames, np.int64),
                want=tuple(want), unit=c.get("unit", 0))


def resume_call(eng, _lib, reqs, mem="host", unit=None, statuses=True, score=True, ld_extra=2, patch=None):
    """One ka_ctc_margins_resume_batch_f32 call.  Host log-prob rows have ld = V + PAD with NaN in the padding; every output
    lies inside a buffer with GUARD sentinels on either side, which must survive; state rows have ld_rows = W + ld_extra with
    sentinels in the padding.  `patch(addr)` may spoil the address tables before the call.  Returns (rc, [answers in
    margin_resume_ref's form: None for what was not asked for])."""
    import torch
    n = len(reqs)
    V = reqs[0]["lp"].shape[1]
    dev = mem == "device"
    keep = []
    keys = ("lp", "lab", "tab", "din", "ein", "path", "thr", "alt", "run", "frames", "rows", "rlo", "dout", "eout")
    addr = {k: [] for k in keys}
    outs, Ks, lds, terms = [], [], [], []

    def place(a):
        if dev:
            t = torch.from_numpy(np.ascontiguousarray(a)).cuda()
            keep.append(t)
            return t, t.data_ptr()
        a = np.ascontiguousarray(a)
        keep.append(a)
        return a, a.ctypes.data

    def guarded(size, dtype, sent):
        buf, base = place(np.full(size + 2 * GUARD, sent, dtype))
        return buf, base + GUARD * np.dtype(dtype).itemsize

    for r in reqs:
        T, S = r["lp"].shape[0], len(r["labels"])
        L, W = 2 * S + 1, max(1, min(r["beam"], 2 * S + 1))
        rows = np.full((T, V + PAD), np.nan, np.float32)
        rows[:, :V] = r["lp"]
        addr["lp"].append(place(rows)[1])
        lab = np.ascontiguousarray(r["labels"], np.int32)
        addr["lab"].append(place(lab if len(lab) else np.zeros(1, np.int32))[1])
        addr["tab"].append(None if r["band_lo"] is None else place(np.ascontiguousarray(r["band_lo"], np.int32))[1])
        addr["din"].append(None if r["d_in"] is None else place(np.asarray(r["d_in"], np.float64))[1])
        addr["ein"].append(None if r["e_in"] is None else place(np.asarray(r["e_in"], np.float64))[1])
        addr["path"].append(None if r["path"] is None else place(np.ascontiguousarray(r["path"], np.int32))[1])
        o, w = {}, r["want"]
        K = len(r["frames"]) if "rows" in w else 0
        fr = np.ascontiguousarray(r["frames"], np.int64)
        keep.append(fr)
        addr["frames"].append(fr.ctypes.data if K else None)       # (host memory in both modes)
        ld = W + ld_extra
        for key, name, size, dtype, sent in (("thr", "through", T, np.float64, F_SENT), ("alt", "alt", T, np.float64, F_SENT),
                                             ("run", "runner_up", T, np.int32, I_SENT), ("dout", "d_out", L, np.float64, F_SENT),
                                             ("eout", "e_out", L, np.float64, F_SENT)):
            if name in w:
                o[key], a = guarded(size, dtype, sent)
                addr[key].append(a)
            else:
                addr[key].append(None)
        if K:
            o["rows"], a = guarded(K * ld, np.float64, F_SENT)
            addr["rows"].append(a)
            o["rlo"], a = guarded(K, np.int64, I_SENT)
            addr["rlo"].append(a)
        else:
            addr["rows"].append(None)
            addr["rlo"].append(None)
        outs.append((o, T, L, W, K, ld))
        Ks.append(K)
        lds.append(ld)
        terms.append(r["terminal"])
    sc = np.full(n, F_SENT, np.float64)
    st = np.full(n, 99, np.int32)
    extra = dict(K=Ks, ld_rows=lds, unit=reqs[0]["unit"] if unit is None else unit)
    if patch:
        patch(addr, extra)
    if dev:
        torch.cuda.synchronize()
    arr = lambda k: _ptrs(addr[k]) if any(a is not None for a in addr[k]) else None
    rc = eng.lib.ka_ctc_margins_resume_batch_f32(
        eng.handle, n, _ptrs(addr["lp"]), _i64([r["lp"].shape[0] for r in reqs]), V, _i64([V + PAD] * n), _ptrs(addr["lab"]),
        _i64([len(r["labels"]) for r in reqs]), int(reqs[0]["beam"]), int(reqs[0]["mm"]), arr("tab"), arr("din"), arr("ein"),
        _i64(terms) if any(t != -1 for t in terms) else None, arr("path"), int(extra["unit"]), arr("thr"), arr("alt"), arr("run"),
        arr("frames"), _i64(extra["K"]) if any(extra["K"]) else None, arr("rows"), _i64(extra["ld_rows"]), arr("rlo"), arr("dout"),
        arr("eout"), sc.ctypes.data if score else None, st.ctypes.data if statuses else None,
        _lib.KA_MEM_DEVICE if dev else _lib.KA_MEM_HOST, None)
    answers = []
    for (o, T, L, W, K, ld), z, s in zip(outs, sc, st):
        h = {k: (v.cpu().numpy() if dev else v) for k, v in o.items()}
        size = dict(thr=T, alt=T, run=T, dout=L, eout=L, rows=K * ld, rlo=K)
        for k, v in h.items():
            sent = I_SENT if k in ("run", "rlo") else F_SENT
            assert np.all(v[:GUARD] == sent) and np.all(v[GUARD + size[k]:] == sent), ("a guard was written", k)
        cut = lambda k: h[k][GUARD:GUARD + size[k]] if k in h else None
        rows = cut("rows")
        if rows is not None:
            rows = rows.reshape(K, ld)
            assert np.all(rows[:, W:] == F_SENT), "the padding of a state row was written"
            rows = rows[:, :W]
        answers.append(dict(status=int(s), score=float(z), through=cut("thr"), alt=cut("alt"), runner_up=cut("run"), rows=rows,
                            rows_lo=cut("rlo"), d_out=cut("dout"), e_out=cut("eout")))
    return rc, answers


def agree(got, ref, keys=None):
    """`got` (resume_call's answer) against `ref` on what was asked for"""
    keys = [k for k in ("through", "alt", "runner_up", "rows", "rows_lo", "d_out", "e_out") if got[k] is not None] if keys is None else keys
    return RR.same(got, ref, keys)


def untouched(a):
    return a["status"] == 99 and a["score"] == F_SENT and all(
        a[k] is None or np.all(a[k] == (I_SENT if k in ("runner_up", "rows_lo") else F_SENT)) for k in ("through", "alt", "runner_up", "rows", "rows_lo", "d_out", "e_out"))


def failed_as_specified(a, status):
    nan = np.int64(0x7ff8000000000000)
    z = R.bits([a["score"]])[0]
    floats = all(a[k] is None or np.all(R.bits(a[k]) == nan) for k in ("through", "alt", "rows", "d_out", "e_out"))
    ints = all(a[k] is None or np.all(a[k] == -1) for k in ("runner_up", "rows_lo"))
    return a["status"] == status and floats and ints and (a["score"] == -np.inf if status == R.ZERO_MASS else z == nan)


def test_the_three_entry_points_exist(env):
    ka, _lib, eng = env
    lib = _lib.load_library()
    for name in ("ka_ctc_margins_resume_f32", "ka_ctc_margins_resume_batch_f32", "ka_margins_resume_workspace_bytes"):
        assert hasattr(lib, name), name
    assert lib.ka_version() == 104


# ---- property 1: with nothing added the call is ka_ctc_path_margins, outputs, statuses and return code ----
@pytest.mark.parametrize("mem", ["host", "device"])
def test_with_nothing_added_the_call_is_the_sibling(env, mem):
    ka, _lib, eng = env
    groups = {}
    for n in C.NAMES:
        c = C.case(n)
        groups.setdefault((c["beam"], c["mm"], c["lp"].shape[1]), []).append(n)
    forms = set()
    for names in groups.values():
        lats = [C.case(n) for n in names]
        forms |= {(C.fast_form(c), c["band_lo"] is None) for c in lats}
        for unit in (0, 1):
            rc0, sib, _ = margin_call(eng, _lib, lats, unit, mem=mem)
            rc, got = resume_call(eng, _lib, [req(c, want=("through", "alt", "runner_up")) for c in lats], mem, unit=unit)
            assert rc == rc0 == 0
            for n, g, s in zip(names, got, sib):
                assert C.same(g, s) and C.same(g, C.want(n, unit)), (n, unit)
    assert forms == {(True, True), (True, False), (False, True)}
    # the failures: every status and the call's return code
    base = C.case("T65")
    L = 2 * len(base["labels"]) + 1
    zero = dict(base, path=base["path"].copy())
    zero["path"][-1] = 0
    dead = dict(base, lp=base["lp"].copy())
    dead["lp"][40, :] = -np.inf
    inf = dict(base, lp=base["lp"].copy())
    inf["lp"][64, 5] = np.inf
    nan = dict(base, lp=base["lp"].copy())
    nan["lp"][0, 0] = np.nan
    out = dict(base, path=base["path"].copy())
    out["path"][7] = -1
    tab = dict(base, band_lo=np.full(65, L, np.int32))
    lab = dict(base, labels=base["labels"] + 100)
    for lats in ([base, zero, dead, inf, nan, out, tab, lab, base], [lab, base], [nan, inf], [out, zero]):
        rc0, sib, _ = margin_call(eng, _lib, lats, 0, mem=mem)
        rc, got = resume_call(eng, _lib, [req(c, want=("through", "alt", "runner_up")) for c in lats], mem)
        assert rc == rc0 != 0
        for g, s in zip(got, sib):
            assert g["status"] == s["status"] and C.same(g, s)
    # the single-lattice entry point, over a table and over the diagonal
    for name in ("stairs", "T33"):
        c = C.case(name)
        T, V = c["lp"].shape
        lp = np.ascontiguousarray(c["lp"])
        path = np.ascontiguousarray(c["path"], np.int32)
        tab = None if c["band_lo"] is None else np.ascontiguousarray(c["band_lo"], np.int32)
        thr, alt, run, sc = np.empty(T), np.empty(T), np.empty(T, np.int32), np.zeros(1)
        if mem == "host":
            rc = eng.lib.ka_ctc_margins_resume_f32(eng.handle, lp.ctypes.data, T, V, V, c["labels"].ctypes.data, len(c["labels"]), c["beam"],
                                                   c["mm"], None if tab is None else tab.ctypes.data, None, None, -1, path.ctypes.data, 1,
                                                   thr.ctypes.data, alt.ctypes.data, run.ctypes.data, None, 0, None, 0, None, None, None,
                                                   sc.ctypes.data, _lib.KA_MEM_HOST, None)
            assert rc == 0 and C.same(dict(status=0, through=thr, alt=alt, runner_up=run, score=sc[0]), C.want(name, 1))


# ---- properties 2, 3 and 5 on every case: the uncut call against the reference, then every cut against the uncut call ----
@pytest.mark.parametrize("name", MC.NAMES)
def test_a_cut_lattice_gives_the_uncut_calls_bits(env, name):
    ka, _lib, eng = env
    c, ref = MC.case(name), MC.uncut(name)
    T = c["lp"].shape[0]
    mem = "device" if MC.NAMES.index(name) % 2 else "host"
    rc, (whole,) = resume_call(eng, _lib, [req(c, e_in=c["e_in"], frames=c["frames"])], mem)
    assert rc == ref["status"]
    if ref["status"] != 0:
        assert failed_as_specified(whole, ref["status"])
    else:
        assert agree(whole, ref), name
        # property 3: a row reproduces its frame's through, alt and runner_up
        for k, f in enumerate(c["frames"]):
            lo, pt = int(whole["rows_lo"][k]), int(c["path"][f])
            w = min(lo + c["beam"], 2 * len(c["labels"]) + 1) - lo
            th = whole["rows"][k][pt - lo] if lo <= pt < lo + w else -np.inf
            alt, runner = RR.row_alt(whole["rows"][k][:w], lo, pt, c["unit"])
            assert R.bits([th, alt]).tolist() == R.bits([whole["through"][f], whole["alt"][f]]).tolist() and runner == whole["runner_up"][f]
    for cut in c["cuts"]:
        edges = [0, *cut, T]
        chunks = list(zip(edges[:-1], edges[1:]))
        starts, row = [], None
        for a, b in chunks[:-1]:          # forward only: d_out and the score alone
            starts.append(row)
            rc, (fw,) = resume_call(eng, _lib, [req(c, a, b, d_in=row, e_in=np.zeros_like(ref["d_out"]), want=("d_out",), path=False)], mem)
            row = fw["d_out"]
        starts.append(row)
        parts, end = [None] * len(chunks), c["e_in"]
        for i in range(len(chunks) - 1, -1, -1):
            a, b = chunks[i]
            sub = c["frames"][(c["frames"] >= a) & (c["frames"] < b)] - a
            rc, (parts[i],) = resume_call(eng, _lib, [req(c, a, b, d_in=starts[i], e_in=end, frames=sub)], mem)
            end = parts[i]["e_out"]
            if i + 1 < len(chunks) and parts[i]["status"] == 0:      # property 5: d_out alone is d_out with everything asked for
                assert np.array_equal(R.bits(parts[i]["d_out"]), R.bits(starts[i + 1])), (name, cut, i)
        cat = lambda key: np.concatenate([p[key] for p in parts])
        got = dict(status=next((p["status"] for p in reversed(parts) if p["status"] != 0), 0), score=parts[-1]["score"],
                   through=cat("through"), alt=cat("alt"), runner_up=cat("runner_up"), rows=cat("rows"), rows_lo=cat("rows_lo"),
                   d_out=parts[-1]["d_out"], e_out=parts[0]["e_out"])
        assert RR.same(got, ref, MC.CUT_KEYS), (name, cut)
        assert RR.same(got, whole, MC.CUT_KEYS), (name, cut)


# ---- property 4, a batch that mixes NULL and given rows, and what runs: outputs asked for one at a time ----
def test_a_lattice_gives_the_same_bits_alone_and_among_neighbours(env):
    ka, _lib, eng = env
    for names in (("T65", "free_end", "gap"), ("gen_mm5",)):
        lats = []
        for n in names:
            c, T = MC.case(n), MC.case(n)["lp"].shape[0]
            k = 32
            a = RR.resume_ref(c["lp"][:k], c["labels"], c["beam"], c["mm"], c["band_lo"][:k], None, None, np.zeros(2 * len(c["labels"]) + 1))
            b = RR.resume_ref(c["lp"][k:], c["labels"], c["beam"], c["mm"], c["band_lo"][k:], c["path"][k:], a["d_out"], c["e_in"], -1, c["unit"])
            lats += [
                (req(c, e_in=c["e_in"], frames=c["frames"]), None),                                       # nothing given
                (req(c, 0, k, e_in=np.zeros_like(a["d_out"]), want=("d_out",), path=False), None),         # forward only
                (req(c, k, T, d_in=a["d_out"], e_in=c["e_in"], frames=[0, T - k - 1]), None),              # a start row
                (req(c, 0, k, e_in=b["e_out"], frames=[0, k - 1], want=("rows",), path=False), None),      # rows alone, no path
                (req(c, 0, k, e_in=b["e_out"], want=("e_out",), path=False), None),                        # the backward pass for e_out alone
                (req(c, 0, k, e_in=b["e_out"], want=("alt",)), None),                                      # one output of the three
            ]
        reqs = [r for r, _ in lats]
        for mem in ("host", "device"):
            rc, together = resume_call(eng, _lib, reqs, mem)
            assert all(g["status"] != 99 for g in together), _lib.last_error()
            for i, (r, g) in enumerate(zip(reqs, together)):
                rc1, (alone,) = resume_call(eng, _lib, [r], mem)
                assert rc1 == g["status"] and agree(alone, g), (names, i, mem)
                ref = RR.resume_ref(r["lp"], r["labels"], r["beam"], r["mm"], r["band_lo"], r["path"], r["d_in"], r["e_in"], r["terminal"],
                                    r["unit"], r["frames"] if "rows" in r["want"] else ())
                assert (agree(g, ref) if ref["status"] == 0 else failed_as_specified(g, ref["status"])), (names, i, mem)
            assert rc == next((g["status"] for g in together if g["status"] != 0), 0)


# ---- more lattices than workgroups: a workgroup serves a lattice with rows after one without, in a slot left dirty ----
@pytest.mark.parametrize("name,slots", [("T65", 1024), ("gen_V65", 512)], ids=["one_wavefront", "generic"])
def test_a_workgroups_second_lattice_is_not_its_first(env, name, slots):
    ka, _lib, eng = env
    c = MC.case(name)
    T, L = c["lp"].shape[0], 2 * len(c["labels"]) + 1
    k = 32
    a = RR.resume_ref(c["lp"][:k], c["labels"], c["beam"], c["mm"], c["band_lo"][:k], None, None, np.zeros(L))
    plain = req(c, want=("through", "alt", "runner_up"))
    rowed = req(c, k, T, d_in=a["d_out"], frames=[0, 5, T - k - 1])
    bad = req(c, k, T, d_in=np.where(np.arange(L) == L - 1, np.nan, a["d_out"]), frames=[3])
    short = req(c, 0, 3, e_in=np.zeros(L), frames=[1], want=("rows", "d_out"), path=False)
    kinds = dict(plain=plain, rowed=rowed, bad=bad, short=short)
    order = ["plain", "bad", "short", "rowed"]
    first = [order[i % 4] for i in range(slots)]
    second = [order[(i + 3) % 4] for i in range(40)]           # rowed after plain, plain after bad, bad after short, short after rowed
    reqs = [kinds[x] for x in first + second]
    refs = {x: RR.resume_ref(r["lp"], r["labels"], r["beam"], r["mm"], r["band_lo"], r["path"], r["d_in"], r["e_in"], -1, 0,
                             r["frames"] if "rows" in r["want"] else ()) for x, r in kinds.items()}
    assert refs["bad"]["status"] == R.BAD_ARGS and all(refs[x]["status"] == 0 for x in ("plain", "rowed", "short"))
    rc, got = resume_call(eng, _lib, reqs, "device")
    assert rc == R.BAD_ARGS
    for i, (x, g) in enumerate(zip(first + second, got)):
        assert (agree(g, refs[x]) if x != "bad" else failed_as_specified(g, R.BAD_ARGS)), (i, x)


# ---- the failure outputs of every status ----
@pytest.mark.parametrize("mem", ["host", "device"])
def test_a_failed_lattice_has_nan_everywhere(env, mem):
    ka, _lib, eng = env
    c = MC.case("T65")
    T, L = 65, 2 * len(c["labels"]) + 1
    fr = [0, 31, 64]
    nan_row = np.zeros(L)
    nan_row[L - 1] = np.nan                      # (a cell no frame reads)
    inf_row = np.zeros(L)
    inf_row[0] = np.inf
    good = req(c, frames=fr)
    lats = [
        (good, 0),
        (req(dict(c, labels=c["labels"] + 100), frames=fr), R.BAD_LABEL),
        (req(dict(c, lp=np.where(np.arange(T)[:, None] == 9, np.nan, c["lp"]).astype(np.float32)), frames=fr), R.NAN),
        (req(dict(c, lp=np.where(np.arange(T)[:, None] == 9, np.inf, c["lp"]).astype(np.float32)), frames=fr), R.NONFINITE),
        (req(c, d_in=nan_row, frames=fr), R.BAD_ARGS),
        (req(c, e_in=inf_row, frames=fr), R.BAD_ARGS),
        (req(c, terminal=L, frames=fr), R.BAD_ARGS),
        (req(dict(c, path=np.where(np.arange(T) == 7, L, c["path"]).astype(np.int32)), frames=fr), R.BAD_ARGS),
        (req(dict(c, band_lo=np.where(np.arange(T) == 7, 5, 0).astype(np.int32)), frames=fr), R.BAD_ARGS),
        (req(c, d_in=np.full(L, -np.inf), frames=fr), R.ZERO_MASS),
        (req(c, terminal=0, frames=fr), R.ZERO_MASS),      # position 0 has left the last frame's band
        (good, 0),
    ]
    rc, got = resume_call(eng, _lib, [r for r, _ in lats], mem)
    assert rc == R.BAD_LABEL and [g["status"] for g in got] == [s for _, s in lats]
    ref = MC.uncut("T65")
    for g, (_, s) in zip(got, lats):
        assert (agree(g, RR.resume_ref(c["lp"], c["labels"], c["beam"], c["mm"], c["band_lo"], c["path"], frames=fr)) if s == 0
                else failed_as_specified(g, s)), s
    assert np.array_equal(R.bits(got[0]["through"]), R.bits(ref["through"]))
    # a chunk resumed from a failed chunk fails too
    rc, (after,) = resume_call(eng, _lib, [req(c, 32, 65, d_in=got[4]["d_out"], frames=[1])], mem)
    assert rc == R.BAD_ARGS and failed_as_specified(after, R.BAD_ARGS)


# ---- what the host refuses before any launch, with every output untouched ----
def test_bad_arguments_write_nothing(env):
    ka, _lib, eng = env
    c = MC.case("T33")
    T, L = 33, 2 * len(c["labels"]) + 1
    row = np.zeros(L)

    def spoil(**kw):
        def patch(addr, extra):
            for k, v in kw.items():
                if k in extra:
                    extra[k] = v
                elif v == "d_in":
                    addr[k][0] = addr["din"][0] + 8          # an output row that overlaps an input row
                elif v == "e_in":
                    addr[k][0] = addr["ein"][0] - 8 * (L - 1)
                else:
                    addr[k][0] = v
        return patch

    cases = [
        (req(c, frames=[3]), dict(unit=2)),
        (req(c, frames=[5, 3]), {}),
        (req(c, frames=[3, 3]), {}),
        (req(c, frames=[T]), {}),
        (req(c, frames=[-1]), {}),
        (req(c, frames=[3]), dict(ld_rows=[min(c["beam"], L) - 1])),
        (req(c, frames=[3]), dict(K=[T + 1])),
        (req(c, frames=[3]), dict(K=[-1])),
        (req(c, frames=[3]), dict(rows=None)),
        (req(c, frames=[3]), dict(rlo=None)),
        (req(c, frames=[3]), dict(frames=None)),
        (req(c, frames=[3], path=False), {}),                          # through without a path
        (req(c, frames=[3], path=False, want=("rows", "d_out")), {}),   # no end at all
        (req(c, frames=[3], terminal=-2), {}),
        (req(c, frames=[3], d_in=row), dict(dout="d_in")),
        (req(c, frames=[3], e_in=row), dict(eout="e_in")),
        (req(c, frames=[3]), dict(lp=None)),
    ]
    for mem in ("host", "device"):
        for r, kw in cases:
            rc, (got,) = resume_call(eng, _lib, [r], mem, patch=spoil(**kw))
            assert rc == _lib.KA_ERR_BAD_ARGS and untouched(got), (mem, kw, r["frames"])
    # K = 0 is legal, and so is a call that asks for nothing but the score
    rc, (got,) = resume_call(eng, _lib, [req(c, frames=[], want=())], "host")
    assert rc == 0 and got["score"] == MC.uncut("T33")["score"]


def test_a_reserved_workspace_covers_the_call(env):
    import torch
    ka, _lib, eng = env
    lib = _lib.load_library()
    for name in ("T65", "gen_mm5"):
        c = MC.case(name)
        T, S, V = c["lp"].shape[0], len(c["labels"]), c["lp"].shape[1]
        r = req(c, d_in=np.zeros(2 * S + 1), e_in=np.zeros(2 * S + 1), frames=c["frames"])
        K = len(c["frames"])
        for mem, code in (("host", _lib.KA_MEM_HOST), ("device", _lib.KA_MEM_DEVICE)):
            need = lib.ka_margins_resume_workspace_bytes(3, _i64([T] * 3), _i64([S] * 3), _i64([K] * 3), V, c["beam"], c["mm"], code)
            sibling = lib.ka_path_margin_workspace_bytes(3, _i64([T] * 3), _i64([S] * 3), V, c["beam"], c["mm"], code)
            assert need > sibling
            resume_call(eng, _lib, [r, r, r], mem)
            fresh = _lib.Engine(torch.cuda.current_device())
            try:
                fresh.reserve(need)
                torch.cuda.synchronize()
                free0 = torch.cuda.mem_get_info()[0]
                rc, got = resume_call(fresh, _lib, [r, r, r], mem)
                assert rc == 0 and torch.cuda.mem_get_info()[0] == free0, (name, mem)
            finally:
                fresh.close()
    assert lib.ka_margins_resume_workspace_bytes(1, _i64([5]), _i64([3]), _i64([6]), 6, 8, 4, 0) == 0
    assert lib.ka_margins_resume_workspace_bytes(1, _i64([5]), _i64([3]), None, 6, 8, 4, 0) > 0
    assert lib.ka_margins_resume_workspace_bytes(1, _i64([5]), _i64([3]), None, 6, 8, 4, 2) == 0


# ---- the Python front end ----
def test_python_front_end(env):
    import torch
    ka, _lib, eng = env
    c, ref = MC.case("T65"), MC.uncut("T65")
    lp, lab, path, tab, beam, mm, fr = c["lp"], c["labels"], c["path"], c["band_lo"], c["beam"], c["mm"], c["frames"]
    margin, runner, rows, lo, d_out, e_out, score = ka.ctc_margins_resume(lp, lab, tab, path, frames=fr, beam_size=beam, max_move=mm)
    assert margin.dtype == rows.dtype == d_out.dtype == np.float64 and runner.dtype == np.int32 and lo.dtype == np.int64 and isinstance(score, float)
    got = dict(status=0, score=score, through=None, alt=None, runner_up=runner, rows=rows, rows_lo=lo, d_out=d_out, e_out=e_out)
    assert RR.same(got, ref, ("runner_up", "rows", "rows_lo", "d_out", "e_out"))
    assert np.array_equal(R.bits(margin), R.bits(R.margin_of(ref["through"], ref["alt"])))
    # the diagonal (band_lo=None) is ctc_path_margins; rows="d" alone; no path: no margins
    m0, r0, z0 = ka.ctc_path_margins(lp, lab, path, beam, mm)
    m1, r1, _s, _l, d1, e1, z1 = ka.ctc_margins_resume(lp, lab, None, path, rows="d", beam_size=beam, max_move=mm)
    assert np.array_equal(R.bits(m0), R.bits(m1)) and np.array_equal(r0, r1) and z0 == z1 and _s is None and e1 is None
    assert np.array_equal(R.bits(d1), R.bits(d_out))             # (T65's table is the diagonal's)
    m2, r2, s2, l2, d2, e2, z2 = ka.ctc_margins_resume(lp, lab, tab, None, None, ka.free_end_scores(len(d_out)), frames=[3], rows=False,
                                                       beam_size=beam, max_move=mm)
    assert m2 is None and r2 is None and d2 is None and e2 is None and s2.shape == (1, beam) and z2 >= score
    # a cut through the front end, on tensors: rows stay on the device
    k = 32
    dev = lambda x: torch.from_numpy(np.ascontiguousarray(x)).cuda()
    a = ka.ctc_margins_resume(dev(lp[:k]), dev(lab), dev(tab[:k]), None, None, ka.free_end_scores(len(d_out)), rows="d", beam_size=beam, max_move=mm)
    assert a[4].is_cuda and a[4].dtype == torch.float64 and a[0] is None
    b = ka.ctc_margins_resume(dev(lp[k:]), dev(lab), dev(tab[k:]), dev(path[k:]), a[4], None, frames=[0], beam_size=beam, max_move=mm)
    a2 = ka.ctc_margins_resume(dev(lp[:k]), dev(lab), dev(tab[:k]), dev(path[:k]), None, b[5], rows=False, beam_size=beam, max_move=mm)
    assert b[0].is_cuda and b[2].is_cuda and b[3].dtype == torch.int64 and b[6] == score
    cat = np.concatenate([a2[0].cpu().numpy(), b[0].cpu().numpy()])
    assert np.array_equal(R.bits(cat), R.bits(margin)) and np.array_equal(np.concatenate([a2[1].cpu().numpy(), b[1].cpu().numpy()]), runner)
    # the batch form: entries that are None, statuses
    res, st = ka.ctc_margins_resume_batch([lp, lp[k:], lp], [lab, lab, lab + 100], [tab, tab[k:], None], [path, None, path],
                                          [None, a[4].cpu().numpy(), None], [None, int(path[-1]), None], frames=[None, [0, 5], None],
                                          beam_size=beam, max_move=mm, return_status=True)
    assert st == [0, 0, _lib.KA_ERR_BAD_LABEL] and res[1][0] is None and res[1][6] == score and np.isnan(res[2][0]).all() and np.isnan(res[2][4]).all()
    assert np.array_equal(R.bits(res[0][0]), R.bits(margin)) and res[0][2] is None
    assert ka.ctc_margins_resume_batch([], [], []) == []
    for bad in (dict(unit="word"), dict(rows="x"), dict(frames=[5, 3]), dict(d_in=np.zeros(3))):
        with pytest.raises(ValueError):
            ka.ctc_margins_resume(lp, lab, tab, path, beam_size=beam, max_move=mm, **bad)
    with pytest.raises(ValueError):
        ka.ctc_margins_resume(lp, lab, tab, None, beam_size=beam, max_move=mm)           # no end and no path
    with pytest.raises(ValueError):
        ka.ctc_margins_resume(lp, lab, tab, path, np.full(len(d_out), np.nan), beam_size=beam, max_move=mm)


@pytest.mark.parametrize("name", ["T65", "stairs", "gen_mm5", "holes_end"])
def test_state_margins_are_the_reference_rows(env, name):
    ka, _lib, eng = env
    c = MC.case(name)
    term = int(c["path"][-1])
    ref = RR.resume_ref(c["lp"], c["labels"], c["beam"], c["mm"], c["band_lo"], None, None, None, term, 0, c["frames"])
    rows, lo, score = ka.ctc_state_margins(c["lp"], c["labels"], c["path"], c["frames"], c["beam"], c["mm"], band_lo=c["band_lo"])
    with np.errstate(invalid="ignore"):
        assert np.array_equal(R.bits(rows), R.bits(ref["rows"] - ref["score"])) and np.array_equal(lo, ref["rows_lo"]) and score == ref["score"]
    assert np.all(rows <= 0) and np.all(rows.max(axis=1) == 0)
    for k, f in enumerate(c["frames"]):          # 0 on the best path's state (these paths are best paths to their last state)
        assert rows[k, c["path"][f] - lo[k]] == 0
    if name == "T65":                            # the diagonal, and tensors
        import torch
        r2, l2, z2 = ka.ctc_state_margins(torch.from_numpy(c["lp"]).cuda(), c["labels"], term, c["frames"], c["beam"], c["mm"])
        assert r2.is_cuda and np.array_equal(R.bits(r2.cpu().numpy()), R.bits(rows)) and z2 == score


@pytest.mark.parametrize("name", ["T65", "stairs", "gen_V65", "T70"])
def test_chunked_margins_are_the_uncut_calls(env, name):
    ka, _lib, eng = env
    c = MC.case(name)
    T = c["lp"].shape[0]
    args = (c["lp"], c["labels"], c["path"])
    for unit in ("state", "text"):
        want = ka.ctc_path_margins(*args, c["beam"], c["mm"], unit, band_lo=c["band_lo"], raw=True)
        for chunks in (1, 2, 3, 8):
            got = ka.ctc_path_margins_chunked(*args, c["band_lo"], -(-T // chunks), unit, c["beam"], c["mm"], raw=True)
            assert len(range(0, T, -(-T // chunks))) == chunks
            assert all(np.array_equal(R.bits(g), R.bits(w)) for g, w in zip(got[:2], want[:2])) and np.array_equal(got[2], want[2]), (name, chunks)
            assert R.bits([got[3]])[0] == R.bits([want[3]])[0]
    m, r, z = ka.ctc_path_margins_chunked(*args, c["band_lo"], 16, "state", c["beam"], c["mm"])
    m0, r0, z0 = ka.ctc_path_margins(*args, c["beam"], c["mm"], band_lo=c["band_lo"])
    assert np.array_equal(R.bits(m), R.bits(m0)) and np.array_equal(r, r0) and z == z0
    with pytest.raises(ValueError):
        ka.ctc_path_margins_chunked(*args, c["band_lo"], 0)


# ---- StreamingAligner(confidence="margin") ----
@pytest.mark.parametrize("T,tensor", [(256, False), (240, False), (256, True)])
def test_streaming_margins(env, T, tensor):
    import torch
    import track_cases as TC
    ka, _lib, eng = env
    S, beam, mm, period, chunk = 30, 24, 4, 8, 32
    t = np.arange(T)
    read = np.where(t < 100, t, np.where(t < 150, 100, t - 50))          # a pause in the middle: the lines stay apart for a while
    lp, lab = TC.planted(93, T, S, np.minimum(read // 3, 2 * S))
    assert not np.isinf(lp).any() and np.all(lp * 8 == np.round(lp * 8))
    if T == 240:
        lp = lp[:236]                                                   # a ragged last chunk
    T = lp.shape[0]
    whole = ka.ctc_best_path_tracking(lp, lab, beam, mm, period)
    path, table = whole[0], whole[3]
    host = lambda x: x.cpu().numpy() if hasattr(x, "cpu") else np.asarray(x)
    feed = torch.from_numpy(lp).cuda() if tensor else lp
    plain = ka.StreamingAligner(lab, beam, mm, period)
    al = ka.StreamingAligner(lab, beam, mm, period, confidence="margin")
    done, early = 0, 0
    for a in list(range(0, T, chunk)) + [None]:
        out = al.push(feed[a:a + chunk]) if a is not None else al.finish()
        base = plain.push(feed[a:a + chunk]) if a is not None else plain.finish()
        assert len(out) == 5 and len(base) == 4
        assert all(np.array_equal(host(x), host(y)) and x.dtype == y.dtype for x, y in zip(out[:4], base))     # the first four arrays
        conf = out[4]
        assert (conf.dtype == torch.float64 and conf.is_cuda) if tensor else conf.dtype == np.float64
        n = out[0].shape[0]
        assert conf.shape[0] == n
        if n:
            pushed = al.frames_pushed
            if a is not None:     # the whole prefix pushed so far under the concatenated table, with a free end
                ref = RR.resume_ref(lp[:pushed], lab, beam, mm, table[:pushed], path[:pushed], None, np.zeros(2 * S + 1))
                early += n
            else:                 # at finish(): the uncut call of the whole input, to the final path's last state
                ref = RR.resume_ref(lp, lab, beam, mm, table, path)
                th, al_, _r, _z = ka.ctc_path_margins(lp, lab, path, beam, mm, band_lo=table, raw=True)
                assert np.array_equal(R.bits(host(conf)), R.bits(R.margin_of(th, al_)[done:done + n]))
            want = R.margin_of(ref["through"], ref["alt"])[done:done + n]
            assert np.array_equal(R.bits(host(conf)), R.bits(want)), (a, done, n)
            if a is not None:
                assert np.all(host(conf) >= 0)
        done += n
    assert done == T and early > 0
    for bad in ("posterior", "", 2, None):
        with pytest.raises(ValueError):
            ka.StreamingAligner(lab, beam, mm, period, confidence=bad)
    assert ka.StreamingAligner(lab, beam, mm, period, confidence=True).confidence is True
