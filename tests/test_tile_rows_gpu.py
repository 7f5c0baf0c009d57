"""The last, partial 32-row block of the tiled forms and its terminal (tests/tile_rows_cases.py; ka_tiled.hpp: stage_rows and
sum_rows; tests/test_tile_rows_cpu.py asserts that the inputs do what their names say and that a copy which stops at the
block's last whole 16-byte piece would show).

Every case in five kernel forms - both tile widths, the 128-position tiles with the chunk-parallel backtrace, the library's
own choice, and the exact one-wavefront form as the control that must agree - and in six layouts of the log-probs, each a
launch of its own because the staging mode is chosen per launch:

  host     host numpy: the library's own contiguous copies
  aligned  device, row pitch V, base a multiple of 16 bytes: a block is copied as it lies in memory (V = 39 and 64)
  off4     device, row pitch V, base 4 bytes past a multiple of 16: row by row
  ld64     device view with a row pitch of 64 (80 for V = 64) and NaN in the padding columns: row by row
  fenced   `aligned` inside a larger allocation with 64 NaN in front of row 0 and 64 NaN behind row T - 1: a read outside the
           lattice shows as a false KA_ERR_NAN, never as a fault
  mixed    aligned and off4 lattices side by side in one launch: the whole launch goes row by row

The explicit forms run all lattices of one V and beam in one launch; `auto` runs every lattice in a launch of its own (two for
`mixed`), which is how a lone lattice reaches the tiled form by the library's choice.  Path, labels, scores, total and status
are compared with the C oracle bit for bit: no tolerance anywhere.
"""
import os

import numpy as np
import pytest

import tile_rows_cases as C

pytestmark = pytest.mark.gpu

NAN, NONFINITE = -6, -7
PAIRS = [(f, l) for f in C.FORMS for l in C.LAYOUTS]
CONTIGUOUS = ("host", "aligned", "fenced")


@pytest.fixture(scope="module")
def env():
    import torch
    assert torch.cuda.is_available()
    import kokoro_align_amd as ka
    from kokoro_align_amd import _lib
    assert os.path.exists(ka.library_path()), "HIP library not built"
    assert (_lib.KA_ERR_NAN, _lib.KA_ERR_NONFINITE) == (NAN, NONFINITE)
    eng = _lib.default_engine(torch.cuda.current_device())
    yield ka, eng, torch
    eng.set_verify(0)
    eng.set_mode("auto")
    eng.set_tile_width(0)
    eng.set_backtrace("auto")


def set_form(eng, form):
    mode, _, bt = form.partition("+")
    mode, _, width = mode.partition("/")
    eng.set_mode(mode)
    eng.set_tile_width(int(width or 0))
    eng.set_backtrace(bt or ("auto" if mode == "auto" else "serial"))


def view_at(torch, lp, ld, front, behind):
    """lp as a [T, V] view with row pitch `ld` that starts `front` floats into a buffer of NaN with `behind` floats after row T - 1"""
    T, V = lp.shape
    buf = torch.full((front + (T - 1) * ld + V + behind,), float("nan"), dtype=torch.float32, device="cuda")
    x = torch.as_strided(buf, (T, V), (ld, 1), front)
    x.copy_(torch.from_numpy(np.array(lp, dtype=np.float32)))
    assert x.stride(0) == ld and x.data_ptr() == buf.data_ptr() + 4 * front and buf.data_ptr() % 16 == 0
    return x


def place(torch, lp, how):
    V = lp.shape[1]
    if how == "aligned":
        x = view_at(torch, lp, V, 0, 0)
        assert x.data_ptr() % 16 == 0 and x.stride(0) == V
    elif how == "off4":
        x = view_at(torch, lp, V, 1, 0)
        assert x.data_ptr() % 16 == 4 and x.stride(0) == V
    elif how == "ld64":
        x = view_at(torch, lp, 64 if V < 64 else 80, 0, 64)
        assert x.data_ptr() % 16 == 0 and x.stride(0) > V
    else:
        assert how == "fenced"
        x = view_at(torch, lp, V, 64, 64)
        assert x.data_ptr() % 16 == 0 and x.stride(0) == V
    return x


def launch(env, layout, cases):
    """One launch over `cases` [(name, lp, labels, beam)] of one V and one beam: per lattice ((path, labels, scores), status, total).
    A HIP error ends the session: nothing more is started on a device that has faulted."""
    from kokoro_align_amd import _lib
    try:
        return _launch(env, layout, cases)
    except _lib.KAError as e:
        pytest.exit(f"{[c[0] for c in cases][:3]} [{layout}]: {e}", returncode=3)


def _launch(env, layout, cases):
    ka, _, torch = env
    beam = cases[0][3]
    assert all(c[3] == beam and c[1].shape[1] == cases[0][1].shape[1] for c in cases)
    if layout == "host":
        res, status, total = ka.ctc_best_path_batch([c[1] for c in cases], [c[2] for c in cases], beam, C.MM, return_status=True)
        return [([np.asarray(x) for x in r], int(s), t) for r, s, t in zip(res, status, total)]
    from kokoro_align_amd.align import DeviceBatch
    hows = [("aligned", "off4")[i % 2] if layout == "mixed" else layout for i in range(len(cases))]
    lps = [place(torch, c[1], how) for c, how in zip(cases, hows)]
    labs = [torch.from_numpy(np.array(c[2], dtype=np.int32)).cuda() for c in cases]
    batch = DeviceBatch(lps, labs, beam, C.MM)
    status = batch.run(raise_on_error=False)
    return [([x.cpu().numpy() for x in r], int(s), t) for r, s, t in zip(batch.results(), status, batch.total.copy())]


def differs(got, status, total, w):
    """None when the result is the oracle's in every bit, else what first differs."""
    if w is None:
        return None if status == -1 else f"status {status}, want -1 (the reference raises)"
    if status != 0:
        return f"status {status}, want 0"
    for g, x, field in zip(got, w[:3], ("path", "labels", "scores")):
        if g.shape != x.shape:
            return f"{field} has shape {g.shape}"
        bad = np.nonzero(g.view(np.int32) != x.view(np.int32))[0]
        if bad.size:
            t = int(bad[0])
            return f"{field} differs at {bad.size} frames, first at frame {t}: got {g[t]}, want {x[t]}"
    if C.bits(total) != C.bits(w[3]):
        return f"total {float(total)!r} (bits {C.bits(total) & 0xffffffff:#010x}), want {float(w[3])!r} (bits {C.bits(w[3]) & 0xffffffff:#010x})"
    return None


def check_all(env, form, layout, cases):
    """Runs `cases` (any V, any beam) in launches of one V and beam each - lone launches for `auto` - and returns what differs."""
    groups = {}
    for c in cases:
        groups.setdefault((c[1].shape[1], c[3]), []).append(c)
    bad = []
    for group in groups.values():
        if form != "auto":
            units = [group]
        elif layout == "mixed":
            units = [[c, c] for c in group]          # the lattice aligned, and 4 bytes off beside it
        else:
            units = [[c] for c in group]
        for unit in units:
            for c, (got, status, total) in zip(unit, launch(env, layout, unit)):
                why = differs(got, status, total, C.want(*c))
                if why is not None:
                    bad.append(f"{c[0]} [{form}, {layout}]: {why}")
    return bad


def report(bad):
    for line in bad:
        print(line)
    assert not bad, f"{len(bad)} results differ from the oracle:\n" + "\n".join(bad)


RESIDUES = [C.residue(T, V, k) for V in C.VS for T in C.RESIDUE_T for k in C.TERMS]
TWO_TILES = [C.two_tile(T, 39, k) for T in C.TWO_TILE_T for k in C.TERMS]
BLANKS = [C.blank(T, V) for V in C.VS for T in C.RESIDUE_T]


@pytest.mark.parametrize("form,layout", PAIRS)
def test_paths_that_end_on_a_label_cell_of_the_last_partial_block(env, form, layout):
    set_form(env[1], form)
    report(check_all(env, form, layout, RESIDUES))


@pytest.mark.parametrize("form,layout", PAIRS)
def test_a_terminal_below_the_highest_tile_alive(env, form, layout):
    set_form(env[1], form)
    report(check_all(env, form, layout, TWO_TILES))


@pytest.mark.parametrize("form,layout", PAIRS)
def test_paths_that_end_on_the_last_blank(env, form, layout):
    set_form(env[1], form)
    report(check_all(env, form, layout, BLANKS))


@pytest.mark.parametrize("form", ("tiled/128", "tiled/256"))
def test_with_the_hand_off_s_self_checks_on(env, form):
    """ka_engine_set_verify(1 | 2): sentinel-filled halos with every consumed packet checked, a full drain before every publish"""
    eng = env[1]
    set_form(eng, form)
    eng.set_verify(3)
    try:
        bad = check_all(env, form, "aligned", RESIDUES + TWO_TILES) + check_all(env, form, "host", RESIDUES[:len(C.RESIDUE_T) * len(C.TERMS)])
    finally:
        eng.set_verify(0)
    report(bad)


def trio(case, T):
    a, b = C.neighbours(T)
    return [a, case, b]


@pytest.mark.parametrize("form,layout", [(f, l) for f in C.TILED for l in CONTIGUOUS + ("off4",)])
def test_a_nan_in_the_tail_is_an_error(env, form, layout):
    """... of its lattice alone: alone in a launch and as the middle one of three"""
    set_form(env[1], form)
    bad = []
    for T in C.NONFINITE_T:
        for cell in C.nonfinite_cells(T):
            case = C.nonfinite(T, cell, "nan")
            (_, status, _), = launch(env, layout, [case])
            if status != NAN:
                bad.append(f"{case[0]} [{form}, {layout}] alone: status {status}, want {NAN}")
            unit = trio(case, T)
            out = launch(env, layout, unit)
            if out[1][1] != NAN:
                bad.append(f"{case[0]} [{form}, {layout}] in a launch of three: status {out[1][1]}, want {NAN}")
            for i in (0, 2):
                why = differs(*out[i], C.want(*unit[i]))
                if why is not None:
                    bad.append(f"{case[0]} [{form}, {layout}] neighbour {unit[i][0]}: {why}")
    report(bad)


def test_a_nan_in_the_tail_raises_on_the_default_user_path(env):
    """ka.ctc_best_path on host numpy with the engine's defaults"""
    ka, eng, _ = env
    set_form(eng, "auto")
    missed = []
    for T in C.NONFINITE_T:
        for cell in C.nonfinite_cells(T):
            name, lp, lab, beam = C.nonfinite(T, cell, "nan")
            try:
                ka.ctc_best_path(lp, lab, beam_size=beam, max_move=C.MM, verbose=False)
                missed.append(f"{name}: no error")
            except ValueError as e:
                if "NaN" not in str(e):
                    missed.append(f"{name}: {e}")
    report(missed)


@pytest.mark.parametrize("form,layout", [(f, l) for f in C.FORMS for l in CONTIGUOUS + ("off4",)])
def test_minus_infinity_and_huge_magnitudes_in_the_tail_give_the_oracle_s_result(env, form, layout):
    """-inf and -3e31: the scores-only tiles hand the lattice to the exact kernels; a path that reads the cell as its terminal included"""
    set_form(env[1], form)
    bad = []
    for T in C.NONFINITE_T:
        for cell in C.nonfinite_cells(T):
            for value in ("ninf", "huge"):
                case = C.nonfinite(T, cell, value)
                (got, status, total), = launch(env, layout, [case])
                why = differs(got, status, total, C.want(*case))
                if why is not None:
                    bad.append(f"{case[0]} [{form}, {layout}] alone: {why}")
                unit = trio(case, T)
                for c, (got, status, total), what in zip(unit, launch(env, layout, unit), ("neighbour", "in a launch of three", "neighbour")):
                    why = differs(got, status, total, C.want(*c))
                    if why is not None:
                        bad.append(f"{case[0]} [{form}, {layout}] {what} {c[0]}: {why}")
    report(bad)


@pytest.mark.parametrize("form", C.TILED + ("auto",))
@pytest.mark.parametrize("layout", ("host", "aligned"))
def test_a_band_too_wide_for_the_exact_kernels(env, form, layout):
    """1011 positions: an explicit tiled form reports KA_ERR_NONFINITE, the library's own choice redoes the lattice"""
    set_form(env[1], form)
    bad = []
    for value in ("ninf", "huge", "nan"):
        lp, lab, beam = C.wide(value)
        case = (f"wide_{value}", lp, lab, beam)
        (got, status, total), = launch(env, layout, [case])
        if value == "nan":
            why = None if status == NAN else f"status {status}, want {NAN}"
        elif form == "auto":
            why = differs(got, status, total, C.want(*case))
        else:
            why = None if status == NONFINITE else f"status {status}, want {NONFINITE}"
        if why is not None:
            bad.append(f"{case[0]} [{form}, {layout}]: {why}")
    report(bad)
