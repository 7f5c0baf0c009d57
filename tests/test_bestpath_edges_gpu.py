"""The best-path kernels on inputs whose path runs on the band's edges, next to a better cell outside the band and across
the tile borders around a checkpoint (tests/bestpath_cases.py; tests/test_bestpath_edges_cpu.py
asserts that the inputs do that).  Every case in every kernel form that can run it - the seven combinations of
tests/test_gpu_parity.py and the library's own choice - alone and as the middle one of three lattices of different T and S
in one launch.  Path, labels, scores and total are compared with the C oracle bit for bit: no tolerance anywhere.
"""
import os

import numpy as np
import pytest

import bestpath_cases as B
import pbt_ref as P
from oracle import oracle as O

pytestmark = pytest.mark.gpu

PAIRS = [(f, n) for f in B.WAVE for n in B.NAMES if f in B.CASES[n][8]]
_want = {}


def want_of(lp, lab, beam, mm, key):
    """The oracle's answer, computed once per lattice and shared by the forms."""
    if key not in _want:
        try:
            _want[key] = O.ctc_best_path_c(lp, lab, beam, mm, return_total=True)
        except ValueError:
            _want[key] = None
    return _want[key]


@pytest.fixture(scope="module")
def env():
    import torch
    assert torch.cuda.is_available()
    import kokoro_align_amd as ka
    from kokoro_align_amd import _lib
    assert os.path.exists(ka.library_path()), "HIP library not built"
    eng = _lib.default_engine(torch.cuda.current_device())
    yield ka, eng
    eng.set_mode("auto")
    eng.set_tile_width(0)
    eng.set_backtrace("auto")


def set_form(eng, form):
    mode, _, bt = form.partition("+")
    mode, _, width = mode.partition("/")
    eng.set_mode(mode)
    eng.set_tile_width(int(width or 0))
    eng.set_backtrace(bt or ("auto" if mode == "auto" else "serial"))


def explain(name, what, got, total, want, beam):
    """None when the result is the oracle's in every bit, else where it first differs and how far that is from the band's edges."""
    path, labels, scores, wtotal, _ = want
    T, L = len(path), 2 * B.CASES[name][2] + 1 if name in B.CASES else None
    for g, w, field in zip(got, (path, labels, scores), ("path", "labels", "scores")):
        g = np.asarray(g)
        if g.shape != w.shape:
            return f"{name} {what}: {field} has shape {g.shape}"
        bad = np.nonzero(g.view(np.int32) != w.view(np.int32))[0]
        if bad.size:
            t = int(bad[0])
            msg = f"{name} {what}: {field} differs at {bad.size} frames, first at frame {t}: got {g[t]}, want {w[t]}"
            if L is not None:
                lo, hi = P.band(T, L, beam)
                msg += (f"; the oracle's position {path[t]} is {path[t] - lo[t]} above lo = {lo[t]} and {hi[t] - 1 - path[t]} below hi - 1 = {hi[t] - 1}"
                        f" (got position {np.asarray(got[0])[t]})")
            return msg
    if np.float32(total).view(np.int32) != np.float32(wtotal).view(np.int32):
        return f"{name} {what}: total {total!r}, want {wtotal!r}"
    return None


@pytest.mark.parametrize("form,name", PAIRS)
def test_path_labels_scores_and_total_are_the_oracle_s(env, form, name):
    ka, eng = env
    set_form(eng, form)
    lp, lab, beam, mm = B.case(name)
    want = want_of(lp, lab, beam, mm, name)
    # alone
    res, status, total = ka.ctc_best_path_batch([lp], [lab], beam, mm, return_status=True)
    assert list(status) == [0], (name, status)
    why = explain(name, f"[{form}] alone", res[0], total[0], want, beam)
    assert why is None, why
    # the middle one of three lattices of different T and S in one launch
    (lp_a, lab_a), (lp_b, lab_b) = B.companions(name)
    res, status, total = ka.ctc_best_path_batch([lp_a, lp, lp_b], [lab_a, lab, lab_b], beam, mm, return_status=True)
    assert status[1] == 0, (name, status)
    why = explain(name, f"[{form}] in a launch of three", res[1], total[1], want, beam)
    assert why is None, why
    for i, (olp, olab) in ((0, (lp_a, lab_a)), (2, (lp_b, lab_b))):
        w = want_of(olp, olab, beam, mm, (name, i))
        if w is None:
            assert status[i] == -1, (name, i)
            continue
        assert status[i] == 0, (name, i, status)
        why = explain((name, i), f"[{form}] companion", res[i], total[i], w, beam)
        assert why is None, why
