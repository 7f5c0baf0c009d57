"""What the best-path batch calls of kokoro_align_amd/align.py send to the C ABI, without a GPU: a stand-in engine writes down
every symbol with its arguments and answers KA_OK.  The lattice is a [:, :5] view of a wider NaN-filled buffer, so the row
pitch and the address show whether the rows were handed over as they lie."""
import ctypes

import numpy as np
import pytest

import band_cases as C

import kokoro_align_amd as ka
from kokoro_align_amd import _lib

T, S, V, LD, BEAM, MM = 12, 4, 5, 9, 4, 4
L = 2 * S + 1
CALLS = ("plain", "banded", "tracking")
SYMBOL = dict(plain="ka_ctc_best_path_batch_f32", banded="ka_ctc_best_path_banded_batch_f32", tracking="ka_ctc_best_path_tracking_batch_f32")
N_ARGS = dict(plain=17, banded=18, tracking=20)
FIRST_OUT = dict(plain=10, banded=11, tracking=12)
OUT_DTYPES = dict(plain=(np.int32, np.int32, np.float32), banded=(np.int32, np.int32, np.float32),
                  tracking=(np.int32, np.int32, np.float32, np.int32))
_TABLES = (ctypes.POINTER(ctypes.c_void_p), ctypes.POINTER(ctypes.c_int64))


class _Recorder:
    """Stands in for ``eng.lib``: every symbol answers KA_OK and is written down with its arguments, the per-lattice tables
    (addresses, int64) as lists, and what the addresses of argument 10 hold as int32 [T_i] (the band tables of a banded call)."""

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        def call(*args):
            n = args[1]
            args = [list(a[:n]) if isinstance(a, _TABLES) else a for a in args]
            behind_max_move = None
            if "_banded_" in name:
                behind_max_move = [np.ctypeslib.as_array(ctypes.cast(ctypes.c_void_p(p), ctypes.POINTER(ctypes.c_int32)), shape=(t,)).copy()
                                   for p, t in zip(args[10], args[3])]
            self.calls.append((name, args, behind_max_move))
            return 0
        return call


@pytest.fixture
def rec(monkeypatch):
    rec = _Recorder()
    monkeypatch.setattr(_lib, "default_engine", lambda device=None: type("Engine", (), dict(lib=rec, handle=None))())
    return rec


@pytest.fixture(scope="module")
def lattice():
    lp, labels = C.random_lattice(12, T, S, V)
    buf = np.full((T, LD), np.nan, np.float32)
    buf[:, :V] = lp
    return buf[:, :V], labels, ka.diagonal_band(T, L, BEAM)


def send(call, lp, labels, table, **kw):
    if call == "plain":
        return ka.ctc_best_path_batch([lp], [labels], BEAM, MM, **kw)
    if call == "banded":
        return ka.ctc_best_path_banded_batch([lp], [labels], [table], BEAM, MM, **kw)
    return ka.ctc_best_path_tracking_batch([lp], [labels], BEAM, MM, 8, "best", **kw)


@pytest.mark.parametrize("call", CALLS)
def test_arguments_at_the_abi(rec, lattice, call):
    lp, labels, table = lattice
    assert table.dtype == np.int64 and lp.strides == (4 * LD, 4)
    results = send(call, lp, labels, table)
    (name, args, behind), = rec.calls
    assert name == SYMBOL[call] and len(args) == N_ARGS[call]
    assert args[1] == 1 and args[3] == [T] and args[4] == V and args[7] == [S] and args[8:10] == [BEAM, MM]
    assert args[-2] == _lib.KA_MEM_HOST and args[-1] is None
    assert args[5] == [LD] and args[2] == [lp.ctypes.data]                 # the rows as they lie: no copy
    first = FIRST_OUT[call]
    if call == "banded":
        assert behind[0].dtype == np.int32 and np.array_equal(behind[0], table)   # int64 in, int32 out, directly behind max_move
        assert args[10] not in (args[11], args[12], args[13])                   # and alive: no output was allocated in its memory
    if call == "tracking":
        assert args[10:12] == [8, 1]                                         # period, end rule "best"
    (res,), n_out = results, len(OUT_DTYPES[call])
    assert len(res) == n_out
    assert [a.dtype for a in res] == [np.dtype(dt) for dt in OUT_DTYPES[call]] and all(a.shape == (T,) for a in res)
    assert [args[first + k] for k in range(n_out)] == [[a.ctypes.data] for a in res]   # (tracking: the table last of the four)
    assert first + n_out + 4 == N_ARGS[call]


@pytest.mark.parametrize("call", ["banded", "tracking"])
def test_outputs_of_the_caller_are_sent(rec, lattice, call):
    lp, labels, table = lattice
    outs = [[np.empty(T, dt)] for dt in OUT_DTYPES[call]]
    (res,), status, total = send(call, lp, labels, table, outputs=outs, return_status=True)
    (name, args, _), = rec.calls
    assert [args[FIRST_OUT[call] + k] for k in range(len(outs))] == [[o[0].ctypes.data] for o in outs]
    assert all(r is o[0] for r, o in zip(res, outs)) and status == [0] and total.dtype == np.float32 and total.shape == (1,)


@pytest.mark.parametrize("call", ["banded", "tracking"])
def test_bad_outputs_are_refused(rec, lattice, call):
    lp, labels, table = lattice
    good = lambda: [[np.empty(T, dt)] for dt in OUT_DTYPES[call]]
    wrong_dtype, wrong_length, strided, short_list, one_missing = good(), good(), good(), good(), good()
    wrong_dtype[2] = [np.empty(T, np.float64)]
    wrong_length[0] = [np.empty(T + 1, np.int32)]
    strided[1] = [np.empty(2 * T, np.int32)[::2]]
    short_list[0] = []
    for outs in (wrong_dtype, wrong_length, strided, short_list, one_missing[:-1]):
        with pytest.raises(ValueError):
            send(call, lp, labels, table, outputs=outs)
    assert rec.calls == []


def test_lists_of_unequal_length_are_refused(rec, lattice):
    lp, labels, table = lattice
    with pytest.raises(ValueError):
        ka.ctc_best_path_batch([lp, lp], [labels], BEAM, MM)
    with pytest.raises(ValueError):
        ka.ctc_best_path_banded_batch([lp, lp], [labels], [table, table], BEAM, MM)
    with pytest.raises(ValueError):
        ka.ctc_best_path_banded_batch([lp], [labels], [table, table], BEAM, MM)
    with pytest.raises(ValueError):
        ka.ctc_best_path_banded_batch([], [], [table], BEAM, MM)
    with pytest.raises(ValueError):
        ka.ctc_best_path_tracking_batch([lp], [labels, labels], BEAM, MM, 8)
    assert rec.calls == []


BANDED = dict(best_path=lambda lp, labels, table: ka.ctc_best_path_banded_batch([lp], [labels], [table], BEAM, MM),
              label_posteriors=lambda lp, labels, table: ka.ctc_label_posteriors_batch([lp], [labels], [L - 1], BEAM, MM, band_lo=[table]),
              mea_path=lambda lp, labels, table: ka.ctc_mea_path_batch([lp], [labels], [L - 1], BEAM, MM, band_lo=[table]))


@pytest.mark.parametrize("call", BANDED)
def test_a_table_that_does_not_fit_is_refused(rec, lattice, call):
    lp, labels, table = lattice
    BANDED[call](lp, labels, table)
    (name, args, behind), = rec.calls
    assert name == f"ka_ctc_{call}_banded_batch_f32" and np.array_equal(behind[0], table)
    assert args[5] == [LD] and args[2] == [lp.ctypes.data]
    for bad in (table[:-1], np.concatenate([table, table[-1:]]), table + 2 ** 32, table - 2 ** 32, np.where(np.arange(T) == 5, 2 ** 31, table)):
        with pytest.raises(ValueError):
            BANDED[call](lp, labels, bad)
    assert len(rec.calls) == 1
    BANDED[call](lp, labels, table.reshape(T, 1).astype(np.int32))           # flattened; int32 goes in as it is
    assert np.array_equal(rec.calls[1][2][0], table)


@pytest.mark.parametrize("call", CALLS)
def test_an_empty_batch_is_answered_without_a_call(rec, call):
    empty = dict(plain=lambda **kw: ka.ctc_best_path_batch([], [], BEAM, MM, **kw),
                 banded=lambda **kw: ka.ctc_best_path_banded_batch([], [], [], BEAM, MM, **kw),
                 tracking=lambda **kw: ka.ctc_best_path_tracking_batch([], [], BEAM, MM, 8, **kw))[call]
    assert empty() == [] and empty(return_status=True) == ([], [], [])
    assert rec.calls == []


@pytest.mark.parametrize("call", CALLS)
def test_no_frames_is_an_index_error(rec, lattice, call):
    lp, labels, table = lattice
    with pytest.raises(IndexError, match="list index out of range"):
        send(call, lp[:0], labels, table[:0])
    assert rec.calls == []


def test_other_layouts_are_copied_to_contiguous_float32(rec, lattice):
    lp, labels, table = lattice
    for other in (lp.astype(np.float64), np.asfortranarray(lp), lp[:, ::-1]):
        rec.calls.clear()
        ka.ctc_best_path_batch([other], [labels.astype(np.int64)], BEAM, MM)
        (_, args, _), = rec.calls
        assert args[5] == [V] and args[2] != [other.ctypes.data]


def test_the_private_names_stay_importable():
    import importlib
    from kokoro_align_amd import _lattices, posteriors
    align = importlib.import_module("kokoro_align_amd.align")        # (the package's ``align`` is the function)
    for name in ("_i64_array", "_ptr_array", "_stream_ptr", "_is_tensor", "_current_device"):
        assert getattr(align, name) is getattr(_lattices, name)
    assert callable(align._host_log_softmax) and posteriors._host_lattices is _lattices._host_lattices
    assert not hasattr(align, "_check_band") and not hasattr(align, "_banded_call") and not hasattr(align, "_tracking_call")
