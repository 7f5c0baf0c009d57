"""What the band best-path family refuses before it launches anything, through the raw C ABI: the return code, the text of
ka_last_error() and, where two refusals apply, which one wins.  The six batch entry points (banded, tracking, resume, tracking
resume, determined, tracking determined) and the banded single-lattice call share one driver; its checks run in this order:

    period / end_rule (tracking calls; before the engine is looked at), engine NULL, batch pending, NULL array argument, mem,
    determined NULL, [n == 0: done], unsupported shape, every lattice's end, every lattice's first_lo, then per lattice ld < V
    and NULL buffers

No refusal reaches a launch, so two tiny lattices on host buffers do; the outputs start as sentinels and must stay so."""
import numpy as np
import pytest

import fb_harness as H
from test_engine_state_gpu import RawBatch, _small

pytestmark = pytest.mark.gpu

T, S, V, BEAM, MM = 8, 3, 5, 4, 2
L = 2 * S + 1

NULL_ARRAY = "banded best path: NULL array argument"
BAD_MEM = "mem must be KA_MEM_HOST or KA_MEM_DEVICE"
BAD_SHAPE = "banded best path: unsupported T/S/V/beam_size/max_move"
BAD_END = "lattice %d: end must be -1 (highest live), -2 (best live) or a position in [0, 2S+1)"
BAD_FIRST_LO = "lattice %d: first_lo must be a position in [0, 2S+1)"
BAD_LD = "lattice %d: ld < V"
NULL_BUFFER = "lattice %d: NULL buffer"
NO_DETERMINED = "determined best path: determined is NULL"
BAD_PERIOD = "tracking best path: period must be a multiple of 4 in [4, 65536]"
BAD_END_RULE = "tracking best path: end_rule must be 0 (highest live) or 1 (best live)"
PENDING = "a batch is already enqueued: call ka_batch_finish first"
NO_ENGINE = "engine is NULL"

HEAD = ("n", "log_probs", "T", "V", "ld", "labels", "S", "beam_size", "max_move")
OUT = ("best_path", "best_labels", "best_scores")
TAIL = ("total_score", "status", "mem", "stream")
RESUME = ("band_lo", "init_scores", "end") + OUT + ("final_scores", "entry")
TRACK_RESUME = ("period", "first_lo", "init_scores", "end") + OUT + ("band_lo", "final_scores", "entry", "next_lo")
ARGS = {   # the arguments behind the engine, in the order of include/kokoro_align_amd.h (band_lo: the table read, or the table written)
    "banded": HEAD + ("band_lo",) + OUT + TAIL,
    "tracking": HEAD + ("period", "end_rule") + OUT + ("band_lo",) + TAIL,
    "resume": HEAD + RESUME + TAIL,
    "tracking_resume": HEAD + TRACK_RESUME + TAIL,
    "determined": HEAD + RESUME + ("determined",) + TAIL,
    "tracking_determined": HEAD + TRACK_RESUME + ("determined",) + TAIL,
}
KINDS = tuple(ARGS)
RESUMED = KINDS[2:]
TRACKING = tuple(k for k in KINDS if "tracking" in k)
POINTER_TABLES = ("log_probs", "labels", "band_lo", "init_scores", "final_scores") + OUT     # [n] pointers to per-lattice buffers
INT64_TABLES = ("T", "ld", "S")
INT32_TABLES = ("end", "first_lo", "entry", "next_lo", "determined", "status")


@pytest.fixture(scope="module")
def env():
    _, _lib, eng = H.engine()
    return _lib, eng


class Call:
    """The arguments of one call over n valid lattices; what a test changes makes it refusable."""

    def __init__(self, n=2):
        rng = np.random.default_rng(5)
        self.n = n
        self.a = dict(
            n=n, V=V, beam_size=BEAM, max_move=MM, period=4, end_rule=0, mem=0, stream=None,
            log_probs=[np.log(rng.dirichlet(np.ones(V), T)).astype(np.float32) for _ in range(n)],
            labels=[rng.integers(1, V, S).astype(np.int32) for _ in range(n)],
            band_lo=[np.minimum(np.arange(T, dtype=np.int32), L - 1) for _ in range(n)],
            init_scores=[np.zeros(L, np.float32) for _ in range(n)],
            final_scores=[np.full(L, H.SENTINEL, np.float32) for _ in range(n)],
            best_path=[np.full(T, -9, np.int32) for _ in range(n)],
            best_labels=[np.full(T, -9, np.int32) for _ in range(n)],
            best_scores=[np.full(T, H.SENTINEL, np.float32) for _ in range(n)],
            T=[T] * n, ld=[V] * n, S=[S] * n, end=[-1] * n, first_lo=[0] * n,
            entry=[-9] * n, next_lo=[-9] * n, determined=[-9] * n, status=[99] * n,
            total_score=np.full(n, H.SENTINEL, np.float32))

    def but(self, **changes):
        """A changed argument: a new value; for a table, None (the NULL array) or {lattice: value} (None: a NULL buffer)."""
        for name, v in changes.items():
            if isinstance(v, dict):
                self.a[name] = list(self.a[name])
                for i, x in v.items():
                    self.a[name][i] = x
            else:
                self.a[name] = v
        return self

    def _c(self, name):
        v = self.a[name]
        if v is None:
            return None
        if name in POINTER_TABLES:
            return H._addresses([None if x is None else x.ctypes.data for x in v])
        if name in INT64_TABLES:
            return H.I(v)
        if name in INT32_TABLES:
            self.a[name] = v = np.asarray(v, np.int32)
        return v.ctypes.data if isinstance(v, np.ndarray) else v

    def run(self, eng, kind, handle=True):
        fn = getattr(eng.lib, f"ka_ctc_best_path_{kind}_batch_f32")
        return fn(eng.handle if handle else None, *[self._c(name) for name in ARGS[kind]])

    def run_single(self, eng, handle=True):
        """ka_ctc_best_path_banded_f32 on lattice 0."""
        a = self.a
        ptr = lambda name: None if a[name][0] is None else a[name][0].ctypes.data
        return eng.lib.ka_ctc_best_path_banded_f32(eng.handle if handle else None, ptr("log_probs"), a["T"][0], a["V"], a["ld"][0], ptr("labels"),
                                                   a["S"][0], a["beam_size"], a["max_move"], ptr("band_lo"), ptr("best_path"), ptr("best_labels"),
                                                   ptr("best_scores"), a["total_score"].ctypes.data, a["mem"], None)

    def untouched(self):
        a = self.a
        for name in OUT + ("final_scores",):
            assert all((x == (-9 if x.dtype == np.int32 else H.SENTINEL)).all() for x in (a[name] or []) if x is not None), name
        for name in ("entry", "next_lo", "determined"):
            assert a[name] is None or (np.asarray(a[name]) == -9).all(), name
        assert (np.asarray(a["status"]) == 99).all() and (a["total_score"] == H.SENTINEL).all()


def refused(env, kind, call, text, **kw):
    _lib, eng = env
    rc = call.run_single(eng, **kw) if kind == "single" else call.run(eng, kind, **kw)
    assert (rc, _lib.last_error()) == (_lib.KA_ERR_BAD_ARGS, text), (kind, rc, _lib.last_error())
    call.untouched()


def test_valid_arguments_are_accepted(env):
    """The arguments every case below starts from run: each refusal comes from the one thing its case changes."""
    _lib, eng = env
    for kind in KINDS:
        assert Call().run(eng, kind) == _lib.KA_OK, (kind, _lib.last_error())
    assert Call().run_single(eng) == _lib.KA_OK, _lib.last_error()


@pytest.mark.parametrize("kind", KINDS)
def test_refusals_every_call_shares(env, kind):
    refused(env, kind, Call(), NO_ENGINE, handle=False)
    for name in ("log_probs", "T", "ld", "labels", "S", "band_lo") + OUT:
        refused(env, kind, Call().but(**{name: None}), NULL_ARRAY)
    refused(env, kind, Call().but(n=-1), NULL_ARRAY)
    refused(env, kind, Call().but(mem=7), BAD_MEM)
    refused(env, kind, Call().but(max_move=300), BAD_SHAPE)
    refused(env, kind, Call().but(T={1: 0}), BAD_SHAPE)
    refused(env, kind, Call().but(ld={1: V - 1}), BAD_LD % 1)
    for name in ("log_probs", "labels", "band_lo") + OUT:
        refused(env, kind, Call().but(**{name: {1: None}}), NULL_BUFFER % 1)
    # which refusal wins: a NULL array before mem, mem before the shape, the shape before a lattice's buffers, and of two
    # lattices the first
    refused(env, kind, Call().but(S=None, mem=7), NULL_ARRAY)
    refused(env, kind, Call().but(mem=7, max_move=300), BAD_MEM)
    refused(env, kind, Call().but(max_move=300, log_probs={0: None}), BAD_SHAPE)
    refused(env, kind, Call().but(max_move=300, ld={0: V - 1}), BAD_SHAPE)
    refused(env, kind, Call().but(ld={1: V - 1}, best_path={0: None}), NULL_BUFFER % 0)
    refused(env, kind, Call().but(ld={0: V - 1}, log_probs={0: None}), BAD_LD % 0)


def test_refusals_of_the_single_lattice_call(env):
    refused(env, "single", Call(1), NO_ENGINE, handle=False)
    refused(env, "single", Call(1).but(mem=7), BAD_MEM)
    refused(env, "single", Call(1).but(max_move=300), BAD_SHAPE)
    refused(env, "single", Call(1).but(ld=[V - 1]), BAD_LD % 0)
    for name in ("log_probs", "labels", "band_lo") + OUT:
        refused(env, "single", Call(1).but(**{name: {0: None}}), NULL_BUFFER % 0)
    refused(env, "single", Call(1).but(max_move=300, log_probs={0: None}), BAD_SHAPE)


@pytest.mark.parametrize("kind", RESUMED)
def test_refusals_of_the_resumed_calls(env, kind):
    for end in (-3, L):
        refused(env, kind, Call().but(end={1: end}), BAD_END % 1)
    # every lattice's end is looked at before any lattice's ld or buffers, and the shape before any end
    refused(env, kind, Call().but(end={0: -3}, ld={1: V - 1}), BAD_END % 0)
    refused(env, kind, Call().but(end={1: L}, ld={0: V - 1}), BAD_END % 1)
    refused(env, kind, Call().but(end={1: L}, log_probs={0: None}), BAD_END % 1)
    refused(env, kind, Call().but(end={0: -3}, max_move=300), BAD_SHAPE)
    # what may be NULL is: the rows, end, entry
    _lib, eng = env
    assert Call().but(init_scores=None, end=None, final_scores=None, entry=None).run(eng, kind) == _lib.KA_OK, _lib.last_error()
    if "tracking" in kind:
        for lo in (-1, L):
            refused(env, kind, Call().but(first_lo={1: lo}), BAD_FIRST_LO % 1)
        refused(env, kind, Call().but(first_lo={0: -1}, end={1: -3}), BAD_END % 1)
        refused(env, kind, Call().but(first_lo={1: L}, ld={0: V - 1}), BAD_FIRST_LO % 1)
        refused(env, kind, Call().but(first_lo={0: -1}, max_move=300), BAD_SHAPE)
        assert Call().but(first_lo=None, next_lo=None).run(eng, kind) == _lib.KA_OK, _lib.last_error()
    if "determined" in kind:
        refused(env, kind, Call().but(determined=None), NO_DETERMINED)
        refused(env, kind, Call().but(determined=None, n=0), NO_DETERMINED)
        refused(env, kind, Call().but(determined=None, max_move=300), NO_DETERMINED)
        refused(env, kind, Call().but(determined=None, mem=7), BAD_MEM)


@pytest.mark.parametrize("kind", TRACKING)
def test_refusals_of_the_tracking_calls(env, kind):
    for period in (0, 2, 6, 65540, -4):
        refused(env, kind, Call().but(period=period), BAD_PERIOD)
    # ... before anything else, the engine included
    refused(env, kind, Call().but(period=6), BAD_PERIOD, handle=False)
    refused(env, kind, Call().but(period=6, log_probs=None, mem=7), BAD_PERIOD)
    if kind == "tracking":
        for rule in (-1, 2):
            refused(env, kind, Call().but(end_rule=rule), BAD_END_RULE)
        refused(env, kind, Call().but(end_rule=2), BAD_END_RULE, handle=False)
        refused(env, kind, Call().but(end_rule=2, period=6), BAD_PERIOD)


def test_a_pending_batch_refuses_every_call(env):
    _lib, eng = env
    lat, want = _small()
    b = RawBatch([lat], 1000)
    assert b.enqueue(eng) == _lib.KA_OK
    try:
        for kind in KINDS:
            refused(env, kind, Call(), PENDING)
            refused(env, kind, Call().but(log_probs=None, mem=7), PENDING)      # (before the arguments are looked at)
        refused(env, "single", Call(1), PENDING)
        refused(env, "tracking", Call().but(period=6), BAD_PERIOD)
    finally:
        rc = b.finish(eng)
    assert rc == _lib.KA_OK
    b.check(0, want, "after the refused calls")
