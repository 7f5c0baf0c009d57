"""The state visit callers of tests/test_state_visits_gpu.py: duration_harness.py's one caller on the visit symbols."""
from duration_harness import GUARD, SENTINEL, pair_call, pair_call_one  # noqa: F401


def visit_call(eng, _lib, lps, labs, terms, beam, mm, exit_time=True, device=False):
    return pair_call("state_visits", eng, _lib, lps, labs, terms, beam, mm, exit_time, device)


def visit_call_one(eng, _lib, lp, labels, terminal, beam, mm, exit_time=True, ld=None):
    return pair_call_one("state_visits", eng, _lib, lp, labels, terminal, beam, mm, exit_time, ld)
