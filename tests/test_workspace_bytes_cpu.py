"""Every ka_*_workspace_bytes export answers what tests/golden/workspace_bytes.json recorded (tools/workspace_bytes.py
--golden): the byte counts are host arithmetic over the workspace layouts of ka_plan.hpp, so a planner that moves a region,
changes an alignment or refuses another shape shows here, without a GPU.  The grid covers both memory modes, `tracking` where a
call takes it, T no multiple of 4, the three thresholds between the one-wavefront and the generic form (V 64, max_move 4, a
band of 1009) within one batch, the calls with K, M or n_samples, and the refusals (0 bytes)."""
import json
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import workspace_bytes as wb  # noqa: E402


@pytest.fixture(scope="module")
def golden():
    with open(wb.GOLDEN) as f:
        return json.load(f)


def test_golden_covers_the_grid(golden):
    assert [(g["fn"], g["args"]) for g in golden] == wb.grid()
    assert {g["fn"] for g in golden} == set(wb.SIGNATURES)


def test_every_answer_is_reproduced(golden):
    from kokoro_align_amd import _lib
    lib = _lib.load_library()
    wrong = [(g["fn"], g["args"], g["bytes"], got) for g in golden if (got := wb.call(lib, g["fn"], g["args"])) != g["bytes"]]
    assert not wrong, f"{len(wrong)} of {len(golden)} byte counts differ; first (fn, args, recorded, now): {wrong[0]}"


def test_refusals_answer_zero(golden):
    kinds = {"max_move": lambda a: a.get("max_move") == 300, "mem": lambda a: a.get("mem") == 7,
             "n": lambda a: a["n"] == -1, "T": lambda a: a["T"] is None}
    for fn, sig in wb.SIGNATURES.items():
        for arg, is_refusal in kinds.items():
            hits = [g for g in golden if g["fn"] == fn and is_refusal(g["args"])]
            assert bool(hits) == (arg in sig), (fn, arg)
            assert all(g["bytes"] == 0 for g in hits), (fn, arg)
    # ... and a batch of supported shapes is not refused
    assert all(g["bytes"] > 0 for g in golden if g["args"]["n"] == 3 and g["args"].get("M", 3) in (1, 3))
