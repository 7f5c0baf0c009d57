"""The determined prefix without a GPU: tests/determined_cases.py's families do what their names say
under tests/determined_ref.py alone, every planted fault of the reference changes ``determined`` on some case (so the GPU test,
which runs the same cases, would catch it), and the new symbols are in the header and the binding table.
"""
import os
import re

import numpy as np
import pytest

import determined_cases as K
import determined_ref as DR
import resume_ref as RR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("ka_ctc_best_path_determined_f32", "ka_ctc_best_path_determined_batch_f32", "ka_ctc_best_path_tracking_determined_f32",
           "ka_ctc_best_path_tracking_determined_batch_f32", "ka_determined_workspace_bytes")


def frames(name):
    return K.case(name)["lp"].shape[0]


def test_every_value_class_occurs():
    got = {name: K.want(name)[0] for name in K.NAMES}
    assert any(d == -1 for d in got.values()) and any(d == 0 for d in got.values())
    assert any(0 < d < frames(n) for n, d in got.items()) and any(d == frames(n) for n, d in got.items())
    for name, d in got.items():
        assert -1 <= d <= frames(name), name


def test_short_lattices_cover_the_code_groups():
    assert K.SHORT_T == (1, 2, 5, 17, 33, 66)
    for T in K.SHORT_T:
        for name in (f"T{T}", f"track_T{T}"):
            assert frames(name) == T and K.want(name)[0] >= 0, name


def test_one_live_cell_is_determined_to_the_end():
    for name in ("S0", "one_cell", "mm1"):
        d, stats = K.want(name)
        assert d == frames(name) and stats["frames"] == 0, name


def test_flat_wide_band_null_start_is_0_and_free_start_is_minus_1():
    c = K.case("flat_wide_null")
    assert c["lp"].shape == (120, 8) and len(c["lab"]) == 12 and c["beam"] == 1000 and not np.any(c["lp"])
    assert K.want("flat_wide_null")[0] == 0 and K.want("flat_wide_null")[1]["frames"] == 120
    assert K.want("flat_wide_free")[0] == -1 and K.want("flat_wide_free")[1]["frames"] == 120
    assert K.want("track_free")[0] == -1


def test_merges_strictly_inside():
    lags = {}
    for name in K.INSIDE:
        d, stats = K.want(name)
        T = frames(name)
        assert 0 < d < T and stats["frames"] == T - d, name
        lags[name] = T - d
    assert lags["flat_small"] == 23 and lags["flat_big"] == 94   # (all ties: the band's drift alone merges the lines)
    assert min(lags.values()) <= 13 and max(lags.values()) > 160, lags


def test_boundary_crossings_and_the_ring_wrap_are_reached():
    d, stats = K.want("ring_wrap")
    c = K.case("ring_wrap")
    assert c["table"][-1] < 1024 <= c["table"][-1] + c["beam"] and stats["wrap"] and 0 <= d < frames("ring_wrap")
    assert K.RING_CUT in K.find_ring_cut()
    for name in ("hash_small", "hash_big", "wide1009", "wide1010", "track_generic", "mm5"):
        stats = K.want(name)[1]
        assert stats["cross1"] and stats["cross2"] and stats["cross3"], name
    # per max_move, the largest move crosses a block boundary somewhere
    assert K.want("mm2")[1]["cross1"] and K.want("mm4")[1]["cross3"]


def test_forms():
    for name in K.NAMES:
        c = K.case(name)
        L = 2 * len(c["lab"]) + 1
        generic = min(c["beam"], L) > 1009 or c["lp"].shape[1] > 64 or c["mm"] > 4
        assert generic == (c["form"] == "generic"), name
    assert min(K.case("wide1009")["beam"], 1041) == 1009 and min(K.case("wide1010")["beam"], 1041) == 1010
    assert K.case("V65")["lp"].shape[1] == 65 and K.case("mm5")["mm"] == 5


def test_special_inputs_are_what_they_say():
    assert np.any(K.case("label0")["lab"] == 0)
    c = K.case("ninf_cells")
    assert np.any(np.isneginf(c["lp"]))
    c = K.case("ninf_frames")
    fw = DR.forward_trail(c["lp"], c["lab"], c["table"], None, c["beam"], c["mm"])
    assert fw[2].size > 1 and np.all(np.isneginf(fw[3])) and 0 < K.want("ninf_frames")[0] < frames("ninf_frames")
    c = K.case("ninf_row")
    assert np.any(np.isneginf(c["init"])) and K.reference(c, fault="ninf_as_dead") != K.want("ninf_row")[0]
    c = K.case("empties")
    assert DR.live_cells(c["lp"], c["lab"], c["table"], None, c["beam"], c["mm"]).size == 0 and K.want("empties")[0] == -1


def test_a_dead_end_keeps_determined():
    c = K.case("dead_end")
    with pytest.raises(RR.EmptyBeam):
        RR.best_path_resume(c["lp"], c["lab"], c["table"], None, c["end"], c["beam"], c["mm"])
    assert K.want("dead_end")[0] == K.want("hash_small")[0] == K.want("live_end")[0] > 0
    live = K.case("live_end")
    RR.best_path_resume(live["lp"], live["lab"], live["table"], None, live["end"], live["beam"], live["mm"])


def test_failing_lattices_are_undetermined():
    for name in K.FAILING:
        assert K.want(name)[0] == -1, name


def test_tracking_chunks_are_cut_at_multiples_of_the_period():
    for kind in ("hash", "peaked"):
        for period in (4, 16):
            a, b = K.case(f"track_{kind}_p{period}_a"), K.case(f"track_{kind}_p{period}_b")
            assert a["lp"].shape[0] % period == 0 and a["period"] == b["period"] == period
            assert b["init"] is not None and np.sum(~np.isnan(b["init"])) > 1


def test_finality_under_the_reference():
    """frames [0, d) agree whichever live cell the path ends at, and frame d does not (d < T)"""
    for name in ("hash_small", "peaked_small", "T33", "ninf_cells"):
        c = K.case(name)
        d = K.want(name)[0]
        live = DR.live_cells(c["lp"], c["lab"], c["table"], c["init"], c["beam"], c["mm"])
        paths = np.array([RR.best_path_resume(c["lp"], c["lab"], c["table"], c["init"], int(q), c["beam"], c["mm"])[0] for q in live])
        assert len(live) > 1 and np.all(paths[:, :d] == paths[0, :d]) and np.unique(paths[:, d]).size > 1, name


@pytest.mark.parametrize("fault", DR.FAULTS)
def test_every_planted_fault_changes_determined_on_some_case(fault):
    caught = [name for name in K.NAMES if K.reference(K.case(name), fault=fault) != K.want(name)[0]]
    assert caught, fault


def test_symbols_in_header_and_binding_table():
    with open(os.path.join(ROOT, "include", "kokoro_align_amd.h")) as f:
        header = f.read()
    with open(os.path.join(ROOT, "kokoro-align_amd", "_lib.py")) as f:
        binding = f.read()
    exports = re.search(r"EXPORTS = \[(.*?)\]", binding, re.S).group(1)
    for sym in SYMBOLS:
        assert re.search(r"\b%s\(" % sym, header), sym
        assert f'"{sym}"' in exports, sym
    assert "int32_t *determined" in header and "section 4.36" in header
