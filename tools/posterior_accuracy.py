"""Reduces the JSON lines that the posterior GPU tests append under KA_ACCURACY_OUT=<file> (tests/fb_harness.record) to
profiles/posterior_accuracy.json: per call the worst ratio |kernel - float64| / E of every test, and m = twice the worst of
them, rounded up to two digits (tests/posterior_ref.py).

    KA_ACCURACY_OUT=ratios.jsonl python -m pytest tests -q -m gpu -k posterior
    python tools/posterior_accuracy.py ratios.jsonl profiles/posterior_accuracy.json

The state duration call (tests/test_durations_gpu.py, tests/duration_ref.py) records four figures of
its own under the multiplier of the state call.  With call names after the two files only those are reduced and every other
key of the existing file stays as it is:

    KA_ACCURACY_OUT=ratios.jsonl python -m pytest tests/test_durations_gpu.py -q -m gpu
    python tools/posterior_accuracy.py ratios.jsonl profiles/posterior_accuracy.json duration time_sum duration_sum time_sum_sum

The maximum-expected-accuracy call (tests/test_mea_path_gpu.py, tests/mea_ref.py) records three
figures, held against a multiplier that is derived, not measured (each of the two values a choice compares is off by at
most E), and taken here from the records the tests wrote:

    KA_ACCURACY_OUT=ratios.jsonl python -m pytest tests/test_mea_path_gpu.py -q -m gpu
    python tools/posterior_accuracy.py ratios.jsonl profiles/posterior_accuracy.json mea mea_total mea_value

The state visit call (tests/test_state_visits_gpu.py, tests/visit_ref.py) records visit and exit_time
against a model and a multiplier of their own, set by the rule above, and z, whose records join those the file holds (a test's
earlier record is replaced, every other one stays):

    KA_ACCURACY_OUT=ratios.jsonl python -m pytest tests/test_state_visits_gpu.py -q -m gpu
    python tools/posterior_accuracy.py ratios.jsonl profiles/posterior_accuracy.json visit exit_time z

The boundary-quantile call (tests/test_boundary_quantiles_gpu.py, tests/quantile_ref.py) is an integer
result: its keys are shares of a case's (cut, level) pairs - those left out of the comparison with the float64 frames because F
comes within twice its margin of the level (held against the cap of 0.02), and those of the others that differ (held against 0) -
and z, which joins the file's records:

    KA_ACCURACY_OUT=ratios.jsonl python -m pytest tests/test_boundary_quantiles_gpu.py -q -m gpu
    python tools/posterior_accuracy.py ratios.jsonl profiles/posterior_accuracy.json quantile_left_out quantile_mismatch z

The deep inputs (tests/test_posterior_deep_gpu.py, DESIGN.md section 4.21, "magnitude") record each call against its deep model
under keys of their own, deep_*, whose multipliers follow the rule above (the two duration figures are held to deep_state's);
the file's masked-cell tests record state, label, path and z, which join the file's records:

    KA_ACCURACY_OUT=ratios.jsonl python -m pytest tests/test_posterior_deep_gpu.py -q -m gpu
    python tools/posterior_accuracy.py ratios.jsonl profiles/posterior_accuracy.json deep_state deep_label deep_path deep_z \
        deep_duration deep_time_sum deep_visit deep_exit_time deep_alpha_out deep_beta_out state label path z
"""
import json
import math
import sys

CALLS = ("state", "label", "path", "z")
DURATION_CALLS = ("duration", "time_sum", "duration_sum", "time_sum_sum")
MEA_CALLS = ("mea", "mea_total", "mea_value")
VISIT_CALLS = ("visit", "exit_time")
QUANTILE_CALLS = ("quantile_left_out", "quantile_mismatch")
DEEP_CALLS = ("deep_state", "deep_label", "deep_path", "deep_z", "deep_duration", "deep_time_sum", "deep_visit", "deep_exit_time",
              "deep_alpha_out", "deep_beta_out")


def round_up(x):
    """x rounded up to two significant digits."""
    if x <= 0:
        return 0.0
    e = math.floor(math.log10(x)) - 1
    return round(math.ceil(x / 10 ** e - 1e-9) * 10 ** e, 10)


def main(src, dst, only=()):
    calls = tuple(only) or CALLS
    assert all(c in CALLS + DURATION_CALLS + MEA_CALLS + VISIT_CALLS + QUANTILE_CALLS + DEEP_CALLS for c in calls), calls
    worst = {c: {} for c in calls}
    held = {}                                    # the multiplier the tests held a call against (every record carries it)
    with open(src) as f:
        for line in f:
            rec = json.loads(line)
            if rec.get("call") in worst:
                per = worst[rec["call"]]
                r = rec["ratio"] if rec["ratio"] == rec["ratio"] else math.inf       # a NaN ratio is a failure, not a figure
                per[rec["test"]] = max(per.get(rec["test"], 0.0), r)
                assert held.setdefault(rec["call"], rec["m"]) == rec["m"], rec
    out = {"device": "MI355X (gfx950)",
           "unit": "max over the cells of a test of |kernel - float64| / E; E = posterior_ref.*_error_model of the float64 reference",
           "rule": "m = twice the worst measured ratio of its call, rounded up to two digits (tests/posterior_ref.py)",
           "calls": {}}
    if only:                                     # the file as it is, with the named calls replaced
        with open(dst) as f:
            out = json.load(f)
    for c in calls:
        if only and c in CALLS and c in out["calls"]:        # one more file's records of a call the file already holds
            worst[c] = {**{r["test"]: r["ratio"] for r in out["calls"][c]["records"]}, **worst[c]}
        top = max(worst[c].values(), default=0.0)
        # (the duration figures are held against the state call's multiplier: their model is a sum of its per-cell model)
        m = out["calls"]["state"]["m"] if c in DURATION_CALLS and "state" in out["calls"] else held[c] if c in MEA_CALLS + QUANTILE_CALLS else round_up(2 * top)
        if c in ("deep_duration", "deep_time_sum") and "deep_state" in out["calls"]:
            m = out["calls"]["deep_state"]["m"]
        out["calls"][c] = {"m": m, "worst_ratio": top, "tests": len(worst[c]),
                           "records": [{"test": t, "ratio": r} for t, r in sorted(worst[c].items())]}
    with open(dst, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    for c in calls:
        print(c, out["calls"][c]["tests"], "tests, worst", out["calls"][c]["worst_ratio"], "m", out["calls"][c]["m"])


if __name__ == "__main__":
    main(sys.argv[1], sys.argv[2], sys.argv[3:])
