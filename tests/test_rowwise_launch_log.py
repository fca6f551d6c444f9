"""`odeint_rowwise`, `odeint_rowwise_event` and `odeint_rowwise_dense` launch, call for call and argument for argument,
what they launched when golden/rowwise_family_launch_log.json was recorded (golden/make_rowwise_launch_log.py: before the
three entry points shared one driver loop, one step hook and one bisection) — `func` and `event_fn` are called with the same
shapes and rows in the same places, and every returned tensor and every `stats` entry has the same bits."""
import importlib.util
import json
import os

import pytest

_GOLDEN = os.path.join(os.path.dirname(__file__), "golden")
_spec = importlib.util.spec_from_file_location("make_rowwise_launch_log", os.path.join(_GOLDEN, "make_rowwise_launch_log.py"))
rec = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(rec)

FIELDS = ("calls", "trial_steps", "sha256", "counts", "failed", "tensors", "stats")


@pytest.fixture(scope="module")
def recorded():
    return rec.load()


def _first_difference(got, want):
    for i, (g, w) in enumerate(zip(got, want)):
        if g != w:
            return "call {}: launched {} where the fixture has {}".format(i, g, w)
    return "{} calls logged where the fixture has {}".format(len(got), len(want))


@pytest.mark.parametrize("case", rec.CASES)
def test_solve_launches_what_it_launched(recorded, case):
    want = recorded[case]
    got = json.loads(json.dumps(rec.run_case(case)))
    assert got["head"] == want["head"], _first_difference(got["head"], want["head"])
    assert sorted(got) == sorted(FIELDS + ("head",))
    for field in FIELDS:
        assert got[field] == want[field], (case, field)


def test_every_regime_is_recorded(recorded):
    assert sorted(recorded) == sorted(rec.CASES)
    for name in rec.REGIMES:
        dev, host = recorded["dev/" + name], recorded["host/" + name]
        # the host backend launches nothing: its log is the calls of func and event_fn, and those are the device driver's
        assert set(host["counts"]) <= {"f", "e"}
        assert {k: v for k, v in dev["counts"].items() if k in ("f", "e")} == host["counts"]
        assert dev["trial_steps"] == host["trial_steps"] and dev["failed"] == host["failed"]
        if "/compact=None" in name:
            # compact= changes what is launched and never a bit of what comes back
            for c in ("0.5", "1.0"):
                other = recorded["dev/" + name.replace("compact=None", "compact=" + c)] \
                    if name.replace("compact=None", "compact=" + c) in rec.REGIMES else None
                if other is not None and dev["failed"] is None:
                    assert other["tensors"] == dev["tensors"]
                    assert all(other["stats"][k] == v for k, v in dev["stats"].items())
