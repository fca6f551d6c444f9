"""`odeint`'s adaptive trial step launches, call for call and argument for argument, what it launched when
golden/odeint_launch_log.json was recorded (golden/make_odeint_launch_log.py: before the eager step and the captured step
became one loop over a launch plan each) — and computes the same bits, evaluations and accept / reject decisions."""
import importlib.util
import json
import os

import pytest

from torchdiffeq_amd import tableaus as tb

_GOLDEN = os.path.join(os.path.dirname(__file__), "golden")
_spec = importlib.util.spec_from_file_location("make_odeint_launch_log", os.path.join(_GOLDEN, "make_odeint_launch_log.py"))
rec = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(rec)


@pytest.fixture(scope="module")
def recorded():
    return rec.load()


def _first_difference(got, want):
    for i, (g, w) in enumerate(zip(got, want)):
        if g != w:
            return "call {}: launched {} where the fixture has {}".format(i, g, w)
    return "{} calls logged where the fixture has {}".format(len(got), len(want))


@pytest.mark.parametrize("regime", list(rec.REGIMES))
def test_solve_launches_what_it_launched(recorded, regime):
    want = recorded["solves"][regime]
    got = json.loads(json.dumps(rec.run_regime(regime)))
    assert got["head"] == want["head"], _first_difference(got["head"], want["head"])
    for field in ("calls", "trial_steps", "sha256", "solution", "nfe", "steps", "failed"):
        assert got[field] == want[field], (regime, field)


def test_every_regime_is_recorded(recorded):
    assert sorted(recorded["solves"]) == sorted(rec.REGIMES)
    assert sorted(recorded["graph_body"]) == sorted(rec.body_cases())
    # the regimes differ where they should: the carry plan changes the launches of the tableaus that have one, and only there
    for m in rec.METHODS:
        a, b = (recorded["solves"]["{}/f64/no_grad/carry{}".format(m, c)] for c in "01")
        assert (a["sha256"] != b["sha256"]) == (tb.carry_plan(m) is not None) and a["solution"] == b["solution"]
        # func closing over a Parameter: whole rows + error_norm under either setting
        a, b = (recorded["solves"]["{}/f64/parameter/carry{}".format(m, c)] for c in "01")
        assert a["sha256"] == b["sha256"]
        assert {c.split("(")[0] for c in a["head"]} & {"stage_combine_err", "stage_combine_multi", "error_norm_partial"} == set()
    assert any(isinstance(r["steps"], dict) and r["steps"]["n_rejected"] for n, r in recorded["solves"].items()
               if n.startswith("dopri5/"))


@pytest.mark.parametrize("case", rec.body_cases())
def test_graph_step_body_launches_what_it_launched(recorded, case):
    want = recorded["graph_body"][case]
    got = rec.run_body_case(case)
    assert got["log"] == want["log"], _first_difference(got["log"], want["log"])
    assert got["sha256"] == want["sha256"]


def _old_form(op, i, R, row):
    """The launch form as the three interpreters derived it from an op's shape before `CarryOp.form` existed."""
    if len(op.targets) == 1 and not op.continues:
        return "whole"
    if op.targets == (i, R) and i == R - 1 and not op.continues and op.idx == row.idx:
        return "pair"
    return "multi"


@pytest.mark.parametrize("name", ["dopri5", "bosh3", "tsit5", "fehlberg2", "adaptive_heun", "dopri8"])
def test_launch_form_is_the_old_rule(name):
    tab = tb.ADAPTIVE_TABLEAUS[name]
    rows = tab.beta_rows() + ([] if tab.fsal_solution else [tb.SparseRow.from_dense(tab.c_sol)])
    plans = [tb.tableau_row_plan(name, tb.FUSE_ROWWISE), tb.tableau_row_plan(name, tb.FUSE_ODEINT),
             tb.row_by_row_plan(rows, tb.SparseRow.from_dense(tab.c_error), 0)]
    if tb.carry_plan(name) is not None:
        plans.append(tb.carry_plan(name))
    seen = set()
    for plan in plans:
        R = len(plan.ops)
        assert R == len(rows) and plan.ops[0] is None
        for i in range(1, R):
            op = plan.ops[i]
            if op is not None:
                assert op.form == _old_form(op, i, R, rows[i]), (name, i)
                seen.add(op.form)
    assert "whole" in seen and ("pair" in seen) == (name != "fehlberg2")
    assert plans[2].err_idx == tb.SparseRow.from_dense(tab.c_error).idx and \
        all(op.form == "whole" for op in plans[2].ops[1:])
