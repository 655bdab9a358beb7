"""CPU: the planner's sole mode (hb_refgen.hpp refgen_plan<MAP, 1>, compiled for the host by tests/host_emu/soleemu.cpp in the one-thread form
the four lanes of an instance share) against its numpy twin (tests/_soletwin.py), on profile maps and on field maps.

Tolerances of the parity tests are those of tests/test_groundmap_host.py for the same quantities: grid and x_ref 1e-12, swing tables 1e-10
with an identical NaN pattern, IK knots 1e-8; the stance memory and the defect of the choice read-back are positions of the swing tables'
kind (1e-10); the shift and the level flag of the read-back are integers and must be equal.  The twin's own run is asserted valid first:
its decisions are at least DECISIVE = 1e-9 from a tie (ten times the position tolerance), so both sides take the same branch."""
import numpy as np
import pytest

import _groundemu as ge
import _groundfieldemu as gfe
import _groundfieldtwin as gft
import _groundtwin as gt
import _soleemu as se
import _soletwin as stw
from _cmp import maxdiff_nan
from hunter_bipedal_control_amd import abi
from oracle import refgen

NMAX = gt.N + 8
READBACK = ("shift", "defect", "level")


@pytest.fixture(scope="module")
def mdl(params):
    return abi.make_model(params)


def _emu_case(params, mdl, case, rec, fcfg, emu=None):
    """Both calls of a case through the emulated pass on the map rec -> list of output dicts.  emu: the emulator of another file (the
    per-point forms as they were compiled before this mode existed in the source that calls them)."""
    c = params["config"]
    rcfg = abi.make_refgen_config(params, joint_ik=case["joint_ik"])
    ls = np.array(refgen.foot_positions(params["model"], case["calls"][0][1]), dtype=np.float64).copy()
    outs = []
    for t0, x_now in case["calls"]:
        if emu is None:
            st, o = se.refgen(mdl, rcfg, rec, fcfg, case["sched"], t0, gt.N * c["dt"], np.array(x_now, dtype=float), case["cmd"], ls, NMAX)
        else:
            st, o = emu.refgen(mdl, rcfg, rec, case["sched"], t0, gt.N * c["dt"], np.array(x_now, dtype=float), case["cmd"], ls, NMAX)
        assert st == 0
        outs.append(o)
    return outs


def _same(a, b):
    """Every output two passes share, byte for byte (NaN == NaN); the choice read-back is the sole mode's own."""
    for k in a:
        if k in READBACK or k not in b:
            continue
        assert np.array_equal(np.asarray(a[k]), np.asarray(b[k]), equal_nan=np.asarray(a[k]).dtype.kind == "f"), k


def _level_maps():
    return [("zero profile", ge.record([1.0, 0.0], [[0.0, 0.0], [1.0, 0.0]]), ge),
            ("level 16 knots", ge.record([0.6, 0.8], [[0.1 * k - 0.4, 0.0] for k in range(16)]), ge),
            ("zero field", gfe.record_of(gft.zero_field_map()), gfe),
            ("level field", gfe.record_of(gft.level_field_map()), gfe)]


def _plane_maps(params, case):
    s_now = float(case["calls"][0][1][6])
    sp = np.array([0.11, 0.09])
    uu, ww = np.meshgrid(np.arange(32) * sp[0], np.arange(32) * sp[1], indexing="ij")
    x0 = case["calls"][0][1][6:8]
    a = np.array([0.8, 0.6])
    org = np.array([a @ x0, np.array([-0.6, 0.8]) @ x0]) - 15.5 * sp
    return [("ramp 0.2", ge.record([1.0, 0.0], [[s_now - 1.0, -0.2], [s_now + 4.0, 0.8]]), ge),
            ("tilted field", gfe.record(a * 2.5, org, sp, 0.12 * uu - 0.07 * ww), gfe)]


# ---- 1. anchors -------------------------------------------------------------------------------------------------------------------------------
def test_sole_mode_on_level_maps_is_the_per_point_mode(params, mdl):
    fcfg = se.foothold_config()
    saw_nan = False
    for case in gt.case_inputs(params):
        for name, rec, emu in _level_maps():
            base = _emu_case(params, mdl, case, rec, None)
            sole = _emu_case(params, mdl, case, rec, fcfg)
            for a, b in zip(base, sole):
                _same(a, b)
            for o in sole:     # every first foothold taken where it was, flat
                planned = o["shift"] != se.no_foothold()
                assert (o["shift"][planned] == 0).all() and (o["level"] == 0).all() and (o["defect"] == 0.0).all(), (name, o["shift"], o["defect"])
            saw_nan = saw_nan or any(np.isnan(o["swing"]).any() for o in base)
    assert saw_nan                                                      # the NaN window at gait start was part of the comparison


def test_sole_mode_on_single_planes_is_the_per_point_mode(params, mdl):
    fcfg = se.foothold_config()
    worst = 0.0
    for case in gt.case_inputs(params):
        for name, rec, emu in _plane_maps(params, case):
            base = _emu_case(params, mdl, case, rec, None)
            sole = _emu_case(params, mdl, case, rec, fcfg)
            for a, b in zip(base, sole):
                _same(a, b)
            for o in sole:
                planned = o["shift"] != se.no_foothold()
                assert (o["shift"][planned] == 0).all() and (o["level"] == 0).all(), (name, o["shift"])
                worst = max(worst, o["defect"].max())
    assert worst < 1e-15, worst                                         # a plane's defect is rounding, far below any tolerance in use


def test_mode_0_and_no_config_are_no_call_at_all(params, mdl):
    off = se.foothold_config(mode=0, n_shift=5, shift_step=0.03, flat_tol=0.001)
    _, maps, _ = stw.cases(params, "profile")
    _, fmaps, _ = stw.cases(params, "field")
    for i, case in enumerate(gt.case_inputs(params)):
        for rec, emu in ((ge.record(maps[i].dir_given, maps[i].knots), ge), (gfe.record_of(fmaps[i]), gfe)):
            never = _emu_case(params, mdl, case, rec, None, emu=emu)      # the emulator of the per-point forms: no such argument exists there
            for other in (_emu_case(params, mdl, case, rec, None), _emu_case(params, mdl, case, rec, off)):
                for a, b in zip(never, other):
                    _same(a, b)
                assert all((o["shift"] == -7).all() for o in other)       # the read-back is not touched


def test_form_rule(params):
    for profile in (0, 1):
        for field in (0, 1):
            have_map = bool(profile or field)
            assert se.sole_form(profile, field) == 0                    # the defaulted call: what every earlier site computes
            assert se.sole_form(profile, field, 0) == 0
            assert se.sole_form(profile, field, 1) == int(have_map)


# ---- 2. parity with the twin, 3. structure, 4. mutants --------------------------------------------------------------------------------------
def _record(which, m):
    return ge.record(m.dir_given, m.knots) if which == "profile" else gfe.record_of(m)


def _parity(params, mdl, which, **mutant):
    """Largest differences emulated code - twin over the cases -> dict; raises AssertionError on a structural difference (grid, NaN
    pattern, a different candidate or level flag in the read-back)."""
    inputs, maps, runs = stw.cases(params, which)
    if mutant:
        runs = [stw.run_twin(params, case, type(m)(*_ctor(m)), NMAX, **mutant) for case, m in zip(inputs, maps)]
    worst = dict(t=0.0, x_ref=0.0, swing=0.0, ik=0.0, stance=0.0, defect=0.0)
    fcfg = se.foothold_config(**stw.CFG)
    for case, m, run in zip(inputs, maps, runs):
        outs = _emu_case(params, mdl, case, _record(which, m), fcfg)
        for got, ref, choice, stance in zip(outs, run["tabs"], run["choice"], run["stance"]):
            assert got["n_nodes"] == ref["n_nodes"] and np.array_equal(got["mode"], ref["mode"])
            assert np.array_equal(got["shift"], choice[0]) and np.array_equal(got["level"], choice[2]), (got["shift"], choice[0], got["level"], choice[2])
            worst["defect"] = max(worst["defect"], np.abs(got["defect"] - choice[1]).max())
            worst["stance"] = max(worst["stance"], np.abs(got["stance"] - stance).max())
            worst["t"] = max(worst["t"], np.abs(got["t"] - ref["t"]).max())
            worst["x_ref"] = max(worst["x_ref"], np.abs(got["x_ref"][:, :12] - ref["x_ref"][:, :12]).max())
            worst["ik"] = max(worst["ik"], np.abs(got["x_ref"][:, 12:] - ref["x_ref"][:, 12:]).max())
            worst["swing"] = max(worst["swing"], maxdiff_nan(got["swing"], ref["swing"]))
    return worst


def _ctor(m):
    return (m.dir_given, m.knots) if isinstance(m, gt.GroundMap) else (m.dir_given, m.origin, m.spacing, m.g)


def _within(w):
    return w["t"] < 1e-12 and w["x_ref"] < 1e-12 and w["swing"] < 1e-10 and w["ik"] < 1e-8 and w["stance"] < 1e-10 and w["defect"] < 1e-10


def test_cases_are_valid(params):
    """Asserted first, on the twin's own log: no evaluated point within MARGIN of a line where the facet changes, no decision within
    DECISIVE of a tie, and across the cases a foothold accepted off the nominal one, a foothold levelled and a stance memory levelled."""
    total = np.zeros(3, dtype=int)
    for which, margin in (("profile", gt.MARGIN), ("field", gft.MARGIN)):
        inputs, maps, runs = stw.cases(params, which)
        assert len(inputs) == gt.B
        assert min(m.margin for m in maps) > margin, (which, [m.margin for m in maps])
        assert min(stw.decisive(r) for r in runs) > stw.DECISIVE, (which, [stw.decisive(r) for r in runs])
        per = np.array([stw.counts(r) for r in runs])
        print(which, "accepted off nominal / levelled footholds / levelled stance memories per case:", per.tolist())
        total += per.sum(axis=0)
    assert (total >= 1).all(), total
    _, pmaps, _ = stw.cases(params, "profile")
    assert sorted({len(m.knots) for m in pmaps}) == [4, 8, 16] and any(abs(m.a[0]) != 1.0 for m in pmaps)


@pytest.mark.parametrize("which", ["profile", "field"])
def test_parity_with_the_twin(params, mdl, which):
    test_cases_are_valid(params)
    worst = _parity(params, mdl, which)
    print("sole mode,", which, "maps, emulated planner - twin:", worst)
    assert _within(worst), worst


@pytest.mark.parametrize("mutant", ["fallback_nominal", "minus_first", "level_chord", "stance_per_point"])
def test_mutants_break_the_parity(params, mdl, mutant):
    red = 0
    for which in ("profile", "field"):
        try:
            red += 0 if _within(_parity(params, mdl, which, **{mutant: True})) else 1
        except AssertionError:
            red += 1                                                    # (a different candidate, NaN pattern or grid: red as well)
    assert red >= 1, mutant


def test_structure_of_every_planned_swing(params, mdl):
    """The touch-downs are the emulated code's own phase records (every foothold the twin planned must be among them); the nominal
    footholds they are measured from, the sole's axis and the candidate are the TWIN's (the compiled code does not export them), so this
    complements the parity tests and does not replace them: the two points of a foot land the same vector off their nominal footholds
    (to the position tolerance), that vector is shift x shift_step along the sole's axis, a levelled pair has equal z and an accepted
    pair stands on the map under its own x, y."""
    fcfg = se.foothold_config(**stw.CFG)
    npz = params["config"]["swing"]["next_position_z"]
    seen = 0
    for which in ("profile", "field"):
        inputs, maps, runs = stw.cases(params, which)
        for case, m, run in zip(inputs, maps, runs):
            rec = _record(which, m)
            for got, log, (t0, _) in zip(_emu_case(params, mdl, case, rec, fcfg), run["log"], case["calls"]):
                sw = [e for e in log if e["kind"] == "swing"]
                ev = np.asarray(case["sched"].event_times)
                for leg in (0, 1):
                    toe = [e for e in sw if e["foot"] == leg]
                    heel = [e for e in sw if e["foot"] == leg + 2]
                    assert len(toe) == len(heel)
                    # the touch-down record of every swing phase that ends after t0 (the ones a pass plans a foothold for), one per phase
                    td = []
                    for f in (leg, leg + 2):
                        seen_tf, rows = set(), []
                        for r in got["phases"][f][:len(ev) + 1]:
                            if r[0] <= r[1] and r[1] > t0 and r[1] not in seen_tf:
                                seen_tf.add(r[1])
                                rows.append(r[5:8])
                        td.append(rows)
                    assert len(td[0]) == len(toe) and len(td[1]) == len(heel), (which, leg, len(td[0]), len(td[1]), len(toe))
                    for n, (et, eh) in enumerate(zip(toe, heel)):
                        pt, ph_ = td[0][n], td[1][n]
                        mt, mh = pt[:2] - et["nominal"][:2], ph_[:2] - eh["nominal"][:2]
                        assert np.abs(mt - mh).max() < 1e-10
                        assert np.abs(mt - et["k"] * stw.CFG["shift_step"] * np.array(et["e"])).max() < 1e-10
                        emu = ge if which == "profile" else gfe
                        if et["level"]:
                            assert pt[2] == ph_[2]
                        else:
                            h = emu.height(rec, [pt[:2], ph_[:2]])[0]
                            assert pt[2] == h[0] + npz and ph_[2] == h[1] + npz
                        seen += 1
    assert seen >= 20, seen


# ---- 5. the setter's argument check (round trip and survival of the resets: tests/test_gpu_sole.py) --------------------------------------------
def test_setter_refusals():
    ok = dict(mode=1, n_shift=3, shift_step=0.02, flat_tol=0.005)
    assert not se.refused(se.foothold_config(**ok))
    assert not se.refused(se.foothold_config(mode=1, n_shift=0, shift_step=0.0, flat_tol=0.0))      # no candidates: the step is not read
    assert not se.refused(se.foothold_config(**dict(ok, n_shift=abi.HB_FOOTHOLD_MAX_SHIFT)))
    for bad in (dict(mode=2), dict(mode=-1), dict(n_shift=-1), dict(n_shift=abi.HB_FOOTHOLD_MAX_SHIFT + 1), dict(shift_step=0.0),
                dict(shift_step=-0.01), dict(shift_step=np.nan), dict(shift_step=np.inf), dict(flat_tol=-1e-9), dict(flat_tol=np.nan),
                dict(flat_tol=np.inf)):
        assert se.refused(se.foothold_config(**dict(ok, **bad))), bad
