"""-m gpu: k_estimator, k_estimator_ground and k_estimator_gfield through the C ABI against the extended-precision twin of the filter
(tests/_kftwin.py) on the edge streams of tests/_kfcases.py — what tests/test_estimator_twin_host.py holds the host emulator to, on the device.

Bound of every compared quantity: |device - twin| <= max(8 x the oracle's worst distance from the twin on that stream and quantity, 64 eps),
relative to max(1, |value|); the oracle's distance is recomputed here on the CPU.  The 8: the device factorises S by Cholesky, forms
Pm - (C Pm)' S^-1 (C Pm) and sums in another order, each a small multiple of the same rounding level.  pytest -s prints the measured ratios
(DESIGN.md 5 item 32 carries them next to the emulator's)."""
import numpy as np
import pytest

import _kfcases as kc

pytestmark = pytest.mark.gpu


def _device(params, s, rows=None, setup=None):
    """The stream (its instances `rows`, in that order) through estimator_reset / estimator_update / estimator_filter, every tick."""
    from hunter_bipedal_control_amd.solver import HunterSolver
    rows = np.arange(s["B"]) if rows is None else np.asarray(rows)
    cfg = kc.config_of(params, s)
    sel = lambda a: None if a is None else np.ascontiguousarray(np.asarray(a)[rows])
    solver = HunterSolver(params, batch=len(rows), max_nodes=4)
    try:
        if setup:
            setup(solver)
        solver.estimator_reset(cfg, sel(s["x_hat0"]))
        out = []
        for k in range(s["T"]):
            if k in s["resets"]:
                solver.estimator_reset(cfg, sel(s["resets"][k]))
            rbd, x = solver.estimator_update(float(s["dt"][k]), *[sel(a) for a in kc.sensors_at(s, k)])
            out.append(kc.pack_tick(rbd, x, *solver.estimator_filter()))
        return kc.collect(out)
    finally:
        solver.close()


@pytest.mark.parametrize("name", kc.NAMES)
def test_device_matches_the_twin(params, oracle, name):
    s, twin, orc, lev = kc.runs(params, oracle, name)
    assert kc.det_band(twin) >= kc.DET_BAND
    dev = _device(params, s)
    kc.assert_matches_twin(dev, twin, lev, name)
    assert kc.rel_err(dev["x"][..., 9], twin["yaw"]) <= kc.bounds(lev)["yaw"] and np.array_equal(dev["x"][..., 12:], s["qj"])
    worst = kc.momentum_ratio(oracle, dev)
    print("%-19s momentum: %.2f x its bound" % (name, worst))
    assert worst <= 1.0
    # for information only (code under test against itself): the device against the host emulator
    emu = kc.run_emu(params, s)
    print("%-19s device - emulator: " % name + "  ".join("%s %.1e" % (q, kc.rel_err(dev[q], emu[q])) for q in kc.QUANTITIES))


def test_instances_are_independent(params):
    """The contacts stream with the instance order reversed gives the same rows bit for bit, and so does instance 7 alone in a batch of 1."""
    s = kc.stream(params, "contacts")
    base = _device(params, s)
    rev = _device(params, s, rows=np.arange(s["B"])[::-1])
    one = _device(params, s, rows=[7])
    for key in ("rbd", "x", "xhat", "P"):
        assert np.array_equal(rev[key][:, ::-1], base[key]), key
        assert np.array_equal(one[key][:, 0], base[key][:, 7]), key


@pytest.mark.parametrize("kind", ["profile", "field"])
def test_map_forms_match_the_twin(params, oracle, kind):
    """The cases of tests/_groundtwin.py (profile) and tests/_groundfieldtwin.py (field), ten ticks per map: the twin's foot-height measurements
    are the numpy map's G at the twin's predicted foot x, y.  xhat, P, rbd[3:6], x[6:9]."""
    import _groundfieldtwin as gft
    import _groundtwin as gt
    s, maps, fresh, twin, lev = kc.map_case(params, oracle, kind)
    assert min(m.margin for m in fresh) > (gt.MARGIN if kind == "profile" else gft.MARGIN)      # no evaluated point sits on a riser
    if kind == "profile":
        assert max(abs(h) for m in maps for h in m.knots[:, 1]) > 0.0
        setup = lambda solver: solver.ground_set_profile(*gt.pack(maps))
    else:
        assert all(np.abs(m.g).max() > 0.0 for m in maps)
        setup = lambda solver: solver.ground_set_field(*gft.pack(maps))
    dev = _device(params, s, setup=setup)
    kc.assert_matches_twin(dev, twin, lev, "map_" + kind, quantities=("pos", "xhat", "P"))
