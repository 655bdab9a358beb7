"""--ground-map {none,profile,field} of tools/bench_refgen.py and tools/bench_estimator.py: a map of its own per instance, set before the
timed loop, so that the base, ground and field forms of k_refgen and k_estimator can each be timed by a tool of the tree."""
import numpy as np


def add_argument(ap):
    ap.add_argument("--ground-map", choices=("none", "profile", "field"), default="none",
                    help="the controller's ground map during the run: none (base forms), a ramp per instance as a profile map (ground forms) "
                         "or an oblique plane per instance as a field map (field forms)")


def apply(s, kind):
    """Instance i of the solver s gets a slope of its own (instance 0: level): a ramp along x from x = 0.05 on, or the plane
    z = p x + r y on a 32 x 32 grid turned against both axes, zero at the world origin."""
    B = s.B
    p, r = 0.01 * (np.arange(B) % 7), 0.005 * ((np.arange(B) % 5) - 2) * (np.arange(B) > 0)
    if kind == "profile":
        knots = np.zeros((B, 4, 2))
        knots[:, :, 0] = [-1.0, 0.05, 1.0, 3.0]
        knots[:, 2, 1], knots[:, 3, 1] = 0.95 * p, 2.95 * p
        s.ground_set_profile(np.full(B, 4, dtype=np.int32), np.tile([1.0, 0.0], (B, 1)), knots)
    elif kind == "field":
        a = np.array([0.8, 0.6])
        b = np.array([-a[1], a[0]])
        sp, org = np.array([0.06, 0.06]), np.array([-0.7, -0.9])
        uu, ww = np.meshgrid(org[0] + np.arange(32) * sp[0], org[1] + np.arange(32) * sp[1], indexing="ij")
        x, y = uu * a[0] + ww * b[0], uu * a[1] + ww * b[1]
        s.ground_set_field(np.tile(a, (B, 1)), np.tile(org, (B, 1)), np.tile(sp, (B, 1)), p[:, None, None] * x + r[:, None, None] * y)
