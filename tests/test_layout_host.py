"""CPU: the layout descriptions of csrc/hb_layout.hpp (one per batch struct: every device array with its per-instance extent) compiled
for the host (tests/host_emu/layoutemu.cpp), against a table written out by hand from the expressions the library used before the
descriptions existed — the allocation lists of hb_create / hb_plant_reset / hb_refgen_reset / hb_gait_reset / hb_estimator_reset /
hb_*_set_certificate / hb_mpc_get_certificate and batch_view, wbc_view, est_view, refgen_view, gait_view.

B = 3 instances, Nmax = 4 nodes, view of the instance range (i0 = 2, cnt = 1).  Per array: elements the view moves the base pointer by,
elements allocated for the batch, bytes per element.  With the constants of the headers (22 states / inputs, 32 rbd, 38 WBC unknowns,
16 generalised velocities, 10 joints, records of 2112 and gains of 288 doubles, parked images of 1024 doubles and trips of 16 nodes,
16 line-search step sizes, 64 events, 8 doubles per swing phase, 24 knots, templates of 8 phases, a velocity history of 50, certificate
nodes of 56 doubles, certificates of 8 (MPC), 8 + 60 duals (WBC), 3 levels x 10 with 40 inequality rows (HWBC))."""
import subprocess
from pathlib import Path

import pytest

HERE = Path(__file__).resolve().parent / "host_emu"
B, N, I0, CNT = 3, 4, 2, 1
D, I = 8, 4   # bytes of a double, an int

# struct -> [(member, view offset = o * per-instance extent with o = 2, elements allocated = 3 * extent, bytes per element)]
EXPECTED = {
    "Batch": [
        ("n_nodes", 2, 3, I), ("t", 2 * 5, 3 * 5, D), ("mode", 2 * 4, 3 * 4, I), ("xref", 2 * 4 * 22, 3 * 4 * 22, D), ("swing", 2 * 4 * 24, 3 * 4 * 24, D),
        ("x", 2 * 5 * 22, 3 * 5 * 22, D), ("u", 2 * 4 * 22, 3 * 4 * 22, D), ("x0", 2 * 22, 3 * 22, D), ("recs", 2 * 4 * 2112, 3 * 4 * 2112, D),
        ("gains", 2 * 4 * 288, 3 * 4 * 288, D), ("dx", 2 * 5 * 22, 3 * 5 * 22, D), ("du", 2 * 4 * 22, 3 * 4 * 22, D), ("acc", 2 * 4, 3 * 4, D),
        ("partial", 2 * 4 * 3, 3 * 4 * 3, D), ("ls_tail", 2 * 16 * 4 * 3, 3 * 16 * 4 * 3, D), ("ls_norm", 2 * 2, 3 * 2, D), ("accepted", 2, 3, I),
        ("perf", 2 * 4, 3 * 4, D), ("ric_fail", 2, 3, I), ("mpc_status", 2, 3, I), ("xp", 2 * 5 * 22, 3 * 5 * 22, D), ("up", 2 * 4 * 22, 3 * 4 * 22, D),
        ("tp", 2 * 5, 3 * 5, D), ("modep", 2 * 4, 3 * 4, I), ("np_nodes", 2, 3, I), ("grid_dirty", 2, 3, I),
        ("lqpark", 2 * (4 + 16) * 1024, 3 * (4 + 16) * 1024, D)],
    "WbcBatch": [
        ("t_now", 2, 3, D), ("rbd", 2 * 32, 3 * 32, D), ("walk", 2, 3, I), ("xdes", 2 * 22, 3 * 22, D), ("udes", 2 * 22, 3 * 22, D), ("mode", 2, 3, I),
        ("stance", 2, 3, I), ("sol", 2 * 38, 3 * 38, D), ("status", 2, 3, I), ("iters", 2, 3, I), ("px", 2 * 5 * 22, 3 * 5 * 22, D),
        ("pu", 2 * 4 * 22, 3 * 4 * 22, D), ("pt", 2 * 5, 3 * 5, D), ("pmode", 2 * 4, 3 * 4, I), ("pn", 2, 3, I)],
    # est_view leaves the contact-force observer (cf_*) where it is; res_rbd / res_x0 are the caller's: not moved, not allocated
    "EstBatch": [
        ("xhat", 2 * 18, 3 * 18, D), ("P", 2 * 324, 3 * 324, D), ("yaw_last", 2, 3, D), ("quat", 2 * 4, 3 * 4, D), ("w_local", 2 * 3, 3 * 3, D),
        ("a_local", 2 * 3, 3 * 3, D), ("qj", 2 * 10, 3 * 10, D), ("qdj", 2 * 10, 3 * 10, D), ("contact", 2 * 4, 3 * 4, I), ("rbd", 2 * 32, 3 * 32, D),
        ("x", 2 * 22, 3 * 22, D), ("res_rbd", 0, None, D), ("res_x0", 0, None, D), ("cf_z", 0, 3 * 16, D), ("cf_tau", 0, 3 * 10, D),
        ("cf_dist", 0, 3 * 16, D), ("cf_out", 0, 3 * 16, D), ("cf_rbd", 0, 3 * 32, D)],
    "RefgenBatch": [
        ("n_ev", 2, 3, I), ("ev", 2 * 64, 3 * 64, D), ("modes", 2 * 65, 3 * 65, I), ("stance", 2 * 12, 3 * 12, D), ("phases", 2 * 4 * 65 * 8, 3 * 4 * 65 * 8, D),
        ("t0", 2, 3, D), ("cmd", 2 * 4, 3 * 4, D), ("status", 2, 3, I), ("n_knots", 2, 3, I), ("knot_t", 2 * 24, 3 * 24, D),
        ("knot_x", 2 * 24 * 22, 3 * 24 * 22, D)],
    # slot-major arrays [slots][B]: the view moves them by o = 2 (the pitch stays the whole batch), only cmd is instance-major
    "GaitBatch": [
        ("n_ev", 2, 3, I), ("ev", 2, 3 * 64, D), ("modes", 2, 3 * 65, I), ("tpl_n", 2, 3, I), ("tpl_sw", 2, 3 * 9, D), ("tpl_modes", 2, 3 * 8, I),
        ("last_vel", 2, 3 * 4, D), ("cmd", 2 * 4, 3 * 4, D), ("hist", 2, 3 * 50, D), ("hist_n", 2, 3, I), ("hist_head", 2, 3, I), ("level", 2, 3, I),
        ("vel_abs", 2, 3, D), ("vel_avg", 2, 3, D), ("status", 2, 3, I)],
    "MpcCertBuf": [("node", 2 * 4 * 56, 3 * 4 * 56, D), ("costate", 2 * 5 * 22, 3 * 5 * 22, D), ("cert", 2 * 8, 3 * 8, D), ("util", 2 * 4 * 12, 3 * 4 * 12, D)],
    "WbcCertBuf": [("cert", 2 * 8, 3 * 8, D), ("dual", 2 * 60, 3 * 60, D)],
    "HwbcCertBuf": [("cert", 2 * 3 * 10, 3 * 3 * 10, D), ("xlev", 2 * 3 * 38, 3 * 3 * 38, D), ("slack", 2 * 40, 3 * 40, D), ("dual", 2 * 3 * 40, 3 * 3 * 40, D)],
    # the plant runs on the whole batch only: allocation alone
    "PlantBatch": [
        ("q", None, 3 * 16, D), ("v", None, 3 * 16, D), ("anchor", None, 3 * 12, D), ("pinned", None, 3 * 4, I), ("lambda", None, 3 * 12, D),
        ("vdot", None, 3 * 16, D), ("tau", None, 3 * 10, D), ("contact", None, 3 * 4, I), ("rbd", None, 3 * 32, D), ("tau_last", None, 3 * 10, D),
        ("contact_last", None, 3 * 4, I), ("s_quat", None, 3 * 4, D), ("s_gyro", None, 3 * 3, D), ("s_accel", None, 3 * 3, D), ("s_jp", None, 3 * 10, D),
        ("s_jv", None, 3 * 10, D), ("s_jt", None, 3 * 10, D), ("s_contact", None, 3 * 4, I)],
}
# bytes hb_create (Batch, WbcBatch) and the first-use allocations request for the three instances
TOTAL_BYTES = {"Batch": 746664, "WbcBatch": 7752, "EstBatch": 12456, "RefgenBatch": 65928, "GaitBatch": 4140, "MpcCertBuf": 9360, "WbcCertBuf": 1632,
               "HwbcCertBuf": 7296, "PlantBatch": 4128}


@pytest.fixture(scope="module")
def layout(tmp_path_factory):
    exe = tmp_path_factory.mktemp("layoutemu") / "layoutemu"
    subprocess.check_call(["g++", "-O0", "-std=c++17", "-w", "-o", str(exe), str(HERE / "layoutemu.cpp")])
    out = subprocess.check_output([str(exe), str(B), str(N), str(I0), str(CNT)], text=True)
    got = {"view": {}, "alloc": [], "bytes": {}, "scalars": {}}
    for line in out.splitlines():
        kind, name, *rest = line.split()
        if kind == "view":
            got["view"][name] = int(rest[0])
        elif kind == "alloc":
            got["alloc"].append((name, int(rest[0]), int(rest[1])))
        elif kind == "bytes":
            got["bytes"][name] = int(rest[0])
        else:
            got["scalars"][name] = tuple(int(v) for v in rest)
    return got


@pytest.mark.parametrize("struct", sorted(EXPECTED))
def test_instance_range_view_moves_every_array_by_its_extent(layout, struct):
    want = {f"{struct}.{m}": off for m, off, _, _ in EXPECTED[struct] if off is not None}
    got = {k: v for k, v in layout["view"].items() if k.startswith(struct + ".")}
    assert got == want


@pytest.mark.parametrize("struct", sorted(EXPECTED))
def test_allocation_requests_every_array_in_order_with_its_size(layout, struct):
    want = [(f"{struct}.{m}", n, size) for m, _, n, size in EXPECTED[struct] if n is not None]
    got = [a for a in layout["alloc"] if a[0].startswith(struct + ".")]
    assert got == want   # (in allocation order: hb_create allocates ls_tail ahead of ls_norm)
    assert layout["bytes"][struct] == TOTAL_BYTES[struct] == sum(n * size for _, n, size in want)


def test_linesearch_arrays_have_the_extents_the_getter_documents(layout):
    """hb_mpc_get_linesearch copies acc [4], partial [N][3], ls_tail [HB_LS_TAIL_MAX][N][3], ls_norm [2], accepted, ric_fail per instance:
    the extents of the description (the copy is sized by them) are the shapes hunter_hip.h and HunterSolver.mpc_linesearch give."""
    from hunter_bipedal_control_amd import abi
    want = {"acc": (4, D), "partial": (N * 3, D), "ls_tail": (abi.HB_LS_TAIL_MAX * N * 3, D), "ls_norm": (2, D), "accepted": (1, I), "ric_fail": (1, I)}
    alloc = {name: (n, size) for name, n, size in layout["alloc"]}
    for member, (extent, size) in want.items():
        assert alloc[f"Batch.{member}"] == (B * extent, size) and layout["view"][f"Batch.{member}"] == I0 * extent, member


def test_view_sets_the_instance_count_and_keeps_the_other_scalars(layout):
    # (B of the view, the remaining scalar unchanged: Nmax, policy_valid, init_stance, and the pitch of the slot-major gait arrays)
    assert layout["scalars"] == {s: (CNT, 1) for s in ("Batch", "WbcBatch", "EstBatch", "RefgenBatch", "GaitBatch")}
