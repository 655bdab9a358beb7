"""The lane primitives of hb_math.hpp (DPP row shifts with bank masks, bound_ctrl and carriers; all behind __HIP_DEVICE_COMPILE__), one
per kernel of tests/gpu_unit/primitives.hip on a full wavefront: every lane active, 64 distinct values per case, each primitive once
with small integers (every sum exact) and once with random f64.  A wrong mask or a stale carrier gives a plausible number; these
tests compare with the exact result (math.fsum) lane by lane."""
import numpy as np
import pytest

import _gpuunit
import _primcheck as pc

pytestmark = pytest.mark.gpu
KINDS = ["int", "f64"]


@pytest.fixture(scope="module")
def dev():
    return _gpuunit.device()


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("op,width,depth", [("wave_sum_f64", 64, 6), ("quad_sum_f64", 4, 2), ("seg8_allsum", 8, 3)])
def test_sums(dev, op, width, depth, kind):
    """bit-exact for integers; otherwise within gamma_d sum |v| with d the depth of the ladder (6 shifts for the wavefront, 2 for a
    quad, 3 for a group of eight: every input passes through d additions), the same bits in every lane of a group"""
    v = pc.lane_values(kind, 8, np.random.default_rng(31))
    pc.check_group_sum(f"{op} {kind}", v, dev.lanes(op, v), width, depth, exact=kind == "int")


def max_cases(kind):
    """64 cases: the maximum of the wavefront sits in lane p of case p"""
    v = pc.lane_values(kind, 64, np.random.default_rng(32))
    for p in range(64):
        q = int(np.argmax(v[p]))
        v[p, [p, q]] = v[p, [q, p]]
        assert np.argmax(v[p]) == p
    return v


@pytest.mark.parametrize("kind", KINDS)
def test_wave_max(dev, kind):
    """bit-equal to the true maximum wherever it sits, the same bits in every lane"""
    v = max_cases(kind)
    pc.check_bits_equal(f"wave_max_f64 {kind}", dev.lanes("wave_max_f64", v), np.repeat(v.max(axis=1)[:, None], 64, axis=1))


@pytest.mark.parametrize("kind", KINDS)
def test_seg8_allmax(dev, kind):
    v = max_cases(kind)
    pc.check_bits_equal(f"seg8_allmax {kind}", dev.lanes("seg8_allmax", v), pc.group_reduce(v, 8, max))


@pytest.mark.parametrize("kind", KINDS)
def test_wave_max_nonneg(dev, kind):
    """max(0, max v), bit-equal and the same in every lane: with the (positive) maximum in each lane in turn, with every lane negative
    (-> +0.0) and with -0.0 in every lane (-> +0.0).
    wave_max_pos_f64, the ladder without the final zero that the two call sites use (hb_lq.hpp, pivot search of the rank-revealing
    Cholesky): they compare the result with `!(best > tol)`, tol >= 0, and pick the pivot with `v == best`, so what they rely on is
    the exact maximum when it is positive and a value that is not positive otherwise, the same in every lane.
    A NaN in one lane: a NaN lane is never picked by `v == best`, and either outcome of `best > tol` ends or continues a
    factorisation whose instance is marked non-finite elsewhere.  The call sites rely on nothing here, so nothing is asserted for NaN."""
    v = max_cases(kind)
    assert (v.max(axis=1) > 0).all()
    neg = -np.abs(pc.lane_values(kind, 2, np.random.default_rng(33))) - 1.0
    v = np.concatenate([v, neg, np.full((1, 64), -0.0)])
    ref = np.repeat(np.maximum(v.max(axis=1), 0.0)[:, None], 64, axis=1) + 0.0     # (+ 0.0: the -0.0-only case is +0.0 as well)
    pc.check_bits_equal(f"wave_max_nonneg_f64 {kind}", dev.lanes("wave_max_nonneg_f64", v), ref)
    pos = dev.lanes("wave_max_pos_f64", v)
    pc.check_bits_equal(f"wave_max_pos_f64 {kind}, positive maxima", pos[:64], ref[:64])
    assert not (pos[64:] > 0.0).any() and (pos[64:].view(np.uint64) == pos[64:, :1].view(np.uint64)).all(), pos[64:, :2]


@pytest.mark.parametrize("kind", KINDS)
def test_wave_bcast(dev, kind):
    """every src"""
    v = pc.lane_values(kind, 64, np.random.default_rng(34))
    idx = np.repeat(np.arange(64, dtype=np.int32)[:, None], 64, axis=1)
    pc.check_bits_equal(f"wave_bcast_f64 {kind}", dev.lanes("wave_bcast_f64", v, idx), np.repeat(v[np.arange(64), np.arange(64)][:, None], 64, axis=1))


@pytest.mark.parametrize("kind", KINDS)
def test_wave_gather(dev, kind):
    """the identity, a random permutation, a non-injective map and the three index expressions of the constant gather of hb_lq.hpp
    (lq_node: limits and R_FF weights out of the lane-indexed constant table)"""
    rng = np.random.default_rng(35)
    l = np.arange(64)
    foot = (l - 56) & 3
    maps = [l, rng.permutation(64), rng.integers(0, 64, 64) // 7 * 7,
            np.where(l < 22, l + 22, np.where(l < 44, l + 20, 22 + 3 * foot)), np.where(l < 22, l + 32, 23 + 3 * foot), 24 + 3 * foot]
    idx = np.array(maps, dtype=np.int32)
    assert idx.min() >= 0 and idx.max() < 64
    v = pc.lane_values(kind, len(maps), rng)
    pc.check_bits_equal(f"wave_gather_f64 {kind}", dev.lanes("wave_gather_f64", v, idx), np.take_along_axis(v, idx.astype(np.int64), axis=1))


@pytest.mark.parametrize("kind", KINDS)
def test_seg8_get(dev, kind):
    """a different k in every group"""
    rng = np.random.default_rng(36)
    v = pc.lane_values(kind, 8, rng)
    k = np.stack([rng.permutation(8) for _ in range(8)])
    idx = np.repeat(k, 8, axis=1).astype(np.int32)
    src = (np.arange(64)[None, :] & 56) | idx
    pc.check_bits_equal(f"seg8_get {kind}", dev.lanes("seg8_get", v, idx), np.take_along_axis(v, src.astype(np.int64), axis=1))


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("op", ["seg8_suffix_sum", "seg8_prefix_sum"])
def test_seg8_scans(dev, op, kind):
    """lanes 5..7 of every group zero (the contract), different data in all eight groups, lanes 0..4 compared: exact for integers, within
    gamma_3 sum |v| otherwise — over three calls ON THE SAME Seg8Carry with new data each time ("never has to be re-initialised")."""
    v = pc.seg8_scan_inputs(kind, 6, np.random.default_rng(37))
    out = dev.lanes(op, v.reshape(6, 576)).reshape(v.shape)
    pc.check_seg8_scan(f"{op} {kind}", v, out, suffix=op == "seg8_suffix_sum", exact=kind == "int")


@pytest.mark.parametrize("op", ["seg8_suffix_sum", "seg8_prefix_sum"])
def test_seg8_scans_keep_to_their_group(dev, op):
    """no group's result depends on its neighbour in the DPP row of 16: perturb one group (all eight lanes, in every round) and the other
    seven come back bit-unchanged"""
    base = pc.seg8_scan_inputs("f64", 1, np.random.default_rng(38))[0]
    cases = [base]
    for g in range(8):
        p = base.copy()
        p[..., 8 * g:8 * g + 5] += 1000.0 * (1 + np.arange(5))
        cases.append(p)
    out = dev.lanes(op, np.array(cases).reshape(9, 576)).reshape(9, 3, 3, 64)
    live = (np.arange(64) % 8) < 5
    for g in range(8):
        others = live & ((np.arange(64) // 8) != g)
        pc.check_bits_equal(f"{op}: groups other than {g}", out[1 + g][..., others], out[0][..., others])
        assert (out[1 + g][..., 8 * g:8 * g + 5] != out[0][..., 8 * g:8 * g + 5]).any()


def test_seg8_prefix_product(dev):
    """lane k < 5 of a group holds a random rotation; afterwards it holds M_0 ... M_k in that order (seg8_prefix_product, the three
    seg8_prefix_mat3 steps of hb_model.hpp and hb_refgen.hpp), within 16 u per entry of the product in mpmath"""
    inp = pc.prefix_product_inputs(3, np.random.default_rng(39))
    out = dev.lanes("seg8_prefix_product", inp.reshape(3, 576)).reshape(inp.shape)
    pc.check_prefix_product("seg8_prefix_product", inp, out)
