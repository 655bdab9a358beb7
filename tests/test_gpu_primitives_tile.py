"""The tile GEMMs of hb_tile.hpp as the DEVICE compiles them (MFMA fragments, KR < K selects, PRE, weights, step_live), instantiated
with exactly the template argument lists and (Mr, Nr) pairs of the product's call sites (tests/gpu_unit/prim_cases.hpp HBP_TILE_SPECS,
tests/_primcheck.py TILE_SITES).  The wrapper places the operands in an LDS block, starts the accumulators through tile_init and
returns the result through tile_store_rm into a destination pre-filled with a sentinel.  tests/test_primitives_host.py runs the same
scenarios on the host loops."""
import pytest

import _gpuunit
import _primcheck as pc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    return _gpuunit.device()


def test_every_instantiation_is_visited(dev):
    assert {s[0] for s in pc.TILE_SITES} == set(range(dev.n_tile_specs))


@pytest.mark.parametrize("site", pc.TILE_SITES, ids=pc.TILE_SITE_IDS)
def test_exact_product_and_poison(dev, site):
    """Small-integer A, B, C0 (every partial sum exact): the live Mr x Nr block equals the integer product bit for bit and every other
    destination word still holds the sentinel.  Then the same operands in a hostile image, each contract taken literally — NaN in
    k >= KR where the product masks (zero padding where it does not), NaN in rows >= Mr and columns >= Nr of the operands, 1e300 in the
    rows of Bt beyond the real depth, NaN behind every K-step that step_live rules out: bit-identical.  Weighted products run under
    six contact masks with the 0 / 1 and soft-weight lambdas of the call sites."""
    pc.tile_exact_scenario(dev, site)


@pytest.mark.parametrize("site", pc.TILE_SITES, ids=pc.TILE_SITE_IDS)
def test_unit_matrix_probes(dev, site):
    """A = E_ik, B = E_kj gives w(k) E_ij, for the first and last live row, column and k among others: pins transposes and tnb0"""
    pc.tile_unit_scenario(dev, site)


@pytest.mark.parametrize("site", pc.TILE_SITES, ids=pc.TILE_SITE_IDS)
def test_rounding(dev, site):
    """random f64 operands spread over 12 decades: |err_ij| <= gamma_(K+1) (|C0| + |A||B|)_ij against the exact product"""
    pc.tile_rounding_scenario(dev, site)


@pytest.mark.parametrize("Mr,Nr", pc.RT_SHAPES)
def test_initialisers_and_stores(dev, Mr, Nr):
    """tile_init, tile_init_rm, tile_init_col, tile_set_col, tile_add, tile_store, tile_store_pre, tile_store_rm and tile_store_rm_cols
    (a window inside Nr and one that reaches behind it), each a round trip against numpy on a 2 x 3 block of tiles; the functions
    handed to tile_init, tile_store_pre and tile_set_col count every call with an index outside the live range (the clamped-index
    rule): none."""
    pc.tile_roundtrip_scenario(dev, Mr, Nr)
