"""No GPU: the tolerance rules of tests/tolerance.py and the keep mask of tests/dense_twin.py bite where they should.

The inputs are built so that the figures are exact to rounding: r64 = (1, 0.5, -0.25) has max |r64| = 1, so an entry moved by e has
rel_err e; the element-wise bound of the entry 1 is 1e-4 + 2e-5 = 1.2e-4, so an entry moved by k 1.2e-4 has excess k."""
import numpy as np
import pytest
import torch

import camera_grad_common as cg
import dense_twin
import tolerance

R64 = np.array([1.0, 0.5, -0.25])


def _off(e, at=0):
    a = R64.copy()
    a[at] += e
    return a


@pytest.mark.parametrize("err, floor, passes", [(2e-4, 0.0, False), (3.1e-3, 1e-3, False), (0.9e-4, 0.0, True), (2.9e-3, 1e-3, True)])
def test_rule3_bound(err, floor, passes):
    assert tolerance.rel_err(_off(err), R64) == pytest.approx(err, rel=1e-9) and tolerance.rel_err(_off(floor, 1), R64) == pytest.approx(floor, rel=1e-9)
    if passes:
        tolerance.assert_rule3(_off(err), R64, _off(floor, 1), "case")
    else:
        with pytest.raises(AssertionError, match="rel err"):
            tolerance.assert_rule3(_off(err), R64, _off(floor, 1), "case")


def test_rule3_refuses_nan_and_a_zero_reference():
    got = R64.copy()
    got[2] = np.nan
    with pytest.raises(AssertionError, match="not finite"):
        tolerance.assert_rule3(got, R64, R64, "nan")
    with pytest.raises(AssertionError, match="reference is zero"):
        tolerance.assert_rule3(np.zeros(3), np.zeros(3), np.zeros(3), "zero")
    tolerance.assert_rule3(np.zeros(3), np.zeros(3), np.zeros(3), "zero", zero_means_zero=True)


def test_campos_with_a_zero_twin_gradient_demands_exact_zeros():
    vm = np.arange(1.0, 17.0).reshape(4, 4)
    ref = {d: dict(viewmatrix=vm, projmatrix=2 * vm, campos=np.zeros(3)) for d in ("float64", "float32")}
    got = dict(viewmatrix=vm.reshape(-1), projmatrix=2 * vm, campos=np.zeros(3))
    cg.assert_rule3(got, ref, "exact")
    with pytest.raises(AssertionError, match="exact zeros"):
        cg.assert_rule3(dict(got, campos=np.array([0.0, 1e-30, 0.0])), ref, "tiny")
    # only campos, and only where both references are zero
    zero_vm = {d: dict(ref[d], viewmatrix=np.zeros((4, 4))) for d in ref}
    with pytest.raises(AssertionError, match="reference is zero"):
        cg.assert_rule3(dict(got, viewmatrix=np.zeros(16)), zero_vm, "viewmatrix")
    half = dict(ref, float32=dict(ref["float32"], campos=np.array([0.0, 1e-9, 0.0])))
    with pytest.raises(AssertionError, match="reference is zero"):
        cg.assert_rule3(got, half, "float32 twin not zero")


def test_elementwise_bound_and_the_index_of_the_worst_element():
    unit = tolerance.RTOL + tolerance.ATOL_FRAC          # the bound of the entry 1.0
    a = _off(0.9 * unit, 0)
    a[2] -= 0.6 * unit                                      # the smaller error, against the smaller bound of the entry -0.25
    ex, where = tolerance.elem_excess(a.reshape(3, 1), R64.reshape(3, 1))
    assert where == 2 and ex == pytest.approx(0.6 * unit / (tolerance.RTOL * 0.25 + tolerance.ATOL_FRAC), rel=1e-9) and ex > 0.9
    with pytest.raises(AssertionError, match="worst element 0 off by 1.10x"):
        tolerance.assert_elementwise(_off(1.1 * unit), R64, _off(0.2 * unit), "case")
    assert tolerance.assert_elementwise(_off(2.9 * unit), R64, _off(1.0 * unit), "case") == pytest.approx((2.9, 1.0), rel=1e-9)
    with pytest.raises(AssertionError, match="well-conditioned"):
        tolerance.assert_elementwise(_off(2.9 * unit), R64, _off(1.0 * unit), "case", well_conditioned=True)
    with pytest.raises(AssertionError, match="off by 3.10x"):
        tolerance.assert_elementwise(_off(3.1 * unit), R64, _off(1.0 * unit), "case")


def test_quantiles_notice_a_broad_loss_that_the_worst_element_hides():
    rs = np.random.RandomState(0)
    r64 = rs.randn(4000)
    bound = tolerance.RTOL * np.abs(r64) + tolerance.ATOL_FRAC * np.abs(r64).max()
    r32 = r64 + 0.05 * bound * rs.uniform(-1, 1, 4000)
    r32[0] = r64[0] + 0.9 * bound[0]                       # one unlucky entry: the excess of the float32 reference is 0.9
    got = r64 + 0.5 * bound * rs.choice([-1.0, 1.0], 4000)      # every entry at half its bound
    tolerance.assert_elementwise(got, r64, r32, "broad")      # the worst element alone does not see it
    with pytest.raises(AssertionError, match="quantile"):
        tolerance.assert_quantiles(got, r64, r32, "broad")
    tolerance.assert_quantiles(r64 + 0.09 * bound, r64, r32, "under the floor")


def test_front_keeps_what_the_near_plane_may_let_through():
    vm = torch.eye(4)
    vm[3, 2] = 0.125                                        # z_view = z + 0.125, exact in float32
    z = torch.tensor([0.195, 0.185, 5.0, -3.0]) - 0.125
    kw = dict(viewmatrix=vm, means3D=torch.stack([torch.zeros(4), torch.zeros(4), z], 1))
    assert dense_twin.front(kw).tolist() == [True, False, True, False]
    assert dense_twin.front(dict(kw, viewmatrix=vm.double(), means3D=kw["means3D"].double())).tolist() == [True, False, True, False]
