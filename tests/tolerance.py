"""The tolerance rules of the test-suite, each stated once (test infrastructure).

Rule 3, per tensor in the max norm, against a float64 reference r64 and the same reference evaluated in float32, r32:
    rel_err(got, r64) <= max(1e-4, 3 rel_err(r32, r64)).
Element-wise: |a - b| <= 1e-4 |b| + 2e-5 max|b| (the second term an absolute floor for entries that are small only through
cancellation); the excess -- the worst ratio of an error to that bound -- must not be above max(1, 3 x the float32 reference's), and
the 0.5 / 0.99 / 0.999 quantiles of the ratios not above max(0.1, 3 x the float32 reference's).
Every figure is printed before it is asserted."""
import numpy as np

TOL = 1e-4                      # rule 3: the bound where the float32 reference is better than a third of it
SLACK = 3.0                     # ... and how many times the float32 reference's own figure is allowed
RTOL, ATOL_FRAC = 1e-4, 2e-5    # the element-wise bound
QUANTILES = (0.5, 0.99, 0.999)
QUANTILE_FLOOR = 0.1


def rel_err(a, b):
    """max |a - b| relative to max |b|."""
    a = np.asarray(a, np.float64); b = np.asarray(b, np.float64)
    return float(np.abs(a - b).max() / (np.abs(b).max() + 1e-30))


def rule3_bound(floor, tol=TOL):
    return max(tol, SLACK * floor)


def elem_ratios(a, b, rtol=RTOL, atol_frac=ATOL_FRAC):
    """|a - b| / (rtol |b| + atol_frac max|b|), flat."""
    a = np.asarray(a, np.float64).reshape(-1); b = np.asarray(b, np.float64).reshape(-1)
    return np.abs(a - b) / (rtol * np.abs(b) + atol_frac * (np.abs(b).max() + 1e-300))


def elem_excess(a, b, rtol=RTOL, atol_frac=ATOL_FRAC):
    """(worst ratio of elem_ratios, flat index of the worst element): <= 1 passes."""
    ratio = elem_ratios(a, b, rtol, atol_frac)
    i = int(ratio.argmax())
    return float(ratio[i]), i


def assert_rule3(got, r64, r32, what, *, tol=TOL, ref="twin", nonzero=True, zero_means_zero=False):
    """Rule 3 for one tensor: got finite, r64 not all zero (nonzero=False: not asked) and the rule.  ref: what the references are called
    in the printed line.  zero_means_zero: where both references are identically zero, got must be exact zeros instead."""
    r64 = np.asarray(r64, np.float64)
    g = np.asarray(got, np.float64).reshape(r64.shape)
    if zero_means_zero and not r64.any() and not np.asarray(r32).any():
        print(f"{what}: the {ref}'s gradient is identically zero")
        assert not g.any(), f"{what}: must be exact zeros"
        return
    floor, err = rel_err(r32, r64), rel_err(g, r64)
    print(f"{what}: rel_err {err:.3e} (float32 {ref} {floor:.3e}, max |d64| {np.abs(r64).max():.3e})")
    assert np.isfinite(g).all(), f"{what}: not finite"
    assert not nonzero or np.abs(r64).max() > 0, f"{what}: the reference is zero"
    assert err <= rule3_bound(floor, tol), f"{what}: rel err {err:.3e} (float32 {ref} floor {floor:.3e})"


def assert_elementwise(got, r64, r32, what, *, ref="oracle", well_conditioned=False):
    """The element-wise excess of got within max(1, 3 x the float32 reference's); well_conditioned: both within 1.  Returns both."""
    r64 = np.asarray(r64, np.float64)
    g = np.asarray(got, np.float64).reshape(r64.shape)
    (ex, where), (ex32, _) = elem_excess(g, r64), elem_excess(r32, r64)
    print(f"{what}: elem_excess {ex:.3f} (float32 {ref} {ex32:.3f})")
    assert ex <= max(1.0, SLACK * ex32), (f"{what}: worst element {where} off by {ex:.2f}x the element-wise bound (float32 {ref}: {ex32:.2f}x); "
                                          f"got {g.reshape(-1)[where]:.6e} ref {r64.reshape(-1)[where]:.6e}")
    if well_conditioned:
        assert ex32 <= 1.0 and ex <= 1.0, f"{what}: element-wise bound missed on a well-conditioned scene ({ex:.2f}x, float32 {ref} {ex32:.2f}x)"
    return ex, ex32


def assert_quantiles(got, r64, r32, what, *, ref="oracle"):
    """The DISTRIBUTION of got's element errors (in units of the element bound) must not be worse than 3x that of the float32 reference,
    at the median, the 99th and the 99.9th percentile (floor: a tenth of the bound).  A single entry proves nothing on an ill-conditioned
    scene (where float32 lands is luck); a broad loss of accuracy moves the quantiles."""
    rh, ro = elem_ratios(got, r64), elem_ratios(r32, r64)
    for q in QUANTILES:
        qh, qo = float(np.quantile(rh, q)), float(np.quantile(ro, q))
        print(f"{what}: {q:.3f}-quantile of the element error {qh:.3f}x the bound (float32 {ref} {qo:.3f}x)")
        assert qh <= max(QUANTILE_FLOOR, SLACK * qo), f"{what}: {q:.3f}-quantile of the element error is {qh:.3f}x the bound (float32 {ref}: {qo:.3f}x)"
