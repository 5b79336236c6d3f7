"""The covariance model of the restatements (tests/cov_restatement.py) without a device: for every
legal (family, kind, bias, linear) its dK against central differences of its own Gram, and its
theta length, C-ABI value and name against the library's Python layer."""
import numpy as np
import pytest

import cov_restatement as cr
from cov_restatement import Cov

LEGAL = [(f, k, b, l) for f, k in cr.FAMILY_KINDS for b in (False, True) for l in (False, True)
         if f == 'se' or not l]


def test_dk_is_the_derivative_of_gram_and_the_kinds_are_the_librarys():
    """n = 7, d = 3, the 16 legal kinds. Every dK/dtheta_j against central differences (h = 1e-5)
    of Cov.gram, entry by entry, to 1e-6 of max(1, max|fd|) (the bound of the host tests' gradient
    checks); epsilon is in none of them, so it is taken large. theta_len, native_kind and name are
    those of gpdemo._native.theta_len and gpdemo.kernels.make_kernel_func, and the linear term on
    a Matern family is refused as the library refuses it."""
    from gpdemo import _native
    import gpdemo.kernels as krn
    assert len(LEGAL) == 16
    rng = np.random.RandomState(17)
    X = rng.normal(size=(7, 3))
    for family, kind, bias, linear in LEGAL:
        cov = Cov(family, kind, bias, linear)
        P, p0 = cov.theta_len(3), cov.n_base(3)
        assert P == (4 if kind == 'ard' else 2) + bias + linear
        th = np.r_[0.3, rng.uniform(-0.3, 0.5, size=p0 - 1), [1.5, -0.5][:P - p0]]
        D = cov.dK(X, th, 1e-2)
        assert len(D) == P
        for j in range(P):
            e = np.zeros(P)
            e[j] = 1e-5
            fd = (cov.gram(X, th + e, 1e-2) - cov.gram(X, th - e, 1e-2)) / 2e-5
            assert np.abs(D[j] - fd).max() <= 1e-6 * max(1.0, np.abs(fd).max()), (cov, j)
        kf = krn.make_kernel_func(cov.name, 1e-8, bias=bias, linear=linear)
        assert kf.native_kind == cov.native_kind, cov
        for d in (1, 3, 5):
            assert _native.theta_len(cov.native_kind, d) == cov.theta_len(d), (cov, d)
        with pytest.raises(IndexError):
            cov.split(th[:-1], 3)
    for family in cr.MATERN:
        for kind in ('iso', 'ard'):
            with pytest.raises(ValueError):
                Cov(family, kind, linear=True)
            with pytest.raises(ValueError):
                krn.make_kernel_func(Cov(family, kind).name, 1e-8, linear=True)
