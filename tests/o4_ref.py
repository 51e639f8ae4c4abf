"""o4_ref -- numpy references of the fourth-order defect correction (TEST INFRASTRUCTURE; mg_o4_*, include/mg_hip.h).

* residual_np / correct_np: the arithmetic contract of mg_o4.hip restated in the working dtype, one rounding per operation;
  the same functions on long-double arrays are the high-precision version the bounds are taken from;
* a4_mag: the sum of the magnitudes of every term of A4 u, the scale of any rounding bound on it;
* level0_coef: the fp64 coefficients a handle reports for level 0, restated (no handle needed on the CPU);
* Manufactured: the non-polynomial solution the convergence checks use, its right-hand side and Dirichlet data;
* sparse_a2 / defect_correction: the scheme itself with an exact inner solve (scipy's sparse LU).
Imports nothing from oracle/.
"""
from __future__ import annotations

import numpy as np

LD = np.longdouble


# kernel parity cases of tests/test_o4_gpu.py: (dim, n, levels, extra descriptor fields) -- the smallest shapes at which each
# piece can go wrong: n = 7 (every interior node of a closure row sees both closures), rows of several waves (2-D 129, 257),
# the first full-width row of the marching tile (3-D 129), a grid that is not 2^k + 1, semi-coarsening, anisotropy, and the row
# ends of the marching tile other than the single tail column of an odd n: even rows (34, 66, 68: no tail line, the last lane
# owns column nx-2 and the Dirichlet column; one level, since n - 1 is odd) and a partial last vector stored element by
# element (fp32: 66 -> 2 elements, 67 -> 3; 67 is the tail column in fp64)
ANISO = (1.0, 2.5, 0.3)
KERNEL_CASES = [
    (2, 7, 2, {}), (2, 9, 2, {}), (2, 33, 3, dict(aniso=ANISO)), (2, 129, 3, {}), (2, 257, 3, {}),
    (3, 7, 2, {}), (3, 9, 2, {}), (3, 17, 3, dict(aniso=ANISO)), (3, 33, 3, dict(aniso=ANISO)), (3, 65, 3, dict(aniso=ANISO)),
    (3, 129, 3, {}), (3, 25, 4, {}), (3, 33, 3, dict(semi_xy=1)),
    (3, 34, 1, {}), (3, 66, 1, dict(aniso=ANISO)), (3, 67, 2, {}), (3, 68, 1, {}),
]


def kernel_side(dim, n, elem_size):
    """which form of mg_o4.hip a level-0 shape takes (o4_march_ok, mg_geom.h, pinned by tests/test_o4_cpu.py)"""
    return "march" if dim == 3 and n // (16 // elem_size) >= 16 else "plain"


def level0_coef(dim, n, length=1.0, alpha=1.0, aniso=(1.0, 1.0, 1.0)):
    """(cx, cy, cz, cd) of level 0 in fp64, operation by operation as the library computes them"""
    m_h = float(length) / float(n - 1)
    k = (m_h * 1.0) * (m_h * 1.0)
    cx, cy, cz = (-(float(alpha) * float(a)) / k for a in aniso)
    s = (aniso[0] + aniso[1] + aniso[2]) if dim == 3 else (aniso[0] + aniso[1])
    return cx, cy, cz, ((2.0 * s) * float(alpha)) / k


def interior(ndim):
    return (slice(1, -1),) * ndim


def boundary_mask(shape):
    m = np.ones(shape, bool)
    m[interior(len(shape))] = False
    return m


def p_axis(u, axis, mag=False):
    """p_a of the contract along `axis` at the nodes 1 .. n-2 of that axis (every node of the other axes), in u's dtype;
    mag=True: the same expressions with every term replaced by its magnitude"""
    T = u.dtype.type
    n = u.shape[axis]
    assert n >= 7
    v = np.moveaxis(abs(u) if mag else u, axis, 0)
    sgn = T(1) if mag else T(-1)   # the sign the subtracted terms enter with
    p = np.empty((n - 2,) + v.shape[1:], u.dtype)
    p[1:n - 3] = ((T(16) * (v[1:n - 3] + v[3:n - 1])) + sgn * (v[0:n - 4] + v[4:n])) + sgn * (T(30) * v[2:n - 2])

    def closure(t):
        return (((((T(10) * t[0] + sgn * (T(15) * t[1])) + sgn * (T(4) * t[2])) + T(14) * t[3]) + sgn * (T(6) * t[4])) + t[5])
    p[0] = closure([v[k] for k in range(6)])
    p[n - 3] = closure([v[n - 1 - k] for k in range(6)])
    return np.moveaxis(p, 0, axis)


def _weights(coef, T):
    """(wz, wy, wx) = (T)(c_a / 12), the division in fp64 -- for long double the fp64 quotient is taken as it is"""
    cx, cy, cz = (float(c) / 12.0 for c in coef[:3])
    return T(cz), T(cy), T(cx)


def a4_np(u, coef, sigma, mag=False):
    """((sigma u + wz p_z) + wy p_y) + wx p_x at the interior nodes, in u's dtype, every operation rounded separately"""
    T = u.dtype.type
    wz, wy, wx = _weights(coef, T)
    sg = T(sigma)
    if mag:
        wz, wy, wx, sg = abs(wz), abs(wy), abs(wx), abs(sg)
    nd = u.ndim
    I = interior(nd)

    def inner(p, axis):   # p has the interior extent along `axis` only
        sl = [slice(1, -1)] * nd
        sl[axis] = slice(None)
        return p[tuple(sl)]
    s = sg * (abs(u[I]) if mag else u[I])
    if nd == 3:
        s = s + wz * inner(p_axis(u, 0, mag), 0)
    s = s + wy * inner(p_axis(u, nd - 2, mag), nd - 2)
    s = s + wx * inner(p_axis(u, nd - 1, mag), nd - 1)
    return s


def a4_mag(u, coef, sigma):
    return a4_np(u, coef, sigma, mag=True)


def residual_np(u, b, coef, sigma):
    """r = b - A4u on interior nodes, 0 on Dirichlet nodes"""
    r = np.zeros_like(u)
    I = interior(u.ndim)
    r[I] = b[I] - a4_np(u, coef, sigma)
    return r


def correct_np(u, e):
    """u + e on interior nodes, u on Dirichlet nodes (e is not looked at there)"""
    out = u.copy()
    I = interior(u.ndim)
    out[I] = u[I] + e[I]
    return out


def sumsq(r) -> float:
    rr = np.asarray(r, LD).ravel()
    return float(np.sum(rr * rr))


# ---------------------------------------------------------------- the manufactured problem
class Manufactured:
    """u* = sin(2.3 x + 0.4) exp(1.1 y) cos(1.7 z - 0.2) + x y z on [0, length]^dim (2-D: the z factor is cos(-0.2), z = 0),
    for -sum_a kappa_a d^2/da^2 u + sigma u = f with kappa_a = alpha aniso_a; b = f inside, u* on Dirichlet nodes"""

    def __init__(self, dim, n, length=1.0, alpha=1.0, aniso=(1.0, 1.0, 1.0), sigma=0.0):
        self.dim, self.n, self.sigma = dim, n, sigma
        self.coef = level0_coef(dim, n, length, alpha, aniso)
        t = LD(length) * np.arange(n, dtype=LD) / LD(n - 1)
        if dim == 3:
            z, y, x = np.meshgrid(t, t, t, indexing="ij")
        else:
            y, x = np.meshgrid(t, t, indexing="ij")
            z = np.zeros_like(x)
        P = np.sin(LD(2.3) * x + LD(0.4)) * np.exp(LD(1.1) * y) * np.cos(LD(1.7) * z - LD(0.2))
        self.u = P + x * y * z
        kx, ky, kz = (LD(alpha) * LD(a) for a in aniso)
        f = kx * LD(2.3) ** 2 * P - ky * LD(1.1) ** 2 * P + LD(sigma) * self.u
        if dim == 3:
            f = f + kz * LD(1.7) ** 2 * P
        self.b = self.u.copy()
        I = interior(dim)
        self.b[I] = f[I]

    def err(self, u):
        return float(np.max(abs(np.asarray(u, LD) - self.u)))


# ---------------------------------------------------------------- the scheme with an exact inner solve
def sparse_a2(shape, coef, sigma):
    """sigma I + A2 on the interior unknowns (scipy.sparse, fp64): the 5- / 7-point operator of level 0"""
    import scipy.sparse as sp
    dim = len(shape)
    ca = ([coef[2], coef[1], coef[0]] if dim == 3 else [coef[1], coef[0]])
    m = [s - 2 for s in shape]
    A = (float(coef[3]) + float(sigma)) * sp.identity(int(np.prod(m)), format="csr")
    for a in range(dim):
        mats = [sp.diags([np.ones(m[i] - 1), np.ones(m[i] - 1)], [-1, 1]) if i == a else sp.identity(m[i]) for i in range(dim)]
        K = mats[0]
        for M_ in mats[1:]:
            K = sp.kron(K, M_, format="csr")
        A = A + float(ca[a]) * K
    return A.tocsc()


def solve_a2(lu, u_bnd, b, coef, sigma):
    """the second-order answer on the grid: (sigma I + A2) u = b inside, u = b on Dirichlet nodes"""
    I = interior(b.ndim)
    x = np.where(boundary_mask(b.shape), b, 0.0)
    cx, cy, cz, cd = coef
    ca = [cz, cy, cx] if b.ndim == 3 else [cy, cx]
    s = np.zeros_like(x[I])   # the boundary's contribution
    for a in range(b.ndim):
        lo = [slice(1, -1)] * b.ndim; hi = [slice(1, -1)] * b.ndim
        lo[a] = slice(0, -2); hi[a] = slice(2, None)
        s = s + ca[a] * (x[tuple(lo)] + x[tuple(hi)])
    x[I] = lu.solve((b[I] - s).ravel()).reshape(x[I].shape)
    return x


def defect_correction(b, coef, sigma, ncorr):
    """u = 0 inside, b on Dirichlet nodes; ncorr times: r = b - A4 u, (sigma I + A2) e = r exactly, u += e
    -> (u, [||r_k|| / ||b||], the LU of sigma I + A2)"""
    import scipy.sparse.linalg as spl
    b = np.asarray(b, np.float64)
    lu = spl.splu(sparse_a2(b.shape, coef, sigma))
    I = interior(b.ndim)
    u = np.where(boundary_mask(b.shape), b, 0.0)
    bb = sumsq(b)
    hist = []
    for k in range(ncorr + 1):
        r = residual_np(u, b, coef, sigma)
        hist.append(float(np.sqrt(sumsq(r) / bb)))
        if k == ncorr:
            break
        u[I] += lu.solve(r[I].ravel()).reshape(r[I].shape)
    return u, hist, lu
