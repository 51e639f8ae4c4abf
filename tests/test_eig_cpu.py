"""mg_eig_solve on the CPU: the host-only dense algebra of multigrid_prj_amd/csrc/mg_dense.h through a stand-alone g++
program (no HIP), the closed-form spectrum of tests/eig_ref.py against dense eigh, and the numpy reference LOBPCG (the
CPU oracle's cycle as preconditioner) on the cases tests/test_eig_gpu.py runs on the GPU.

Iteration counts of the reference LOBPCG at tol = 1e-8 (REF_ITERS below; tests/test_eig_gpu.py allows the GPU two more):
    3d9 26, 3d33 33, 2d65 15, 3d25-degenerate 18
(m = nev on the two anisotropic 3-D cases: no guard vector, so the last column converges at the rate the gap to
lambda_5 allows)
"""
import os
import subprocess

import numpy as np
import pytest

from tests import eig_ref as er

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
CSRC = os.path.join(ROOT, "multigrid_prj_amd", "csrc")

REF_ITERS = {"3d9": 26, "3d33": 33, "2d65": 15, "3d25-degenerate": 18}
TOL = 1e-8

MAIN = r"""
#include <cstdio>
#include <vector>
#include "mg_dense.h"
// stdin: s nvec, then G (s*s), then H (s*s); stdout: status, then theta (nvec) and c (s*nvec) when status == 0
int main()
{
    int s, nvec;
    while (scanf("%d %d", &s, &nvec) == 2) {
        if (s < 1 || s > mg::DENSE_MAX) return 2;
        std::vector<double> G(s * s), H(s * s), theta(s), c(s * s);
        for (double &v : G) if (scanf("%lf", &v) != 1) return 2;
        for (double &v : H) if (scanf("%lf", &v) != 1) return 2;
        const int rc = mg::dense_rayleigh_ritz(s, nvec, G.data(), H.data(), mg::DENSE_PIVOT_MIN, theta.data(), c.data());
        printf("%d\n", rc);
        if (rc) continue;
        for (int j = 0; j < nvec; j++) printf("%.17g ", theta[j]);
        printf("\n");
        for (int i = 0; i < s * nvec; i++) printf("%.17g ", c[i]);
        printf("\n");
    }
    return 0;
}
"""


def _build(tmp, flags):
    src, exe = tmp / "dense.cpp", tmp / "dense"
    src.write_text(MAIN)
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", *flags, "-I" + CSRC, str(src), "-o", str(exe)], check=True)
    return exe


@pytest.fixture(scope="module", params=["plain", "sanitized"])
def dense(request, tmp_path_factory):
    flags = [] if request.param == "plain" else ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
    exe = _build(tmp_path_factory.mktemp("dense_" + request.param), flags)

    def run(pencils):
        """[(G, H, nvec)] -> [(status, theta, C)]"""
        text = ""
        for G, H, nvec in pencils:
            text += f"{G.shape[0]} {nvec}\n" + " ".join(repr(float(v)) for v in G.ravel()) + "\n"
            text += " ".join(repr(float(v)) for v in H.ravel()) + "\n"
        tok = subprocess.run([str(exe)], input=text, check=True, capture_output=True, text=True).stdout.split()
        out, k = [], 0
        for G, H, nvec in pencils:
            rc = int(tok[k]); k += 1
            if rc:
                out.append((rc, None, None))
                continue
            s = G.shape[0]
            theta = np.array(tok[k:k + nvec], float); k += nvec
            C = np.array(tok[k:k + s * nvec], float).reshape(s, nvec); k += s * nvec
            out.append((rc, theta, C))
        assert k == len(tok)
        return out
    return run


def spd_pencil(rng, s):
    B = rng.standard_normal((s + 3, s)) * np.exp(rng.uniform(-3, 3, s))   # badly scaled columns: the diagonal scaling matters
    G = B.T @ B
    Hs =rng.standard_normal((s + 3, s + 3))
    Hs = Hs @ Hs.T + np.diag(rng.uniform(1.0, 50.0, s + 3))
    H = B.T @ Hs @ B
    return G, 0.5 * (H + H.T)


def test_dense_rayleigh_ritz_matches_numpy(dense):
    rng = np.random.default_rng(7)
    pencils = []
    for s in range(1, 25):
        G, H = spd_pencil(rng, s)
        pencils.append((G, H, s))
        pencils.append((G, H, max(1, s // 3)))
    for (G, H, nvec), (rc, theta, C) in zip(pencils, dense(pencils)):
        assert rc == 0
        L = np.linalg.cholesky(G)
        Li = np.linalg.inv(L)
        want = np.linalg.eigvalsh(Li @ H @ Li.T)[:nvec]
        np.testing.assert_allclose(theta, want, rtol=1e-12)
        assert np.all(np.diff(theta) >= 0)
        # G-orthonormal Ritz vectors that diagonalise H
        scale = np.sqrt(np.outer(np.diag(C.T @ H @ C), np.diag(C.T @ H @ C)))
        np.testing.assert_allclose(C.T @ G @ C, np.eye(nvec), atol=1e-10)
        assert np.max(np.abs(C.T @ H @ C - np.diag(theta)) / scale) < 1e-10


def test_dense_only_upper_triangles_are_read(dense):
    rng = np.random.default_rng(8)
    G, H = spd_pencil(rng, 9)
    Gu, Hu = np.triu(G) + np.tril(np.full_like(G, np.nan), -1), np.triu(H) + np.tril(np.full_like(H, 7.0), -1)
    (rc0, t0, _), (rc1, t1, _) = dense([(G, H, 4), (Gu, Hu, 4)])
    assert rc0 == 0 and rc1 == 0
    assert np.array_equal(t0, t1)


def test_dense_rank_deficient_is_reported(dense):
    rng = np.random.default_rng(9)
    B = rng.standard_normal((30, 6))
    B[:, 4] = B[:, 1] - 2.0 * B[:, 2]                 # exactly dependent
    B2 = B.copy(); B2[:, 4] += 1e-7 * rng.standard_normal(30)   # nearly: pivot ~ 1e-14, below DENSE_PIVOT_MIN
    H = lambda M_: M_.T @ np.diag(np.arange(1.0, 31.0)) @ M_
    Gz = B.T @ B; Gz[3, 3] = 0.0
    Gn = B.T @ B; Gn[0, 2] = np.nan
    res = dense([(B.T @ B, H(B), 3), (B2.T @ B2, H(B2), 3), (Gz, H(B), 3), (Gn, H(B), 3), (np.eye(3), np.diag([3.0, 1.0, 2.0]), 2)])
    assert [r[0] for r in res] == [2, 2, 1, 1, 0]
    np.testing.assert_allclose(res[4][1], [1.0, 2.0], rtol=1e-15)


# ---------------------------------------------------------------- closed form against dense eigh
@pytest.mark.parametrize("kw", [dict(dim=3, n=9, levels=2, aniso=(1.0, 0.7, 0.3), length=1.0),
                                dict(dim=2, n=17, levels=2, length=10.0)])
def test_closed_form_matches_dense_eigh(kw):
    d = er.po.make_desc(**kw)
    coef, shape = er.po.level_coef(d, 0), er.po.level_shape(d, 0)
    A = er.dense_matrix(coef, shape)
    w, V = np.linalg.eigh(A)
    lam, idx = er.closed_form(coef, shape, len(w))
    np.testing.assert_allclose(lam, w, rtol=1e-12)
    # the dense matrix is the kernels' operator, and the sine products are its eigenvectors
    rng = np.random.default_rng(1)
    v = np.zeros(shape); v[er.interior(len(shape))] = rng.standard_normal([n - 2 for n in shape])
    np.testing.assert_allclose(er.apply_A(v, coef)[er.interior(len(shape))].ravel(), A @ v[er.interior(len(shape))].ravel(), rtol=1e-12, atol=1e-9)
    for k in (0, 1, 5):
        x = er.mode(shape, idx[k])
        np.testing.assert_allclose(er.apply_A(x, coef), lam[k] * x, atol=1e-10 * abs(lam[k]))


# ---------------------------------------------------------------- the reference LOBPCG
@pytest.mark.parametrize("name", list(er.SOLVE_CASES))
def test_reference_lobpcg_converges(name):
    kw, m, nev = er.SOLVE_CASES[name]
    d = er.po.make_desc(**kw)
    coef, shape = er.po.level_coef(d, 0), er.po.level_shape(d, 0)
    M, S = er.oracle_preconditioner(kw)
    out = er.lobpcg(coef, er.start_vectors(shape, m), nev, TOL, 80, M)
    S.close()
    print(name, "iters", out["iters"], "cycles", out["cycles"], "restarts", out["restarts"], "hist", out["hist"])
    assert out["status"] == 0
    assert abs(out["iters"] - REF_ITERS[name]) <= 1   # numpy's own eigh / cholesky may round differently from build to build
    exact, _ = er.closed_form(coef, shape, m)
    assert np.all(np.abs(out["lam"][:nev] - exact[:nev]) <= 2 * TOL * np.abs(exact[:nev]))
    assert np.all(out["relres"][:nev] <= 1.01 * TOL)
    if name == "3d25-degenerate":
        assert out["cycles"] < out["iters"] * m   # soft locking saves preconditioner applications
        np.testing.assert_allclose(exact[1], exact[3], rtol=1e-13)
