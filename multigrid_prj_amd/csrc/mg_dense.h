// mg_dense.h -- the small dense algebra of mg_eig_solve's Rayleigh-Ritz step, on the host in fp64: Cholesky, triangular
// solves, a cyclic Jacobi eigensolver and the reduced generalised eigenproblem H c = theta G c built from them. Host only:
// no HIP include, usable from a plain g++ program (tests/test_eig_cpu.py builds one), like mg_geom.h.
// Matrices are dense, row-major, n <= DENSE_MAX = 24 (three blocks of MG_EIG_MAX_BLOCK columns).
#ifndef MG_DENSE_H
#define MG_DENSE_H

#include <cmath>

namespace mg {

constexpr int DENSE_MAX = 24;
// Smallest pivot (the squared diagonal entry of the Cholesky factor) accepted for a basis Gram matrix scaled to a unit
// diagonal. Such a pivot is the squared distance of the basis vector from the span of the ones before it, so 1e-10 means
// an angle of 1e-5: below it the reduced pencil L^-1 H L^-T loses more than ten of its sixteen digits and the basis is
// not "safely positive definite" (mg_eig_solve then drops the P block and counts a restart).
constexpr double DENSE_PIVOT_MIN = 1e-10;

enum DenseStatus {
    DENSE_OK = 0,
    DENSE_NOT_FINITE = 1,   // an entry of G or H is not finite, or a diagonal entry of G is not positive
    DENSE_RANK = 2,         // a Cholesky pivot of the scaled G is below pivot_min (rank-deficient or nearly so)
    DENSE_NO_CONVERGENCE = 3
};

// A = L L^T in place (lower triangle of a <- L; the strict upper triangle is left alone). Returns the index of the first
// pivot that is not > pivot_min (nothing beyond that column is valid), or -1 when the factorisation went through.
inline int dense_cholesky(int n, double *a, int ld, double pivot_min)
{
    for (int k = 0; k < n; k++) {
        double v = a[k * ld + k];
        for (int j = 0; j < k; j++) v -= a[k * ld + j] * a[k * ld + j];
        if (!(v > pivot_min) || !std::isfinite(v)) return k;
        const double d = std::sqrt(v);
        a[k * ld + k] = d;
        for (int i = k + 1; i < n; i++) {
            double s = a[i * ld + k];
            for (int j = 0; j < k; j++) s -= a[i * ld + j] * a[k * ld + j];
            a[i * ld + k] = s / d;
        }
    }
    return -1;
}

// B <- L^-1 B (forward substitution on the nrhs columns of the n x nrhs matrix b)
inline void dense_solve_lower(int n, const double *l, int ldl, double *b, int ldb, int nrhs)
{
    for (int c = 0; c < nrhs; c++)
        for (int i = 0; i < n; i++) {
            double s = b[i * ldb + c];
            for (int j = 0; j < i; j++) s -= l[i * ldl + j] * b[j * ldb + c];
            b[i * ldb + c] = s / l[i * ldl + i];
        }
}

// B <- L^-T B (back substitution)
inline void dense_solve_lower_t(int n, const double *l, int ldl, double *b, int ldb, int nrhs)
{
    for (int c = 0; c < nrhs; c++)
        for (int i = n - 1; i >= 0; i--) {
            double s = b[i * ldb + c];
            for (int j = i + 1; j < n; j++) s -= l[j * ldl + i] * b[j * ldb + c];
            b[i * ldb + c] = s / l[i * ldl + i];
        }
}

// Cyclic Jacobi on the symmetric n x n matrix a (destroyed: its diagonal ends as the eigenvalues): a = V diag(w) V^T,
// eigenvalues ascending in w, eigenvectors in the COLUMNS of v. Rotations in row-cyclic order, until the off-diagonal
// mass is below 1e-30 of the diagonal's (or nothing is left to rotate); at most 60 sweeps. Returns the sweeps used, -1
// when they did not suffice.
inline int dense_jacobi_eig(int n, double *a, int ld, double *v, int ldv, double *w)
{
    for (int i = 0; i < n; i++)
        for (int j = 0; j < n; j++) v[i * ldv + j] = i == j ? 1.0 : 0.0;
    int sweeps = -1;
    for (int sweep = 0; sweep < 60; sweep++) {
        double off = 0, diag = 0;
        for (int i = 0; i < n; i++) {
            diag += a[i * ld + i] * a[i * ld + i];
            for (int j = i + 1; j < n; j++) off += a[i * ld + j] * a[i * ld + j];
        }
        if (!(off > 1e-30 * diag)) { sweeps = sweep; break; }
        for (int p = 0; p < n - 1; p++)
            for (int q = p + 1; q < n; q++) {
                const double apq = a[p * ld + q];
                if (apq == 0.0) continue;
                const double tau = (a[q * ld + q] - a[p * ld + p]) / (2.0 * apq);
                const double t = (tau >= 0 ? 1.0 : -1.0) / (std::fabs(tau) + std::sqrt(1.0 + tau * tau));
                const double c = 1.0 / std::sqrt(1.0 + t * t), s = t * c;
                for (int k = 0; k < n; k++) {   // columns p, q
                    const double akp = a[k * ld + p], akq = a[k * ld + q];
                    a[k * ld + p] = c * akp - s * akq;
                    a[k * ld + q] = s * akp + c * akq;
                }
                for (int k = 0; k < n; k++) {   // rows p, q
                    const double apk = a[p * ld + k], aqk = a[q * ld + k];
                    a[p * ld + k] = c * apk - s * aqk;
                    a[q * ld + k] = s * apk + c * aqk;
                }
                for (int k = 0; k < n; k++) {
                    const double vkp = v[k * ldv + p], vkq = v[k * ldv + q];
                    v[k * ldv + p] = c * vkp - s * vkq;
                    v[k * ldv + q] = s * vkp + c * vkq;
                }
            }
    }
    if (sweeps < 0) return -1;
    for (int i = 0; i < n; i++) w[i] = a[i * ld + i];
    for (int i = 0; i < n - 1; i++) {   // selection sort, ascending; columns of v follow
        int k = i;
        for (int j = i + 1; j < n; j++)
            if (w[j] < w[k]) k = j;
        if (k != i) {
            const double t = w[i]; w[i] = w[k]; w[k] = t;
            for (int r = 0; r < n; r++) { const double u = v[r * ldv + i]; v[r * ldv + i] = v[r * ldv + k]; v[r * ldv + k] = u; }
        }
    }
    return sweeps;
}

// The Rayleigh-Ritz step on a basis S of s vectors with G = S^T S, H = S^T A S (s x s, row-major, only the UPPER
// triangles are read): the nvec smallest eigenpairs of H c = theta G c. G and H are scaled by diag(G)^-1/2 on both sides,
// the scaled G is factored L L^T (pivots above pivot_min), L^-1 H L^-T goes to the Jacobi eigensolver, and
// c = D L^-T q. On DENSE_OK: theta[0 .. nvec) ascending and c (s x nvec, row-major) with c^T G c = I.
inline int dense_rayleigh_ritz(int s, int nvec, const double *G, const double *H, double pivot_min, double *theta, double *c)
{
    if (s < 1 || s > DENSE_MAX || nvec < 1 || nvec > s) return DENSE_NOT_FINITE;
    double d[DENSE_MAX], l[DENSE_MAX * DENSE_MAX], a[DENSE_MAX * DENSE_MAX], q[DENSE_MAX * DENSE_MAX], w[DENSE_MAX];
    for (int i = 0; i < s; i++) {
        const double g = G[i * s + i];
        if (!std::isfinite(g) || !(g > 0.0)) return DENSE_NOT_FINITE;
        d[i] = 1.0 / std::sqrt(g);
    }
    for (int i = 0; i < s; i++)
        for (int j = i; j < s; j++) {
            if (!std::isfinite(G[i * s + j]) || !std::isfinite(H[i * s + j])) return DENSE_NOT_FINITE;
            l[j * s + i] = l[i * s + j] = d[i] * G[i * s + j] * d[j];
            a[j * s + i] = a[i * s + j] = d[i] * H[i * s + j] * d[j];
        }
    if (dense_cholesky(s, l, s, pivot_min) >= 0) return DENSE_RANK;
    dense_solve_lower(s, l, s, a, s, s);                       // a <- L^-1 a
    for (int i = 0; i < s; i++)                                // a <- a^T, then L^-1 again: L^-1 a L^-T
        for (int j = i + 1; j < s; j++) { const double t = a[i * s + j]; a[i * s + j] = a[j * s + i]; a[j * s + i] = t; }
    dense_solve_lower(s, l, s, a, s, s);
    for (int i = 0; i < s; i++)                                // symmetrise what rounding left
        for (int j = i + 1; j < s; j++) a[i * s + j] = a[j * s + i] = 0.5 * (a[i * s + j] + a[j * s + i]);
    if (dense_jacobi_eig(s, a, s, q, s, w) < 0) return DENSE_NO_CONVERGENCE;
    dense_solve_lower_t(s, l, s, q, s, s);                     // q <- L^-T q (all columns; the first nvec are kept)
    for (int j = 0; j < nvec; j++) {
        theta[j] = w[j];
        for (int i = 0; i < s; i++) c[i * nvec + j] = d[i] * q[i * s + j];
    }
    return DENSE_OK;
}

}  // namespace mg
#endif
