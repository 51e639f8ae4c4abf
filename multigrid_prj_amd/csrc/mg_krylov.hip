// mg_krylov.hip -- fine-grid vector kernels of the multigrid-preconditioned flexible conjugate-gradient solver
// (mg_pcg_solve, include/mg_hip.h; driver: Solver::pcg_t in mg_solver.cpp).
//
// Per CG iteration, besides the preconditioning cycle, three streaming passes over level 0:
//   k_cg_update           x += a p,  r -= a q,  partial sums of r.r                         4 R + 2 W
//   k_cg_dots             partial sums of z.r and z.q                                        3 R
//   k_cg_direction_apply  p' = z + b p (at the point and its stencil neighbours), q = A p',
//                         partial sums of p'.q                                               2 R + 2 W
// and a one-workgroup tail after each (k_cg_tail) that adds the partials in a fixed order and turns them into the
// scalars alpha / beta / gamma on the device: nothing goes through the host between launches, and two runs give the
// same bits (no atomics).
//
// Layout: the padded level-0 arrays of mg_geom.h. A lane owns one 16-byte vector of a row (2 fp64 / 4 fp32 elements,
// rows are whole multiples of it), workgroups of 256 lanes, at most 2048 workgroups striding over the level.
// Padding columns (x >= nx) are neither written nor summed.
//
// Arithmetic contract (compiled with -ffp-contract=off, tests/test_pcg_gpu.py restates it in numpy):
//   x' = x + a*p;  r' = r - a*q                                       a = (T) alpha
//   p' = z + b*p   inside;  p' = 0 on Dirichlet nodes                 b = (T) beta
//   q  = 0 on Dirichlet nodes; inside, in the residual kernel's row order
//        ((((((0 + cz p'[k-1]) + cy p'[j-1]) + cx p'[i-1]) + cd p') + cx p'[i+1]) + cy p'[j+1]) + cz p'[k+1]
//   dots: products and sums in double.
// Zeroing p' on the boundary is what keeps the iteration on the interior whatever the preconditioner leaves there.
#include "mg_kernels.h"
#include "mg_device.h"

namespace mg {

namespace {

constexpr int CG_THREADS = 256;
constexpr int CG_MAX_BLOCKS = 2048;
constexpr int TAIL_THREADS = 1024;

template <typename T>
__device__ __forceinline__ void vload(const T *p, T (&v)[Vec16<T>::n])
{
    const typename Vec16<T>::type w = *reinterpret_cast<const typename Vec16<T>::type *>(p);
    __builtin_memcpy(v, &w, sizeof(w));
}

template <typename T>
__device__ __forceinline__ void vstore(T *p, const T (&v)[Vec16<T>::n])
{
    typename Vec16<T>::type w;
    __builtin_memcpy(&w, v, sizeof(w));
    *reinterpret_cast<typename Vec16<T>::type *>(p) = w;
}

// stores the first `valid` elements (all of them with one 16-byte store when the vector lies inside the row)
template <typename T>
__device__ __forceinline__ void vstore_masked(T *p, const T (&v)[Vec16<T>::n], int valid)
{
    constexpr int V = Vec16<T>::n;
    if (valid >= V) { vstore(p, v); return; }
#pragma unroll
    for (int e = 0; e < V; e++)
        if (e < valid) p[e] = v[e];
}

// one work item = one 16-byte vector of one row: item -> (plane, row, first x)
struct Item {
    int z, y, x0;
};
__device__ __forceinline__ Item item_of(unsigned it, unsigned vpr, unsigned ny, int V)
{
    const unsigned row = it / vpr;
    Item r;
    r.x0 = (int)(it - row * vpr) * V;
    r.y = (int)(row % ny);
    r.z = (int)(row / ny);
    return r;
}

__device__ __forceinline__ bool plane_or_row_boundary(const Geom &g, int z, int y)
{
    bool b = (y == 0) | (y == g.ny - 1);
    if (g.dim == 3) {
        const int gz = g.gz0 + z;
        b |= (gz == 0) | (gz == g.gnz - 1);
    }
    return b;
}

__device__ __forceinline__ bool cg_skip(const CgScalars *sc) { return sc->bad != 0; }

// ---------------------------------------------------------------- x += a p, r -= a q, sum r^2
template <typename T>
__global__ __launch_bounds__(CG_THREADS) void k_cg_update(Geom g, T *__restrict__ x, const T *__restrict__ p, T *__restrict__ r,
                                                          const T *__restrict__ q, const CgScalars *__restrict__ sc,
                                                          double *__restrict__ partials)
{
    constexpr int V = Vec16<T>::n;
    __shared__ double sh[CG_THREADS / 64];
    if (cg_skip(sc)) return;   // breakdown flagged by an earlier tail: x and r stay as they are
    const T a = (T)sc->alpha;
    const unsigned vpr = (unsigned)(g.pitch / V), nitems = vpr * (unsigned)g.ny * (unsigned)g.nz;
    double acc = 0.;
    for (unsigned it = blockIdx.x * CG_THREADS + threadIdx.x; it < nitems; it += gridDim.x * CG_THREADS) {
        const Item t = item_of(it, vpr, (unsigned)g.ny, V);
        const int valid = g.nx - t.x0;
        if (valid <= 0) continue;
        const long long i = (long long)t.z * g.plane + (long long)t.y * g.pitch + t.x0;
        T xv[V], pv[V], rv[V], qv[V];
        vload(x + i, xv); vload(p + i, pv); vload(r + i, rv); vload(q + i, qv);
#pragma unroll
        for (int e = 0; e < V; e++) {
            xv[e] = xv[e] + a * pv[e];
            rv[e] = rv[e] - a * qv[e];
            if (e < valid) acc += (double)rv[e] * (double)rv[e];
        }
        vstore_masked(x + i, xv, valid);
        vstore_masked(r + i, rv, valid);
    }
    const double s = block_sum(acc, sh);
    if (threadIdx.x == 0) partials[blockIdx.x] = s;
}

// ---------------------------------------------------------------- sum z.r, sum z.q
template <typename T>
__global__ __launch_bounds__(CG_THREADS) void k_cg_dots(Geom g, const T *__restrict__ z, const T *__restrict__ r,
                                                        const T *__restrict__ q, const CgScalars *__restrict__ sc,
                                                        double *__restrict__ partials)
{
    constexpr int V = Vec16<T>::n;
    __shared__ double sh[CG_THREADS / 64];
    if (cg_skip(sc)) return;
    const unsigned vpr = (unsigned)(g.pitch / V), nitems = vpr * (unsigned)g.ny * (unsigned)g.nz;
    double zr = 0., zq = 0.;
    for (unsigned it = blockIdx.x * CG_THREADS + threadIdx.x; it < nitems; it += gridDim.x * CG_THREADS) {
        const Item t = item_of(it, vpr, (unsigned)g.ny, V);
        const int valid = g.nx - t.x0;
        if (valid <= 0) continue;
        const long long i = (long long)t.z * g.plane + (long long)t.y * g.pitch + t.x0;
        T zv[V], rv[V], qv[V];
        vload(z + i, zv); vload(r + i, rv); vload(q + i, qv);
#pragma unroll
        for (int e = 0; e < V; e++)
            if (e < valid) {
                zr += (double)zv[e] * (double)rv[e];
                zq += (double)zv[e] * (double)qv[e];
            }
    }
    const double s0 = block_sum(zr, sh);
    const double s1 = block_sum(zq, sh);
    if (threadIdx.x == 0) { partials[blockIdx.x] = s0; partials[gridDim.x + blockIdx.x] = s1; }
}

// ---------------------------------------------------------------- p' = z + b p, q = A p', sum p'.q
// p' of one 16-byte vector of row (zz, yy); `mask_row`: the row lies on a Dirichlet plane / row (all zero)
template <typename T>
__device__ __forceinline__ void dir_vec(const Geom &g, const T *z, const T *p, T b, long long i, int x0, bool mask_row,
                                        T (&out)[Vec16<T>::n])
{
    constexpr int V = Vec16<T>::n;
    if (mask_row) {
#pragma unroll
        for (int e = 0; e < V; e++) out[e] = (T)0;
        return;
    }
    T zv[V], pv[V];
    vload(z + i, zv); vload(p + i, pv);
#pragma unroll
    for (int e = 0; e < V; e++) {
        const int xx = x0 + e;
        out[e] = (xx == 0 || xx >= g.nx - 1) ? (T)0 : zv[e] + b * pv[e];
    }
}

template <typename T, int DIM>
__global__ __launch_bounds__(CG_THREADS) void k_cg_direction_apply(Geom g, Coef<T> c, const T *__restrict__ z,
                                                                   const T *__restrict__ p, T *__restrict__ pn,
                                                                   T *__restrict__ q, const CgScalars *__restrict__ sc,
                                                                   double *__restrict__ partials)
{
    constexpr int V = Vec16<T>::n;
    __shared__ double sh[CG_THREADS / 64];
    if (cg_skip(sc)) return;
    const T b = (T)sc->beta;
    const unsigned vpr = (unsigned)(g.pitch / V), nitems = vpr * (unsigned)g.ny * (unsigned)g.nz;
    double acc = 0.;
    for (unsigned it = blockIdx.x * CG_THREADS + threadIdx.x; it < nitems; it += gridDim.x * CG_THREADS) {
        const Item t = item_of(it, vpr, (unsigned)g.ny, V);
        const int valid = g.nx - t.x0;
        if (valid <= 0) continue;
        const long long i = (long long)t.z * g.plane + (long long)t.y * g.pitch + t.x0;
        T pc[V], qv[V];
        if (plane_or_row_boundary(g, t.z, t.y)) {
#pragma unroll
            for (int e = 0; e < V; e++) { pc[e] = (T)0; qv[e] = (T)0; }
        } else {
            dir_vec<T>(g, z, p, b, i, t.x0, false, pc);
            T ps[V], pn_[V], pd[V], pu[V];
            dir_vec<T>(g, z, p, b, i - g.pitch, t.x0, t.y - 1 == 0, ps);
            dir_vec<T>(g, z, p, b, i + g.pitch, t.x0, t.y + 1 == g.ny - 1, pn_);
            if (DIM == 3) {
                const int gz = g.gz0 + t.z;
                dir_vec<T>(g, z, p, b, i - g.plane, t.x0, gz - 1 == 0, pd);
                dir_vec<T>(g, z, p, b, i + g.plane, t.x0, gz + 1 == g.gnz - 1, pu);
            }
            // x-neighbours across the vector's ends: one element each, zero on the Dirichlet columns
            const T pl = (t.x0 - 1 >= 1) ? z[i - 1] + b * p[i - 1] : (T)0;
            const T pr = (t.x0 + V <= g.nx - 2) ? z[i + V] + b * p[i + V] : (T)0;
#pragma unroll
            for (int e = 0; e < V; e++) {
                const int xx = t.x0 + e;
                if (xx == 0 || xx >= g.nx - 1) { qv[e] = (T)0; continue; }
                const T w = e == 0 ? pl : pc[e - 1 < 0 ? 0 : e - 1];
                const T ea = e == V - 1 ? pr : pc[e + 1 > V - 1 ? V - 1 : e + 1];
                T s = 0;
                if (DIM == 3) s += c.cz * pd[e];
                s += c.cy * ps[e];
                s += c.cx * w;
                s += c.cd * pc[e];
                s += c.cx * ea;
                s += c.cy * pn_[e];
                if (DIM == 3) s += c.cz * pu[e];
                qv[e] = s;
            }
        }
#pragma unroll
        for (int e = 0; e < V; e++)
            if (e < valid) acc += (double)pc[e] * (double)qv[e];
        vstore_masked(pn + i, pc, valid);
        vstore_masked(q + i, qv, valid);
    }
    const double s = block_sum(acc, sh);
    if (threadIdx.x == 0) partials[blockIdx.x] = s;
}

// ---------------------------------------------------------------- Dirichlet rows: x = b there
template <typename T>
__global__ __launch_bounds__(CG_THREADS) void k_cg_boundary_copy(Geom g, T *__restrict__ x, const T *__restrict__ rhs)
{
    const unsigned n = (unsigned)g.pitch * (unsigned)g.ny * (unsigned)g.nz;
    for (unsigned it = blockIdx.x * CG_THREADS + threadIdx.x; it < n; it += gridDim.x * CG_THREADS) {
        const unsigned row = it / (unsigned)g.pitch;
        const int xx = (int)(it - row * (unsigned)g.pitch), y = (int)(row % (unsigned)g.ny), zz = (int)(row / (unsigned)g.ny);
        if (xx >= g.nx) continue;
        if (plane_or_row_boundary(g, zz, y) || xx == 0 || xx == g.nx - 1) {
            const long long i = (long long)zz * g.plane + (long long)y * g.pitch + xx;
            x[i] = rhs[i];
        }
    }
}

// ---------------------------------------------------------------- fixed-order sums -> scalars (one workgroup)
__device__ __forceinline__ bool finite(double v) { return __builtin_isfinite(v); }

__global__ __launch_bounds__(TAIL_THREADS) void k_cg_tail(int mode, const double *__restrict__ partials, int nb,
                                                          CgScalars *__restrict__ sc)
{
    __shared__ double sh[TAIL_THREADS / 64];
    const int nsum = mode == CG_TAIL_BETA || mode == CG_TAIL_FIRST ? 2 : 1;
    double s[2] = {0., 0.};
    for (int k = 0; k < nsum; k++) {
        double a = 0.;
        for (int i = threadIdx.x; i < nb; i += TAIL_THREADS) a += partials[(long long)k * nb + i];
        s[k] = block_sum(a, sh);
    }
    if (threadIdx.x != 0 || sc->bad) return;
    if (mode == CG_TAIL_RR) {
        sc->rr = s[0];
        if (!finite(s[0])) sc->bad = 1;
    } else if (mode == CG_TAIL_FIRST || mode == CG_TAIL_BETA) {
        const double gamma = s[0], delta = s[1];
        const double beta = mode == CG_TAIL_FIRST ? 0.0 : -sc->alpha * delta / sc->gamma;   // Polak-Ribiere: z.(r' - r) / gamma
        if (!(gamma > 0.0) || !finite(gamma) || !finite(beta)) { sc->bad = 2; return; }
        sc->gamma = gamma; sc->delta = delta; sc->beta = beta;
    } else {   // CG_TAIL_ALPHA
        const double pq = s[0];
        const double alpha = sc->gamma / pq;
        if (!(pq > 0.0) || !finite(pq) || !finite(alpha)) { sc->bad = 3; return; }
        sc->pq = pq; sc->alpha = alpha;
    }
}

template <typename T>
int cg_grid(const Geom &g, int per_item)
{
    const long long items = (long long)(g.pitch / per_item) * g.ny * g.nz;
    return (int)std::min<long long>(CG_MAX_BLOCKS, std::max<long long>(1, (items + CG_THREADS - 1) / CG_THREADS));
}

}  // namespace

int cg_partials_capacity() { return 2 * CG_MAX_BLOCKS; }

template <typename T>
int launch_cg_update(hipStream_t s, const Geom &g, T *x, const T *p, T *r, const T *q, const CgScalars *sc, double *partials)
{
    const int nb = cg_grid<T>(g, Vec16<T>::n);
    hipLaunchKernelGGL((k_cg_update<T>), dim3(nb), dim3(CG_THREADS), 0, s, g, x, p, r, q, sc, partials);
    return nb;
}

template <typename T>
int launch_cg_dots(hipStream_t s, const Geom &g, const T *z, const T *r, const T *q, const CgScalars *sc, double *partials)
{
    const int nb = cg_grid<T>(g, Vec16<T>::n);
    hipLaunchKernelGGL((k_cg_dots<T>), dim3(nb), dim3(CG_THREADS), 0, s, g, z, r, q, sc, partials);
    return nb;
}

template <typename T>
int launch_cg_direction_apply(hipStream_t s, const Geom &g, const Coef<T> &c, const T *z, const T *p, T *pn, T *q,
                              const CgScalars *sc, double *partials)
{
    const int nb = cg_grid<T>(g, Vec16<T>::n);
    if (g.dim == 3)
        hipLaunchKernelGGL((k_cg_direction_apply<T, 3>), dim3(nb), dim3(CG_THREADS), 0, s, g, c, z, p, pn, q, sc, partials);
    else
        hipLaunchKernelGGL((k_cg_direction_apply<T, 2>), dim3(nb), dim3(CG_THREADS), 0, s, g, c, z, p, pn, q, sc, partials);
    return nb;
}

template <typename T>
void launch_cg_boundary_copy(hipStream_t s, const Geom &g, T *x, const T *rhs)
{
    hipLaunchKernelGGL((k_cg_boundary_copy<T>), dim3(cg_grid<T>(g, 1)), dim3(CG_THREADS), 0, s, g, x, rhs);
}

void launch_cg_tail(hipStream_t s, int mode, const double *partials, int nb, CgScalars *sc)
{
    hipLaunchKernelGGL(k_cg_tail, dim3(1), dim3(TAIL_THREADS), 0, s, mode, partials, nb, sc);
}

#define MG_CG_INST(T)                                                                                                      \
    template int launch_cg_update<T>(hipStream_t, const Geom &, T *, const T *, T *, const T *, const CgScalars *, double *); \
    template int launch_cg_dots<T>(hipStream_t, const Geom &, const T *, const T *, const T *, const CgScalars *, double *); \
    template int launch_cg_direction_apply<T>(hipStream_t, const Geom &, const Coef<T> &, const T *, const T *, T *, T *,  \
                                              const CgScalars *, double *);                                                \
    template void launch_cg_boundary_copy<T>(hipStream_t, const Geom &, T *, const T *);
MG_CG_INST(double)
MG_CG_INST(float)
#undef MG_CG_INST

}  // namespace mg
