// mg_subcycle.hip -- the whole multigrid recursion below a ROOT level in one launch, gfx950 (extension: the W- and F-cycles).
//
// A W-cycle visits level l about 2^l times, so nearly all of its level visits fall on grids of a few thousand points, where a
// visit costs five or six launches of a few microseconds each and next to no arithmetic. Those levels fit one CU's LDS
// together (mg::subcycle_plan, mg_geom.h), so ONE workgroup of 1024 threads runs cyc(root, kind) -- and the second visit of
// the root its parent would make -- out of LDS: it reads RHS(root) (and U(root) unless the guess is zero) once, writes
// U(root) and one CoarseOut once. The levels below the root never touch HBM.
//
// Arithmetic: the generic per-point expressions and one-workgroup passes of mg_device.h on dense LDS geometries (pitch = nx),
// so the result has the bits of the launch-by-launch path (tests/test_cycle_kinds_gpu.py compares them). The coarsest solve
// is the loop of k_coarse_solve_lds. Sums of squares: per-thread accumulation in double, block_sum_bcast -- no atomics.
//
// Control flow: the recursion is unrolled into a loop over (level, direction) with the kind of every level's current visit
// and its "second visit begun" flag packed in two integers. Every branch is decided from kernel arguments or from a
// broadcast block sum (the tolerance test of the coarsest solve), values all 1024 threads hold alike: every barrier is
// reached by every thread.
#include "mg_kernels.h"
#include "mg_device.h"

#include <atomic>

namespace mg {

namespace {

enum { KIND_V = 1, KIND_W = 2, KIND_F = 3 };   // enum mg_cycle_kind

// dense geometry of resident level k
template <typename T, int DIM>
__device__ __forceinline__ Geom sub_geom(const SubcycleArgs<T> &a, int k)
{
    Geom g;
    g.dim = DIM;
    g.nx = a.nx[k]; g.ny = a.ny[k]; g.nz = a.nz[k];
    g.pitch = g.nx;
    g.plane = (long long)g.nx * g.ny;
    g.gz0 = 0;
    g.gnz = g.nz;
    return g;
}

// `sweeps` smoothing sweeps of level geometry g on (u, b); Jacobi writes out of place into t and the two change roles
template <typename T, int DIM>
__device__ __forceinline__ void sub_smooth(const Geom &g, const Coef<T> &c, T omega, int smoother, int sweeps, T *&u, T *&t, const T *b)
{
    const bool damped = (omega != (T)1);
    for (int s = 0; s < sweeps; s++) {
        if (smoother == 1) {
            if (damped) wg_jacobi<T, DIM, true>(g, c, omega, u, b, t);
            else wg_jacobi<T, DIM, false>(g, c, omega, u, b, t);
            T *x = u; u = t; t = x;
        } else {
            wg_rbgs<T, DIM>(g, c, u, b);
        }
    }
}

template <typename T, int DIM>
__global__ __launch_bounds__(SWG) void k_subcycle(SubcycleArgs<T> a)
{
    extern __shared__ __align__(16) unsigned char smem[];
    double *sh = reinterpret_cast<double *>(smem);   // SUBCYCLE_SCRATCH bytes: block_sum_bcast's 18 doubles
    const int K = a.nres;
    auto arr = [&](int k, int which) -> T * { return reinterpret_cast<T *>(smem + a.off[k][which]); };
    unsigned swapped = 0;   // bit k: U of level k lives in the level's t array (an odd number of Jacobi sweeps so far)
    auto U = [&](int k) -> T * { return arr(k, (swapped >> k) & 1u ? 1 : 0); };
    auto TT = [&](int k) -> T * { return arr(k, (swapped >> k) & 1u ? 0 : 1); };

    // ---- RHS(root), U(root) -> LDS
    {
        const Geom g = sub_geom<T, DIM>(a, 0);
        const int npl = g.nx * g.ny, total = npl * g.nz;
        T *su = arr(0, 0), *sb = arr(0, 2);
        for (int q = threadIdx.x; q < total; q += SWG) {
            const int z = q / npl, rem = q - z * npl, y = rem / g.nx, x = rem - y * g.nx;
            const long long gi = lidx(a.groot, z, y, x);
            sb[q] = a.rhs[gi];
            su[q] = a.u_zero ? (T)0 : a.u[gi];
        }
        __syncthreads();
    }

    // kinds[2k+1 : 2k]: kind of the visit level k is in; parent_kind: what the root's parent runs (V: no second visit)
    unsigned kinds = (unsigned)a.kind;
    const int parent_kind = a.second ? a.kind : (int)KIND_V;
    unsigned second = 0;    // bit k: the second visit of level k (within its parent's current visit) has begun
    auto kind_of = [&](int k) -> int { return (int)((kinds >> (2 * k)) & 3u); };
    auto set_kind = [&](int k, int v) { kinds = (kinds & ~(3u << (2 * k))) | ((unsigned)v << (2 * k)); };

    int iters = 0, flag = 0;
    double nb = 0., nr = 0.;
    int k = 0;
    bool down = true;
    for (;;) {
        const Geom g = sub_geom<T, DIM>(a, k);
        const Coef<T> c = a.c[k];
        const int npl = g.nx * g.ny, total = npl * g.nz;
        if (down && k == K - 1) {
            // ---- coarsest grid: Solver::Solve as k_coarse_solve_lds runs it, from the zero guess its parent stored
            T *u = U(k), *t = TT(k);
            const T *b = arr(k, 2);
            nb = wg_sumsq<T>(g, b, sh);
            if (a.fixed) {
                sub_smooth<T, DIM>(g, c, a.omega, a.smoother, a.maxit, u, t, b);
                iters += a.maxit;
                nr = wg_residual_sumsq<T, DIM>(g, c, u, b, sh);
            } else {
                int counter = a.maxit;
                nr = wg_residual_sumsq<T, DIM>(g, c, u, b, sh);
                while (sqrt(nr / nb) > a.tol) {   // the broadcast sums: the same decision in every thread
                    if (counter > 0) {
                        sub_smooth<T, DIM>(g, c, a.omega, a.smoother, 1, u, t, b);
                        counter -= 1;
                        iters++;
                        nr = wg_residual_sumsq<T, DIM>(g, c, u, b, sh);
                    } else {
                        flag = 1;
                        break;
                    }
                }
            }
            if (u != arr(k, 0)) swapped |= 1u << k; else swapped &= ~(1u << k);
            down = false;
            k--;
            continue;
        }
        if (down) {
            // ---- nu_pre sweeps, residual, restriction, zero guess below
            T *u = U(k), *t = TT(k);
            const T *b = arr(k, 2);
            sub_smooth<T, DIM>(g, c, a.omega, a.smoother, a.nu_pre, u, t, b);
            if (u != arr(k, 0)) swapped |= 1u << k; else swapped &= ~(1u << k);
            for (int q = threadIdx.x; q < total; q += SWG) {
                const int z = q / npl, rem = q - z * npl, y = rem / g.nx, x = rem - y * g.nx;
                T sum;
                if (on_boundary(g, z, y, x)) sum = (T)1 * u[q];
                else sum = full_sum<T, DIM>(u, q, g.pitch, g.plane, c);
                t[q] = b[q] - sum;
            }
            __syncthreads();
            const Geom gc = sub_geom<T, DIM>(a, k + 1);
            const int cnpl = gc.nx * gc.ny, ctotal = cnpl * gc.nz;
            swapped &= ~(1u << (k + 1));
            T *cu = arr(k + 1, 0), *cb = arr(k + 1, 2);
            for (int q = threadIdx.x; q < ctotal; q += SWG) {
                const int z = q / cnpl, rem = q - z * cnpl, y = rem / gc.nx, x = rem - y * gc.nx;
                T v;
                if (a.restriction == 1) v = restrict_fw_point<T, DIM, DIM == 3>(g, gc, t, z, y, x);
                else v = t[lidx(g, DIM == 3 ? 2 * z : 0, 2 * y, 2 * x)];
                cb[q] = v;
                cu[q] = (T)0;
            }
            __syncthreads();
            set_kind(k + 1, kind_of(k));
            second &= ~(1u << (k + 1));
            k++;
            continue;
        }
        // ---- level k + 1 has finished a visit
        const int mine = kind_of(k);
        if (k + 1 < K - 1 && !((second >> (k + 1)) & 1u) && mine != KIND_V) {
            second |= 1u << (k + 1);
            set_kind(k + 1, mine == KIND_W ? KIND_W : KIND_V);
            k++;
            down = true;
            continue;
        }
        {
            // ---- U(k) += P U(k + 1), nu_post sweeps
            const Geom gc = sub_geom<T, DIM>(a, k + 1);
            T *u = U(k), *t = TT(k);
            const T *b = arr(k, 2);
            const T *cu = U(k + 1);
            for (int q = threadIdx.x; q < total; q += SWG) {
                const int z = q / npl, rem = q - z * npl, y = rem / g.nx, x = rem - y * g.nx;
                const T v = prolong_point<T, DIM>(gc, g, cu, z, y, x);
                u[q] += v;
            }
            __syncthreads();
            sub_smooth<T, DIM>(g, c, a.omega, a.smoother, a.nu_post, u, t, b);
            if (u != arr(k, 0)) swapped |= 1u << k; else swapped &= ~(1u << k);
        }
        if (k == 0) {
            if (!(second & 1u) && parent_kind != KIND_V) {   // the second visit the root's parent makes
                second |= 1u;
                set_kind(0, parent_kind == KIND_W ? KIND_W : KIND_V);
                down = true;
                continue;
            }
            break;
        }
        k--;
    }

    // ---- U(root) -> HBM, the statistics of the coarse solves
    {
        const Geom g = sub_geom<T, DIM>(a, 0);
        const int npl = g.nx * g.ny, total = npl * g.nz;
        const T *su = U(0);
        for (int q = threadIdx.x; q < total; q += SWG) {
            const int z = q / npl, rem = q - z * npl, y = rem / g.nx, x = rem - y * g.nx;
            a.u[lidx(a.groot, z, y, x)] = su[q];
        }
    }
    if (threadIdx.x == 0) {
        a.out->iters = iters;
        a.out->flag = flag;
        a.out->relres = sqrt(nr / nb);
        a.out->sumsq_rhs = nb;
        a.out->sumsq_r = nr;
    }
}

// acc += cur the way mg_cycle_stats reports a W / F cycle: iterations summed, flags or-ed, the norms of the last solve
__global__ void k_coarse_accum(CoarseOut *acc, const CoarseOut *cur)
{
    if (threadIdx.x == 0 && blockIdx.x == 0) {
        acc->iters += cur->iters;
        acc->flag |= cur->flag;
        acc->relres = cur->relres;
        acc->sumsq_rhs = cur->sumsq_rhs;
        acc->sumsq_r = cur->sumsq_r;
    }
}

// LDS above the default limit needs the attribute once per kernel and device; `done` has one bit per device id
template <typename K>
bool subcycle_lds_attr(K kern, std::atomic<unsigned long long> &done)
{
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) return false;
    const unsigned long long bit = 1ull << (dev & 63);
    if (done.load(std::memory_order_acquire) & bit) return true;
    if (hipFuncSetAttribute(reinterpret_cast<const void *>(kern), hipFuncAttributeMaxDynamicSharedMemorySize,
                            (int)COARSE_LDS_MAX) != hipSuccess) return false;
    done.fetch_or(bit, std::memory_order_release);   // setting it twice from two threads is harmless
    return true;
}

template <typename T, int DIM>
bool launch_subcycle_dim(hipStream_t s, const SubcycleArgs<T> &a, size_t lds_bytes)
{
    auto kern = k_subcycle<T, DIM>;
    static std::atomic<unsigned long long> done{0};   // per instantiation
    if (!subcycle_lds_attr(kern, done)) return false;
    hipLaunchKernelGGL(kern, dim3(1), dim3(SWG), lds_bytes, s, a);
    return true;
}

}  // namespace

template <typename T>
bool launch_subcycle(hipStream_t s, const SubcycleArgs<T> &a, int dim, size_t lds_bytes)
{
    if (a.nres < 2 || a.nres > SUBCYCLE_MAX_LEVELS || lds_bytes > (size_t)COARSE_LDS_MAX) return false;
    return dim == 3 ? launch_subcycle_dim<T, 3>(s, a, lds_bytes) : launch_subcycle_dim<T, 2>(s, a, lds_bytes);
}

void launch_coarse_accum(hipStream_t s, CoarseOut *acc, const CoarseOut *cur)
{
    hipLaunchKernelGGL(k_coarse_accum, dim3(1), dim3(64), 0, s, acc, cur);
}

template bool launch_subcycle<double>(hipStream_t, const SubcycleArgs<double> &, int, size_t);
template bool launch_subcycle<float>(hipStream_t, const SubcycleArgs<float> &, int, size_t);

}  // namespace mg
