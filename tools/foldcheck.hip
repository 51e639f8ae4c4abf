// tools/foldcheck.hip -- bit-for-bit check of the wide-tile smoothing pairs (k_pairw, mg_pair_wide.hip) against k_jacobi2
// (mg_jacobi_fast.hip, the kernel the parity suite pins to the oracle) on the smallest geometries at which every code path
// of the tile engages: both row widths, a partial last tile, even and odd plane counts, slab pieces with ghost planes and
// coarse planes addressed by global index, the two-copies launch, and -- through the process switches MG_PW_ZC / MG_PW_MODE
// set by the caller -- chunk starts on odd and even planes and tile changes inside a launch. Every case runs the product's
// launcher twice (set_pair_wide(1) / set_pair_wide(0)) on the same random arrays and compares every 32-bit word of the
// output allocation, ghost planes and padding included.
//
// build: hipcc -O3 --offload-arch=gfx950 -ffp-contract=off -std=c++17 -Iinclude tools/foldcheck.hip \
//            multigrid_prj_amd/csrc/mg_jacobi_fast.hip multigrid_prj_amd/csrc/mg_pair_wide.hip -o tools/foldcheck
// usage: foldcheck [f64-513|f64-257|f32-1025|f32-513|slab|fold]     (exit status = number of differing cases)
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../multigrid_prj_amd/csrc/mg_kernels.h"

using namespace mg;

#define CK(x)                                                                        \
    do {                                                                             \
        hipError_t e_ = (x);                                                         \
        if (e_ != hipSuccess) {                                                      \
            fprintf(stderr, "%s:%d %s\n", __FILE__, __LINE__, hipGetErrorString(e_)); \
            exit(99);                                                                \
        }                                                                            \
    } while (0)

__global__ void k_diff(const unsigned *a, const unsigned *b, size_t nwords, unsigned long long *bad)
{
    size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x, st = (size_t)gridDim.x * blockDim.x;
    unsigned long long n = 0;
    for (; i < nwords; i += st) n += a[i] != b[i];
    if (n) atomicAdd(bad, n);
}

static unsigned long long lcg = 88172645463325252ull;
static double rnd()
{
    lcg ^= lcg << 13; lcg ^= lcg >> 7; lcg ^= lcg << 17;
    return (double)(lcg >> 11) / 9007199254740992.0 - 0.5;
}

template <typename T>
struct Level {
    Geom g;
    int gh;
    size_t elems;
    T *base[4];  // u, rhs, outA, outB (allocation starts; local plane 0 is gh planes in)
    T *p(int k) const { return base[k] + (size_t)gh * g.plane; }
};

template <typename T>
static Level<T> make_level(int nx, int ny, int nz, int narr)
{
    Level<T> L{};
    Geom &g = L.g;
    g.dim = 3; g.nx = nx; g.ny = ny; g.nz = nz;
    const int line = 128 / (int)sizeof(T);
    g.pitch = ((nx + line - 1) / line) * line;
    g.plane = (long long)g.ny * g.pitch;
    g.gz0 = 0; g.gnz = nz;
    L.gh = 2;
    L.elems = (size_t)(nz + 2 * L.gh) * g.plane;
    for (int k = 0; k < narr; k++) CK(hipMalloc(&L.base[k], L.elems * sizeof(T)));
    return L;
}

template <typename T>
static void free_level(Level<T> &L, int narr)
{
    for (int k = 0; k < narr; k++) CK(hipFree(L.base[k]));
}

// random values on every node, ghost planes included; padding columns zero
template <typename T>
static void fill_random(const Level<T> &L, int k, double scale)
{
    const Geom &g = L.g;
    std::vector<T> h(L.elems, (T)0);
    for (int z = -L.gh; z < g.nz + L.gh; z++)
        for (int y = 0; y < g.ny; y++)
            for (int x = 0; x < g.nx; x++) h[(size_t)(z + L.gh) * g.plane + (size_t)y * g.pitch + x] = (T)(scale * rnd());
    CK(hipMemcpy(L.base[k], h.data(), L.elems * sizeof(T), hipMemcpyHostToDevice));
}

template <typename T>
struct Check {
    hipStream_t s;
    Level<T> F, C;
    Coef<T> c;
    unsigned long long *d_bad;
    double *d_part;
    int cases = 0, fails = 0;

    Check(int nx, int ny, int nz)
    {
        CK(hipStreamCreate(&s));
        F = make_level<T>(nx, ny, nz, 4);
        C = make_level<T>((nx + 1) / 2, (ny + 1) / 2, (nz + 1) / 2, 1);
        fill_random(F, 0, 1.0); fill_random(F, 1, 100.0); fill_random(C, 0, 0.3);
        const double h = 1.0 / (nx - 1);
        c = make_coef<T>(-1.0 / (h * h), -1.0 / (h * h), -1.0 / (h * h), 6.0 / (h * h));
        CK(hipMalloc(&d_bad, 8));
        CK(hipMalloc(&d_part, sizeof(double) * 65536));
    }
    ~Check()
    {
        CK(hipFree(d_bad)); CK(hipFree(d_part));
        free_level(F, 4); free_level(C, 1);
        CK(hipStreamDestroy(s));
    }
    // fn(wide): enqueue the launch under test writing F.p(wide ? 3 : 2)
    template <typename Fn>
    void ab(const std::string &name, Fn fn)
    {
        for (int wide = 0; wide < 2; wide++) {
            set_pair_wide(wide);
            CK(hipMemsetAsync(F.base[2 + wide], 0x5a, F.elems * sizeof(T), s));
            fn(wide);
            CK(hipStreamSynchronize(s));
            CK(hipGetLastError());
        }
        set_pair_wide(-1);
        CK(hipMemsetAsync(d_bad, 0, 8, s));
        hipLaunchKernelGGL(k_diff, dim3(1024), dim3(256), 0, s, (const unsigned *)F.base[2], (const unsigned *)F.base[3],
                           F.elems * sizeof(T) / 4, d_bad);
        unsigned long long bad = 0;
        CK(hipMemcpyAsync(&bad, d_bad, 8, hipMemcpyDeviceToHost, s));
        CK(hipStreamSynchronize(s));
        printf("%4dx%dx%d %s %-44s %s", F.g.nx, F.g.ny, F.g.nz, sizeof(T) == 8 ? "f64" : "f32", name.c_str(), bad ? "MISMATCH" : "bit-equal");
        if (bad) { printf("  (%llu differing 32-bit words)", bad); fails++; }
        printf("\n");
        fflush(stdout);
        cases++;
    }
};

static const char *om_name(int k) { return k == 0 ? "omega=6/7" : "omega=1"; }

// every variant on a whole level (fold_only: the prolongation-folding pair alone)
template <typename T>
static void whole(int nx, int ny, int nz, bool fold_only, int &cases, int &fails)
{
    Check<T> k(nx, ny, nz);
    if (!pair_wide_ok<T>(k.F.g)) { printf("%dx%dx%d: the wide tile does not take this shape\n", nx, ny, nz); fails++; }
    const Geom &g = k.F.g, &gc = k.C.g;
    auto &F = k.F; auto &C = k.C; auto s = k.s; auto c = k.c;
    for (int o = 0; o < 2; o++) {
        const T om = o == 0 ? (T)(6.0 / 7.0) : (T)1;
        const std::string on = om_name(o);
        k.ab("J(J(u+Pe)) " + on, [&](int w) { launch_jacobi2_corr<T>(s, g, gc, c, om, F.p(0), C.p(0), F.p(1), F.p(2 + w), 0); });
        if (fold_only) continue;
        k.ab("J(J(u)) " + on, [&](int w) { launch_jacobi2<T>(s, g, c, om, F.p(0), F.p(1), F.p(2 + w), false, 0); });
        k.ab("J(J(0)) " + on, [&](int w) { launch_jacobi2<T>(s, g, c, om, F.p(0), F.p(1), F.p(2 + w), true, 0); });
        k.ab("J(J(u)) + norm " + on, [&](int w) { launch_jacobi2<T>(s, g, c, om, F.p(0), F.p(1), F.p(2 + w), false, 0, k.d_part); });
        k.ab("RB(u) " + on, [&](int w) { launch_rb_fused<T>(s, g, c, F.p(0), F.p(1), F.p(2 + w), (const T *)nullptr, g, 0); });
        k.ab("RB(0) " + on, [&](int w) { launch_rb_fused<T>(s, g, c, F.p(0), F.p(1), F.p(2 + w), (const T *)nullptr, g, 0, true); });
        k.ab("RB(u) + norm " + on, [&](int w) { launch_rb_fused<T>(s, g, c, F.p(0), F.p(1), F.p(2 + w), (const T *)nullptr, g, 0, false, k.d_part); });
        k.ab("RB(u+Pe) " + on, [&](int w) { launch_rb_fused<T>(s, g, c, F.p(0), F.p(1), F.p(2 + w), C.p(0), gc, 0); });
    }
    cases += k.cases; fails += k.fails;
}

// the folding pair on the pieces of a z-slab inside a level of nzg planes: nzs planes from global plane zs (even), two ghost
// planes either side, the coarse slab = the coarse planes under it, addressed by global index
template <typename T>
static void slabs(int nx, int ny, int &cases, int &fails)
{
    const int nzg = 33, zs = 8;
    Check<T> k(nx, ny, nzg);
    auto &F = k.F; auto &C = k.C; auto s = k.s; auto c = k.c;
    const long long pl = F.g.plane;
    for (int nzs : {10, 11, 12, 13}) {
        Geom gs = F.g; gs.nz = nzs; gs.gz0 = zs;
        Geom gcs = C.g; gcs.nz = (nzs + 1) / 2; gcs.gz0 = zs / 2;
        const long long off = (long long)zs * pl, offc = (long long)(zs / 2) * C.g.plane;
        for (int o = 0; o < 2; o++) {
            const T om = o == 0 ? (T)(6.0 / 7.0) : (T)1;
            char nm[96];
            snprintf(nm, sizeof nm, "slab %d planes: whole, J(J(u+Pe)) %s", nzs, om_name(o));
            k.ab(nm, [&](int w) { launch_jacobi2_corr<T>(s, gs, gcs, c, om, F.p(0) + off, C.p(0) + offc, F.p(1) + off, F.p(2 + w) + off, 0); });
            // the interior piece engages the tile from 12 planes on (the gate wants 8); below that both runs are k_jacobi2's
            Geom gi = gs; gi.nz = nzs - 4; gi.gz0 = zs + 2;
            snprintf(nm, sizeof nm, "slab %d planes: interior, J(J(u+Pe)) %s", nzs, om_name(o));
            k.ab(nm, [&](int w) { launch_jacobi2_corr<T>(s, gi, gcs, c, om, F.p(0) + off + 2 * pl, C.p(0) + offc, F.p(1) + off + 2 * pl, F.p(2 + w) + off + 2 * pl, 0); });
            Geom glo = gs; glo.nz = 2;
            snprintf(nm, sizeof nm, "slab %d planes: boundary x2, J(J(u+Pe)) %s", nzs, om_name(o));
            k.ab(nm, [&](int w) { launch_jacobi2_corr<T>(s, glo, gcs, c, om, F.p(0) + off, C.p(0) + offc, F.p(1) + off, F.p(2 + w) + off, nzs - 2); });
        }
    }
    // two pieces of 8 planes in one launch, the second an odd / an even number of planes further up: the tile's own
    // two-copies path, with the coarse planes' parity that of the global plane, not of the local one
    for (int dup : {11, 12}) {
        const int nzs = dup + 8;
        Geom gs = F.g; gs.nz = 8; gs.gz0 = zs;
        Geom gcs = C.g; gcs.nz = (nzs + 1) / 2; gcs.gz0 = zs / 2;
        const long long off = (long long)zs * pl, offc = (long long)(zs / 2) * C.g.plane;
        for (int o = 0; o < 2; o++) {
            const T om = o == 0 ? (T)(6.0 / 7.0) : (T)1;
            char nm[96];
            snprintf(nm, sizeof nm, "slab %d planes: 8-plane pieces x2, dup %d, J(J(u+Pe)) %s", nzs, dup, om_name(o));
            k.ab(nm, [&](int w) { launch_jacobi2_corr<T>(s, gs, gcs, c, om, F.p(0) + off, C.p(0) + offc, F.p(1) + off, F.p(2 + w) + off, dup); });
        }
    }
    cases += k.cases; fails += k.fails;
}

int main(int argc, char **argv)
{
    const std::string what = argc > 1 ? argv[1] : "fold";
    int cases = 0, fails = 0;
    if (what == "f64-513") { whole<double>(513, 203, 9, false, cases, fails); whole<double>(513, 203, 23, false, cases, fails); }
    else if (what == "f64-257") whole<double>(257, 201, 9, false, cases, fails);
    else if (what == "f32-1025") whole<float>(1025, 201, 9, false, cases, fails);
    else if (what == "f32-513") whole<float>(513, 201, 9, false, cases, fails);
    else if (what == "slab") { slabs<double>(513, 203, cases, fails); slabs<double>(257, 201, cases, fails); slabs<float>(1025, 201, cases, fails); }
    else if (what == "fold") {
        // the folding pair alone on every shape: the group the caller repeats with MG_PW_ZC = 3, 4 and MG_PW_MODE = 0
        whole<double>(513, 203, 9, true, cases, fails); whole<double>(513, 203, 23, true, cases, fails);
        whole<double>(257, 201, 9, true, cases, fails);
        whole<float>(1025, 201, 9, true, cases, fails); whole<float>(513, 201, 9, true, cases, fails);
        slabs<double>(513, 203, cases, fails);
    } else { fprintf(stderr, "unknown group %s\n", what.c_str()); return 98; }
    printf("foldcheck %s: %d cases, %s\n", what.c_str(), cases, fails ? "FAILED" : "all bit-equal");
    return fails;
}
