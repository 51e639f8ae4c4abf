// mg_io.hip -- a level-shaped array <-> a dense device array of the caller (mg_*_device, include/mg_hip.h; driver:
// Solver::device_copy in mg_solver.cpp). One streaming pass: the dense array is read or written once, and so is the padded
// one. The two layouts differ in the row pitch (padded rows start on 128-byte lines, dense rows follow each other) and
// possibly in the element type (fp64 <-> fp32), so a row's elements sit at different 16-byte phases on the two sides --
// and on the dense side at EVERY phase: a row of 513 doubles is 4104 bytes, consecutive rows start 8 bytes further into
// their 16-byte word, and the base may be a slice of a larger buffer. Only element alignment is assumed there.
//
//  * A row is "row R" on both sides: dense element R * nx, padded element R * pitch (plane = ny * pitch), R < ny * nz. A
//    workgroup takes a CHUNK of whole rows, at most IO_CAP dense elements: ONE contiguous dense span. (Rows longer than
//    IO_CAP are cut into column segments of IO_CAP elements -- a multiple of the 128-byte line in both types -- one row per
//    chunk; the span is then that segment.)
//  * Dense side: the span rounded OUT to 16-byte words is loaded with 16-byte accesses (every word holds at least one byte
//    of the array, none lies wholly outside it); for stores only the words that lie wholly INSIDE the span are written
//    that way, and the ragged head and tail (fewer than 16 bytes each) element by element: no byte next to the array is
//    written, it belongs to somebody else's tensor.
//  * Padded side: one lane owns one aligned 16-byte vector of a row (Vec16), over the whole pitch: the padding columns are
//    written as the zeros they hold, like the host path does.
//  * The re-alignment between the two runs through LDS: an image of the span at the dense side's 16-byte phase, filled
//    and drained with 16-byte accesses on one side and element accesses (ds_read/write_b32/b64) on the other.
//  * Nothing is reused: non-temporal loads and stores. The grid is capped (IO_MAX_GRID) and strides over the chunks.
//
// Conversion is the C++ cast per element: double -> float rounds to nearest even (overflow: +-inf, NaN stays NaN),
// float -> double is exact; with equal types the value is only moved, every bit pattern survives.
// Instantiations: padded type x dense type x direction.
#include "mg_kernels.h"
#include "mg_device.h"

#include <algorithm>
#include <cstdint>

namespace mg {
namespace {

constexpr int IO_NT = 256;          // threads per workgroup
constexpr int IO_CAP = 4096;        // dense elements per chunk: 32 KiB of LDS in fp64 (4 workgroups per CU), 16 KiB in fp32
constexpr int IO_MAX_GRID = 2048;
constexpr int IO_U = 4;             // 16-byte global loads a lane keeps in flight

typedef unsigned int word16 __attribute__((ext_vector_type(4)));   // one 16-byte word of the dense side, moved as bits

struct IoPlan {
    int nx, pitch;      // elements per dense / padded row
    int rows;           // ny * nz
    int rpc;            // rows per chunk
    int segw, nseg;     // columns per chunk (a multiple of 32; >= pitch when rows are not cut) and segments per row
    int nchunks;
};

template <typename P, typename D, bool TO_PADDED>
__global__ __launch_bounds__(IO_NT) void k_io_copy(IoPlan pl, P *__restrict__ padded, D *__restrict__ dense)
{
    constexpr int VP = Vec16<P>::n;
    typedef typename Vec16<P>::type vecp;
    __shared__ word16 img[IO_CAP * sizeof(D) / 16 + 2];   // the span at the dense side's phase: up to 15 bytes before and after it
    const int tid = threadIdx.x;

    for (int ch = blockIdx.x; ch < pl.nchunks; ch += gridDim.x) {
        const int rc = ch / pl.nseg, sg = ch - rc * pl.nseg;
        const int r0 = rc * pl.rpc, nr = min(pl.rpc, pl.rows - r0);
        const int c0 = sg * pl.segw;                         // first column of the chunk (0 unless rows are cut)
        const int ncol = min(pl.segw, pl.nx - c0);           // dense columns of a row of the chunk (nx unless rows are cut)
        const int pcol = min(pl.segw, pl.pitch - c0);        // padded columns: a multiple of 32
        const int nel = (nr - 1) * pl.nx + ncol;             // dense elements of the span (nr > 1 only with whole rows)
        const uintptr_t b0 = (uintptr_t)(dense + ((size_t)r0 * pl.nx + c0)), b1 = b0 + (size_t)nel * sizeof(D);
        const uintptr_t a0 = b0 & ~(uintptr_t)15, a1 = (b1 + 15) & ~(uintptr_t)15;
        const int nw = (int)((a1 - a0) >> 4);                // <= IO_CAP * sizeof(D) / 16 + 2
        D *const el = reinterpret_cast<D *>(reinterpret_cast<char *>(img) + (b0 - a0));   // element 0 of the span in the image
        P *const prow = padded + (size_t)r0 * pl.pitch + c0;
        const int vpr = pcol / VP, nvec = nr * vpr;

        if (TO_PADDED) {
            // IO_U loads in flight per lane before the first of them is waited for
            for (int w = tid; w < nw; w += IO_U * IO_NT) {
                word16 q[IO_U];
#pragma unroll
                for (int k = 0; k < IO_U; k++)
                    if (w + k * IO_NT < nw) q[k] = __builtin_nontemporal_load(reinterpret_cast<const word16 *>(a0) + w + k * IO_NT);
#pragma unroll
                for (int k = 0; k < IO_U; k++)
                    if (w + k * IO_NT < nw) img[w + k * IO_NT] = q[k];
            }
            __syncthreads();
            for (int t = tid; t < nvec; t += IO_NT) {
                const int r = t / vpr, x = (t - r * vpr) * VP;
                const D *const src = el + r * pl.nx + x;
                vecp v;
#pragma unroll
                for (int e = 0; e < VP; e++) v[e] = (x + e < ncol) ? (P)src[e] : (P)0;
                __builtin_nontemporal_store(v, reinterpret_cast<vecp *>(prow + (size_t)r * pl.pitch + x));
            }
        } else {
            for (int t0 = tid; t0 < nvec; t0 += IO_U * IO_NT) {
                vecp v[IO_U];
                int r[IO_U], x[IO_U];
#pragma unroll
                for (int k = 0; k < IO_U; k++) {
                    const int t = t0 + k * IO_NT;
                    r[k] = t / vpr; x[k] = (t - r[k] * vpr) * VP;
                    if (t < nvec) v[k] = __builtin_nontemporal_load(reinterpret_cast<const vecp *>(prow + (size_t)r[k] * pl.pitch + x[k]));
                }
#pragma unroll
                for (int k = 0; k < IO_U; k++) {
                    if (t0 + k * IO_NT >= nvec) continue;
                    D *const dst = el + r[k] * pl.nx + x[k];
#pragma unroll
                    for (int e = 0; e < VP; e++)
                        if (x[k] + e < ncol) dst[e] = (D)v[k][e];
                }
            }
            __syncthreads();
            // words wholly inside the span; the head [b0, he) and the tail [ts, b1) element by element
            const int w0 = (b0 == a0) ? 0 : 1, w1 = (b1 == a1) ? nw : nw - 1;
            for (int w = w0 + tid; w < w1; w += IO_NT) __builtin_nontemporal_store(img[w], reinterpret_cast<word16 *>(a0) + w);
            const uintptr_t he = (b0 == a0) ? b0 : min(b1, a0 + 16);
            const uintptr_t ts = (b1 == a1) ? b1 : max(a1 - 16, he);
            const int nh = (int)((he - b0) / sizeof(D)), nt = (int)((b1 - ts) / sizeof(D));
            if (tid < nh) reinterpret_cast<D *>(b0)[tid] = el[tid];
            else if (tid - nh < nt) reinterpret_cast<D *>(ts)[tid - nh] = el[(ts - b0) / sizeof(D) + (tid - nh)];
        }
        __syncthreads();   // the image is refilled by the next chunk
    }
}

}  // namespace

template <typename P, typename D>
void launch_io_copy(hipStream_t s, const Geom &g, P *padded, D *dense, bool to_padded)
{
    IoPlan pl;
    pl.nx = g.nx; pl.pitch = g.pitch;
    pl.rows = g.ny * g.nz;
    if (g.nx <= IO_CAP) { pl.rpc = std::min(IO_CAP / g.nx, pl.rows); pl.segw = ((g.pitch + 31) / 32) * 32; pl.nseg = 1; }
    else { pl.rpc = 1; pl.segw = IO_CAP; pl.nseg = (g.nx + IO_CAP - 1) / IO_CAP; }
    pl.nchunks = ((pl.rows + pl.rpc - 1) / pl.rpc) * pl.nseg;
    const dim3 gr(std::min(pl.nchunks, IO_MAX_GRID)), bl(IO_NT);
    if (to_padded) hipLaunchKernelGGL((k_io_copy<P, D, true>), gr, bl, 0, s, pl, padded, dense);
    else hipLaunchKernelGGL((k_io_copy<P, D, false>), gr, bl, 0, s, pl, padded, dense);
}

template void launch_io_copy<double, double>(hipStream_t, const Geom &, double *, double *, bool);
template void launch_io_copy<double, float>(hipStream_t, const Geom &, double *, float *, bool);
template void launch_io_copy<float, double>(hipStream_t, const Geom &, float *, double *, bool);
template void launch_io_copy<float, float>(hipStream_t, const Geom &, float *, float *, bool);

}  // namespace mg
