// csrc/ctx_fill.hip -- the small tables of the new contexts of a part of a spectrum, in one launch (gfx950).
//
// sosgpu_create fills a context's block with one copy [mu | ga | coef | fres | rowmap] and one memset [mp_vt | mp_uf] and waits
// for both.  sosgpu_create_spectrum sends the images of all its contexts to the caller's work area in one copy, behind a job
// table, and k_ctx_fill moves each image into its context's block and clears what the memset cleared: workgroup (tile, context)
// takes 1024 16-byte pairs of its context's n_copy + n_clear doubles.  Memory-bound and small (2-140 KB per context); every
// access is one 16-byte load or store per lane, consecutive lanes at consecutive addresses.  No LDS, no barrier, no atomic.
#include "sos_common.h"
#include "kernels.h"

#define CTX_FILL_THREADS 256
#define CTX_FILL_PAIRS 4          // 16-byte pairs per thread: a workgroup covers 2048 doubles

// Bounds: pair p of context blockIdx.y is touched only for p < (n_copy + n_clear) / 2, so no index reaches past
// n_copy + n_clear doubles of dst, and the image is read only for p < n_copy / 2, so never past its n_copy doubles.  The counts
// are multiples of 32 doubles (every offset of a context's block is one): whole pairs, no tail.
__global__ __launch_bounds__(CTX_FILL_THREADS) void k_ctx_fill(const CtxFillJob *__restrict__ jobs,
                                                                const double *__restrict__ images)
{
    const CtxFillJob jb = jobs[blockIdx.y];
    const size_t n_pairs = ((size_t)jb.n_copy + jb.n_clear) >> 1, n_src = (size_t)jb.n_copy >> 1;
    const size_t first = (size_t)blockIdx.x * (CTX_FILL_THREADS * CTX_FILL_PAIRS);
    if (first >= n_pairs) return;                        // the grid takes the largest context of the call
    double2 *__restrict__ dst = reinterpret_cast<double2 *>(jb.dst);
    const double2 *__restrict__ src = reinterpret_cast<const double2 *>(images + jb.src_off);
#pragma unroll
    for (int u = 0; u < CTX_FILL_PAIRS; u++) {
        const size_t p = first + (size_t)u * CTX_FILL_THREADS + threadIdx.x;
        if (p < n_src) dst[p] = src[p];
        else if (p < n_pairs) dst[p] = make_double2(0., 0.);
    }
}

void launch_ctx_fill(const CtxFillJob *d_jobs, const double *d_images, int nctx, size_t max_doubles, hipStream_t st)
{
    const size_t per_wg = (size_t)2 * CTX_FILL_THREADS * CTX_FILL_PAIRS;
    if (nctx < 1 || max_doubles == 0) return;
    dim3 grid((unsigned)((max_doubles + per_wg - 1) / per_wg), (unsigned)nctx);
    k_ctx_fill<<<grid, CTX_FILL_THREADS, 0, st>>>(d_jobs, d_images);
}
