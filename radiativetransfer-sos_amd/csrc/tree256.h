// csrc/tree256.h -- the fixed-shape tree over the 256 per-thread partials of a workgroup, shared by the band sums of
// aggregate.hip (k_aggregate_scal, k_level_transmission) and albedo.hip (k_albedo_band), so that equal terms give equal bits.
// sm[256][NC] holds the partials (written, then __syncthreads() by the caller); columns in MAXMASK combine with MAX, the
// others with +.  The result is sm[0][.].  Include it inside the file's `fp contract(off)` region.
#pragma once

template <int NC, unsigned MAXMASK>
__device__ __forceinline__ void tree256(double (*sm)[NC], const int t)
{
    for (int st = 128; st > 0; st >>= 1) {
        if (t < st)
            for (int i = 0; i < NC; i++)
                sm[t][i] = ((MAXMASK >> i) & 1u) ? fmax(sm[t][i], sm[t + st][i]) : sm[t][i] + sm[t + st][i];
        __syncthreads();
    }
}
