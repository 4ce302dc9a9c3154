// What the two resampling kernels (fit.hip, restore.hip) share: a row of a tap table, and the launchers' rows-per-workgroup hint.
#pragma once
#include "drn_common.h"

struct Taps {
    int lo, n;
};

// a row of a table, forced into [0, n_in): n in 1..K, lo in 0..n_in - n (valid tables pass unchanged; n_in >= 1)
__device__ __forceinline__ Taps taps_of(const int* __restrict__ lo_n, int i, int K, int n_in) {
    Taps t;
    t.n = min(max(lo_n[2 * i + 1], 1), min(K, n_in));
    t.lo = min(max(lo_n[2 * i], 0), n_in - t.n);
    return t;
}

// rows per workgroup: what a down-scale of about (K - 1) / 2 source rows per output row lets into a stage of `stage_rows` source
// rows, `cap` at most.  A hint only: the kernels cut their rows into chunks that fit, whatever the tables hold
inline int resample_tile_rows(int K, int stage_rows, int cap) {
    const double step = K > 3 ? 0.5 * (K - 1) : 1.0;
    const int tile_h = (int)((stage_rows - K) / step) + 1;
    return tile_h < 1 ? 1 : (tile_h > cap ? cap : tile_h);
}
