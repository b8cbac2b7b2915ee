// The body of k_pixels_sweep<PASS> and of k_pixels_sweep_tiles<PASS> (csrc/kernels_pixels.hpp), included inside either
// kernel -- not a header of its own: the text is shared, so that the untiled kernels keep, instruction for instruction,
// the code they had before the tiled ones existed (a device function called from both does not leave them so).  In scope:
// PASS, `constexpr bool TILED`, `PixSweep p`, `PixTiles t`, `PixStep st` (TILED = false: never read).
//
// The walk of one workgroup over rows [r_lo, r_hi) x columns [c_lo, c_hi) of its plane.  TILED = false: the whole plane of
// blockIdx.z.  TILED = true: blockIdx.z = plane * n_tiles + tile, the bounds are the tile's -- its origin (ty sy, tx sx), the
// step of the window grid (the tile shape itself for disjoint tiles) -- uniform over the workgroup, and the sums go to the
// tile's own block [n_rot][n_dy][n_dx][3].
    __shared__ double lds_a[kPixTile];
    constexpr bool RESID = PASS >= kPixR0;
    __shared__ double lds_b[(RESID ? 2 : 1) * kPixLdsB];  // residus passes: the roots of the box pixels behind them
    __shared__ double lds_red[kPixThreads / 64][3 * kPixG];
    const int tid = threadIdx.x;
    const PixGroup g = p.groups[blockIdx.x];
    const int jy = blockIdx.y, kr = TILED ? (int)blockIdx.z / t.n_tiles : blockIdx.z;
    const int row_off = p.lag_dy[jy] - p.min_dy;  // box row of the window's first row
    const int col_off = g.dx_min - p.min_dx;      // box column of the group's first window's first column
    const int tile = TILED ? (int)blockIdx.z - kr * t.n_tiles : 0;
    const long long lag0 = (((long long)tile * (TILED ? t.n_rot : 0) + kr) * p.n_dy + jy) * p.n_dx + g.first;
    const int ty = TILED ? tile / t.n_tx : 0, tx = TILED ? tile - ty * t.n_tx : 0;
    const int r_lo = TILED ? ty * st.sy : 0, r_hi = TILED ? min(p.h, r_lo + t.th) : p.h;
    const int c_lo = TILED ? tx * st.sx : 0, c_hi = TILED ? min(p.w, c_lo + t.tw) : p.w;
    const double* plane = p.planes + (size_t)kr * p.w * p.h;

    int off[kPixG];
    double ma[kPixG], mb[kPixG];
#pragma unroll
    for (int s = 0; s < kPixG; ++s) {
        const bool used = s < g.count;
        off[s] = used ? p.lag_dx[g.first + s] - g.dx_min : 0;
        ma[s] = mb[s] = 0.0;
        if (PASS == 1 && used) {
            const double* s0 = p.sums0 + 3 * (lag0 + s);
            ma[s] = s0[1] / s0[0];
            mb[s] = s0[2] / s0[0];
        }
        if (PASS == kPixR1 && used) {
            const double* s0 = p.sums0 + 3 * (lag0 + s);
            ma[s] = s0[1] / s0[0];  // mean of the finite terms
        }
    }
    double acc0[kPixG], acc1[kPixG], acc2[kPixG];
#pragma unroll
    for (int s = 0; s < kPixG; ++s) acc0[s] = acc1[s] = acc2[s] = 0.0;

    for (int r0 = r_lo; r0 < r_hi; r0 += p.bh) {
        const int nr = min(p.bh, r_hi - r0);
        for (int c0 = c_lo; c0 < c_hi; c0 += p.cw) {
            const int nc = min(p.cw, c_hi - c0);
            const int ncb = nc + kPixG - 1;
            __syncthreads();  // the previous band has been read
            for (int q = tid; q < nr * nc; q += kPixThreads) {
                const int r = q / nc, c = q - r * nc;
                lds_a[q] = plane[(size_t)(r0 + r) * p.w + c0 + c];
            }
            for (int q = tid; q < nr * ncb; q += kPixThreads) {
                const int r = q / ncb, c = q - r * ncb;
                const int bc = col_off + c0 + c;  // (columns past the box belong to unused slots only)
                if (!RESID) {
                    lds_b[q] = bc < p.bW ? p.box[(size_t)(row_off + r0 + r) * p.bW + bc] : 0.0;
                } else {
                    // a pixel that is not finite, and a column past the box, is staged as NaN: never kept, never poisoned
                    double b = bc < p.bW ? p.box[(size_t)(row_off + r0 + r) * p.bW + bc] : __builtin_nan("");
                    if (!(fabs(b) < __builtin_inf())) b = __builtin_nan("");
                    lds_b[q] = b;
                    lds_b[kPixLdsB + q] = sqrt(b);
                }
            }
            __syncthreads();
            for (int q = tid; q < nr * nc; q += kPixThreads) {
                const int r = q / nc, c = q - r * nc;
                const double a = lds_a[q];
                const double* brow = lds_b + r * ncb + c;
                const bool a_ok = RESID ? fabs(a) < __builtin_inf() : a == a;
#pragma unroll
                for (int s = 0; s < kPixG; ++s) {
                    const double b = brow[off[s]];
                    const bool keep = a_ok & (b == b);
                    if (PASS == 0) {
                        acc0[s] += keep ? 1.0 : 0.0;
                        acc1[s] += keep ? a : 0.0;
                        acc2[s] += keep ? b : 0.0;
                    } else if (PASS == 1) {
                        const double da = a - ma[s], db = b - mb[s];
                        acc0[s] += keep ? da * db : 0.0;
                        acc1[s] += keep ? da * da : 0.0;
                        acc2[s] += keep ? db * db : 0.0;
                    } else {
                        // IEEE division by the staged root; a kept term is finite unless b <= 0
                        const double d = (b - a) / brow[kPixLdsB + off[s]];
                        const bool fin = keep & (fabs(d) < __builtin_inf());
                        if (PASS == kPixR0) {
                            acc0[s] += fin ? 1.0 : 0.0;
                            acc1[s] += fin ? d : 0.0;
                            acc2[s] += (keep & !fin) ? 1.0 : 0.0;
                        } else {
                            const double dd = d - ma[s];
                            acc0[s] += fin ? dd * dd : 0.0;
                        }
                    }
                }
            }
        }
    }
    // lanes of a wave, then the four waves in a fixed order
    const int lane = tid & 63, wave = tid >> 6;
#pragma unroll
    for (int s = 0; s < kPixG; ++s) {
        double v0 = acc0[s], v1 = acc1[s], v2 = acc2[s];
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) {
            v0 += __shfl_down(v0, d, 64);
            v1 += __shfl_down(v1, d, 64);
            v2 += __shfl_down(v2, d, 64);
        }
        if (lane == 0) {
            lds_red[wave][3 * s + 0] = v0;
            lds_red[wave][3 * s + 1] = v1;
            lds_red[wave][3 * s + 2] = v2;
        }
    }
    __syncthreads();
    if (tid < 3 * g.count) {
        double v = lds_red[0][tid];
#pragma unroll
        for (int k = 1; k < kPixThreads / 64; ++k) v += lds_red[k][tid];
        p.sums[3 * lag0 + tid] = v;
    }
