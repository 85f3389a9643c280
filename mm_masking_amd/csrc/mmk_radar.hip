// Radar image operators of the hot path on gfx950 (HBM-bound byte/float streaming):
// GO-CFAR, blob-centre extraction with stable compaction, polar -> Cartesian bilinear
// resampling, bilinear weight gather / scatter-add, BEV rasterisation.
// Semantics: /root/reference/mm_masking/radar_utils.py (line numbers per kernel);
// CPU restatement: oracle/radar_ref.py; golden vectors: tests/golden/radar_*.npz.
#include <math.h>

#include "mmk_common.h"

namespace {

constexpr int RT = 256;  // threads per block for the row kernels

// Block-wide exclusive scan of one double per thread (RT threads); returns the exclusive
// prefix of `v`, *total gets the block sum.  `sm` holds RT/64 doubles.
template <int NTHR = RT>
__device__ __forceinline__ double block_excl_scan(double v, double *sm, double *total)
{
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    double inc = v;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        double o = __shfl_up(inc, off, 64);
        if (lane >= off) inc += o;
    }
    if (lane == 63) sm[wv] = inc;
    __syncthreads();
    double base = 0.0, tot = 0.0;
#pragma unroll
    for (int w = 0; w < NTHR / 64; ++w) {
        if (w < wv) base += sm[w];
        tot += sm[w];
    }
    __syncthreads();
    *total = tot;
    return base + inc - v;
}

__device__ __forceinline__ int block_excl_scan_i(int v, int *sm, int *total)
{
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    int inc = v;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        int o = __shfl_up(inc, off, 64);
        if (lane >= off) inc += o;
    }
    if (lane == 63) sm[wv] = inc;
    __syncthreads();
    int base = 0, tot = 0;
#pragma unroll
    for (int w = 0; w < RT / 64; ++w) {
        if (w < wv) base += sm[w];
        tot += sm[w];
    }
    __syncthreads();
    *total = tot;
    return base + inc - v;
}

// ------------------------------------------------------------------------------------------
// R2 cfar_mask (radar_utils.py:29-69).  One block per azimuth row: the row is staged in
// LDS, an fp64 prefix sum gives every 50-cell window sum exactly rounded to fp32, and the
// mask row is written back coalesced: one read + one write of the image.
// (CFAR_T = 512 threads per row: the 40 KB row buffer admits four blocks per CU, and with 256 threads each that was 16 waves per
// CU in a launch that is load -> scan -> compute -> store latency from end to end; 32 waves hide twice as much of it)
constexpr int CFAR_T = 512;

// The two thresholds of radar_utils.py:56, by value (one pair for the launch) or read from device memory (one pair for the
// batch, stride 0, or one per scan, stride 1; scan = row / A).  Both forms hand the same two floats to the same expression
// a_th * stat + b_th, so equal values give equal bits.
struct CfarThVal {
    static constexpr bool per_row = false, params = false;
    float a, b;
    __device__ __forceinline__ int scan_of(int) const { return 0; }
    __device__ __forceinline__ float a_of(int) const { return a; }
    __device__ __forceinline__ float b_of(int) const { return b; }
};
struct CfarThPtr {
    static constexpr bool per_row = true, params = true;
    const float *a, *b;
    int stride, A;
    double *part;                                                   // backward only: one (sum k stat, sum k) pair per row
    __device__ __forceinline__ int scan_of(int row) const { return row / A; }
    __device__ __forceinline__ float a_of(int scan) const { return a[scan * stride]; }
    __device__ __forceinline__ float b_of(int scan) const { return b[scan * stride]; }
};

template <class TH>
__global__ __launch_bounds__(CFAR_T) void cfar_mask_kernel(const float *__restrict__ raw, int R, int w2, int guard,
                                                       int mincol, int maxcol, TH thr, int diff,
                                                       float steep, float *__restrict__ mask)
{
    const float a_th = thr.a_of(blockIdx.y), b_th = thr.b_of(blockIdx.y);
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    double *cs = reinterpret_cast<double *>(smem);                 // R + 1
    float *row = reinterpret_cast<float *>(cs + (R + 1));          // R
    __shared__ double wsum[CFAR_T / 64];
    const size_t base = ((size_t)blockIdx.y * gridDim.x + blockIdx.x) * R;
    // (16-byte loads / stores were tried in round 4: no change, 107 -> 112 us -- the kernel is bound by the latency of one row per
    // block at four blocks per CU (40 KB of LDS each), not by the width of its accesses)
    for (int c = threadIdx.x; c < R; c += CFAR_T) row[c] = raw[base + c];
    __syncthreads();
    const int L = (R + CFAR_T - 1) / CFAR_T;
    const int c0 = min(R, (int)threadIdx.x * L), c1 = min(R, c0 + L);
    double s = 0.0;
    for (int c = c0; c < c1; ++c) s += (double)row[c];
    double tot;
    double run = block_excl_scan<CFAR_T>(s, wsum, &tot);
    for (int c = c0; c < c1; ++c) {
        cs[c] = run;
        run += (double)row[c];
    }
    if (threadIdx.x == CFAR_T - 1) cs[R] = tot;
    __syncthreads();
    auto cell = [&](int c) -> float {
        float th = 1000.0f;
        if (c >= mincol && c < maxcol) {
            const float left = (float)(cs[c - guard] - cs[c - w2 - guard]);
            const float right = (float)(cs[min(R, c + w2 + guard + 1)] - cs[min(R, c + guard + 1)]);
            const float stat = fmaxf(left, right) / (float)w2;
            th = a_th * stat + b_th;
        }
        const float x = row[c];
        float m;
        if (diff) {
            m = 0.5f * tanhf(steep * (x - th) + 2.5f) + 0.5f;
            m = (fabsf(m) > 0.99f) ? m : 0.0f;
        } else {
            m = (x > th) ? 1.0f : 0.0f;
        }
        return m;
    };
    for (int c = threadIdx.x; c < R; c += CFAR_T) mask[base + c] = cell(c);
}

// The same, persistent (round 5): a block walks rows blockIdx.x, + gridDim.x, ... and holds the NEXT row in registers while it
// scans / thresholds / stores the current one from LDS, so that no row's HBM latency is exposed (the one-row-per-block form is a
// load -> scan -> compute -> store latency chain end to end, at four rows in flight per CU).  Same thread -> cell partition and
// the same fp64 sums as cfar_mask_kernel: bit-identical masks.  NPRE >= ceil(R / CFAR_T).
template <int NPRE, class TH>
__global__ __launch_bounds__(CFAR_T) void cfar_mask_rows_kernel(const float *__restrict__ raw, int rows, int R, int w2, int guard,
                                                                int mincol, int maxcol, TH thr, int diff,
                                                                float steep, float *__restrict__ mask)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    double *cs = reinterpret_cast<double *>(smem);                 // R + 1
    float *row = reinterpret_cast<float *>(cs + (R + 1));          // R
    __shared__ double wsum[CFAR_T / 64];
    float nx[NPRE];
    int r = blockIdx.x;
    if (r >= rows) return;
    auto fetch = [&](int rr) {
        const float *src = raw + (size_t)rr * R;
#pragma unroll
        for (int i = 0; i < NPRE; ++i) {
            const int c = threadIdx.x + i * CFAR_T;
            nx[i] = src[c < R ? c : R - 1];
        }
    };
    auto stage = [&]() {
#pragma unroll
        for (int i = 0; i < NPRE; ++i) {
            const int c = threadIdx.x + i * CFAR_T;
            if (c < R) row[c] = nx[i];
        }
    };
    fetch(r);
    stage();
    __syncthreads();
    const int L = (R + CFAR_T - 1) / CFAR_T;
    const int c0 = min(R, (int)threadIdx.x * L), c1 = min(R, c0 + L);
    float a_th = thr.a_of(thr.scan_of(r)), b_th = thr.b_of(thr.scan_of(r));
    while (true) {
        const int rn = r + gridDim.x;
        fetch(rn < rows ? rn : r);                                  // (unconditional: past the last row the current one again)
        double s = 0.0;
        for (int c = c0; c < c1; ++c) s += (double)row[c];
        double tot;
        double run = block_excl_scan<CFAR_T>(s, wsum, &tot);
        for (int c = c0; c < c1; ++c) {
            cs[c] = run;
            run += (double)row[c];
        }
        if (threadIdx.x == CFAR_T - 1) cs[R] = tot;
        __syncthreads();
        float *out = mask + (size_t)r * R;
        for (int c = threadIdx.x; c < R; c += CFAR_T) {
            float th = 1000.0f;
            if (c >= mincol && c < maxcol) {
                const float left = (float)(cs[c - guard] - cs[c - w2 - guard]);
                const float right = (float)(cs[min(R, c + w2 + guard + 1)] - cs[min(R, c + guard + 1)]);
                const float stat = fmaxf(left, right) / (float)w2;
                th = a_th * stat + b_th;
            }
            const float x = row[c];
            float m;
            if (diff) {
                m = 0.5f * tanhf(steep * (x - th) + 2.5f) + 0.5f;
                m = (fabsf(m) > 0.99f) ? m : 0.0f;
            } else {
                m = (x > th) ? 1.0f : 0.0f;
            }
            out[c] = m;
        }
        if (rn >= rows) break;
        __syncthreads();                                            // everyone is done with this row's LDS image
        stage();
        __syncthreads();
        r = rn;
        if (TH::per_row) {
            a_th = thr.a_of(thr.scan_of(r));
            b_th = thr.b_of(thr.scan_of(r));
        }
    }
}

// ------------------------------------------------------------------------------------------
// R3 + R4: mean_peaks_parallel_fast (radar_utils.py:167-185) + extract_pc (:71-106).
__device__ __forceinline__ float peak_value(const float *__restrict__ mrow, int j, int R, float res, int diff,
                                            float steep)
{
    // marker stored at column j (< R-1): arr[j]*z[j+1] + arr[j+1]*z[j]
    const float a0 = (res * (float)j) * mrow[j];
    const float a1 = (res * (float)(j + 1)) * mrow[j + 1];
    float z0, z1;
    if (diff) {
        z0 = 1.0f - tanhf(steep * a0);
        z1 = 1.0f - tanhf(steep * a1);
    } else {
        z0 = (a0 == 0.0f) ? 1.0f : 0.0f;
        z1 = (a1 == 0.0f) ? 1.0f : 0.0f;
    }
    return a0 * z1 + a1 * z0;
}

// (both row kernels stage the mask row in LDS with 16-byte loads -- every cell is needed twice, as mrow[j] and mrow[j + 1] --
// instead of two dword loads per cell)
__device__ __forceinline__ const float *stage_row(const float *__restrict__ grow, int R, float *lrow)
{
    if ((R & 3) == 0 && ((uintptr_t)grow & 15) == 0) {
        for (int c = threadIdx.x * 4; c < R; c += RT * 4) *reinterpret_cast<float4 *>(lrow + c) = *reinterpret_cast<const float4 *>(grow + c);
    } else {
        for (int c = threadIdx.x; c < R; c += RT) lrow[c] = grow[c];
    }
    __syncthreads();
    return lrow;
}

__global__ __launch_bounds__(RT) void peaks_count_kernel(const float *__restrict__ mask, int R, float res, int diff,
                                                         float steep, int32_t *__restrict__ row_count)
{
    extern __shared__ __attribute__((aligned(16))) float lrow_dyn[];
    __shared__ int sm[RT / 64];
    const int rowid = blockIdx.y * gridDim.x + blockIdx.x;
    const float *mrow = stage_row(mask + (size_t)rowid * R, R, lrow_dyn);
    int cnt = 0;
    for (int j = threadIdx.x; j < R - 1; j += RT) cnt += (peak_value(mrow, j, R, res, diff, steep) != 0.0f) ? 1 : 0;
    int tot;
    block_excl_scan_i(cnt, sm, &tot);
    if (threadIdx.x == 0) row_count[rowid] = tot;
}

__global__ __launch_bounds__(RT) void peaks_scan_kernel(const int32_t *__restrict__ row_count, int A,
                                                        int32_t *__restrict__ row_off, int32_t *__restrict__ total)
{
    __shared__ int sm[RT / 64];
    const int b = blockIdx.x;
    const int L = (A + RT - 1) / RT;
    const int a0 = min(A, (int)threadIdx.x * L), a1 = min(A, a0 + L);
    int s = 0;
    for (int a = a0; a < a1; ++a) s += row_count[b * A + a];
    int tot;
    int run = block_excl_scan_i(s, sm, &tot);
    for (int a = a0; a < a1; ++a) {
        row_off[b * A + a] = run;
        run += row_count[b * A + a];
    }
    if (threadIdx.x == 0) total[b] = tot;
}

__global__ __launch_bounds__(RT) void peaks_emit_kernel(const float *__restrict__ mask, int R, float res, int diff,
                                                        float steep, const int32_t *__restrict__ row_off, int cap,
                                                        float *__restrict__ mval, int32_t *__restrict__ mrow_out)
{
    extern __shared__ __attribute__((aligned(16))) float lrow_dyn[];
    __shared__ int sm[RT / 64];
    const int a = blockIdx.x, b = blockIdx.y, A = gridDim.x;
    const int rowid = b * A + a;
    const float *mrow = stage_row(mask + (size_t)rowid * R, R, lrow_dyn);
    // A thread owns a run of consecutive cells: ONE block scan of the runs' marker counts places every marker (the markers
    // of a row keep their column order: run t precedes run t + 1) -- instead of a block scan (two barriers) per 256 cells,
    // thirteen per row of 3 360, in a launch that is latency from end to end.
    const int L = (R - 1 + RT - 1) / RT;
    const int j0 = min(R - 1, (int)threadIdx.x * L), j1 = min(R - 1, j0 + L);
    int cnt = 0;
    for (int j = j0; j < j1; ++j) cnt += (peak_value(mrow, j, R, res, diff, steep) != 0.0f) ? 1 : 0;
    int tot;
    int g = row_off[rowid] + block_excl_scan_i(cnt, sm, &tot);
    if (cnt != 0) {
        for (int j = j0; j < j1; ++j) {
            const float v = peak_value(mrow, j, R, res, diff, steep);
            if (v != 0.0f) {
                if (g < cap) {
                    mval[(size_t)b * cap + g] = v;
                    mrow_out[(size_t)b * cap + g] = a;
                }
                ++g;
            }
        }
    }
}

__global__ void peaks_pair_kernel(const float *__restrict__ mval, const int32_t *__restrict__ mrow, int cap,
                                  const int32_t *__restrict__ total, const float *__restrict__ az,
                                  const float *__restrict__ T_ab, int A, int max_pts, float *__restrict__ out_pc,
                                  int32_t *__restrict__ out_count)
{
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    const int b = blockIdx.y;
    const int npts = total[b] / 2;
    if (k == 0) out_count[b] = npts;
    if (k >= max_pts) return;
    float x = 0.f, y = 0.f, z = 0.f;
    if (k < npts && 2 * k + 1 < cap) {
        const size_t m = (size_t)b * cap + 2 * k;
        const float rho = (mval[m + 1] + mval[m]) / 2.0f;
        const float phi = (az[b * A + mrow[m + 1]] + az[b * A + mrow[m]]) / 2.0f;
        x = rho * cosf(phi);
        y = rho * sinf(phi);
        if (T_ab) {
            const float *T = T_ab + (size_t)b * 16;
            const float xx = ((T[0] * x + T[1] * y) + T[2] * z) + T[3];
            const float yy = ((T[4] * x + T[5] * y) + T[6] * z) + T[7];
            const float zz = ((T[8] * x + T[9] * y) + T[10] * z) + T[11];
            x = xx; y = yy; z = zz;
        }
    }
    float *o = out_pc + ((size_t)b * max_pts + k) * 3;
    o[0] = x; o[1] = y; o[2] = z;
}

// The third column of the pair mean (radar_utils.py:97): the time of point k is the mean of its two markers' azimuth times, one
// fp32 add and an exact halving; padding rows get 0.  peaks_pair_kernel's grid and its rule for which rows hold a point.
__global__ void peaks_time_kernel(const int32_t *__restrict__ mrow, int cap, const int32_t *__restrict__ total,
                                  const float *__restrict__ times, int A, int max_pts, float *__restrict__ out_time)
{
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    const int b = blockIdx.y;
    if (k >= max_pts) return;
    const int npts = total[b] / 2;
    float tv = 0.f;
    if (k < npts && 2 * k + 1 < cap) {
        const size_t m = (size_t)b * cap + 2 * k;
        tv = (times[b * A + mrow[m + 1]] + times[b * A + mrow[m]]) / 2.0f;
    }
    out_time[(size_t)b * max_pts + k] = tv;
}

// ------------------------------------------------------------------------------------------
// D1: constant-twist motion compensation, p' = Exp(s (v; omega)) p per point in fp64, one rounding per output.
//   w = s omega, u = s v, th2 = w.w,  a1 = w x p, a2 = w x a1, b1 = w x u, b2 = w x b1
//   p' = p + A a1 + B a2 + u + B b1 + C b2
// and its reverse, written out by hand (c = x cross y: x_bar += y cross c_bar, y_bar += c_bar cross x).
struct D3 {
    double x, y, z;
};
__device__ __forceinline__ D3 cross3(const D3 &a, const D3 &b) { return {a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x}; }
__device__ __forceinline__ double dot3(const D3 &a, const D3 &b) { return (a.x * b.x + a.y * b.y) + a.z * b.z; }
__device__ __forceinline__ D3 scale3(double s, const D3 &a) { return {s * a.x, s * a.y, s * a.z}; }
__device__ __forceinline__ D3 add3(const D3 &a, const D3 &b) { return {a.x + b.x, a.y + b.y, a.z + b.z}; }

constexpr double DESKEW_SERIES_CUT = 1e-4;   // th2 below it: the Taylor series to th^6
constexpr int DESKEW_T = 256;

// A = sin th / th, B = (1 - cos th) / th2, C = (th - sin th) / th^3 and, when WITH_D, their derivatives in th2.
template <bool WITH_D>
__device__ __forceinline__ void deskew_coef(double th2, double &A, double &B, double &C, double &dA, double &dB, double &dC)
{
    if (th2 < DESKEW_SERIES_CUT) {
        const double th4 = th2 * th2, th6 = th4 * th2;
        A = ((1.0 - th2 / 6.0) + th4 / 120.0) - th6 / 5040.0;
        B = ((0.5 - th2 / 24.0) + th4 / 720.0) - th6 / 40320.0;
        C = ((1.0 / 6.0 - th2 / 120.0) + th4 / 5040.0) - th6 / 362880.0;
        if (WITH_D) {
            dA = (-1.0 / 6.0 + th2 / 60.0) - th4 / 1680.0;
            dB = (-1.0 / 24.0 + th2 / 360.0) - th4 / 13440.0;
            dC = (-1.0 / 120.0 + th2 / 2520.0) - th4 / 120960.0;
        }
    } else {
        const double th = sqrt(th2), s = sin(th), c = cos(th);
        A = s / th;
        B = (1.0 - c) / th2;
        C = (th - s) / (th2 * th);
        if (WITH_D) {
            dA = (C - B) * 0.5;                  // (th cos th - sin th) / (2 th^3)
            dB = (A - 2.0 * B) / (2.0 * th2);
            dC = (B - 3.0 * C) / (2.0 * th2);
        }
    }
}

__global__ __launch_bounds__(DESKEW_T) void deskew_points_kernel(const float *__restrict__ pc, const float *__restrict__ t,
                                                                 const float *__restrict__ twist, int N,
                                                                 float *__restrict__ out)
{
    const int i = blockIdx.x * DESKEW_T + threadIdx.x;
    const int b = blockIdx.y;
    if (i >= N) return;
    const float *tw = twist + (size_t)b * 6;                        // a block-uniform address
    const size_t r = (size_t)b * N + i;
    const float fx = pc[r * 3], fy = pc[r * 3 + 1], fz = pc[r * 3 + 2];
    float *o = out + r * 3;
    if (fx == 0.f && fy == 0.f && fz == 0.f) {                      // a padding row stays one
        o[0] = 0.f; o[1] = 0.f; o[2] = 0.f;
        return;
    }
    const double s = (double)t[r];
    const D3 p = {(double)fx, (double)fy, (double)fz};
    const D3 u = {s * (double)tw[0], s * (double)tw[1], s * (double)tw[2]};
    const D3 w = {s * (double)tw[3], s * (double)tw[4], s * (double)tw[5]};
    double A, B, C, d0, d1, d2;
    deskew_coef<false>(dot3(w, w), A, B, C, d0, d1, d2);
    const D3 a1 = cross3(w, p), a2 = cross3(w, a1), b1 = cross3(w, u), b2 = cross3(w, b1);
    o[0] = (float)(((((p.x + A * a1.x) + B * a2.x) + u.x) + B * b1.x) + C * b2.x);
    o[1] = (float)(((((p.y + A * a1.y) + B * a2.y) + u.y) + B * b1.y) + C * b2.y);
    o[2] = (float)(((((p.z + A * a1.z) + B * a2.z) + u.z) + B * b1.z) + C * b2.z);
}

// One point per thread; gpc (may be NULL) = R^T g, and the point's share s (u_bar; w_bar) of the twist's gradient goes
// thread -> wave64 shuffle -> LDS -> one fp64 partial per block (part (B,nblk,6), every entry written; NULL: not asked for).
__global__ __launch_bounds__(DESKEW_T) void deskew_points_bwd_kernel(const float *__restrict__ pc, const float *__restrict__ t,
                                                                     const float *__restrict__ twist, int N,
                                                                     const float *__restrict__ gout, float *__restrict__ gpc,
                                                                     double *__restrict__ part)
{
    __shared__ double sm[DESKEW_T / 64][6];
    const int i = blockIdx.x * DESKEW_T + threadIdx.x;
    const int b = blockIdx.y;
    double c0 = 0.0, c1 = 0.0, c2 = 0.0, c3 = 0.0, c4 = 0.0, c5 = 0.0;
    if (i < N) {
        const float *tw = twist + (size_t)b * 6;
        const size_t r = (size_t)b * N + i;
        const float fx = pc[r * 3], fy = pc[r * 3 + 1], fz = pc[r * 3 + 2];
        D3 pb = {0.0, 0.0, 0.0};
        if (!(fx == 0.f && fy == 0.f && fz == 0.f)) {
            const double s = (double)t[r];
            const D3 p = {(double)fx, (double)fy, (double)fz};
            const D3 g = {(double)gout[r * 3], (double)gout[r * 3 + 1], (double)gout[r * 3 + 2]};
            const D3 u = {s * (double)tw[0], s * (double)tw[1], s * (double)tw[2]};
            const D3 w = {s * (double)tw[3], s * (double)tw[4], s * (double)tw[5]};
            double A, B, C, dA, dB, dC;
            deskew_coef<true>(dot3(w, w), A, B, C, dA, dB, dC);
            const D3 a1 = cross3(w, p), a2 = cross3(w, a1), b1 = cross3(w, u), b2 = cross3(w, b1);
            const double Ab = dot3(g, a1), Bb = dot3(g, a2) + dot3(g, b1), Cb = dot3(g, b2);
            const D3 b2b = scale3(C, g);
            const D3 b1b = add3(scale3(B, g), cross3(b2b, w));
            const D3 ub = add3(g, cross3(b1b, w));
            const D3 a2b = scale3(B, g);
            const D3 a1b = add3(scale3(A, g), cross3(a2b, w));
            D3 wb = add3(cross3(b1, b2b), cross3(u, b1b));
            wb = add3(wb, add3(cross3(a1, a2b), cross3(p, a1b)));
            wb = add3(wb, scale3(2.0 * ((dA * Ab + dB * Bb) + dC * Cb), w));
            pb = add3(g, cross3(a1b, w));
            c0 = s * ub.x; c1 = s * ub.y; c2 = s * ub.z;
            c3 = s * wb.x; c4 = s * wb.y; c5 = s * wb.z;
        }
        if (gpc) {
            gpc[r * 3] = (float)pb.x; gpc[r * 3 + 1] = (float)pb.y; gpc[r * 3 + 2] = (float)pb.z;
        }
    }
    if (part == nullptr) return;                                    // (the same for every thread of the launch)
    c0 = wave_sum(c0); c1 = wave_sum(c1); c2 = wave_sum(c2);
    c3 = wave_sum(c3); c4 = wave_sum(c4); c5 = wave_sum(c5);
    if ((threadIdx.x & 63) == 0) {
        double *row = sm[threadIdx.x >> 6];
        row[0] = c0; row[1] = c1; row[2] = c2; row[3] = c3; row[4] = c4; row[5] = c5;
    }
    __syncthreads();
    if (threadIdx.x < 6) {
        double acc = sm[0][threadIdx.x];
        for (int wv = 1; wv < DESKEW_T / 64; ++wv) acc += sm[wv][threadIdx.x];
        part[((size_t)b * gridDim.x + blockIdx.x) * 6 + threadIdx.x] = acc;
    }
}

// One wave per item: lane l adds the partials of blocks l, l + 64, ... in index order, the fixed shuffle tree adds the
// lanes, and the sum is rounded once to fp32.
__global__ __launch_bounds__(64) void deskew_twist_sum_kernel(const double *__restrict__ part, int nblk,
                                                              float *__restrict__ grad_twist)
{
    const int b = blockIdx.x;
    double c0 = 0.0, c1 = 0.0, c2 = 0.0, c3 = 0.0, c4 = 0.0, c5 = 0.0;
    for (int r = threadIdx.x; r < nblk; r += 64) {
        const double *row = part + ((size_t)b * nblk + r) * 6;
        c0 += row[0]; c1 += row[1]; c2 += row[2]; c3 += row[3]; c4 += row[4]; c5 += row[5];
    }
    c0 = wave_sum(c0); c1 = wave_sum(c1); c2 = wave_sum(c2);
    c3 = wave_sum(c3); c4 = wave_sum(c4); c5 = wave_sum(c5);
    if (threadIdx.x == 0) {
        float *o = grad_twist + (size_t)b * 6;
        o[0] = (float)c0; o[1] = (float)c1; o[2] = (float)c2; o[3] = (float)c3; o[4] = (float)c4; o[5] = (float)c5;
    }
}

// ------------------------------------------------------------------------------------------
// Bilinear tap fetch with zero padding; `rows` > H means the image is wrap-padded by one
// row at both ends (interpolate_crossover, radar_utils.py:317-319) without materialising it.
__device__ __forceinline__ float tap_polar(const float *__restrict__ img, int A, int R, int yi, int xi, int wrap)
{
    const int rows = wrap ? A + 2 : A;
    if (xi < 0 || xi >= R || yi < 0 || yi >= rows) return 0.0f;
    int r = yi;
    if (wrap) r = (yi == 0) ? (A - 1) : ((yi == A + 1) ? 0 : yi - 1);
    return img[(size_t)r * R + xi];
}

// 8f.3 radar_cartesian_to_polar (radar_utils.py:338-372).  One thread per polar cell; fp64 throughout, as
// the reference (its sampling grid is cast to double at :370, so it only accepts an fp64 image).  sin / cos
// of the azimuths and the range coordinates come from the host (torch's CPU sin / cos / linspace, the
// reference's own library calls: device libm results differ in the last bit); every later operation is an
// IEEE fp64 operation in the reference's order, the four-tap blend the FMA chain of PyTorch's CPU
// grid_sample kernel (oracle/nn_search.c: mmk_oracle_blend4_f64) -> bit-identical output.
// Sampling position of one polar cell in the Cartesian image: radar_utils.py:352-370 and the normalise / denormalise round
// trip of F.grid_sample(align_corners=True), in the reference's order of operations.  Shared by cart_to_polar_kernel, its
// adjoint and the mask_polar_scan kernels, which therefore see the same taps and weights bit for bit.
struct CartTaps {
    int xi, yi;          // top-left tap: column, row (clamped to [-2, W] / [-2, H]: such a sample has no tap in the image)
    double wx, wy;       // ix - x0, iy - y0
    bool inimg;          // at least one of the four taps lies in the image
};

__device__ __forceinline__ CartTaps cart_taps(double s_az, double c_az, double rc, int H, int W, double cart_resolution)
{
    const double sx = s_az * rc, sy = c_az * rc;
    double u = sx / cart_resolution, v = -sy / cart_resolution;
    u = u / (double)(W - 1) * 2.0;
    v = v / (double)(H - 1) * 2.0;
    const double ix = ((u + 1.0) / 2.0) * (double)(W - 1), iy = ((v + 1.0) / 2.0) * (double)(H - 1);
    const double x0 = floor(ix), y0 = floor(iy);
    CartTaps t;
    t.wx = ix - x0;
    t.wy = iy - y0;
    // (a sample far outside the image has no tap in it: clamping keeps the conversion to int defined)
    t.xi = (int)fmin(fmax(x0, -2.0), (double)W);
    t.yi = (int)fmin(fmax(y0, -2.0), (double)H);
    t.inimg = t.xi >= -1 && t.xi < W && t.yi >= -1 && t.yi < H;
    return t;
}

// The four-tap blend of PyTorch's CPU grid_sample kernel (oracle/nn_search.c: mmk_oracle_blend4_f64) over an image of T
// (fp64, or fp32 widened, which is exact); taps outside the image are 0.
template <typename T>
__device__ __forceinline__ double cart_blend(const T *__restrict__ img, const CartTaps &t, int H, int W)
{
    const double ex = 1.0 - t.wx, sy1 = 1.0 - t.wy;
    auto tap = [&](int y, int x) -> double {
        return (x >= 0 && x < W && y >= 0 && y < H) ? (double)img[(size_t)y * W + x] : 0.0;
    };
    const double t0 = tap(t.yi, t.xi), t1 = tap(t.yi, t.xi + 1), t2 = tap(t.yi + 1, t.xi), t3 = tap(t.yi + 1, t.xi + 1);
    return fma(t3, t.wy * t.wx, fma(t2, t.wy * ex, fma(t1, sy1 * t.wx, t0 * (sy1 * ex))));
}

__global__ __launch_bounds__(256) void cart_to_polar_kernel(const double *__restrict__ cart, const double *__restrict__ sin_az,
                                                            const double *__restrict__ cos_az, const double *__restrict__ range_coords,
                                                            int A, int R, int H, int W, double cart_resolution,
                                                            double *__restrict__ polar)
{
    const int r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= R) return;
    const int a = blockIdx.y, b = blockIdx.z;
    const CartTaps t = cart_taps(sin_az[(size_t)b * A + a], cos_az[(size_t)b * A + a], range_coords[r], H, W, cart_resolution);
    polar[((size_t)b * A + a) * R + r] = cart_blend(cart + (size_t)b * H * W, t, H, W);
}

// mask_polar_scan: out = fl32(radar_cartesian_to_polar(mask as fp64)) * scan in one pass -- one read of the scan and one write
// per polar cell, the mask taps from cache; no polar image of the mask is formed.  The blend is cart_to_polar_kernel's, rounded
// to fp32 once, then one fp32 multiplication: the composition `radar_cartesian_to_polar(mask.double()).float() * scan` bit for
// bit.  A cell without a tap in the image blends four zeros and writes +0.0 * scan.
__global__ __launch_bounds__(256) void mask_polar_scan_kernel(const float *__restrict__ scan, const float *__restrict__ mask,
                                                              const double *__restrict__ sin_az, const double *__restrict__ cos_az,
                                                              const double *__restrict__ range_coords, int A, int R, int H, int W,
                                                              double cart_resolution, float *__restrict__ out)
{
    const int r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= R) return;
    const int a = blockIdx.y, b = blockIdx.z;
    const CartTaps t = cart_taps(sin_az[(size_t)b * A + a], cos_az[(size_t)b * A + a], range_coords[r], H, W, cart_resolution);
    const size_t cell = ((size_t)b * A + a) * R + r;
    out[cell] = (float)cart_blend(mask + (size_t)b * H * W, t, H, W) * scan[cell];
}

// Sampling position of one Cartesian pixel in the (wrap-padded) polar image: radar_utils.py:286-323 and the normalise /
// denormalise round trip of F.grid_sample(align_corners=True).  Shared by the forward kernel and its adjoint, which therefore
// see the same taps and weights bit for bit (the library is built with -ffp-contract=off).  `laz`: the item's azimuth table.
struct PolarTaps {
    int xi, yi;          // top-left tap: column, row of the padded image
    float wx, wy;        // ix - x0, iy - y0
};

// (the form with the two slopes: du = du/drng -- 1 / res, 0 where u is clamped at 0 -- and dv = dv/dang -- with the wobble fix
// the slope of the table's segment below c3, 0 where delta is gated off; without it 1 / step.  The normalise / denormalise
// round trip has slope 1.  polar_taps() below discards them and compiles to what it was before they existed.)
__device__ __forceinline__ PolarTaps polar_taps_slopes(const float *laz, float rng, float ang, int A, int R, float res, float half_res,
                                                       int wrap, int fix_wobble, float &du, float &dv)
{
    float u = (rng - half_res) / res;
    float v;
    du = (u < 0.f) ? 0.f : 1.0f / res;
    if (fix_wobble) {
        // lower_bound: first i with laz[i] >= ang.  The table is ascending and nearly uniform (the wobble is a fraction of a
        // step), so the search starts from the uniform table's answer and walks: two or three dependent LDS reads instead
        // of the nine of a bisection over 400 entries, the same index for any ascending table (both loops end at the first
        // entry that is not below ang); a table that is far from uniform only costs more steps.
        const float a0 = laz[0];
        const float inv_step = (float)(A - 1) / ((laz[A - 1] - a0) + 1e-30f);
        int lo = (int)fminf(fmaxf((ang - a0) * inv_step, 0.f), (float)(A - 1));
        while (lo > 0 && laz[lo - 1] >= ang) --lo;
        while (lo < A && laz[lo] < ang) ++lo;
        int c3 = lo;
        if (c3 == A) c3 -= 1;
        int c2 = c3 - 1;
        if (c2 < 0) c2 += 1;
        const float a3 = laz[c3], a2 = laz[c2];
        const float df = ang - a3;
        const float delta = ((df * ((df < 0.f) ? 1.f : 0.f)) * ((c3 > 0) ? 1.f : 0.f)) / ((a3 - a2) + 1e-14f);
        v = (float)c3 + delta;
        dv = (df < 0.f && c3 > 0) ? 1.0f / ((a3 - a2) + 1e-14f) : 0.f;
    } else {
        const float step = (laz[A - 1] - laz[0]) / (float)(A - 1);
        v = (ang - laz[0]) / step;
        dv = 1.0f / step;
    }
    if (u < 0.f) u = 0.f;
    const int rows = wrap ? A + 2 : A;
    if (wrap) v = v + 1.0f;
    // normalise to [-1,1] and back exactly as F.grid_sample(align_corners=True) does
    const float gx = u / (float)(R - 1) * 2.0f - 1.0f;
    const float gy = v / (float)(rows - 1) * 2.0f - 1.0f;
    const float ix = ((gx + 1.0f) / 2.0f) * (float)(R - 1);
    const float iy = ((gy + 1.0f) / 2.0f) * (float)(rows - 1);
    const float x0 = floorf(ix), y0 = floorf(iy);
    PolarTaps t;
    t.wx = ix - x0;
    t.wy = iy - y0;
    t.xi = (int)x0;
    t.yi = (int)y0;
    return t;
}

__device__ __forceinline__ PolarTaps polar_taps(const float *laz, float rng, float ang, int A, int R, float res, float half_res,
                                                int wrap, int fix_wobble)
{
    float du, dv;
    return polar_taps_slopes(laz, rng, ang, A, R, res, half_res, wrap, fix_wobble, du, dv);
}

// R5 radar_polar_to_cartesian_diff (radar_utils.py:258-336).  One thread per Cartesian
// pixel; the batch item's azimuth table sits in LDS for the binary search (wobble fix).
__global__ __launch_bounds__(256) void polar_to_cart_kernel(const float *__restrict__ polar,
                                                            const float *__restrict__ az,
                                                            const float *__restrict__ rgrid,
                                                            const float *__restrict__ agrid, int A, int R, int W,
                                                            float res, float half_res, int wrap, int fix_wobble,
                                                            float *__restrict__ cart, const float *__restrict__ polar2,
                                                            float *__restrict__ cart2)
{
    extern __shared__ float laz[];
    const int b = blockIdx.y;
    for (int i = threadIdx.x; i < A; i += blockDim.x) laz[i] = az[(size_t)b * A + i];
    __syncthreads();
    // a block is a 32 x 8 patch of the Cartesian image (compact footprint in the polar one: the taps of
    // neighbouring lanes share cache lines), not a 256-pixel strip of one row
    const int tiles_x = (W + 31) >> 5;
    const int px = (blockIdx.x % tiles_x) * 32 + (threadIdx.x & 31), py = (blockIdx.x / tiles_x) * 8 + (threadIdx.x >> 5);
    if (px >= W || py >= W) return;
    const int pix = py * W + px;
    const int rows = wrap ? A + 2 : A;
    const PolarTaps t = polar_taps(laz, rgrid[pix], agrid[pix], A, R, res, half_res, wrap, fix_wobble);
    const int xi = t.xi, yi = t.yi;
    const float wx = t.wx, wy = t.wy;
    const float ex = 1.0f - wx, sy = 1.0f - wy;
    // The gather is bound by the number of load instructions (64 scattered addresses each), not by bytes: the two taps of a
    // row are neighbours in memory, so each row of each image is ONE 8-byte load (4-byte aligned) instead of two 4-byte ones, all
    // four issued back to back; the zero padding is applied as selects afterwards.  Same products, same order of additions as
    // tap_polar() per tap.  (xi >= 0 because u >= 0; xi = R - 1 shifts the pair one cell left and takes its second element.)
    typedef float f32x2u __attribute__((ext_vector_type(2), aligned(4)));
    const int xa = min(max(xi, 0), R - 2);
    const bool shifted = xi > xa;                   // xi == R - 1
    int roff[2];
    bool okr[2];
#pragma unroll
    for (int k = 0; k < 2; ++k) {
        const int yk = yi + k;
        okr[k] = !(yk < 0 || yk >= rows);
        int r = yk;
        if (wrap) r = (yk == 0) ? (A - 1) : ((yk == A + 1) ? 0 : yk - 1);
        roff[k] = min(max(r, 0), A - 1) * R + xa;
    }
    const bool okx0 = xi >= 0 && xi < R, okx1 = xi + 1 >= 0 && xi + 1 < R;
    const float *img = polar + (size_t)b * A * R;
    const float *img2 = polar2 != nullptr ? polar2 + (size_t)b * A * R : img;
    f32x2u p1[2], p2[2];
#pragma unroll
    for (int k = 0; k < 2; ++k) p1[k] = *reinterpret_cast<const f32x2u *>(img + roff[k]);
#pragma unroll
    for (int k = 0; k < 2; ++k) p2[k] = *reinterpret_cast<const f32x2u *>(img2 + roff[k]);
    float t1[4], t2[4];
#pragma unroll
    for (int k = 0; k < 2; ++k) {
        t1[2 * k] = (okr[k] && okx0) ? (shifted ? p1[k].y : p1[k].x) : 0.0f;
        t1[2 * k + 1] = (okr[k] && okx1) ? p1[k].y : 0.0f;
        t2[2 * k] = (okr[k] && okx0) ? (shifted ? p2[k].y : p2[k].x) : 0.0f;
        t2[2 * k + 1] = (okr[k] && okx1) ? p2[k].y : 0.0f;
    }
    cart[(size_t)b * W * W + pix] = t1[0] * (sy * ex) + t1[1] * (sy * wx) + t1[2] * (wy * ex) + t1[3] * (wy * wx);
    // a second image on the same grid (the dataset resamples the FFT and the CFAR image with the same
    // azimuths, icp_weight_dataset.py:350-352): the coordinates and tap weights are shared
    if (polar2 != nullptr) cart2[(size_t)b * W * W + pix] = t2[0] * (sy * ex) + t2[1] * (sy * wx) + t2[2] * (wy * ex) + t2[3] * (wy * wx);
}

// ------------------------------------------------------------------------------------------
// R8 + R9: point_to_cart_idx(min_to_plus_1=True) (radar_utils.py:374-391) feeding the
// bilinear sampler of extract_weights (:108-128).
struct Taps {
    int xi, yi;
    float w00, w01, w10, w11;
    float wx, wy;        // ix − x0, iy − y0
};

// cw = cart_pixel_width of point_to_cart_idx: the normalisation is by the Cartesian grid's width
// whatever the mask's own shape is (grid_sample then maps [-1,1] onto the mask's H and W).
__device__ __forceinline__ Taps weight_taps(const float *__restrict__ p, int H, int W, int cw, float cres)
{
    const float x = p[0], y = p[1];
    const bool fake = (x == 0.0f) && (y == 0.0f);
    const float gu = -x / cres;
    const float gv = y / cres;
    float gx = gv / (float)(cw - 1) * 2.0f;
    float gy = gu / (float)(cw - 1) * 2.0f;
    if (fake) {
        gx = -100.0f;
        gy = -100.0f;
    }
    const float ix = ((gx + 1.0f) / 2.0f) * (float)(W - 1);
    const float iy = ((gy + 1.0f) / 2.0f) * (float)(H - 1);
    const float x0 = floorf(ix), y0 = floorf(iy);
    const float wx = ix - x0, wy = iy - y0;
    Taps t;
    t.xi = (int)x0;
    t.yi = (int)y0;
    t.w00 = (1.0f - wy) * (1.0f - wx);
    t.w01 = (1.0f - wy) * wx;
    t.w10 = wy * (1.0f - wx);
    t.w11 = wy * wx;
    t.wx = wx;
    t.wy = wy;
    return t;
}

// The polar counterpart (extract_weights_polar): where the point lies in a POLAR mask (A, R).  rng and ang are the point's
// own (the geometry of form_cart_range_angle_grid: pixel (i, j) is the point x = -coords[i], y = coords[j], so that
// ang = atan2(y, x) brought into [0, 2 pi)), the position in the image is polar_taps' -- the arithmetic of
// radar_polar_to_cartesian_diff, so a point at a Cartesian pixel's centre reads what that pixel gets -- and the four weights
// are formed as weight_taps forms them.  A fake point (0, 0) has no taps (`fake`; its Taps are not to be used).
__device__ __forceinline__ Taps polar_weight_taps(const float *__restrict__ p, const float *laz, int A, int R, float res,
                                                  float half_res, int wrap, int fix_wobble, bool &fake, float &rng, float &du,
                                                  float &dv)
{
    const float x = p[0], y = p[1];
    fake = (x == 0.0f) && (y == 0.0f);
    rng = sqrtf(y * y + x * x);
    float ang = atan2f(y, x);
    if (ang < 0.0f) ang = ang + 6.2831855f;        // 2 pi in fp32
    const PolarTaps pt = polar_taps_slopes(laz, rng, ang, A, R, res, half_res, wrap, fix_wobble, du, dv);
    Taps t;
    t.xi = pt.xi;
    t.yi = pt.yi;
    t.w00 = (1.0f - pt.wy) * (1.0f - pt.wx);
    t.w01 = (1.0f - pt.wy) * pt.wx;
    t.w10 = pt.wy * (1.0f - pt.wx);
    t.w11 = pt.wy * pt.wx;
    t.wx = pt.wx;
    t.wy = pt.wy;
    return t;
}

// Cell of the polar image behind tap (yk, xk) of the (wrap-padded) one, -1 outside it: with the crossover rows, padded row 0
// is row A - 1 and padded row A + 1 is row 0 (the concatenation at radar_utils.py:318), every other row yk - 1.
__device__ __forceinline__ int polar_cell(int yk, int xk, int A, int R, int wrap)
{
    const int rows = wrap ? A + 2 : A;
    if (xk < 0 || xk >= R || yk < 0 || yk >= rows) return -1;
    int r = yk;
    if (wrap) r = (yk == 0) ? (A - 1) : ((yk == A + 1) ? 0 : yk - 1);
    return r * R + xk;
}

// The two tap-to-cell mappings of the ordered scatter below: how a point becomes four taps (`taps`; `live` false: none) and
// which cell of the gradient image a tap falls on (`cell`, -1: none).  `stage` brings what `taps` reads from LDS there
// (every thread of the block calls it before any returns).
struct CartWeightGeom {
    int H, W, cw;
    float cres;
    __device__ __forceinline__ void stage(float *, int) const {}
    __device__ __forceinline__ Taps taps(const float *__restrict__ p, const float *, bool &live) const
    {
        live = true;                               // a fake point's taps lie outside every image (weight_taps)
        return weight_taps(p, H, W, cw, cres);
    }
    __device__ __forceinline__ int cell(int yy, int xx) const { return (xx >= 0 && xx < W && yy >= 0 && yy < H) ? yy * W + xx : -1; }
    __host__ __device__ size_t cells() const { return (size_t)H * W; }
};

struct PolarWeightGeom {
    const float *az;                               // (B, A)
    int A, R;
    float res, half_res;
    int wrap, fix_wobble;
    __device__ __forceinline__ void stage(float *laz, int b) const
    {
        for (int i = threadIdx.x; i < A; i += blockDim.x) laz[i] = az[(size_t)b * A + i];
        __syncthreads();
    }
    __device__ __forceinline__ Taps taps(const float *__restrict__ p, const float *laz, bool &live) const
    {
        bool fake;
        float rng, du, dv;
        const Taps t = polar_weight_taps(p, laz, A, R, res, half_res, wrap, fix_wobble, fake, rng, du, dv);
        live = !fake;
        return t;
    }
    __device__ __forceinline__ int cell(int yk, int xk) const { return polar_cell(yk, xk, A, R, wrap); }
    __host__ __device__ size_t cells() const { return (size_t)A * R; }
};

__global__ void sample_weights_fwd_kernel(const float *__restrict__ mask, const float *__restrict__ pc, int N,
                                          int cols, int H, int W, int cw, float cres, float *__restrict__ out)
{
    const int n = blockIdx.x * blockDim.x + threadIdx.x;
    const int b = blockIdx.y;
    if (n >= N) return;
    const Taps t = weight_taps(pc + ((size_t)b * N + n) * cols, H, W, cw, cres);
    const float *m = mask + (size_t)b * H * W;
    auto tap = [&](int yy, int xx) -> float {
        return (xx >= 0 && xx < W && yy >= 0 && yy < H) ? m[(size_t)yy * W + xx] : 0.0f;
    };
    out[(size_t)b * N + n] = tap(t.yi, t.xi) * t.w00 + tap(t.yi, t.xi + 1) * t.w01 + tap(t.yi + 1, t.xi) * t.w10 +
                             tap(t.yi + 1, t.xi + 1) * t.w11;
}

// extract_weights_polar: the same gather from a polar mask, the item's azimuth table in LDS.  The sum is formed in
// sample_weights_fwd_kernel's order; taps outside the padded image read 0, a fake point gets 0.
__global__ __launch_bounds__(256) void sample_weights_polar_fwd_kernel(const float *__restrict__ mask, const float *__restrict__ pc,
                                                                       int N, int cols, PolarWeightGeom g, float *__restrict__ out)
{
    extern __shared__ float laz[];
    const int b = blockIdx.y;
    g.stage(laz, b);
    const int n = blockIdx.x * blockDim.x + threadIdx.x;
    if (n >= N) return;
    bool live;
    const Taps t = g.taps(pc + ((size_t)b * N + n) * cols, laz, live);
    const float *m = mask + (size_t)b * g.cells();
    auto tap = [&](int yy, int xx) -> float {
        const int c = g.cell(yy, xx);
        return c >= 0 ? m[c] : 0.0f;
    };
    out[(size_t)b * N + n] = live ? tap(t.yi, t.xi) * t.w00 + tap(t.yi, t.xi + 1) * t.w01 + tap(t.yi + 1, t.xi) * t.w10 +
                                        tap(t.yi + 1, t.xi + 1) * t.w11
                                  : 0.0f;
}

// Backward of the gather = scatter-add of g * w into the four taps of every point, WITHOUT float atomics (their order of
// arrival would make the mask gradient differ from run to run where several taps fall on one pixel: neighbouring
// azimuths near the sensor, neighbouring peaks of one azimuth).  Three passes over the 4 N entries e = 4 n + q of an image:
//   link   every in-image entry pushes itself on its pixel's chain with an INTEGER exchange on the (zero-filled)
//          gradient word itself: head = e + 1, next[e] = previous head - 1 (0 = empty -> -1).  The chain's ORDER
//          depends on arrival; its SET of entries does not.
//   sum    every entry walks its pixel's chain; the entry with the lowest index owns the pixel and adds the chain's
//          values in ascending entry order (repeated selection of the next-larger index: chains are short) -- the order
//          of a sequential loop over points and taps, as PyTorch's CPU grid_sample backward runs it.
//   store  the owners write the sums over the chain heads.
// The passes are shared by the Cartesian and the polar sampler: only `link` knows the geometry (Geom: CartWeightGeom or
// PolarWeightGeom above); `sum` and `store` see cells of an image of H * W words.  Two taps of one point may fall on the same
// cell (a polar point between the last and the first azimuth, A = 2): they are two entries of that cell's chain.
template <class Geom>
__device__ __forceinline__ int tap_pixel(const Geom &g, const Taps &t, int q, float &w)
{
    w = q == 0 ? t.w00 : (q == 1 ? t.w01 : (q == 2 ? t.w10 : t.w11));
    return g.cell(t.yi + (q >> 1), t.xi + (q & 1));
}

template <class Geom>
__global__ void sample_weights_bwd_link_kernel(const float *__restrict__ gw, const float *__restrict__ pc, int N, int cols,
                                               Geom g, float *__restrict__ gmask, int *__restrict__ next,
                                               float *__restrict__ val, int *__restrict__ pix)
{
    extern __shared__ float lds[];
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    const int b = blockIdx.y;
    g.stage(lds, b);
    if (e >= 4 * N) return;
    const int n = e >> 2, q = e & 3;
    bool live;
    const Taps t = g.taps(pc + ((size_t)b * N + n) * cols, lds, live);
    float w;
    const int p = live ? tap_pixel(g, t, q, w) : -1;
    const size_t o = (size_t)b * 4 * N + e;
    pix[o] = p;
    if (p < 0) return;
    val[o] = gw[(size_t)b * N + n] * w;
    int *head = reinterpret_cast<int *>(gmask + g.cells() * b + p);
    next[o] = atomicExch(head, e + 1) - 1;
}

__global__ void sample_weights_bwd_sum_kernel(int N, int H, int W, const float *__restrict__ gmask, const int *__restrict__ next,
                                              const float *__restrict__ val, int *__restrict__ pix, float *__restrict__ res)
{
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    const int b = blockIdx.y;
    if (e >= 4 * N) return;
    const size_t base = (size_t)b * 4 * N;
    const int p = pix[base + e];
    if (p < 0) return;
    const int head = reinterpret_cast<const int *>(gmask + (size_t)b * H * W)[p] - 1;
    // the owner is the chain's lowest entry index
    int lo = head, len = 0;
    for (int c = head; c >= 0 && len < 4 * N; c = next[base + c], ++len) lo = c < lo ? c : lo;
    if (lo != e) {
        pix[base + e] = -1;                    // not the owner: nothing to store
        return;
    }
    float sum = 0.f;
    int last = -1;
    for (int k = 0; k < len; ++k) {            // the next-larger index, len times: ascending order of the entries
        int pick = 0x7fffffff;
        for (int c = head, j = 0; c >= 0 && j < len; c = next[base + c], ++j)
            if (c > last && c < pick) pick = c;
        sum += val[base + pick];
        last = pick;
    }
    res[base + e] = sum;
}

__global__ void sample_weights_bwd_store_kernel(int N, int H, int W, const int *__restrict__ pix, const float *__restrict__ res,
                                                float *__restrict__ gmask)
{
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    const int b = blockIdx.y;
    if (e >= 4 * N) return;
    const int p = pix[(size_t)b * 4 * N + e];
    if (p >= 0) gmask[(size_t)b * H * W + p] = res[(size_t)b * 4 * N + e];
}

// dL/dpc of the gather: F.grid_sample's gradient with respect to its grid (PyTorch's CPU form: ((ne − nw)·s + (se − sw)·n)·g
// along x, ((sw − nw)·e + (se − ne)·w)·g along y, times (size − 1) / 2 for align_corners=True), chained through
// point_to_cart_idx.  One thread per point, which owns its output row: no scatter.  Fake rows get 0 (the reference overwrites
// their grid in place, radar_utils.py:118-122), and so does every column but x, y.
__global__ void sample_weights_bwd_pc_kernel(const float *__restrict__ gw, const float *__restrict__ mask,
                                             const float *__restrict__ pc, int N, int cols, int H, int W, int cw, float cres,
                                             float *__restrict__ gpc)
{
    const int n = blockIdx.x * blockDim.x + threadIdx.x;
    const int b = blockIdx.y;
    if (n >= N) return;
    const float *p = pc + ((size_t)b * N + n) * cols;
    float *g = gpc + ((size_t)b * N + n) * cols;
    for (int c = 2; c < cols; ++c) g[c] = 0.0f;
    if (p[0] == 0.0f && p[1] == 0.0f) {
        g[0] = 0.0f;
        g[1] = 0.0f;
        return;
    }
    const Taps t = weight_taps(p, H, W, cw, cres);
    const float *m = mask + (size_t)b * H * W;
    auto tap = [&](int yy, int xx) -> float {
        return (xx >= 0 && xx < W && yy >= 0 && yy < H) ? m[(size_t)yy * W + xx] : 0.0f;
    };
    const float nw = tap(t.yi, t.xi), ne = tap(t.yi, t.xi + 1), sw = tap(t.yi + 1, t.xi), se = tap(t.yi + 1, t.xi + 1);
    const float go = gw[(size_t)b * N + n];
    const float gix = ((ne - nw) * (1.0f - t.wy) + (se - sw) * t.wy) * go;
    const float giy = ((sw - nw) * (1.0f - t.wx) + (se - ne) * t.wx) * go;
    const float ggx = gix * ((float)(W - 1) / 2.0f), ggy = giy * ((float)(H - 1) / 2.0f);
    // gx = ((y / cres) / (cw − 1)) · 2,  gy = ((−x / cres) / (cw − 1)) · 2
    g[0] = -(((ggy * 2.0f) / (float)(cw - 1)) / cres);
    g[1] = ((ggx * 2.0f) / (float)(cw - 1)) / cres;
}

// dL/dpc of the polar gather.  With (u, v) the position in the image, gu and gv are the bilinear slopes of
// sample_weights_bwd_pc_kernel (times g); du/drng and dv/dang come from polar_taps_slopes, and rng = sqrt(x^2 + y^2),
// ang = atan2(y, x) give drng/d(x, y) = (x, y) / rng, dang/d(x, y) = (-y, x) / rng^2.  One thread per point, no scatter; fake
// rows and every column but x, y get 0.  (A real point whose squares underflow to rng = 0 has no direction: 0 as well.)
__global__ __launch_bounds__(256) void sample_weights_polar_bwd_pc_kernel(const float *__restrict__ gw, const float *__restrict__ mask,
                                                                          const float *__restrict__ pc, int N, int cols,
                                                                          PolarWeightGeom g, float *__restrict__ gpc)
{
    extern __shared__ float laz[];
    const int b = blockIdx.y;
    g.stage(laz, b);
    const int n = blockIdx.x * blockDim.x + threadIdx.x;
    if (n >= N) return;
    const float *p = pc + ((size_t)b * N + n) * cols;
    float *o = gpc + ((size_t)b * N + n) * cols;
    for (int c = 2; c < cols; ++c) o[c] = 0.0f;
    bool fake;
    float rng, du, dv;
    const Taps t = polar_weight_taps(p, laz, g.A, g.R, g.res, g.half_res, g.wrap, g.fix_wobble, fake, rng, du, dv);
    if (fake || !(rng > 0.0f)) {
        o[0] = 0.0f;
        o[1] = 0.0f;
        return;
    }
    const float *m = mask + (size_t)b * g.cells();
    auto tap = [&](int yy, int xx) -> float {
        const int c = g.cell(yy, xx);
        return c >= 0 ? m[c] : 0.0f;
    };
    const float m00 = tap(t.yi, t.xi), m01 = tap(t.yi, t.xi + 1), m10 = tap(t.yi + 1, t.xi), m11 = tap(t.yi + 1, t.xi + 1);
    const float go = gw[(size_t)b * N + n];
    const float gu = ((m01 - m00) * (1.0f - t.wy) + (m11 - m10) * t.wy) * go;
    const float gv = ((m10 - m00) * (1.0f - t.wx) + (m11 - m01) * t.wx) * go;
    const float x = p[0], y = p[1];
    const float gr = gu * du, ga = gv * dv, r2 = rng * rng;
    o[0] = gr * (x / rng) - ga * (y / r2);
    o[1] = gr * (y / rng) + ga * (x / r2);
}

// ------------------------------------------------------------------------------------------
// R10 extract_bev_from_pts (radar_utils.py:142-165): idempotent stores of 1.0.
__global__ void bev_raster_kernel(const float *__restrict__ pc, int M, int cols, int W, float cres,
                                  float *__restrict__ bev)
{
    const int j = blockIdx.x * blockDim.x + threadIdx.x;
    const int b = blockIdx.y;
    if (j >= M) return;
    const float *p = pc + ((size_t)b * M + j) * cols;
    float iu = -p[0] / cres + (float)W / 2.0f;
    float iv = p[1] / cres + (float)W / 2.0f;
    const float mid = (float)(W / 2);
    if (iu < 0.f || iu > (float)(W - 1)) iu = mid;
    if (iv < 0.f || iv > (float)(W - 1)) iv = mid;
    const int uf = (int)floorf(iu), uc = (int)ceilf(iu), vf = (int)floorf(iv), vc = (int)ceilf(iv);
    float *o = bev + (size_t)b * W * W;
    o[(size_t)uc * W + vf] = 1.0f;
    o[(size_t)uc * W + vc] = 1.0f;
    o[(size_t)uf * W + vf] = 1.0f;
    o[(size_t)uf * W + vc] = 1.0f;
}

__global__ void bev_centre_kernel(float *__restrict__ bev, int B, int W)
{
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b < B) bev[(size_t)b * W * W + (size_t)(W / 2) * W + (W / 2)] = 0.0f;
}

// ------------------------------------------------------------------------------------------
// Statistics of extract_weights (radar_utils.py:130-138) and the point count the policy logs
// (icp_weight_policy.py:209-212) in two launches instead of ~25 small reductions: one block per scan
// forms its partial sums in a fixed order, one wave combines the scans in index order (deterministic).
// out[0] = sum_real(0.5 tanh(5 w) + 0.5) / B     (diff_mean_num_non0)
// out[1] = count(w > 0.05 & real) / B            (mean_num_non0)
// out[2] = sum_real(w) / n_real                  (mean_w; NaN when no real point, as torch.mean of nothing)
// out[3] = max_real(w), out[4] = min_real(w)     (-inf / +inf when no real point)
// out[5] = count(x != 0 & y != 0) / B            (mean_all_pts)
// out[6] = n_real
constexpr int WS_NPART = 8;

__global__ __launch_bounds__(256) void weight_stats_partial_kernel(const float *__restrict__ w, const float *__restrict__ pc, int N,
                                                                   int cols, float *__restrict__ part)
{
    __shared__ float red[4][WS_NPART];
    const int b = blockIdx.x;
    float soft = 0.f, cnt = 0.f, sum = 0.f, mx = -INFINITY, mn = INFINITY, nz = 0.f, nr = 0.f;
    for (int n = threadIdx.x; n < N; n += blockDim.x) {
        const float *p = pc + ((size_t)b * N + n) * cols;
        const float x = p[0], y = p[1];
        const float v = w[(size_t)b * N + n];
        const bool real = !(x == 0.0f && y == 0.0f);
        if (real) {
            soft += 0.5f * tanhf(5.0f * v) + 0.5f;
            cnt += (v > 0.05f) ? 1.f : 0.f;
            sum += v;
            mx = fmaxf(mx, v);
            mn = fminf(mn, v);
            nr += 1.f;
        }
        nz += (x != 0.0f && y != 0.0f) ? 1.f : 0.f;
    }
    float vals[WS_NPART] = {soft, cnt, sum, mx, mn, nz, nr, 0.f};
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
#pragma unroll
        for (int i = 0; i < WS_NPART; ++i) {
            const float o = __shfl_down(vals[i], off, 64);
            vals[i] = (i == 3) ? fmaxf(vals[i], o) : (i == 4) ? fminf(vals[i], o) : vals[i] + o;
        }
    }
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    if (lane == 0)
#pragma unroll
        for (int i = 0; i < WS_NPART; ++i) red[wv][i] = vals[i];
    __syncthreads();
    if (threadIdx.x < WS_NPART) {
        const int i = threadIdx.x;
        float t = red[0][i];
        for (int k = 1; k < 4; ++k) t = (i == 3) ? fmaxf(t, red[k][i]) : (i == 4) ? fminf(t, red[k][i]) : t + red[k][i];
        part[(size_t)b * WS_NPART + i] = t;
    }
}

__global__ void weight_stats_final_kernel(const float *__restrict__ part, int B, float *__restrict__ out)
{
    const int i = threadIdx.x;
    if (i >= WS_NPART) return;
    float t = part[i], nr = part[6];
    for (int b = 1; b < B; ++b) {
        const float o = part[(size_t)b * WS_NPART + i];
        t = (i == 3) ? fmaxf(t, o) : (i == 4) ? fminf(t, o) : t + o;
        nr += part[(size_t)b * WS_NPART + 6];
    }
    if (i == 0 || i == 1 || i == 5) t = t / (float)B;
    if (i == 2) t = t / nr;
    out[i] = t;
}

struct PeakWs {
    int32_t *row_count, *row_off, *total, *mrow;
    float *mval;
    int cap;
    size_t bytes;
};

PeakWs carve_peaks(int B, int A, int max_pts, void *ws, size_t cap_bytes)
{
    mmk::Arena ar(ws, cap_bytes);
    PeakWs w;
    w.cap = 2 * max_pts;
    w.row_count = ar.take<int32_t>((size_t)B * A);
    w.row_off = ar.take<int32_t>((size_t)B * A);
    w.total = ar.take<int32_t>((size_t)B);
    w.mrow = ar.take<int32_t>((size_t)B * w.cap);
    w.mval = ar.take<float>((size_t)B * w.cap);
    w.bytes = mmk::align_up(ar.off, 256);
    return w;
}

// ------------------------------------------------------------------------------------------
// Backward of R2 cfar_mask(diff=True) with respect to the scan: the derivative autograd takes through
// radar_utils.py:29-69 (hardshrink's gate and torch.maximum's winner are constants; an exact tie halves).
//   k_c   = keep_c ? g_c * 0.5 * steep * (1 - t_c^2) : 0          t_c = tanh(steep (x_c - th_c) + 2.5)
//   gx_i  = k_i - a_th / w2 * ( sum of k_c over the cells c whose LEFT window won and holds i
//                             + sum of k_c over the cells c whose RIGHT window won and holds i )
// The adjoint of a windowed sum is a windowed sum: i lies in the left window [c-w2-g, c-g) of the cells
// c in [i+g+1, i+w2+g+1) and in the right window [c+g+1, c+w2+g+1) of the cells c in [i-w2-g, i-g), so both
// terms are differences of ordered prefix sums of kL / kR (k of the cells whose left / right window won,
// half of it in both on a tie).  One block per row, a gather per output cell, no atomics.
// LDS is the forward's 12 bytes per cell: the fp32 row and ONE fp64 prefix array, used three times over.
//   1. prefix of x, summed exactly as cfar_mask_kernel sums it -> gate, winner and ties are the forward's;
//      k and kR stay in registers (NPRE cells per thread), kL overwrites the thread's own cells of the row
//   2. prefix of kL over the same array -> the left-window term goes to registers; kR overwrites the row
//   3. prefix of kR over the same array -> the right-window term, and the store
// All three prefixes are fp64 (a window sum is the difference of two prefixes as long as the row).
// NPRE >= ceil(R / CFAR_T).
// With TH::params (device thresholds) the same step 1 also gives the gradients of the two thresholds (th_c = a_th stat_c + b_th, radar_utils.py:56):
//   ga = - sum of k_c stat_c,  gb = - sum of k_c   over the cells c in [mincol, maxcol) (outside, th is the constant 1000).
// Each thread adds its cells in fp64 in ascending i, the block adds the 512 pairs in a fixed order (a shuffle tree per
// wave, then the eight wave totals of each sum through the scan's eight doubles of LDS) and writes one pair of doubles per row to `part`;
// cfar_param_sum_kernel finishes the sum.  No atomics.  graw == nullptr (only the thresholds require grad): the block stops
// after step 1.
template <int NPRE, class TH>
__global__ __launch_bounds__(CFAR_T) void cfar_mask_bwd_kernel(const float *__restrict__ raw, const float *__restrict__ gmask,
                                                               int R, int w2, int guard, int mincol, int maxcol, TH thr,
                                                               float steep, float *__restrict__ graw)
{
    constexpr bool PARAMS = TH::params;
    const float a_th = thr.a_of(blockIdx.y), b_th = thr.b_of(blockIdx.y);
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    double *cs = reinterpret_cast<double *>(smem);                 // R + 1
    float *row = reinterpret_cast<float *>(cs + (R + 1));          // R
    __shared__ double wsum[CFAR_T / 64];
    const size_t base = ((size_t)blockIdx.y * gridDim.x + blockIdx.x) * R;
    float kd[NPRE], kr[NPRE], sl[NPRE];
#pragma unroll
    for (int i = 0; i < NPRE; ++i) {
        const int c = threadIdx.x + i * CFAR_T;
        kd[i] = (c < R) ? gmask[base + c] : 0.0f;                  // the upstream gradient until step 1 turns it into k
        if (c < R) row[c] = raw[base + c];
    }
    __syncthreads();
    const int L = (R + CFAR_T - 1) / CFAR_T;
    const int c0 = min(R, (int)threadIdx.x * L), c1 = min(R, c0 + L);
    auto prefix = [&]() {                                          // cs[c] = sum of row[0..c), as the forward forms it
        double s = 0.0;
        for (int c = c0; c < c1; ++c) s += (double)row[c];
        double tot;
        double run = block_excl_scan<CFAR_T>(s, wsum, &tot);
        for (int c = c0; c < c1; ++c) {
            cs[c] = run;
            run += (double)row[c];
        }
        if (threadIdx.x == CFAR_T - 1) cs[R] = tot;
        __syncthreads();
    };
    prefix();
    // (in steps 1 and 2 a cell of `row` is touched by its own thread only, while every thread reads windows of cs)
    double pa = 0.0, pb = 0.0;
#pragma unroll
    for (int i = 0; i < NPRE; ++i) {
        const int c = threadIdx.x + i * CFAR_T;
        kr[i] = 0.0f;
        if (c < R) {
            float th = 1000.0f, left = 0.0f, right = 0.0f, kl = 0.0f;
            const bool inr = c >= mincol && c < maxcol;
            if (inr) {
                left = (float)(cs[c - guard] - cs[c - w2 - guard]);
                right = (float)(cs[min(R, c + w2 + guard + 1)] - cs[min(R, c + guard + 1)]);
                const float stat = fmaxf(left, right) / (float)w2;
                th = a_th * stat + b_th;
            }
            const float t = tanhf(steep * (row[c] - th) + 2.5f);
            const float m = 0.5f * t + 0.5f;
            const float k = (fabsf(m) > 0.99f) ? ((kd[i] * 0.5f) * (1.0f - t * t)) * steep : 0.0f;
            kd[i] = k;
            if (inr) {
                kl = (left > right) ? k : ((left == right) ? 0.5f * k : 0.0f);
                kr[i] = (right > left) ? k : ((left == right) ? 0.5f * k : 0.0f);
                if constexpr (PARAMS) {
                    const float stat = fmaxf(left, right) / (float)w2;     // the threshold's, bit for bit
                    pa += (double)k * (double)stat;
                    pb += (double)k;
                }
            }
            row[c] = kl;
        }
    }
    if constexpr (PARAMS) {
        // (the two sums go through wsum one after the other: an array of their own would be static LDS beyond the 64 bytes
        // cfar_args leaves beside the longest row, and the launch of R = 13 637 .. 13 647 would be refused)
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) {
            pa += __shfl_down(pa, off, 64);
            pb += __shfl_down(pb, off, 64);
        }
        double ta = 0.0, tb = 0.0;
        if ((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6] = pa;
        __syncthreads();
        if (threadIdx.x == 0) {
#pragma unroll
            for (int w = 0; w < CFAR_T / 64; ++w) ta += wsum[w];
        }
        __syncthreads();
        if ((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6] = pb;
        __syncthreads();
        if (threadIdx.x == 0) {
#pragma unroll
            for (int w = 0; w < CFAR_T / 64; ++w) tb += wsum[w];
            const size_t rowid = (size_t)blockIdx.y * gridDim.x + blockIdx.x;
            thr.part[2 * rowid] = ta;
            thr.part[2 * rowid + 1] = tb;
        }
        if (graw == nullptr) return;                               // (uniform over the block)
    }
    __syncthreads();
    prefix();
#pragma unroll
    for (int i = 0; i < NPRE; ++i) {
        const int c = threadIdx.x + i * CFAR_T;
        sl[i] = 0.0f;
        if (c < R) {
            sl[i] = (float)(cs[min(R, c + w2 + guard + 1)] - cs[min(R, c + guard + 1)]);
            row[c] = kr[i];
        }
    }
    __syncthreads();
    prefix();
    const float coef = a_th / (float)w2;
#pragma unroll
    for (int i = 0; i < NPRE; ++i) {
        const int c = threadIdx.x + i * CFAR_T;
        if (c < R) {
            const float sr = (float)(cs[max(0, c - guard)] - cs[max(0, c - w2 - guard)]);
            graw[base + c] = kd[i] - coef * (sl[i] + sr);
        }
    }
}

// The row partials of cfar_mask_bwd_kernel<NPRE, CfarThPtr> summed in a fixed order: one block per output (one for shared thresholds, over
// all B A rows; one per scan otherwise, over its A rows, so that a scan's gradient does not depend on the rest of the
// batch).  Thread t adds the rows t, t + RT, ... in ascending order, then the same shuffle tree and wave totals.  Writes
// the negated sums (dth/da = stat, dth/db = 1, dm/dth = -k) as fp32.
__global__ __launch_bounds__(RT) void cfar_param_sum_kernel(const double *__restrict__ part, int rows_per_out,
                                                            float *__restrict__ grad_a, float *__restrict__ grad_b)
{
    __shared__ double psum[2 * (RT / 64)];
    const double *src = part + (size_t)blockIdx.x * rows_per_out * 2;
    double pa = 0.0, pb = 0.0;
    for (int r = threadIdx.x; r < rows_per_out; r += RT) {
        pa += src[2 * r];
        pb += src[2 * r + 1];
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        pa += __shfl_down(pa, off, 64);
        pb += __shfl_down(pb, off, 64);
    }
    if ((threadIdx.x & 63) == 0) {
        psum[2 * (threadIdx.x >> 6)] = pa;
        psum[2 * (threadIdx.x >> 6) + 1] = pb;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        double ta = 0.0, tb = 0.0;
#pragma unroll
        for (int w = 0; w < RT / 64; ++w) {
            ta += psum[2 * w];
            tb += psum[2 * w + 1];
        }
        grad_a[blockIdx.x] = (float)(0.0 - ta);
        grad_b[blockIdx.x] = (float)(0.0 - tb);
    }
}

// ------------------------------------------------------------------------------------------
// Backward of R3 + R4 with respect to the mask (radar_utils.py:71-106, :167-185).  The set of non-zero markers,
// their order and their pairing are constants: count / scan / emit place them exactly as the forward does, then
//   peaks_bwd_points_kernel   one thread per point: grho = (R_ab^T gp) . (cos phi, sin phi, 0), and grho / 2 is written to
//                             both markers of the pair; every slot of the marker array is written once (0 for the unpaired
//                             last marker of an odd count and for the pairs at or beyond max_pts)
//   peaks_bwd_rows_kernel     one block per row: the row's markers are placed again (the emit kernel's partition and scan)
//                             and their gv spread over an LDS image of the row; every cell then gathers gv[j-1], gv[j] and
//                             the neighbouring a, z:  ga_j = gv_j z_{j+1} + gv_{j-1} z_{j-1},
//                             gz_j = gv_{j-1} a_{j-1} + gv_j a_{j+1},  diff: ga_j -= gz_j steep (1 - tanh^2(steep a_j)),
//                             gm_j = res j ga_j.  Every cell is written; a cell between two zero gv gets exactly 0.
__global__ void peaks_bwd_points_kernel(const int32_t *__restrict__ mrow, int cap, const int32_t *__restrict__ total,
                                        const float *__restrict__ az, const float *__restrict__ T_ab, int A, int max_pts,
                                        const float *__restrict__ grad_pc, float *__restrict__ gv)
{
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    const int b = blockIdx.y;
    if (k >= max_pts) return;
    const int npts = total[b] / 2;
    float g = 0.0f;
    const size_t m = (size_t)b * cap + 2 * k;                       // cap = 2 max_pts: the grid covers every slot
    if (k < npts) {
        const float phi = (az[b * A + mrow[m + 1]] + az[b * A + mrow[m]]) / 2.0f;
        const float *gp = grad_pc + ((size_t)b * max_pts + k) * 3;
        float gx = gp[0], gy = gp[1];
        if (T_ab) {
            const float *T = T_ab + (size_t)b * 16;
            const float gz = gp[2];
            const float tx = (T[0] * gx + T[4] * gy) + T[8] * gz;
            const float ty = (T[1] * gx + T[5] * gy) + T[9] * gz;
            gx = tx; gy = ty;
        }
        g = (gx * cosf(phi) + gy * sinf(phi)) / 2.0f;
    }
    gv[m] = g;
    gv[m + 1] = g;
}

__global__ __launch_bounds__(RT) void peaks_bwd_rows_kernel(const float *__restrict__ mask, int R, float res, int diff,
                                                            float steep, const int32_t *__restrict__ row_off, int cap,
                                                            const float *__restrict__ gv, float *__restrict__ gmask)
{
    extern __shared__ __attribute__((aligned(16))) float lrow_dyn[];
    __shared__ int sm[RT / 64];
    float *gvr = lrow_dyn + R;                                      // R: gv of the marker stored at column j, else 0
    const int a = blockIdx.x, b = blockIdx.y, A = gridDim.x;
    const int rowid = b * A + a;
    for (int c = threadIdx.x; c < R; c += RT) gvr[c] = 0.0f;
    const float *mrow = stage_row(mask + (size_t)rowid * R, R, lrow_dyn);
    const int L = (R - 1 + RT - 1) / RT;
    const int j0 = min(R - 1, (int)threadIdx.x * L), j1 = min(R - 1, j0 + L);
    int cnt = 0;
    for (int j = j0; j < j1; ++j) cnt += (peak_value(mrow, j, R, res, diff, steep) != 0.0f) ? 1 : 0;
    int tot;
    int g = row_off[rowid] + block_excl_scan_i(cnt, sm, &tot);
    if (cnt != 0) {
        for (int j = j0; j < j1; ++j) {
            if (peak_value(mrow, j, R, res, diff, steep) != 0.0f) {
                if (g < cap) gvr[j] = gv[(size_t)b * cap + g];
                ++g;
            }
        }
    }
    __syncthreads();
    float *out = gmask + (size_t)rowid * R;
    auto aval = [&](int j) -> float { return (res * (float)j) * mrow[j]; };
    auto zval = [&](float av) -> float { return diff ? 1.0f - tanhf(steep * av) : ((av == 0.0f) ? 1.0f : 0.0f); };
    for (int j = threadIdx.x; j < R; j += RT) {
        const float g1 = gvr[j], g0 = (j > 0) ? gvr[j - 1] : 0.0f;  // gvr[R - 1] = 0: no marker is stored there
        float gm = 0.0f;
        if (g0 != 0.0f || g1 != 0.0f) {
            const float ap = (j > 0) ? aval(j - 1) : 0.0f, an = (j + 1 < R) ? aval(j + 1) : 0.0f;
            float ga = g1 * zval(an) + g0 * zval(ap);
            if (diff) {
                const float t = tanhf(steep * aval(j));
                const float gz = g0 * ap + g1 * an;
                ga += gz * (-steep * (1.0f - t * t));
            }
            gm = (res * (float)j) * ga;
        }
        out[j] = gm;
    }
}

struct PeakBwdWs {
    PeakWs f;
    float *gv;
    size_t bytes;
};

PeakBwdWs carve_peaks_bwd(int B, int A, int max_pts, void *ws, size_t cap_bytes)
{
    PeakBwdWs w;
    w.f = carve_peaks(B, A, max_pts, ws, cap_bytes);
    mmk::Arena ar(ws, cap_bytes);
    ar.off = w.f.bytes;
    w.gv = ar.take<float>((size_t)B * w.f.cap);
    w.bytes = mmk::align_up(ar.off, 256);
    return w;
}


// ------------------------------------------------------------------------------------------
// Adjoints of the two resamplers with respect to their image.  Both operators are linear in the image, so each adjoint is
// the scatter of g * w_tap over the forward's taps; the taps are recomputed with the forward's own arithmetic.  Several taps
// fall on one destination (up to hundreds: every ray's first samples on the four centre pixels), and float atomics would make
// the sum depend on their order of arrival, so the sums are formed in 64-bit FIXED POINT, as icp_bwd_target_*_kernel forms
// them (mmk_icp.hip): integer additions commute, the result is the same bit pattern whatever the order.
//   absmax   the item's largest |g| as float bits (fp64: the high word), by an integer max
//   scatter  v = llrint(g * w * scale) added to the destination's 64-bit word; scale is the power of two that puts the largest
//            possible sum, count * max|g|, below 2^62: scale = 2^(62 - cnt_bits - e), max|g| < 2^e, count <= 2^cnt_bits
//   final    destination = word / scale; a word no tap touched is 0 and gives exactly 0.  A non-finite g makes the item NaN.
// Resolution: one contribution is rounded to max|g| * 2^(cnt_bits - 62), the sum of n of them to n/2 times that.
template <typename T>
__device__ __forceinline__ unsigned abs_bits(T v);
template <>
__device__ __forceinline__ unsigned abs_bits<float>(float v) { return __float_as_uint(v) & 0x7fffffffu; }
template <>
__device__ __forceinline__ unsigned abs_bits<double>(double v) { return (unsigned)((unsigned long long)__double_as_longlong(v) >> 32) & 0x7fffffffu; }

template <typename T>
__global__ __launch_bounds__(256) void absmax_bits_kernel(const T *__restrict__ g, size_t n, unsigned *__restrict__ pmax)
{
    const int b = blockIdx.y;
    const T *gb = g + (size_t)b * n;
    unsigned m = 0u;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) m = max(m, abs_bits<T>(gb[i]));
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) m = max(m, (unsigned)__shfl_xor((int)m, off, 64));
    if ((threadIdx.x & 63) == 0 && m != 0u) atomicMax(&pmax[b], m);
}

// max|g| < 2^e from the bits above; 0.0 = non-finite gradient.  EXPB / BIAS: 23 / 126 for fp32 bits, 20 / 1022 for the high
// word of an fp64 (subnormals included: their exponent field is 0).  The exponent of the scale is capped so that it stays finite.
template <typename T>
__device__ __forceinline__ double fixed_scale(unsigned mbits, int cnt_bits)
{
    constexpr bool F = sizeof(T) == 4;
    if (mbits >= (F ? 0x7f800000u : 0x7ff00000u)) return 0.0;
    if (mbits == 0u) return 1.0;
    const int e = (int)(mbits >> (F ? 23 : 20)) - (F ? 126 : 1022);
    return ldexp(1.0, min(62 - cnt_bits - e, 1000));
}

template <typename T>
__global__ __launch_bounds__(256) void fixed_final_kernel(const unsigned long long *acc, const unsigned *__restrict__ pmax,
                                                          int cnt_bits, size_t n, T *out)
{
    // (acc and out may be the same buffer when T is 8 bytes wide: a thread reads its word before it writes it)
    const int b = blockIdx.y;
    const double scale = fixed_scale<T>(pmax[b], cnt_bits);
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) {
        const long long a = (long long)acc[(size_t)b * n + i];
        out[(size_t)b * n + i] = scale == 0.0 ? (T)__builtin_nan("") : (T)((double)a / scale);
    }
}

// Adjoint of R5 (radar_utils.py:258-336).  One thread per Cartesian pixel, the forward's tiling; tap (yk, xk) of the padded
// image adds g * w to polar cell (row(yk), xk): with the crossover rows, padded row 0 is row A - 1, padded row A + 1 is row 0
// (the adjoint of the concatenation at :318), every other row yk - 1.  Taps outside the image contribute nowhere.
__global__ __launch_bounds__(256) void polar_to_cart_bwd_scatter_kernel(const float *__restrict__ gcart, const float *__restrict__ az,
                                                                        const float *__restrict__ rgrid,
                                                                        const float *__restrict__ agrid, int A, int R, int W,
                                                                        float res, float half_res, int wrap, int fix_wobble,
                                                                        const unsigned *__restrict__ pmax, int cnt_bits,
                                                                        unsigned long long *__restrict__ acc)
{
    extern __shared__ float laz[];
    const int b = blockIdx.y;
    for (int i = threadIdx.x; i < A; i += blockDim.x) laz[i] = az[(size_t)b * A + i];
    __syncthreads();
    const double scale = fixed_scale<float>(pmax[b], cnt_bits);
    if (scale == 0.0) return;
    const int tiles_x = (W + 31) >> 5;
    const int px = (blockIdx.x % tiles_x) * 32 + (threadIdx.x & 31), py = (blockIdx.x / tiles_x) * 8 + (threadIdx.x >> 5);
    if (px >= W || py >= W) return;
    const int pix = py * W + px;
    const float g = gcart[(size_t)b * W * W + pix];
    if (g == 0.0f) return;
    const int rows = wrap ? A + 2 : A;
    const PolarTaps t = polar_taps(laz, rgrid[pix], agrid[pix], A, R, res, half_res, wrap, fix_wobble);
    const float ex = 1.0f - t.wx, sy = 1.0f - t.wy;
    const float w[4] = {sy * ex, sy * t.wx, t.wy * ex, t.wy * t.wx};        // the forward's four products
    unsigned long long *ab = acc + (size_t)b * A * R;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const int yk = t.yi + (q >> 1), xk = t.xi + (q & 1);
        if (xk < 0 || xk >= R || yk < 0 || yk >= rows) continue;
        int r = yk;
        if (wrap) r = (yk == 0) ? (A - 1) : ((yk == A + 1) ? 0 : yk - 1);
        const long long v = llrint(((double)g * (double)w[q]) * scale);
        if (v != 0) atomicAdd(&ab[(size_t)r * R + xk], (unsigned long long)v);
    }
}

// Adjoint of 8f.3 (radar_utils.py:338-372), fp64.  One thread per polar cell with the forward's arithmetic and its coalesced
// accesses; a cell whose four taps all lie outside the image does not read its gradient.  Neighbouring samples of a ray are
// radar_resolution / cart_resolution of a pixel apart (0.25 at the default sizes), so runs of consecutive lanes share their
// 2 x 2 taps (a ray's coordinates are monotone in the range, so the lanes with one tap corner are contiguous): a segmented
// wave scan adds up their fixed-point values and the first lane of a run adds once per tap -- at the sensor, where every ray's
// first samples meet on the four centre pixels, a quarter of the atomics on those addresses.  A thread walking eight cells
// of a ray and summing in registers was measured too: 2.14 ms against 1.47 ms at B = 32 (its 64-byte-strided reads alone
// cost 1.0 ms).
// (the body shared by cart_to_polar_bwd_scatter_kernel and mask_polar_scan_bwd_kernel: `g` is the cell's gradient as fp64, 0.0
// for a lane past the ray's end or without a tap in the image; every lane of the wave calls it)
__device__ __forceinline__ void cart_scatter_cell(double g, bool valid, const CartTaps &t, int H, int W, double scale,
                                                  unsigned long long *__restrict__ ab)
{
    const int lane = threadIdx.x & 63;
    const double ex = 1.0 - t.wx, sy1 = 1.0 - t.wy;
    const int xi = t.xi, yi = t.yi;
    long long s0 = 0, s1 = 0, s2 = 0, s3 = 0;
    if (g != 0.0) {
        s0 = llrint((g * (sy1 * ex)) * scale);
        s1 = llrint((g * (sy1 * t.wx)) * scale);
        s2 = llrint((g * (t.wy * ex)) * scale);
        s3 = llrint((g * (t.wy * t.wx)) * scale);
    }
    if (__ballot((s0 | s1 | s2 | s3) != 0) == 0ull) return;                 // (uniform over the wave)
    const int key = valid ? yi * (W + 4) + xi : -0x7fffffff;
    const int kprev = __shfl_up(key, 1, 64);
    const bool head = lane == 0 || kprev != key;
    const unsigned long long heads = __ballot(head);
    // first lane of the next run (64 when this run reaches the end of the wave)
    const unsigned long long later = lane == 63 ? 0ull : (heads >> (lane + 1));
    const int next_head = later ? lane + 1 + (__ffsll(later) - 1) : 64;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const long long t0 = __shfl_down(s0, off, 64), t1 = __shfl_down(s1, off, 64), t2 = __shfl_down(s2, off, 64),
                        t3 = __shfl_down(s3, off, 64);
        if (lane + off < next_head) {
            s0 += t0; s1 += t1; s2 += t2; s3 += t3;
        }
    }
    if (!head || !valid) return;
    const bool x0ok = xi >= 0 && xi < W, x1ok = xi + 1 >= 0 && xi + 1 < W;
    const bool y0ok = yi >= 0 && yi < H, y1ok = yi + 1 >= 0 && yi + 1 < H;
    if (s0 != 0 && y0ok && x0ok) atomicAdd(&ab[(size_t)yi * W + xi], (unsigned long long)s0);
    if (s1 != 0 && y0ok && x1ok) atomicAdd(&ab[(size_t)yi * W + xi + 1], (unsigned long long)s1);
    if (s2 != 0 && y1ok && x0ok) atomicAdd(&ab[(size_t)(yi + 1) * W + xi], (unsigned long long)s2);
    if (s3 != 0 && y1ok && x1ok) atomicAdd(&ab[(size_t)(yi + 1) * W + xi + 1], (unsigned long long)s3);
}

__global__ __launch_bounds__(256) void cart_to_polar_bwd_scatter_kernel(const double *__restrict__ gpolar, const double *__restrict__ sin_az,
                                                                        const double *__restrict__ cos_az,
                                                                        const double *__restrict__ range_coords, int A, int R, int H,
                                                                        int W, double cart_resolution,
                                                                        const unsigned *__restrict__ pmax, int cnt_bits,
                                                                        unsigned long long *__restrict__ acc)
{
    const int r = blockIdx.x * blockDim.x + threadIdx.x;
    const int a = blockIdx.y, b = blockIdx.z;
    const double scale = fixed_scale<double>(pmax[b], cnt_bits);
    if (scale == 0.0) return;
    const bool valid = r < R;
    const CartTaps t = cart_taps(sin_az[(size_t)b * A + a], cos_az[(size_t)b * A + a], range_coords[valid ? r : R - 1], H, W,
                                 cart_resolution);
    const double g = (valid && t.inimg) ? gpolar[((size_t)b * A + a) * R + r] : 0.0;
    cart_scatter_cell(g, valid, t, H, W, scale, acc + (size_t)b * H * W);
}

// Backward of mask_polar_scan.  The gradient that reaches the polar mask is the fp32 product grad_out * scan (what autograd
// forms behind the .float() of the composition), widened to fp64, which is exact: absmax, scale rule and sums are those of
// mmk_cart_to_polar_bwd on that image, without the image.
__global__ __launch_bounds__(256) void mask_polar_scan_absmax_kernel(const float *__restrict__ gout, const float *__restrict__ scan,
                                                                     size_t n, unsigned *__restrict__ pmax)
{
    const int b = blockIdx.y;
    const float *gb = gout + (size_t)b * n, *sb = scan + (size_t)b * n;
    unsigned m = 0u;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256)
        m = max(m, abs_bits<double>((double)(gb[i] * sb[i])));
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) m = max(m, (unsigned)__shfl_xor((int)m, off, 64));
    if ((threadIdx.x & 63) == 0 && m != 0u) atomicMax(&pmax[b], m);
}

// One thread per polar cell, r fastest.  grad_scan (when asked for) = grad_out * fl32(P) with P recomputed from the mask;
// grad_mask's sums (when acc is given) by cart_scatter_cell.  pmax / acc are NULL when grad_mask is not wanted.
__global__ __launch_bounds__(256) void mask_polar_scan_bwd_kernel(const float *__restrict__ gout, const float *__restrict__ scan,
                                                                  const float *__restrict__ mask, const double *__restrict__ sin_az,
                                                                  const double *__restrict__ cos_az,
                                                                  const double *__restrict__ range_coords, int A, int R, int H, int W,
                                                                  double cart_resolution, float *__restrict__ grad_scan,
                                                                  const unsigned *__restrict__ pmax, int cnt_bits,
                                                                  unsigned long long *__restrict__ acc)
{
    const int r = blockIdx.x * blockDim.x + threadIdx.x;
    const int a = blockIdx.y, b = blockIdx.z;
    const bool valid = r < R;
    const CartTaps t = cart_taps(sin_az[(size_t)b * A + a], cos_az[(size_t)b * A + a], range_coords[valid ? r : R - 1], H, W,
                                 cart_resolution);
    const size_t cell = ((size_t)b * A + a) * R + (valid ? r : R - 1);
    const float go = gout[cell];
    if (grad_scan != nullptr && valid) grad_scan[cell] = go * (float)cart_blend(mask + (size_t)b * H * W, t, H, W);
    if (acc == nullptr) return;
    const double scale = fixed_scale<double>(pmax[b], cnt_bits);
    if (scale == 0.0) return;
    const double g = (valid && t.inimg) ? (double)(go * scan[cell]) : 0.0;
    cart_scatter_cell(g, valid, t, H, W, scale, acc + (size_t)b * H * W);
}

// word / scale of an fp64-scaled sum, rounded to fp32 once (the .double() of the composition undone)
__global__ __launch_bounds__(256) void mask_polar_scan_final_kernel(const unsigned long long *__restrict__ acc,
                                                                    const unsigned *__restrict__ pmax, int cnt_bits, size_t n,
                                                                    float *__restrict__ out)
{
    const int b = blockIdx.y;
    const double scale = fixed_scale<double>(pmax[b], cnt_bits);
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) {
        const long long a = (long long)acc[(size_t)b * n + i];
        out[(size_t)b * n + i] = scale == 0.0 ? __builtin_nanf("") : (float)((double)a / scale);
    }
}

int ceil_log2(double x)
{
    int bits = 0;
    while (bits < 62 && (double)(1ull << bits) < x) ++bits;
    return bits;
}

struct ResampleBwdWs {
    unsigned *pmax;
    unsigned long long *acc;
    size_t bytes;
};

ResampleBwdWs carve_resample_bwd(int B, size_t acc_words, void *ws, size_t cap_bytes)
{
    mmk::Arena ar(ws, cap_bytes);
    ResampleBwdWs w;
    w.pmax = ar.take<unsigned>((size_t)B);
    w.acc = ar.take<unsigned long long>(acc_words);
    w.bytes = mmk::align_up(ar.off, 256);
    return w;
}

inline int stream_blocks(size_t n) { return (int)std::min<size_t>((n + 2047) / 2048, 2048); }

}  // namespace

// ================================================================================== C ABI
static int check_workspace(const char *who, const void *ws, size_t have, size_t need)
{
    if (ws == nullptr || need > have) {
        mmk::set_error("%s: workspace too small (%zu < %zu)", who, have, need);
        return MMK_ERR_WORKSPACE;
    }
    return MMK_OK;
}

// What the four CFAR entries share: the scans, the window and the stream.
struct CfarCall {
    const float *raw;
    int32_t B, A, R, w2, guard, mincol, maxcol;
    float steep_fact;
    hipStream_t st;
    size_t smem;        // a row's dynamic LDS, the fp64 prefix array and the fp32 row: cfar_args fills it in
};

static int cfar_args(const char *who, CfarCall &c)
{
    MMK_REQUIRE(c.B >= 1 && c.A >= 1 && c.R >= 1, "%s: raw_scans must be 3D with non-empty dims", who);
    MMK_REQUIRE(c.w2 >= 1 && c.guard >= 0, "%s: bad window (w2=%d guard=%d)", who, c.w2, c.guard);
    MMK_REQUIRE(c.mincol >= c.w2 + c.guard && c.maxcol <= c.R, "%s: column range [%d,%d) outside the row", who, c.mincol, c.maxcol);
    c.smem = (size_t)(c.R + 1) * sizeof(double) + (size_t)c.R * sizeof(float);
    // (the 64 bytes are the static LDS of every CFAR kernel, the scan's eight wave totals: none of them may declare more)
    MMK_REQUIRE(c.smem <= 160 * 1024 - 64, "%s: R=%d does not fit the 160 KB LDS row buffer", who, c.R);
    return MMK_OK;
}

template <class TH>
static int launch_cfar_fwd(const CfarCall &c, TH thr, int32_t diff, float *mask)
{
    if (c.smem > 64 * 1024)
        MMK_CHECK_HIP(hipFuncSetAttribute((const void *)cfar_mask_kernel<TH>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)c.smem));
    const int rows = c.A * c.B;
    if (c.R <= 8 * CFAR_T && c.smem <= 40 * 1024) {
        // persistent form: four blocks per CU (40 KB of LDS each), each with its next row in registers
        int dev = 0, cus = 256;
        if (hipGetDevice(&dev) == hipSuccess) {
            int v = 0;
            if (hipDeviceGetAttribute(&v, hipDeviceAttributeMultiprocessorCount, dev) == hipSuccess && v > 0) cus = v;
        }
        const int grid = std::min(rows, 4 * cus);
        hipLaunchKernelGGL((cfar_mask_rows_kernel<8, TH>), dim3(grid), dim3(CFAR_T), c.smem, c.st, c.raw, rows, c.R, c.w2, c.guard,
                           c.mincol, c.maxcol, thr, diff, c.steep_fact, mask);
    } else {
        hipLaunchKernelGGL(cfar_mask_kernel<TH>, dim3(c.A, c.B), dim3(CFAR_T), c.smem, c.st, c.raw, c.R, c.w2, c.guard, c.mincol,
                           c.maxcol, thr, diff, c.steep_fact, mask);
    }
    MMK_LAUNCH_CHECK();
    return MMK_OK;
}

// grad_raw NULL (the pointer-threshold entry only): the kernel stops after its first pass.
template <class TH>
static int launch_cfar_bwd(const CfarCall &c, const float *grad_mask, TH thr, float *grad_raw)
{
    if (c.R <= 8 * CFAR_T) {
        hipLaunchKernelGGL((cfar_mask_bwd_kernel<8, TH>), dim3(c.A, c.B), dim3(CFAR_T), c.smem, c.st, c.raw, grad_mask, c.R, c.w2,
                           c.guard, c.mincol, c.maxcol, thr, c.steep_fact, grad_raw);
    } else {
        // the longest row of the LDS budget: (160 KB - 64) / 12 B = 13 648 cells = 26.7 per thread
        constexpr int NLONG = 27;
        static_assert((size_t)NLONG * CFAR_T * 12 >= 160 * 1024, "cfar_mask_bwd_kernel<NLONG> must hold every row the LDS admits");
        if (c.smem > 64 * 1024)
            MMK_CHECK_HIP(hipFuncSetAttribute((const void *)(cfar_mask_bwd_kernel<NLONG, TH>), hipFuncAttributeMaxDynamicSharedMemorySize,
                                              (int)c.smem));
        hipLaunchKernelGGL((cfar_mask_bwd_kernel<NLONG, TH>), dim3(c.A, c.B), dim3(CFAR_T), c.smem, c.st, c.raw, grad_mask, c.R, c.w2,
                           c.guard, c.mincol, c.maxcol, thr, c.steep_fact, grad_raw);
    }
    MMK_LAUNCH_CHECK();
    return MMK_OK;
}

extern "C" int mmk_cfar_mask(const float *raw, int32_t B, int32_t A, int32_t R, int32_t w2, int32_t guard,
                             int32_t mincol, int32_t maxcol, float a_thresh, float b_thresh, int32_t diff,
                             float steep_fact, float *mask, void *stream)
{
    MMK_REQUIRE(raw && mask, "mmk_cfar_mask: NULL pointer");
    CfarCall c{raw, B, A, R, w2, guard, mincol, maxcol, steep_fact, (hipStream_t)stream, 0};
    if (int rc = cfar_args("mmk_cfar_mask", c)) return rc;
    return launch_cfar_fwd(c, CfarThVal{a_thresh, b_thresh}, diff, mask);
}

extern "C" int mmk_cfar_mask_p(const float *raw, int32_t B, int32_t A, int32_t R, int32_t w2, int32_t guard, int32_t mincol,
                               int32_t maxcol, const float *a_thresh, const float *b_thresh, int32_t per_scan, int32_t diff,
                               float steep_fact, float *mask, void *stream)
{
    MMK_REQUIRE(raw && mask, "mmk_cfar_mask_p: NULL pointer");
    MMK_REQUIRE(a_thresh && b_thresh, "mmk_cfar_mask_p: NULL threshold pointer");
    CfarCall c{raw, B, A, R, w2, guard, mincol, maxcol, steep_fact, (hipStream_t)stream, 0};
    if (int rc = cfar_args("mmk_cfar_mask_p", c)) return rc;
    return launch_cfar_fwd(c, CfarThPtr{a_thresh, b_thresh, per_scan ? 1 : 0, A, nullptr}, diff, mask);
}

extern "C" size_t mmk_cfar_mask_bwd_p_ws_bytes(int32_t B, int32_t A)
{
    if (B < 1 || A < 1) return 0;
    return mmk::align_up((size_t)B * A * 2 * sizeof(double), 256);  // one (sum k stat, sum k) pair per row
}

extern "C" int mmk_cfar_mask_bwd_p(const float *raw, const float *grad_mask, int32_t B, int32_t A, int32_t R, int32_t w2,
                                   int32_t guard, int32_t mincol, int32_t maxcol, const float *a_thresh, const float *b_thresh,
                                   int32_t per_scan, float steep_fact, float *grad_raw, float *grad_a, float *grad_b,
                                   void *workspace, size_t workspace_bytes, void *stream)
{
    MMK_REQUIRE(raw && grad_mask && grad_a && grad_b, "mmk_cfar_mask_bwd_p: NULL pointer");
    MMK_REQUIRE(a_thresh && b_thresh, "mmk_cfar_mask_bwd_p: NULL threshold pointer");
    CfarCall c{raw, B, A, R, w2, guard, mincol, maxcol, steep_fact, (hipStream_t)stream, 0};
    if (int rc = cfar_args("mmk_cfar_mask_bwd_p", c)) return rc;
    if (int rc = check_workspace("mmk_cfar_mask_bwd_p", workspace, workspace_bytes, mmk_cfar_mask_bwd_p_ws_bytes(B, A))) return rc;
    double *part = static_cast<double *>(workspace);
    if (int rc = launch_cfar_bwd(c, grad_mask, CfarThPtr{a_thresh, b_thresh, per_scan ? 1 : 0, A, part}, grad_raw)) return rc;
    hipLaunchKernelGGL(cfar_param_sum_kernel, dim3(per_scan ? B : 1), dim3(RT), 0, c.st, part, per_scan ? A : A * B, grad_a, grad_b);
    MMK_LAUNCH_CHECK();
    return MMK_OK;
}

// The marker placement of a mask into `w`: count, scan, emit.  The backward runs it on the same mask to find the forward's points.
static int launch_peaks_placement(const char *who, const float *mask, int32_t B, int32_t A, int32_t R, float res, int32_t diff,
                                  float steep_fact, const PeakWs &w, hipStream_t st)
{
    const size_t row_lds = (size_t)R * sizeof(float);
    MMK_REQUIRE(row_lds <= 64 * 1024 - 64, "%s: R=%d does not fit the LDS row buffer", who, R);
    hipLaunchKernelGGL(peaks_count_kernel, dim3(A, B), dim3(RT), row_lds, st, mask, R, res, diff, steep_fact, w.row_count);
    MMK_LAUNCH_CHECK();
    hipLaunchKernelGGL(peaks_scan_kernel, dim3(B), dim3(RT), 0, st, w.row_count, A, w.row_off, w.total);
    MMK_LAUNCH_CHECK();
    hipLaunchKernelGGL(peaks_emit_kernel, dim3(A, B), dim3(RT), row_lds, st, mask, R, res, diff, steep_fact, w.row_off, w.cap,
                       w.mval, w.mrow);
    MMK_LAUNCH_CHECK();
    return MMK_OK;
}

extern "C" size_t mmk_extract_peaks_workspace_bytes(int32_t B, int32_t A, int32_t R, int32_t max_pts)
{
    (void)R;
    if (B < 1 || A < 1 || max_pts < 1) return 0;
    return carve_peaks(B, A, max_pts, nullptr, 0).bytes;
}

// Both extractor entries.  out_time NULL: the reference's own result, which averages the azimuth times too but drops them in
// pol_2_cart (radar_utils.py:99,187-195), and `times` is not read; otherwise peaks_time_kernel keeps them.
static int run_extract_peaks(const char *who, const float *mask, int32_t B, int32_t A, int32_t R, float res, const float *azimuths,
                             const float *times, const float *T_ab, int32_t diff, float steep_fact, int32_t max_pts,
                             float *out_pc, int32_t *out_count, void *workspace, size_t workspace_bytes, float *out_time,
                             void *stream)
{
    MMK_REQUIRE(mask && azimuths && out_pc && out_count, "%s: NULL pointer", who);
    MMK_REQUIRE(B >= 1 && A >= 1 && R >= 2 && max_pts >= 1, "%s: bad shape", who);
    const PeakWs w = carve_peaks(B, A, max_pts, workspace, workspace_bytes);
    if (int rc = check_workspace(who, workspace, workspace_bytes, w.bytes)) return rc;
    hipStream_t st = (hipStream_t)stream;
    if (int rc = launch_peaks_placement(who, mask, B, A, R, res, diff, steep_fact, w, st)) return rc;
    hipLaunchKernelGGL(peaks_pair_kernel, dim3((max_pts + 255) / 256, B), dim3(256), 0, st, w.mval, w.mrow, w.cap,
                       w.total, azimuths, T_ab, A, max_pts, out_pc, out_count);
    MMK_LAUNCH_CHECK();
    if (out_time) {
        hipLaunchKernelGGL(peaks_time_kernel, dim3((max_pts + 255) / 256, B), dim3(256), 0, st, w.mrow, w.cap, w.total, times, A,
                           max_pts, out_time);
        MMK_LAUNCH_CHECK();
    }
    return MMK_OK;
}

extern "C" int mmk_extract_peaks(const float *mask, int32_t B, int32_t A, int32_t R, float res, const float *azimuths,
                                 const float *times, const float *T_ab, int32_t diff, float steep_fact,
                                 int32_t max_pts, float *out_pc, int32_t *out_count, void *workspace,
                                 size_t workspace_bytes, void *stream)
{
    return run_extract_peaks("mmk_extract_peaks", mask, B, A, R, res, azimuths, times, T_ab, diff, steep_fact, max_pts, out_pc,
                             out_count, workspace, workspace_bytes, nullptr, stream);
}

extern "C" int mmk_extract_peaks_t(const float *mask, int32_t B, int32_t A, int32_t R, float res, const float *azimuths,
                                   const float *times, const float *T_ab, int32_t diff, float steep_fact,
                                   int32_t max_pts, float *out_pc, int32_t *out_count, void *workspace,
                                   size_t workspace_bytes, float *out_time, void *stream)
{
    MMK_REQUIRE(times && out_time, "mmk_extract_peaks_t: NULL times or out_time");
    return run_extract_peaks("mmk_extract_peaks_t", mask, B, A, R, res, azimuths, times, T_ab, diff, steep_fact, max_pts, out_pc,
                             out_count, workspace, workspace_bytes, out_time, stream);
}

static int deskew_args(const char *who, const float *pc, const float *t, const float *twist, int32_t B, int32_t N)
{
    MMK_REQUIRE(pc && t && twist, "%s: NULL pointer", who);
    MMK_REQUIRE(B >= 1 && B <= 65535 && N >= 1, "%s: bad shape (B=%d in 1..65535, N=%d >= 1)", who, B, N);
    return MMK_OK;
}

extern "C" int mmk_deskew_points(const float *pc, const float *t, const float *twist, int32_t B, int32_t N, float *out,
                                 void *stream)
{
    if (int rc = deskew_args("mmk_deskew_points", pc, t, twist, B, N)) return rc;
    MMK_REQUIRE(out, "mmk_deskew_points: NULL pointer");
    hipLaunchKernelGGL(deskew_points_kernel, dim3((N + DESKEW_T - 1) / DESKEW_T, B), dim3(DESKEW_T), 0, (hipStream_t)stream, pc, t,
                       twist, N, out);
    MMK_LAUNCH_CHECK();
    return MMK_OK;
}

extern "C" size_t mmk_deskew_points_bwd_workspace_bytes(int32_t B, int32_t N)
{
    if (B < 1 || N < 1) return 0;
    return mmk::align_up((size_t)B * ((N + DESKEW_T - 1) / DESKEW_T) * 6 * sizeof(double), 256);    // one partial per block
}

extern "C" int mmk_deskew_points_bwd(const float *pc, const float *t, const float *twist, int32_t B, int32_t N,
                                     const float *grad_out, float *grad_pc, float *grad_twist, void *workspace,
                                     size_t workspace_bytes, void *stream)
{
    if (int rc = deskew_args("mmk_deskew_points_bwd", pc, t, twist, B, N)) return rc;
    MMK_REQUIRE(grad_out, "mmk_deskew_points_bwd: NULL pointer");
    MMK_REQUIRE(grad_pc || grad_twist, "mmk_deskew_points_bwd: neither gradient is asked for");
    double *part = nullptr;
    if (grad_twist) {
        if (int rc = check_workspace("mmk_deskew_points_bwd", workspace, workspace_bytes, mmk_deskew_points_bwd_workspace_bytes(B, N)))
            return rc;
        part = static_cast<double *>(workspace);
    }
    hipStream_t st = (hipStream_t)stream;
    const int nblk = (N + DESKEW_T - 1) / DESKEW_T;
    hipLaunchKernelGGL(deskew_points_bwd_kernel, dim3(nblk, B), dim3(DESKEW_T), 0, st, pc, t, twist, N, grad_out, grad_pc, part);
    MMK_LAUNCH_CHECK();
    if (grad_twist) {
        hipLaunchKernelGGL(deskew_twist_sum_kernel, dim3(B), dim3(64), 0, st, part, nblk, grad_twist);
        MMK_LAUNCH_CHECK();
    }
    return MMK_OK;
}

extern "C" int mmk_cfar_mask_bwd(const float *raw, const float *grad_mask, int32_t B, int32_t A, int32_t R, int32_t w2,
                                 int32_t guard, int32_t mincol, int32_t maxcol, float a_thresh, float b_thresh,
                                 float steep_fact, float *grad_raw, void *stream)
{
    MMK_REQUIRE(raw && grad_mask && grad_raw, "mmk_cfar_mask_bwd: NULL pointer");
    CfarCall c{raw, B, A, R, w2, guard, mincol, maxcol, steep_fact, (hipStream_t)stream, 0};
    if (int rc = cfar_args("mmk_cfar_mask_bwd", c)) return rc;
    return launch_cfar_bwd(c, grad_mask, CfarThVal{a_thresh, b_thresh}, grad_raw);
}

extern "C" size_t mmk_extract_peaks_bwd_workspace_bytes(int32_t B, int32_t A, int32_t R, int32_t max_pts)
{
    (void)R;
    if (B < 1 || A < 1 || max_pts < 1) return 0;
    return carve_peaks_bwd(B, A, max_pts, nullptr, 0).bytes;
}

extern "C" int mmk_extract_peaks_bwd(const float *mask, int32_t B, int32_t A, int32_t R, float res, const float *azimuths,
                                     const float *T_ab, int32_t diff, float steep_fact, int32_t max_pts, const float *grad_pc,
                                     float *grad_mask, void *workspace, size_t workspace_bytes, void *stream)
{
    MMK_REQUIRE(mask && azimuths && grad_pc && grad_mask, "mmk_extract_peaks_bwd: NULL pointer");
    MMK_REQUIRE(B >= 1 && A >= 1 && R >= 2 && max_pts >= 1, "mmk_extract_peaks_bwd: bad shape");
    const PeakBwdWs w = carve_peaks_bwd(B, A, max_pts, workspace, workspace_bytes);
    if (int rc = check_workspace("mmk_extract_peaks_bwd", workspace, workspace_bytes, w.bytes)) return rc;
    hipStream_t st = (hipStream_t)stream;
    if (int rc = launch_peaks_placement("mmk_extract_peaks_bwd", mask, B, A, R, res, diff, steep_fact, w.f, st)) return rc;
    hipLaunchKernelGGL(peaks_bwd_points_kernel, dim3((max_pts + 255) / 256, B), dim3(256), 0, st, w.f.mrow, w.f.cap, w.f.total,
                       azimuths, T_ab, A, max_pts, grad_pc, w.gv);
    MMK_LAUNCH_CHECK();
    const size_t row_lds = (size_t)R * sizeof(float);
    if (2 * row_lds > 64 * 1024)
        MMK_CHECK_HIP(hipFuncSetAttribute((const void *)peaks_bwd_rows_kernel, hipFuncAttributeMaxDynamicSharedMemorySize,
                                          (int)(2 * row_lds)));
    hipLaunchKernelGGL(peaks_bwd_rows_kernel, dim3(A, B), dim3(RT), 2 * row_lds, st, mask, R, res, diff, steep_fact, w.f.row_off,
                       w.f.cap, w.gv, grad_mask);
    MMK_LAUNCH_CHECK();
    return MMK_OK;
}

// One image (polar2 and cart2 NULL) or two that share their azimuths, in one launch.
static int launch_polar_to_cart(const char *who, const float *polar, const float *polar2, const float *azimuths,
                                const float *range_grid, const float *angle_grid, int32_t B, int32_t A, int32_t R, int32_t W,
                                float radar_resolution, int32_t interpolate_crossover, int32_t fix_wobble, float *cart, float *cart2,
                                void *stream)
{
    MMK_REQUIRE(B >= 1 && A >= 2 && R >= 2 && W >= 1, "%s: bad shape", who);
    MMK_REQUIRE((size_t)A * 4 <= 64 * 1024, "%s: too many azimuths (%d)", who, A);
    const float half_res = (float)((double)radar_resolution / 2.0);
    hipLaunchKernelGGL(polar_to_cart_kernel, dim3(((W + 31) / 32) * ((W + 7) / 8), B), dim3(256), (size_t)A * 4, (hipStream_t)stream,
                       polar, azimuths, range_grid, angle_grid, A, R, W, radar_resolution, half_res,
                       interpolate_crossover ? 1 : 0, fix_wobble ? 1 : 0, cart, polar2, cart2);
    MMK_LAUNCH_CHECK();
    return MMK_OK;
}

extern "C" int mmk_polar_to_cart(const float *polar, const float *azimuths, const float *range_grid,
                                 const float *angle_grid, int32_t B, int32_t A, int32_t R, int32_t W,
                                 float radar_resolution, int32_t interpolate_crossover, int32_t fix_wobble, float *cart,
                                 void *stream)
{
    MMK_REQUIRE(polar && azimuths && range_grid && angle_grid && cart, "mmk_polar_to_cart: NULL pointer");
    return launch_polar_to_cart("mmk_polar_to_cart", polar, nullptr, azimuths, range_grid, angle_grid, B, A, R, W, radar_resolution,
                                interpolate_crossover, fix_wobble, cart, nullptr, stream);
}

extern "C" int mmk_polar_to_cart_pair(const float *polar, const float *polar2, const float *azimuths, const float *range_grid,
                                      const float *angle_grid, int32_t B, int32_t A, int32_t R, int32_t W,
                                      float radar_resolution, int32_t interpolate_crossover, int32_t fix_wobble, float *cart,
                                      float *cart2, void *stream)
{
    MMK_REQUIRE(polar && polar2 && azimuths && range_grid && angle_grid && cart && cart2, "mmk_polar_to_cart_pair: NULL pointer");
    return launch_polar_to_cart("mmk_polar_to_cart_pair", polar, polar2, azimuths, range_grid, angle_grid, B, A, R, W,
                                radar_resolution, interpolate_crossover, fix_wobble, cart, cart2, stream);
}

extern "C" int mmk_cart_to_polar(const double *cart, const double *sin_az, const double *cos_az, const double *range_coords,
                                 int32_t B, int32_t A, int32_t R, int32_t H, int32_t W, double cart_resolution, double *polar,
                                 void *stream)
{
    MMK_REQUIRE(cart && sin_az && cos_az && range_coords && polar, "mmk_cart_to_polar: NULL pointer");
    MMK_REQUIRE(B >= 1 && B <= 65535 && A >= 1 && A <= 65535 && R >= 1 && H >= 2 && W >= 2, "mmk_cart_to_polar: bad shape");
    MMK_REQUIRE(cart_resolution > 0.0, "mmk_cart_to_polar: cart_resolution must be positive");
    hipLaunchKernelGGL(cart_to_polar_kernel, dim3((R + 255) / 256, A, B), dim3(256), 0, (hipStream_t)stream, cart, sin_az, cos_az,
                       range_coords, A, R, H, W, cart_resolution, polar);
    MMK_LAUNCH_CHECK();
    return MMK_OK;
}

// What every fixed-point scatter starts from: no maximum yet, all sums zero.
static int clear_fixed_sums(unsigned *pmax, int32_t B, unsigned long long *acc, size_t words_per_item, hipStream_t st)
{
    MMK_CHECK_HIP(hipMemsetAsync(pmax, 0, sizeof(unsigned) * (size_t)B, st));
    MMK_CHECK_HIP(hipMemsetAsync(acc, 0, sizeof(unsigned long long) * (size_t)B * words_per_item, st));
    return MMK_OK;
}

// cnt_bits of the scatters along the rays: a ray crosses the 2 x 2 tap neighbourhood of a pixel (diagonal 2 sqrt 2 pixels) in at
// most per_ray samples, and A rays meet on the centre pixels.
static int ray_taps_bits(int32_t A, int32_t R, double radar_resolution, double cart_resolution)
{
    const double per_ray = std::min((double)R, ceil(2.0 * sqrt(2.0) * cart_resolution / radar_resolution) + 1.0);
    return ceil_log2((double)A * per_ray);
}

extern "C" size_t mmk_polar_to_cart_bwd_ws_bytes(int32_t B, int32_t A, int32_t R, int32_t W)
{
    if (B < 1 || A < 2 || R < 2 || W < 1) return 0;
    return carve_resample_bwd(B, (size_t)B * A * R, nullptr, 0).bytes;
}

extern "C" int mmk_polar_to_cart_bwd(const float *grad_cart, const float *azimuths, const float *range_grid, const float *angle_grid,
                                     int32_t B, int32_t A, int32_t R, int32_t W, float radar_resolution,
                                     int32_t interpolate_crossover, int32_t fix_wobble, float *grad_polar, void *ws,
                                     size_t ws_bytes, void *stream)
{
    MMK_REQUIRE(grad_cart && azimuths && range_grid && angle_grid && grad_polar, "mmk_polar_to_cart_bwd: NULL pointer");
    MMK_REQUIRE(B >= 1 && B <= 65535 && A >= 2 && R >= 2 && W >= 1 && W <= 16384, "mmk_polar_to_cart_bwd: bad shape");
    MMK_REQUIRE((size_t)A * 4 <= 64 * 1024, "mmk_polar_to_cart_bwd: too many azimuths (%d)", A);
    const ResampleBwdWs w = carve_resample_bwd(B, (size_t)B * A * R, ws, ws_bytes);
    if (int rc = check_workspace("mmk_polar_to_cart_bwd", ws, ws_bytes, w.bytes)) return rc;
    hipStream_t st = (hipStream_t)stream;
    const size_t ncart = (size_t)W * W, npolar = (size_t)A * R;
    const int cnt_bits = ceil_log2(4.0 * (double)ncart);               // every tap of every pixel on one cell
    const float half_res = (float)((double)radar_resolution / 2.0);
    if (int rc = clear_fixed_sums(w.pmax, B, w.acc, npolar, st)) return rc;
    hipLaunchKernelGGL(absmax_bits_kernel<float>, dim3(stream_blocks(ncart), B), dim3(256), 0, st, grad_cart, ncart, w.pmax);
    MMK_LAUNCH_CHECK();
    hipLaunchKernelGGL(polar_to_cart_bwd_scatter_kernel, dim3(((W + 31) / 32) * ((W + 7) / 8), B), dim3(256), (size_t)A * 4, st,
                       grad_cart, azimuths, range_grid, angle_grid, A, R, W, radar_resolution, half_res,
                       interpolate_crossover ? 1 : 0, fix_wobble ? 1 : 0, w.pmax, cnt_bits, w.acc);
    MMK_LAUNCH_CHECK();
    hipLaunchKernelGGL(fixed_final_kernel<float>, dim3(stream_blocks(npolar), B), dim3(256), 0, st, w.acc, w.pmax, cnt_bits, npolar,
                       grad_polar);
    MMK_LAUNCH_CHECK();
    return MMK_OK;
}

extern "C" size_t mmk_cart_to_polar_bwd_ws_bytes(int32_t B, int32_t A, int32_t R, int32_t H, int32_t W)
{
    if (B < 1 || A < 1 || R < 1 || H < 2 || W < 2) return 0;
    return carve_resample_bwd(B, 0, nullptr, 0).bytes;                  // the sums are formed in grad_cart itself
}

extern "C" int mmk_cart_to_polar_bwd(const double *grad_polar, const double *sin_az, const double *cos_az, const double *range_coords,
                                     int32_t B, int32_t A, int32_t R, int32_t H, int32_t W, double radar_resolution,
                                     double cart_resolution, double *grad_cart, void *ws, size_t ws_bytes, void *stream)
{
    MMK_REQUIRE(grad_polar && sin_az && cos_az && range_coords && grad_cart, "mmk_cart_to_polar_bwd: NULL pointer");
    MMK_REQUIRE(B >= 1 && B <= 65535 && A >= 1 && R >= 1 && H >= 2 && W >= 2, "mmk_cart_to_polar_bwd: bad shape");
    MMK_REQUIRE(A <= 65535, "mmk_cart_to_polar_bwd: too many azimuths (%d)", A);
    MMK_REQUIRE(cart_resolution > 0.0 && radar_resolution > 0.0, "mmk_cart_to_polar_bwd: resolutions must be positive");
    const ResampleBwdWs w = carve_resample_bwd(B, 0, ws, ws_bytes);
    if (int rc = check_workspace("mmk_cart_to_polar_bwd", ws, ws_bytes, w.bytes)) return rc;
    hipStream_t st = (hipStream_t)stream;
    const size_t ncart = (size_t)H * W, npolar = (size_t)A * R;
    const int cnt_bits = ray_taps_bits(A, R, radar_resolution, cart_resolution);
    unsigned long long *acc = reinterpret_cast<unsigned long long *>(grad_cart);
    if (int rc = clear_fixed_sums(w.pmax, B, acc, ncart, st)) return rc;
    hipLaunchKernelGGL(absmax_bits_kernel<double>, dim3(stream_blocks(npolar), B), dim3(256), 0, st, grad_polar, npolar, w.pmax);
    MMK_LAUNCH_CHECK();
    hipLaunchKernelGGL(cart_to_polar_bwd_scatter_kernel, dim3((R + 255) / 256, A, B), dim3(256), 0, st, grad_polar, sin_az, cos_az,
                       range_coords, A, R, H, W, cart_resolution, w.pmax, cnt_bits, acc);
    MMK_LAUNCH_CHECK();
    hipLaunchKernelGGL(fixed_final_kernel<double>, dim3(stream_blocks(ncart), B), dim3(256), 0, st, acc, w.pmax, cnt_bits, ncart,
                       grad_cart);
    MMK_LAUNCH_CHECK();
    return MMK_OK;
}

extern "C" int mmk_mask_polar_scan(const float *scan, const float *mask_cart, const double *sin_az, const double *cos_az,
                                   const double *range_coords, int32_t B, int32_t A, int32_t R, int32_t H, int32_t W,
                                   double cart_resolution, float *out, void *stream)
{
    MMK_REQUIRE(scan && mask_cart && sin_az && cos_az && range_coords && out, "mmk_mask_polar_scan: NULL pointer");
    MMK_REQUIRE(B >= 1 && B <= 65535 && A >= 1 && A <= 65535 && R >= 1 && H >= 2 && W >= 2, "mmk_mask_polar_scan: bad shape");
    MMK_REQUIRE(cart_resolution > 0.0, "mmk_mask_polar_scan: cart_resolution must be positive");
    hipLaunchKernelGGL(mask_polar_scan_kernel, dim3((R + 255) / 256, A, B), dim3(256), 0, (hipStream_t)stream, scan, mask_cart,
                       sin_az, cos_az, range_coords, A, R, H, W, cart_resolution, out);
    MMK_LAUNCH_CHECK();
    return MMK_OK;
}

extern "C" size_t mmk_mask_polar_scan_bwd_ws_bytes(int32_t B, int32_t A, int32_t R, int32_t H, int32_t W)
{
    if (B < 1 || A < 1 || R < 1 || H < 2 || W < 2) return 0;
    return carve_resample_bwd(B, (size_t)B * H * W, nullptr, 0).bytes;
}

extern "C" int mmk_mask_polar_scan_bwd(const float *grad_out, const float *scan, const float *mask_cart, const double *sin_az,
                                       const double *cos_az, const double *range_coords, int32_t B, int32_t A, int32_t R,
                                       int32_t H, int32_t W, double radar_resolution, double cart_resolution, float *grad_scan,
                                       float *grad_mask, void *ws, size_t ws_bytes, void *stream)
{
    MMK_REQUIRE(grad_out && scan && mask_cart && sin_az && cos_az && range_coords, "mmk_mask_polar_scan_bwd: NULL pointer");
    MMK_REQUIRE(B >= 1 && B <= 65535 && A >= 1 && A <= 65535 && R >= 1 && H >= 2 && W >= 2, "mmk_mask_polar_scan_bwd: bad shape");
    MMK_REQUIRE(cart_resolution > 0.0 && radar_resolution > 0.0, "mmk_mask_polar_scan_bwd: resolutions must be positive");
    if (!grad_scan && !grad_mask) return MMK_OK;
    hipStream_t st = (hipStream_t)stream;
    const size_t ncart = (size_t)H * W, npolar = (size_t)A * R;
    const dim3 cells((R + 255) / 256, A, B);
    if (!grad_mask) {
        hipLaunchKernelGGL(mask_polar_scan_bwd_kernel, cells, dim3(256), 0, st, grad_out, scan, mask_cart, sin_az, cos_az, range_coords,
                           A, R, H, W, cart_resolution, grad_scan, (const unsigned *)nullptr, 0, (unsigned long long *)nullptr);
        MMK_LAUNCH_CHECK();
        return MMK_OK;
    }
    const ResampleBwdWs w = carve_resample_bwd(B, (size_t)B * ncart, ws, ws_bytes);
    if (int rc = check_workspace("mmk_mask_polar_scan_bwd", ws, ws_bytes, w.bytes)) return rc;
    const int cnt_bits = ray_taps_bits(A, R, radar_resolution, cart_resolution);
    if (int rc = clear_fixed_sums(w.pmax, B, w.acc, ncart, st)) return rc;
    hipLaunchKernelGGL(mask_polar_scan_absmax_kernel, dim3(stream_blocks(npolar), B), dim3(256), 0, st, grad_out, scan, npolar, w.pmax);
    MMK_LAUNCH_CHECK();
    hipLaunchKernelGGL(mask_polar_scan_bwd_kernel, cells, dim3(256), 0, st, grad_out, scan, mask_cart, sin_az, cos_az, range_coords, A,
                       R, H, W, cart_resolution, grad_scan, w.pmax, cnt_bits, w.acc);
    MMK_LAUNCH_CHECK();
    hipLaunchKernelGGL(mask_polar_scan_final_kernel, dim3(stream_blocks(ncart), B), dim3(256), 0, st, w.acc, w.pmax, cnt_bits, ncart,
                       grad_mask);
    MMK_LAUNCH_CHECK();
    return MMK_OK;
}

// The chains of the ordered scatter, next | val | pix | res: one word per (point, tap) in each array.
struct ChainWs {
    int *next, *pix;
    float *val, *res;
    size_t bytes;
};

static ChainWs carve_chains(int32_t B, int32_t N, void *ws)
{
    const size_t ne = (size_t)B * N * 4;
    ChainWs c;
    c.next = static_cast<int *>(ws);
    c.val = reinterpret_cast<float *>(c.next + ne);
    c.pix = reinterpret_cast<int *>(c.val + ne);
    c.res = reinterpret_cast<float *>(c.pix + ne);
    c.bytes = 4 * ne * sizeof(float);
    return c;
}

// The ordered scatter of either sampler into its (B, rows, cols) image: link needs `lds_bytes` for what geom.stage brings in.
template <class Geom>
static int run_sample_weights_bwd(const char *who, const Geom &geom, int32_t rows, int32_t cols, size_t lds_bytes,
                                  const float *grad_weights, const float *pc, int32_t B, int32_t N, int32_t pc_cols, float *grad_mask,
                                  void *ws, size_t ws_bytes, hipStream_t st)
{
    MMK_REQUIRE((size_t)N * 4 < ((size_t)1 << 30) && (size_t)rows * cols < ((size_t)1 << 31), "%s: shape too large", who);
    const ChainWs c = carve_chains(B, N, ws);
    MMK_REQUIRE(ws_bytes >= c.bytes, "%s: workspace too small (%zu < %zu bytes)", who, ws_bytes, c.bytes);
    MMK_CHECK_HIP(hipMemsetAsync(grad_mask, 0, sizeof(float) * (size_t)B * rows * cols, st));
    const dim3 grid((4 * N + 255) / 256, B);
    hipLaunchKernelGGL(sample_weights_bwd_link_kernel<Geom>, grid, dim3(256), lds_bytes, st, grad_weights, pc, N, pc_cols, geom,
                       grad_mask, c.next, c.val, c.pix);
    MMK_LAUNCH_CHECK();
    hipLaunchKernelGGL(sample_weights_bwd_sum_kernel, grid, dim3(256), 0, st, N, rows, cols, grad_mask, c.next, c.val, c.pix, c.res);
    MMK_LAUNCH_CHECK();
    hipLaunchKernelGGL(sample_weights_bwd_store_kernel, grid, dim3(256), 0, st, N, rows, cols, c.pix, c.res, grad_mask);
    MMK_LAUNCH_CHECK();
    return MMK_OK;
}

// Argument checks shared by the three Cartesian sampler entries; on success `g` holds the launch's geometry.
static int cart_weight_geom(const char *who, int32_t B, int32_t N, int32_t pc_cols, int32_t H, int32_t W, int32_t cart_pixel_width,
                            float cart_resolution, CartWeightGeom &g)
{
    MMK_REQUIRE(B >= 1 && N >= 1 && pc_cols >= 2 && H >= 2 && W >= 2 && cart_pixel_width >= 2, "%s: bad shape", who);
    g = CartWeightGeom{H, W, cart_pixel_width, cart_resolution};
    return MMK_OK;
}

extern "C" int mmk_sample_weights_fwd(const float *mask, const float *pc, int32_t B, int32_t N, int32_t pc_cols,
                                      int32_t H, int32_t W, int32_t cart_pixel_width, float cart_resolution,
                                      float *weights, void *stream)
{
    MMK_REQUIRE(mask && pc && weights, "mmk_sample_weights_fwd: NULL pointer");
    CartWeightGeom g;
    if (int rc = cart_weight_geom("mmk_sample_weights_fwd", B, N, pc_cols, H, W, cart_pixel_width, cart_resolution, g)) return rc;
    hipLaunchKernelGGL(sample_weights_fwd_kernel, dim3((N + 255) / 256, B), dim3(256), 0, (hipStream_t)stream, mask, pc, N,
                       pc_cols, g.H, g.W, g.cw, g.cres, weights);
    MMK_LAUNCH_CHECK();
    return MMK_OK;
}

extern "C" size_t mmk_sample_weights_bwd_ws_bytes(int32_t B, int32_t N)
{
    return B < 1 || N < 1 ? 0 : carve_chains(B, N, nullptr).bytes;
}

extern "C" int mmk_sample_weights_bwd(const float *grad_weights, const float *pc, int32_t B, int32_t N, int32_t pc_cols,
                                      int32_t H, int32_t W, int32_t cart_pixel_width, float cart_resolution,
                                      float *grad_mask, void *ws, size_t ws_bytes, void *stream)
{
    MMK_REQUIRE(grad_weights && pc && grad_mask && ws, "mmk_sample_weights_bwd: NULL pointer");
    CartWeightGeom g;
    if (int rc = cart_weight_geom("mmk_sample_weights_bwd", B, N, pc_cols, H, W, cart_pixel_width, cart_resolution, g)) return rc;
    return run_sample_weights_bwd("mmk_sample_weights_bwd", g, H, W, 0, grad_weights, pc, B, N, pc_cols, grad_mask, ws, ws_bytes,
                                  (hipStream_t)stream);
}

extern "C" int mmk_sample_weights_bwd_pc(const float *grad_weights, const float *mask, const float *pc, int32_t B, int32_t N,
                                         int32_t pc_cols, int32_t H, int32_t W, int32_t cart_pixel_width, float cart_resolution,
                                         float *grad_pc, void *stream)
{
    MMK_REQUIRE(grad_weights && mask && pc && grad_pc, "mmk_sample_weights_bwd_pc: NULL pointer");
    CartWeightGeom g;
    if (int rc = cart_weight_geom("mmk_sample_weights_bwd_pc", B, N, pc_cols, H, W, cart_pixel_width, cart_resolution, g)) return rc;
    hipLaunchKernelGGL(sample_weights_bwd_pc_kernel, dim3((N + 255) / 256, B), dim3(256), 0, (hipStream_t)stream, grad_weights, mask,
                       pc, N, pc_cols, g.H, g.W, g.cw, g.cres, grad_pc);
    MMK_LAUNCH_CHECK();
    return MMK_OK;
}

// The same for the three polar sampler entries.
static int polar_weight_geom(const char *who, const float *azimuths, int32_t B, int32_t N, int32_t pc_cols, int32_t A, int32_t R,
                             float radar_resolution, int32_t interpolate_crossover, int32_t fix_wobble, PolarWeightGeom &g)
{
    MMK_REQUIRE(B >= 1 && B <= 65535 && N >= 1 && pc_cols >= 2 && A >= 2 && R >= 2, "%s: bad shape", who);
    MMK_REQUIRE(radar_resolution > 0.0f, "%s: radar_resolution must be positive", who);
    MMK_REQUIRE((size_t)A * 4 <= 64 * 1024, "%s: too many azimuths (%d)", who, A);
    MMK_REQUIRE((size_t)(A + 2) * R < ((size_t)1 << 31), "%s: shape too large", who);
    g = PolarWeightGeom{azimuths, A, R, radar_resolution, (float)((double)radar_resolution / 2.0), interpolate_crossover ? 1 : 0,
                        fix_wobble ? 1 : 0};
    return MMK_OK;
}

extern "C" int mmk_sample_weights_polar_fwd(const float *mask, const float *pc, const float *azimuths, int32_t B, int32_t N,
                                            int32_t pc_cols, int32_t A, int32_t R, float radar_resolution,
                                            int32_t interpolate_crossover, int32_t fix_wobble, float *weights, void *stream)
{
    MMK_REQUIRE(mask && pc && azimuths && weights, "mmk_sample_weights_polar_fwd: NULL pointer");
    PolarWeightGeom g;
    if (int rc = polar_weight_geom("mmk_sample_weights_polar_fwd", azimuths, B, N, pc_cols, A, R, radar_resolution,
                                   interpolate_crossover, fix_wobble, g))
        return rc;
    hipLaunchKernelGGL(sample_weights_polar_fwd_kernel, dim3((N + 255) / 256, B), dim3(256), (size_t)A * 4, (hipStream_t)stream, mask,
                       pc, N, pc_cols, g, weights);
    MMK_LAUNCH_CHECK();
    return MMK_OK;
}

extern "C" size_t mmk_sample_weights_polar_bwd_ws_bytes(int32_t B, int32_t N)
{
    return mmk_sample_weights_bwd_ws_bytes(B, N);       // the same chain words: one of each per (point, tap)
}

extern "C" int mmk_sample_weights_polar_bwd(const float *grad_weights, const float *pc, const float *azimuths, int32_t B, int32_t N,
                                            int32_t pc_cols, int32_t A, int32_t R, float radar_resolution,
                                            int32_t interpolate_crossover, int32_t fix_wobble, float *grad_mask, void *ws,
                                            size_t ws_bytes, void *stream)
{
    MMK_REQUIRE(grad_weights && pc && azimuths && grad_mask && ws, "mmk_sample_weights_polar_bwd: NULL pointer");
    PolarWeightGeom g;
    if (int rc = polar_weight_geom("mmk_sample_weights_polar_bwd", azimuths, B, N, pc_cols, A, R, radar_resolution,
                                   interpolate_crossover, fix_wobble, g))
        return rc;
    return run_sample_weights_bwd("mmk_sample_weights_polar_bwd", g, A, R, (size_t)A * 4, grad_weights, pc, B, N, pc_cols, grad_mask,
                                  ws, ws_bytes, (hipStream_t)stream);
}

extern "C" int mmk_sample_weights_polar_bwd_pc(const float *grad_weights, const float *mask, const float *pc, const float *azimuths,
                                               int32_t B, int32_t N, int32_t pc_cols, int32_t A, int32_t R, float radar_resolution,
                                               int32_t interpolate_crossover, int32_t fix_wobble, float *grad_pc, void *stream)
{
    MMK_REQUIRE(grad_weights && mask && pc && azimuths && grad_pc, "mmk_sample_weights_polar_bwd_pc: NULL pointer");
    PolarWeightGeom g;
    if (int rc = polar_weight_geom("mmk_sample_weights_polar_bwd_pc", azimuths, B, N, pc_cols, A, R, radar_resolution,
                                   interpolate_crossover, fix_wobble, g))
        return rc;
    hipLaunchKernelGGL(sample_weights_polar_bwd_pc_kernel, dim3((N + 255) / 256, B), dim3(256), (size_t)A * 4, (hipStream_t)stream,
                       grad_weights, mask, pc, N, pc_cols, g, grad_pc);
    MMK_LAUNCH_CHECK();
    return MMK_OK;
}

extern "C" int mmk_weight_stats(const float *weights, const float *pc, int32_t B, int32_t N, int32_t pc_cols, float *partial,
                                float *out, void *stream)
{
    MMK_REQUIRE(weights && pc && partial && out, "mmk_weight_stats: NULL pointer");
    MMK_REQUIRE(B >= 1 && N >= 1 && pc_cols >= 2, "mmk_weight_stats: bad shape");
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(weight_stats_partial_kernel, dim3(B), dim3(256), 0, st, weights, pc, N, pc_cols, partial);
    MMK_LAUNCH_CHECK();
    hipLaunchKernelGGL(weight_stats_final_kernel, dim3(1), dim3(64), 0, st, partial, B, out);
    MMK_LAUNCH_CHECK();
    return MMK_OK;
}

extern "C" int mmk_bev_raster(const float *pc, int32_t B, int32_t M, int32_t pc_cols, int32_t W, float cart_resolution,
                              float *bev, void *stream)
{
    MMK_REQUIRE(pc && bev, "mmk_bev_raster: NULL pointer");
    MMK_REQUIRE(B >= 1 && M >= 1 && pc_cols >= 2 && W >= 2, "mmk_bev_raster: bad shape");
    hipStream_t st = (hipStream_t)stream;
    MMK_CHECK_HIP(hipMemsetAsync(bev, 0, sizeof(float) * (size_t)B * W * W, st));
    hipLaunchKernelGGL(bev_raster_kernel, dim3((M + 255) / 256, B), dim3(256), 0, st, pc, M, pc_cols, W, cart_resolution,
                       bev);
    MMK_LAUNCH_CHECK();
    hipLaunchKernelGGL(bev_centre_kernel, dim3((B + 255) / 256), dim3(256), 0, st, bev, B, W);
    MMK_LAUNCH_CHECK();
    return MMK_OK;
}
