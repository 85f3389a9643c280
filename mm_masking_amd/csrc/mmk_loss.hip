// Loss terms of the training step as single launches (round 4): the pose terms and the BCE mask terms of
// eval_training_loss (mm_masking/train_icp_weights.py:179-253) and their gradients.  Through PyTorch these were ~45 launches
// of 2-36 us per step (slices, subtractions, norms, means, BCELoss forward / mean / backward, scalings); each is one kernel
// (plus an ordered final sum) here.  Deterministic: block partials in a fixed order, no float atomics.
//
//   pose terms (:192-200, gt_eye):  xi = T_pred - I;  rot = mean_b |xi[b,1,0]|  (torch.norm over a 1-vector),
//                                   trans = mean_b sqrt(xi[b,0,3]^2 + xi[b,1,3]^2)
//   mask terms (:204-226):          torch.nn.BCELoss()(mask, target) = mean(-(t max(log x, -100) + (1 - t) max(log(1 - x), -100)))
//                                   gradient (x - t) / max((1 - x) x, 1e-12) / n, as torch's binary_cross_entropy_backward
//   pose terms (:192-200, not gt_eye): xi = T_pred T_gt^-1 - I, evaluated as (T_pred - T_gt) T_gt^-1 in fp64 with a general
//                                   Gauss-Jordan inverse (partial pivoting): poses read from data are not exactly orthonormal,
//                                   and T_pred = T_gt gives xi = 0 exactly (a zero gradient, as torch.norm's backward at zero)
//   validation metric (:255-273):   mean_b ||(xi[1,0], xi[0,3], xi[1,3])||, mean_b |xi[1,0]|, mean_b ||(xi[0,3], xi[1,3])||
//   SE(3) pose terms (pose_loss="se3"): v = half the skew part of xi's rotation block, s = ||v||, c = 1 + trace / 2,
//                                   theta = atan2(s, c) (the geodesic angle), r = ||xi[0:3,3]||, all in fp64, both forms of xi;
//                                   rot = mean_b theta, trans = mean_b r, metric = (mean_b sqrt(theta^2 + r^2), rot, trans)
//   fft mask term (:204-207):       target = fft > 3 * mean_{H,W}(fft) per image, computed on the fly inside the BCE passes (no
//                                   target tensor); the per-image mean is an ordered fp64 reduction rounded to fp32
#include <math.h>

#include <algorithm>

#include "mmk_common.h"

namespace {

constexpr int BCE_BLOCKS = 2048, BCE_THREADS = 256;
constexpr int FFT_MEAN_BLOCKS = 64;     // partial sums per image of the fft mean (one wave reduces them)

__global__ __launch_bounds__(64) void pose_loss_fwd_kernel(const float *__restrict__ T, int B, float *__restrict__ out)
{
    // one wave; lane l sums pairs l, l + 64, ... in index order, then a fixed shuffle tree
    double rot = 0.0, trans = 0.0;
    for (int b = threadIdx.x; b < B; b += 64) {
        const float *t = T + (size_t)b * 16;
        const float th = t[4], x = t[3], y = t[7];               // xi[1,0]; xi[0,3], xi[1,3] (the identity has zeros there)
        rot += (double)fabsf(th);
        trans += (double)sqrtf(x * x + y * y);
    }
    rot = wave_sum(rot);
    trans = wave_sum(trans);
    if (threadIdx.x == 0) {
        out[0] = (float)(rot / B);
        out[1] = (float)(trans / B);
    }
}

__global__ void pose_loss_bwd_kernel(const float *__restrict__ T, int B, const float *__restrict__ g_rot, const float *__restrict__ g_trans,
                                     float *__restrict__ gT)
{
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    const float gr = g_rot ? g_rot[0] : 0.f, gt = g_trans ? g_trans[0] : 0.f;
    const float *t = T + (size_t)b * 16;
    float *g = gT + (size_t)b * 16;
#pragma unroll
    for (int i = 0; i < 16; ++i) g[i] = 0.f;
    const float th = t[4], x = t[3], y = t[7];
    // d|th| = sign(th) (0 at 0, as torch.norm's backward masks the zero norm); d sqrt(x^2 + y^2) = (x, y) / norm (0 at 0)
    const float inv_b = 1.0f / (float)B;
    g[4] = (th > 0.f ? 1.f : (th < 0.f ? -1.f : 0.f)) * gr * inv_b;
    const float n = sqrtf(x * x + y * y);
    if (n > 0.f) {
        g[3] = x / n * gt * inv_b;
        g[7] = y / n * gt * inv_b;
    }
}

__device__ __forceinline__ float bce_term(float x, float t)
{
    const float lx = fmaxf(logf(x), -100.f), l1 = fmaxf(logf(1.f - x), -100.f);
    return -(t * lx + (1.f - t) * l1);
}

__global__ __launch_bounds__(BCE_THREADS) void bce_partial_kernel(const float *__restrict__ x, const float *__restrict__ t, size_t n,
                                                                  double *__restrict__ part)
{
    __shared__ double red[BCE_THREADS / 64];
    double s = 0.0;
    const size_t n4 = n / 4;
    for (size_t i = (size_t)blockIdx.x * BCE_THREADS + threadIdx.x; i < n4; i += (size_t)gridDim.x * BCE_THREADS) {
        const float4 xv = reinterpret_cast<const float4 *>(x)[i], tv = reinterpret_cast<const float4 *>(t)[i];
        s += (double)((bce_term(xv.x, tv.x) + bce_term(xv.y, tv.y)) + (bce_term(xv.z, tv.z) + bce_term(xv.w, tv.w)));
    }
    if (blockIdx.x == 0)
        for (size_t i = n4 * 4 + threadIdx.x; i < n; i += BCE_THREADS) s += (double)bce_term(x[i], t[i]);
    s = wave_sum(s);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) part[blockIdx.x] = (red[0] + red[1]) + (red[2] + red[3]);
}

__global__ __launch_bounds__(256) void bce_final_kernel(const double *__restrict__ part, int nblk, double inv_n, float *__restrict__ out)
{
    __shared__ double red[4];
    double s = 0.0;
    for (int i = threadIdx.x; i < nblk; i += 256) s += part[i];
    s = wave_sum(s);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) out[0] = (float)(((red[0] + red[1]) + (red[2] + red[3])) * inv_n);
}

__global__ __launch_bounds__(BCE_THREADS) void bce_bwd_kernel(const float *__restrict__ x, const float *__restrict__ t, size_t n,
                                                              const float *__restrict__ gout, float inv_n, float *__restrict__ g)
{
    const float s = gout[0] * inv_n;
    auto grad = [s](float xv, float tv) { return (xv - tv) / fmaxf((1.f - xv) * xv, 1e-12f) * s; };
    const size_t n4 = n / 4;
    for (size_t i = (size_t)blockIdx.x * BCE_THREADS + threadIdx.x; i < n4; i += (size_t)gridDim.x * BCE_THREADS) {
        const float4 xv = reinterpret_cast<const float4 *>(x)[i], tv = reinterpret_cast<const float4 *>(t)[i];
        reinterpret_cast<float4 *>(g)[i] = make_float4(grad(xv.x, tv.x), grad(xv.y, tv.y), grad(xv.z, tv.z), grad(xv.w, tv.w));
    }
    if (blockIdx.x == 0)
        for (size_t i = n4 * 4 + threadIdx.x; i < n; i += BCE_THREADS) g[i] = grad(x[i], t[i]);
}

// ----------------------------------------------------------------------------- pose terms against a ground-truth pose
// General 4x4 inverse of an fp32 matrix in fp64: Gauss-Jordan with partial pivoting (the first row of largest |pivot| on ties).
// Every loop is unrolled, so the row swaps are selects and the matrices stay in registers.
__device__ __forceinline__ void inverse4(const float *__restrict__ A, double (&R)[4][4])
{
    double M[4][4];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            M[i][j] = (double)A[i * 4 + j];
            R[i][j] = i == j ? 1.0 : 0.0;
        }
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        int p = k;
        double best = fabs(M[k][k]);
#pragma unroll
        for (int r = k + 1; r < 4; ++r)
            if (fabs(M[r][k]) > best) {
                best = fabs(M[r][k]);
                p = r;
            }
#pragma unroll
        for (int r = k + 1; r < 4; ++r)
            if (r == p) {
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const double m = M[k][j], q = R[k][j];
                    M[k][j] = M[r][j];
                    R[k][j] = R[r][j];
                    M[r][j] = m;
                    R[r][j] = q;
                }
            }
        const double piv = M[k][k];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            M[k][j] /= piv;
            R[k][j] /= piv;
        }
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            if (r == k) continue;
            const double f = M[r][k];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                M[r][j] -= f * M[k][j];
                R[r][j] -= f * R[k][j];
            }
        }
    }
}

// The three entries of xi the losses read: th = xi[1,0], x = xi[0,3], y = xi[1,3].  Tg == NULL: xi = T - I (the identity has
// zeros there).  Otherwise xi = (T - Tg) Tg^-1 with Tg^-1 returned in R (the backward needs it).
__device__ __forceinline__ void pose_residual(const float *__restrict__ t, const float *__restrict__ tg, double (&R)[4][4], double &th,
                                              double &x, double &y)
{
    if (tg == nullptr) {
        th = (double)t[4];
        x = (double)t[3];
        y = (double)t[7];
        return;
    }
    inverse4(tg, R);
    double d0[4], d1[4];                                       // rows 0 and 1 of T - Tg (exact in fp64)
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        d0[j] = (double)t[j] - (double)tg[j];
        d1[j] = (double)t[4 + j] - (double)tg[4 + j];
    }
    th = (d1[0] * R[0][0] + d1[1] * R[1][0]) + (d1[2] * R[2][0] + d1[3] * R[3][0]);
    x = (d0[0] * R[0][3] + d0[1] * R[1][3]) + (d0[2] * R[2][3] + d0[3] * R[3][3]);
    y = (d1[0] * R[0][3] + d1[1] * R[1][3]) + (d1[2] * R[2][3] + d1[3] * R[3][3]);
}

// one wave; lane l takes pairs l, l + 64, ... in index order, then a fixed shuffle tree (as pose_loss_fwd_kernel).
// NOUT = 2: (rot, trans) of eval_training_loss; NOUT = 3: the 3-vector of eval_validation_loss.
template <int NOUT>
__global__ __launch_bounds__(64) void pose_metric_kernel(const float *__restrict__ T, const float *__restrict__ Tg, int B,
                                                         float *__restrict__ out)
{
    double full = 0.0, rot = 0.0, trans = 0.0;
    for (int b = threadIdx.x; b < B; b += 64) {
        double R[4][4], th, x, y;
        pose_residual(T + (size_t)b * 16, Tg ? Tg + (size_t)b * 16 : nullptr, R, th, x, y);
        rot += fabs(th);
        trans += sqrt(x * x + y * y);
        if (NOUT == 3) full += sqrt(th * th + x * x + y * y);
    }
    rot = wave_sum(rot);
    trans = wave_sum(trans);
    if (NOUT == 3) full = wave_sum(full);
    if (threadIdx.x == 0) {
        if (NOUT == 3) {
            out[0] = (float)(full / B);
            out[1] = (float)(rot / B);
            out[2] = (float)(trans / B);
        } else {
            out[0] = (float)(rot / B);
            out[1] = (float)(trans / B);
        }
    }
}

// d/dT_pred of (g_rot rot + g_trans trans) = G Tg^-T with G nonzero at [1,0] (sign(th) g_rot / B) and [0,3], [1,3]
// ((x, y) / norm g_trans / B; zero where the norm is zero, as torch.norm's backward).  Rows 2 and 3 are zero; Tg gets none.
__global__ void pose_loss_gt_bwd_kernel(const float *__restrict__ T, const float *__restrict__ Tg, int B, const float *__restrict__ g_rot,
                                        const float *__restrict__ g_trans, float *__restrict__ gT)
{
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    const double gr = g_rot ? (double)g_rot[0] / B : 0.0, gt = g_trans ? (double)g_trans[0] / B : 0.0;
    double R[4][4], th, x, y;
    pose_residual(T + (size_t)b * 16, Tg + (size_t)b * 16, R, th, x, y);
    const double G10 = (th > 0.0 ? 1.0 : (th < 0.0 ? -1.0 : 0.0)) * gr;
    const double n = sqrt(x * x + y * y);
    const double G03 = n > 0.0 ? x / n * gt : 0.0, G13 = n > 0.0 ? y / n * gt : 0.0;
    float *g = gT + (size_t)b * 16;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        g[j] = (float)(G03 * R[j][3]);
        g[4 + j] = (float)(G10 * R[j][0] + G13 * R[j][3]);
        g[8 + j] = 0.f;
        g[12 + j] = 0.f;
    }
}

// ----------------------------------------------------------------------------- SE(3) pose terms
// The 3x4 block X of xi = T_pred T_gt^-1 - I.  Tg == NULL: X = T - I.  Otherwise X = (T - Tg) Tg^-1 with Tg^-1 returned in R (the
// backward needs it): T = Tg gives X = 0 exactly.  The differences are exact in fp64, the products are summed as pose_residual's.
__device__ __forceinline__ void pose_residual_se3(const float *__restrict__ t, const float *__restrict__ tg, double (&R)[4][4],
                                                  double (&X)[3][4])
{
    if (tg == nullptr) {
#pragma unroll
        for (int i = 0; i < 3; ++i)
#pragma unroll
            for (int j = 0; j < 4; ++j) X[i][j] = (double)t[i * 4 + j] - (i == j ? 1.0 : 0.0);
        return;
    }
    inverse4(tg, R);
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        double d[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) d[j] = (double)t[i * 4 + j] - (double)tg[i * 4 + j];
#pragma unroll
        for (int j = 0; j < 4; ++j) X[i][j] = (d[0] * R[0][j] + d[1] * R[1][j]) + (d[2] * R[2][j] + d[3] * R[3][j]);
    }
}

// Rotation part of X: v = the axis times sin(theta) (half the skew part), s = ||v||, c = cos(theta) (from the trace) for a
// rotation; theta = atan2(s, c) in [0, pi] is taken from them as they are for a block that is not orthonormal.
struct Se3Terms {
    double v[3], s, c, r;
};

__device__ __forceinline__ Se3Terms se3_terms(const double (&X)[3][4])
{
    Se3Terms q;
    q.v[0] = 0.5 * (X[2][1] - X[1][2]);
    q.v[1] = 0.5 * (X[0][2] - X[2][0]);
    q.v[2] = 0.5 * (X[1][0] - X[0][1]);
    q.s = sqrt(q.v[0] * q.v[0] + q.v[1] * q.v[1] + q.v[2] * q.v[2]);
    q.c = 1.0 + 0.5 * (X[0][0] + X[1][1] + X[2][2]);
    q.r = sqrt(X[0][3] * X[0][3] + X[1][3] * X[1][3] + X[2][3] * X[2][3]);
    return q;
}

// one wave; lane l takes pairs l, l + 64, ... in index order, then a fixed shuffle tree (as pose_metric_kernel).
// NOUT = 2: (mean theta, mean r); NOUT = 3: (mean sqrt(theta^2 + r^2), mean theta, mean r).
template <int NOUT>
__global__ __launch_bounds__(64) void pose_se3_metric_kernel(const float *__restrict__ T, const float *__restrict__ Tg, int B,
                                                             float *__restrict__ out)
{
    double full = 0.0, rot = 0.0, trans = 0.0;
    for (int b = threadIdx.x; b < B; b += 64) {
        double R[4][4], X[3][4];
        pose_residual_se3(T + (size_t)b * 16, Tg ? Tg + (size_t)b * 16 : nullptr, R, X);
        const Se3Terms q = se3_terms(X);
        const double th = atan2(q.s, q.c);
        rot += th;
        trans += q.r;
        if (NOUT == 3) full += sqrt(th * th + q.r * q.r);
    }
    rot = wave_sum(rot);
    trans = wave_sum(trans);
    if (NOUT == 3) full = wave_sum(full);
    if (threadIdx.x == 0) {
        if (NOUT == 3) {
            out[0] = (float)(full / B);
            out[1] = (float)(rot / B);
            out[2] = (float)(trans / B);
        } else {
            out[0] = (float)(rot / B);
            out[1] = (float)(trans / B);
        }
    }
}

// d/dT_pred of (g_rot mean theta + g_trans mean r) = G (Tg == NULL) or G Tg^-T, G = dL/dxi: with d = s^2 + c^2,
// d theta / dv = c v / (s d) (zero at s = 0, as torch.norm's backward) spread with +-1/2 onto the off-diagonal entries,
// d theta / dc = -s / d spread with 1/2 onto the diagonal, d r / dxi[i,3] = xi[i,3] / r (zero at r = 0).  Row 3 is zero.
__global__ void pose_se3_bwd_kernel(const float *__restrict__ T, const float *__restrict__ Tg, int B, const float *__restrict__ g_rot,
                                    const float *__restrict__ g_trans, float *__restrict__ gT)
{
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    const double gr = g_rot ? (double)g_rot[0] / B : 0.0, gt = g_trans ? (double)g_trans[0] / B : 0.0;
    double R[4][4], X[3][4];
    pose_residual_se3(T + (size_t)b * 16, Tg ? Tg + (size_t)b * 16 : nullptr, R, X);
    const Se3Terms q = se3_terms(X);
    const double d = q.s * q.s + q.c * q.c;
    const double kv = q.s > 0.0 ? q.c / (q.s * d) * gr : 0.0;      // d theta / dv = kv v
    const double gc = d > 0.0 ? -q.s / d * gr : 0.0;
    const double kr = q.r > 0.0 ? gt / q.r : 0.0;
    const double h0 = 0.5 * (kv * q.v[0]), h1 = 0.5 * (kv * q.v[1]), h2 = 0.5 * (kv * q.v[2]);
    const double G[3][4] = {{0.5 * gc, -h2, h1, kr * X[0][3]}, {h2, 0.5 * gc, -h0, kr * X[1][3]}, {-h1, h0, 0.5 * gc, kr * X[2][3]}};
    float *g = gT + (size_t)b * 16;
    // (+ 0.0: a zero gradient is stored as +0 whatever the signs of the zeros it came from, so T = Tg gives all-zero bits)
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const double v = Tg ? (G[i][0] * R[j][0] + G[i][1] * R[j][1]) + (G[i][2] * R[j][2] + G[i][3] * R[j][3]) : G[i][j];
            g[i * 4 + j] = (float)(v + 0.0);
        }
#pragma unroll
    for (int j = 0; j < 4; ++j) g[12 + j] = 0.f;
}

// ----------------------------------------------------------------------------- fft-threshold target
// Per-image sums of the fft over (H,W): block (k, b) sums its grid-stride share of image b in fp64 -> part[b * FFT_MEAN_BLOCKS + k]
__global__ __launch_bounds__(256) void image_sum_partial_kernel(const float *__restrict__ x, size_t hw, double *__restrict__ part)
{
    __shared__ double red[4];
    const int b = blockIdx.y;
    const float *xb = x + (size_t)b * hw;
    double s = 0.0;
    const size_t stride = (size_t)FFT_MEAN_BLOCKS * 256;
    if ((hw & 3) == 0) {                                       // every image starts 16-byte aligned (the base is checked on the host)
        const float4 *x4 = reinterpret_cast<const float4 *>(xb);
        for (size_t q = (size_t)blockIdx.x * 256 + threadIdx.x; q < hw / 4; q += stride) {
            const float4 v = x4[q];
            s += ((double)v.x + (double)v.y) + ((double)v.z + (double)v.w);
        }
    } else {
        for (size_t q = (size_t)blockIdx.x * 256 + threadIdx.x; q < hw; q += stride) s += (double)xb[q];
    }
    s = wave_sum(s);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) part[(size_t)b * FFT_MEAN_BLOCKS + blockIdx.x] = (red[0] + red[1]) + (red[2] + red[3]);
}

// one wave per image: thr[b] = 3.0f * mean as an fp32 product of the fp32-rounded mean (3.0 * mean_azimuth of the reference)
__global__ __launch_bounds__(64) void image_threshold_kernel(const double *__restrict__ part, size_t hw, float *__restrict__ thr)
{
    static_assert(FFT_MEAN_BLOCKS == 64, "one partial per lane");
    const double s = wave_sum(part[(size_t)blockIdx.x * FFT_MEAN_BLOCKS + threadIdx.x]);
    if (threadIdx.x == 0) thr[blockIdx.x] = 3.0f * (float)(s / (double)hw);
}

__device__ __forceinline__ float fft_target(float f, float th) { return f > th ? 1.f : 0.f; }

// Thresholds of the four elements i0 .. i0 + 3 of the flattened (B, hw) fft (hw >= 4: at most one image boundary among them)
__device__ __forceinline__ float4 thr4(const float *__restrict__ thr, size_t i0, size_t hw)
{
    const size_t b = i0 / hw, end = (b + 1) * hw;
    const float t0 = thr[b];
    if (i0 + 3 < end) return make_float4(t0, t0, t0, t0);
    const float t1 = thr[b + 1];                               // i0 + 3 < n, so image b + 1 exists
    return make_float4(t0, i0 + 1 < end ? t0 : t1, i0 + 2 < end ? t0 : t1, t1);
}

__global__ __launch_bounds__(256) void fft_mask_kernel(const float *__restrict__ fft, const float *__restrict__ thr, size_t hw, size_t n,
                                                       float *__restrict__ mask)
{
    const size_t n4 = n / 4;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n4; i += (size_t)gridDim.x * 256) {
        const float4 f = reinterpret_cast<const float4 *>(fft)[i], th = thr4(thr, i * 4, hw);
        reinterpret_cast<float4 *>(mask)[i] = make_float4(fft_target(f.x, th.x), fft_target(f.y, th.y), fft_target(f.z, th.z),
                                                          fft_target(f.w, th.w));
    }
    if (blockIdx.x == 0)
        for (size_t i = n4 * 4 + threadIdx.x; i < n; i += 256) mask[i] = fft_target(fft[i], thr[i / hw]);
}

// bce_partial_kernel / bce_bwd_kernel with the target of each element computed from fft and its image's threshold: the same
// blocks, the same grouping of the terms and the same ordered sums, so the same bits as those kernels on the written target
__global__ __launch_bounds__(BCE_THREADS) void bce_fft_partial_kernel(const float *__restrict__ x, const float *__restrict__ fft,
                                                                      const float *__restrict__ thr, size_t hw, size_t n,
                                                                      double *__restrict__ part)
{
    __shared__ double red[BCE_THREADS / 64];
    double s = 0.0;
    const size_t n4 = n / 4;
    for (size_t i = (size_t)blockIdx.x * BCE_THREADS + threadIdx.x; i < n4; i += (size_t)gridDim.x * BCE_THREADS) {
        const float4 xv = reinterpret_cast<const float4 *>(x)[i], f = reinterpret_cast<const float4 *>(fft)[i];
        const float4 th = thr4(thr, i * 4, hw);
        const float4 tv = make_float4(fft_target(f.x, th.x), fft_target(f.y, th.y), fft_target(f.z, th.z), fft_target(f.w, th.w));
        s += (double)((bce_term(xv.x, tv.x) + bce_term(xv.y, tv.y)) + (bce_term(xv.z, tv.z) + bce_term(xv.w, tv.w)));
    }
    if (blockIdx.x == 0)
        for (size_t i = n4 * 4 + threadIdx.x; i < n; i += BCE_THREADS) s += (double)bce_term(x[i], fft_target(fft[i], thr[i / hw]));
    s = wave_sum(s);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) part[blockIdx.x] = (red[0] + red[1]) + (red[2] + red[3]);
}

__global__ __launch_bounds__(BCE_THREADS) void bce_fft_bwd_kernel(const float *__restrict__ x, const float *__restrict__ fft,
                                                                  const float *__restrict__ thr, size_t hw, size_t n,
                                                                  const float *__restrict__ gout, float inv_n, float *__restrict__ g)
{
    const float s = gout[0] * inv_n;
    auto grad = [s](float xv, float tv) { return (xv - tv) / fmaxf((1.f - xv) * xv, 1e-12f) * s; };
    const size_t n4 = n / 4;
    for (size_t i = (size_t)blockIdx.x * BCE_THREADS + threadIdx.x; i < n4; i += (size_t)gridDim.x * BCE_THREADS) {
        const float4 xv = reinterpret_cast<const float4 *>(x)[i], f = reinterpret_cast<const float4 *>(fft)[i];
        const float4 th = thr4(thr, i * 4, hw);
        reinterpret_cast<float4 *>(g)[i] = make_float4(grad(xv.x, fft_target(f.x, th.x)), grad(xv.y, fft_target(f.y, th.y)),
                                                       grad(xv.z, fft_target(f.z, th.z)), grad(xv.w, fft_target(f.w, th.w)));
    }
    if (blockIdx.x == 0)
        for (size_t i = n4 * 4 + threadIdx.x; i < n; i += BCE_THREADS) g[i] = grad(x[i], fft_target(fft[i], thr[i / hw]));
}

}  // namespace

extern "C" int mmk_pose_loss_fwd(const float *T_pred, int32_t B, float *out2, void *stream)
{
    MMK_REQUIRE(T_pred && out2 && B >= 1, "mmk_pose_loss_fwd: bad argument");
    hipLaunchKernelGGL(pose_loss_fwd_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, T_pred, B, out2);
    MMK_LAUNCH_CHECK();
    return MMK_OK;
}

extern "C" int mmk_pose_loss_bwd(const float *T_pred, int32_t B, const float *g_rot, const float *g_trans, float *grad_T, void *stream)
{
    MMK_REQUIRE(T_pred && grad_T && B >= 1, "mmk_pose_loss_bwd: bad argument");
    hipLaunchKernelGGL(pose_loss_bwd_kernel, dim3((B + 63) / 64), dim3(64), 0, (hipStream_t)stream, T_pred, B, g_rot, g_trans, grad_T);
    MMK_LAUNCH_CHECK();
    return MMK_OK;
}

extern "C" size_t mmk_bce_ws_bytes(void) { return (size_t)BCE_BLOCKS * sizeof(double); }

extern "C" int mmk_bce_mean_fwd(const float *x, const float *target, int64_t n, void *ws, size_t ws_bytes, float *out, void *stream)
{
    MMK_REQUIRE(x && target && out && ws && n >= 1, "mmk_bce_mean_fwd: bad argument");
    MMK_REQUIRE(ws_bytes >= mmk_bce_ws_bytes(), "mmk_bce_mean_fwd: workspace too small");
    MMK_REQUIRE((((uintptr_t)x | (uintptr_t)target) & 15) == 0, "mmk_bce_mean_fwd: inputs must be 16-byte aligned");
    const int nblk = (int)std::min<size_t>(BCE_BLOCKS, ((size_t)n / 4 + BCE_THREADS - 1) / BCE_THREADS + 1);
    hipLaunchKernelGGL(bce_partial_kernel, dim3(nblk), dim3(BCE_THREADS), 0, (hipStream_t)stream, x, target, (size_t)n, (double *)ws);
    MMK_LAUNCH_CHECK();
    hipLaunchKernelGGL(bce_final_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, (const double *)ws, nblk, 1.0 / (double)n, out);
    MMK_LAUNCH_CHECK();
    return MMK_OK;
}

extern "C" int mmk_bce_mean_bwd(const float *x, const float *target, int64_t n, const float *grad_out, float *grad_x, void *stream)
{
    MMK_REQUIRE(x && target && grad_out && grad_x && n >= 1, "mmk_bce_mean_bwd: bad argument");
    MMK_REQUIRE((((uintptr_t)x | (uintptr_t)target | (uintptr_t)grad_x) & 15) == 0, "mmk_bce_mean_bwd: buffers must be 16-byte aligned");
    const int nblk = (int)std::min<size_t>(4096, ((size_t)n / 4 + BCE_THREADS - 1) / BCE_THREADS + 1);
    hipLaunchKernelGGL(bce_bwd_kernel, dim3(nblk), dim3(BCE_THREADS), 0, (hipStream_t)stream, x, target, (size_t)n, grad_out,
                       (float)(1.0 / (double)n), grad_x);
    MMK_LAUNCH_CHECK();
    return MMK_OK;
}

extern "C" int mmk_pose_loss_gt_fwd(const float *T_pred, const float *T_gt, int32_t B, float *out2, void *stream)
{
    MMK_REQUIRE(T_pred && T_gt && out2 && B >= 1, "mmk_pose_loss_gt_fwd: bad argument");
    hipLaunchKernelGGL(pose_metric_kernel<2>, dim3(1), dim3(64), 0, (hipStream_t)stream, T_pred, T_gt, B, out2);
    MMK_LAUNCH_CHECK();
    return MMK_OK;
}

extern "C" int mmk_pose_loss_gt_bwd(const float *T_pred, const float *T_gt, int32_t B, const float *g_rot, const float *g_trans,
                                    float *grad_T, void *stream)
{
    MMK_REQUIRE(T_pred && T_gt && grad_T && B >= 1, "mmk_pose_loss_gt_bwd: bad argument");
    hipLaunchKernelGGL(pose_loss_gt_bwd_kernel, dim3((B + 63) / 64), dim3(64), 0, (hipStream_t)stream, T_pred, T_gt, B, g_rot, g_trans,
                       grad_T);
    MMK_LAUNCH_CHECK();
    return MMK_OK;
}

extern "C" int mmk_val_metric(const float *T_pred, const float *T_gt, int32_t B, float *out3, void *stream)
{
    MMK_REQUIRE(T_pred && out3 && B >= 1, "mmk_val_metric: bad argument");
    hipLaunchKernelGGL(pose_metric_kernel<3>, dim3(1), dim3(64), 0, (hipStream_t)stream, T_pred, T_gt, B, out3);
    MMK_LAUNCH_CHECK();
    return MMK_OK;
}

extern "C" int mmk_pose_loss_se3_fwd(const float *T_pred, const float *T_gt, int32_t B, float *out2, void *stream)
{
    MMK_REQUIRE(T_pred, "mmk_pose_loss_se3_fwd: T_pred is NULL");
    MMK_REQUIRE(out2, "mmk_pose_loss_se3_fwd: out2 is NULL");
    MMK_REQUIRE(B >= 1, "mmk_pose_loss_se3_fwd: B = %d < 1", (int)B);
    hipLaunchKernelGGL(pose_se3_metric_kernel<2>, dim3(1), dim3(64), 0, (hipStream_t)stream, T_pred, T_gt, B, out2);
    MMK_LAUNCH_CHECK();
    return MMK_OK;
}

extern "C" int mmk_pose_loss_se3_bwd(const float *T_pred, const float *T_gt, int32_t B, const float *g_rot, const float *g_trans,
                                     float *grad_T, void *stream)
{
    MMK_REQUIRE(T_pred, "mmk_pose_loss_se3_bwd: T_pred is NULL");
    MMK_REQUIRE(grad_T, "mmk_pose_loss_se3_bwd: grad_T is NULL");
    MMK_REQUIRE(B >= 1, "mmk_pose_loss_se3_bwd: B = %d < 1", (int)B);
    hipLaunchKernelGGL(pose_se3_bwd_kernel, dim3((B + 63) / 64), dim3(64), 0, (hipStream_t)stream, T_pred, T_gt, B, g_rot, g_trans,
                       grad_T);
    MMK_LAUNCH_CHECK();
    return MMK_OK;
}

extern "C" int mmk_val_metric_se3(const float *T_pred, const float *T_gt, int32_t B, float *out3, void *stream)
{
    MMK_REQUIRE(T_pred, "mmk_val_metric_se3: T_pred is NULL");
    MMK_REQUIRE(out3, "mmk_val_metric_se3: out3 is NULL");
    MMK_REQUIRE(B >= 1, "mmk_val_metric_se3: B = %d < 1", (int)B);
    hipLaunchKernelGGL(pose_se3_metric_kernel<3>, dim3(1), dim3(64), 0, (hipStream_t)stream, T_pred, T_gt, B, out3);
    MMK_LAUNCH_CHECK();
    return MMK_OK;
}

// workspace of the fft-threshold entry points: the per-image mean partials (reused for the BCE block partials once the
// thresholds are computed), then B thresholds
static size_t fft_partials_bytes(int32_t B)
{
    return mmk::align_up((size_t)std::max<int64_t>((int64_t)B * FFT_MEAN_BLOCKS, BCE_BLOCKS) * sizeof(double), 256);
}

extern "C" size_t mmk_fft_threshold_ws_bytes(int32_t B) { return B < 1 ? 0 : fft_partials_bytes(B) + (size_t)B * sizeof(float); }

static int fft_thresholds(const float *fft, int32_t B, int64_t hw, double *part, float *thr, hipStream_t st)
{
    hipLaunchKernelGGL(image_sum_partial_kernel, dim3(FFT_MEAN_BLOCKS, B), dim3(256), 0, st, fft, (size_t)hw, part);
    MMK_LAUNCH_CHECK();
    hipLaunchKernelGGL(image_threshold_kernel, dim3(B), dim3(64), 0, st, (const double *)part, (size_t)hw, thr);
    MMK_LAUNCH_CHECK();
    return MMK_OK;
}

static int bce_blocks(size_t n) { return (int)std::min<size_t>(BCE_BLOCKS, (n / 4 + BCE_THREADS - 1) / BCE_THREADS + 1); }

extern "C" int mmk_fft_threshold_mask(const float *fft, int32_t B, int64_t hw, void *ws, size_t ws_bytes, float *mask_out, void *stream)
{
    MMK_REQUIRE(fft && ws && mask_out && B >= 1 && B <= 65535 && hw >= 4, "mmk_fft_threshold_mask: bad argument");
    MMK_REQUIRE(ws_bytes >= mmk_fft_threshold_ws_bytes(B), "mmk_fft_threshold_mask: workspace too small");
    MMK_REQUIRE((((uintptr_t)fft | (uintptr_t)mask_out) & 15) == 0, "mmk_fft_threshold_mask: buffers must be 16-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    float *thr = reinterpret_cast<float *>(static_cast<char *>(ws) + fft_partials_bytes(B));
    const int rc = fft_thresholds(fft, B, hw, static_cast<double *>(ws), thr, st);
    if (rc != MMK_OK) return rc;
    const size_t n = (size_t)B * (size_t)hw;
    const int nblk = (int)std::min<size_t>(4096, (n / 4 + 255) / 256 + 1);
    hipLaunchKernelGGL(fft_mask_kernel, dim3(nblk), dim3(256), 0, st, fft, (const float *)thr, (size_t)hw, n, mask_out);
    MMK_LAUNCH_CHECK();
    return MMK_OK;
}

extern "C" int mmk_bce_fft_threshold_fwd(const float *x, const float *fft, int32_t B, int64_t hw, void *ws, size_t ws_bytes,
                                         float *thr_out, float *out, void *stream)
{
    MMK_REQUIRE(x && fft && ws && thr_out && out && B >= 1 && B <= 65535 && hw >= 4, "mmk_bce_fft_threshold_fwd: bad argument");
    MMK_REQUIRE(ws_bytes >= mmk_fft_threshold_ws_bytes(B), "mmk_bce_fft_threshold_fwd: workspace too small");
    MMK_REQUIRE((((uintptr_t)x | (uintptr_t)fft) & 15) == 0, "mmk_bce_fft_threshold_fwd: inputs must be 16-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    double *part = static_cast<double *>(ws);
    const int rc = fft_thresholds(fft, B, hw, part, thr_out, st);
    if (rc != MMK_OK) return rc;
    const size_t n = (size_t)B * (size_t)hw;
    const int nblk = bce_blocks(n);
    hipLaunchKernelGGL(bce_fft_partial_kernel, dim3(nblk), dim3(BCE_THREADS), 0, st, x, fft, (const float *)thr_out, (size_t)hw, n, part);
    MMK_LAUNCH_CHECK();
    hipLaunchKernelGGL(bce_final_kernel, dim3(1), dim3(256), 0, st, (const double *)part, nblk, 1.0 / (double)n, out);
    MMK_LAUNCH_CHECK();
    return MMK_OK;
}

extern "C" int mmk_bce_fft_threshold_bwd(const float *x, const float *fft, int32_t B, int64_t hw, const float *thr, const float *grad_out,
                                         float *grad_x, void *stream)
{
    MMK_REQUIRE(x && fft && thr && grad_out && grad_x && B >= 1 && hw >= 4, "mmk_bce_fft_threshold_bwd: bad argument");
    MMK_REQUIRE((((uintptr_t)x | (uintptr_t)fft | (uintptr_t)grad_x) & 15) == 0,
                "mmk_bce_fft_threshold_bwd: buffers must be 16-byte aligned");
    const size_t n = (size_t)B * (size_t)hw;
    const int nblk = (int)std::min<size_t>(4096, (n / 4 + BCE_THREADS - 1) / BCE_THREADS + 1);
    hipLaunchKernelGGL(bce_fft_bwd_kernel, dim3(nblk), dim3(BCE_THREADS), 0, (hipStream_t)stream, x, fft, thr, (size_t)hw, n, grad_out,
                       (float)(1.0 / (double)n), grad_x);
    MMK_LAUNCH_CHECK();
    return MMK_OK;
}
